"""Checks of the robustness-test transforms (`cistgcn_amd.environment.RobustnessTest` over cg_perturb_sequences), device as an argument:
tests/test_emu_robustness.py runs them on the CPU-only box through the HIP shim, tests/test_gpu_robustness.py on the MI355X.

References: tests/golden/aug_robustness.npz (the reference's own transform classes behind `H36m_Motion3D.__getitem__` with recorded
draws, tools/gen_golden_robustness.py) and the fp64 restatement tests/robustness_ref.py, itself pinned by that fixture.
The bound is the one tests/test_environment.py uses for this pipeline: 1e-4 * max(1, max|ref|) per key - fp32 arithmetic on
coordinates of a few hundred to a thousand millimetres leaves errors of 1e-4 .. 1e-3 mm, a wrong window, weight, centroid or
extent moves a frame by millimetres to metres."""
import ctypes
import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import robustness_ref as R
from helpers import GOLDEN_DIR

KEYS = ("processed", "sample", "sample_vel", "target", "target_vel", "target_gvel")
SHAPES = ((2, 4, 3, 2),          # 12 points: less than one wavefront
          (3, 35, 32, 10),       # 1120 points: several passes of the 256 threads, no multiple of 256
          (2, 75, 64, 50),       # 57600 bytes of LDS: past the 48 KB opt-in
          (5, 20, 7, 12))


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "aug_robustness.npz"))
    return {k: z[k] for k in z.files}


CASES = tuple(str(c) for c in fixture()["cases"])


def bound(ref):
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


def compare(got, ref, what):
    """every key of the item dictionary within the bound; prints each figure before it asserts"""
    for k in KEYS:
        g, r = got[k].cpu().numpy(), np.asarray(ref[k])
        assert g.shape == r.shape and g.dtype == np.float32, (what, k, g.shape, r.shape)
        err = float(np.abs(g.astype(np.float64) - r).max())
        print("%s %s: max err %.3e, bound %.3e" % (what, k, err, bound(r)))
        assert err <= bound(r), "%s %s: %.3e > %.3e" % (what, k, err, bound(r))


def reference_items(case):
    """the six item tensors of the reference for a fixture case: the three it stores and the three that are slices / fp32
    frame differences of its `processed` (h36m_motion_3d.py:97-102)"""
    fx, n = fixture(), int(fixture()["input_n"])
    proc = fx[case + "/processed"]
    return {"processed": proc, "sample": proc[:, :n], "target": proc[:, n:], "sample_vel": np.diff(proc, axis=1)[:, :n],
            "target_vel": fx[case + "/target_vel"], "target_gvel": fx[case + "/target_gvel"]}


@functools.lru_cache(maxsize=None)
def device_run(device, case):
    """(item dictionary of the device, draws consumed) for a fixture case, on its recorded draws; computed once"""
    from cistgcn_amd.environment import RobustnessTest
    fx = fixture()
    raw = fx[case + "/raw"]
    rt = RobustnessTest(R.section(fx[case + "/config"]))
    rng = R.Replay(fx[case + "/draws"])
    params = rt.draw(raw.shape[0], rng, joints=raw.shape[2])
    out = rt(torch.from_numpy(raw).to(device), int(fx["input_n"]), params, keep_processed=True)
    return out, rng.i


def check_against_fixture(device, case):
    out, _ = device_run(device, case)
    compare(out, reference_items(case), case)


def check_draws(device, case):
    fx = fixture()
    _, used = device_run(device, case)
    assert used == len(fx[case + "/draws"]) == int(fx[case + "/ndraws"].sum()), \
        "the host side drew %d numbers, the reference %d" % (used, len(fx[case + "/draws"]))


def check_restatement(case):
    fx = fixture()
    got, used = R.perturb_batch(fx[case + "/raw"], fx[case + "/config"], fx[case + "/draws"], int(fx["input_n"]))
    assert used == len(fx[case + "/draws"])
    ref = reference_items(case)
    for k in KEYS:
        err = float(np.abs(got[k] - ref[k]).max())
        assert err <= bound(ref[k]), "%s %s: %.3e" % (case, k, err)


def fixture_covers_the_issue():
    """what the generator promises about the threshold-0.5 cases, re-derived from the recorded draw counts: in each of them some
    sample draws more numbers than another (a step applied here, skipped there)"""
    fx = fixture()
    for case in ("thr_half_ramps", "thr_half_flip_invert"):
        assert len(set(int(v) for v in fx[case + "/ndraws"])) > 1, case
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "aug_robustness.npz")) < os.path.getsize(os.path.join(GOLDEN_DIR, "aug_h36m_noise_inv.npz"))


def chain_section(L, J):
    """every kind the section can hold, windows scaled to L (all satisfy 0 <= s0 < s1 <= L for L >= 4); inversion needs the 32-joint
    skeleton"""
    w = lambda s0, s1, cont, keep: dict(prob_threshold=0.5, seq_idx=[s0, s1], continuous=cont, keep=keep)
    cfg = NS(random_flip=NS(x=True, y="", z=True), random_rotation=NS(x=[-20, 20], y=[-180, 180], z=""),
             random_scale=NS(x=[0.8, 1.2], y=1.1, z=""), random_noise=0.03, random_translation=NS(x=[-0.2, 0.2], y="", z=0.1),
             rotation=NS(x=[-60, 60], y=45.0, z=[-10, 10], **w(1, L - 1, True, True)),
             scale=NS(x=1.3, y=[0.6, 0.9], z=0, **w(0, max(1, L // 2), False, False)),
             noise=NS(noise=0.05, **w(L // 2, L, True, True)),
             translation=NS(x=0.2, y=[-0.3, 0.3], z="", **w(1, L, True, False)),
             flip=NS(x="", y=True, z=True, prob_threshold=0.5, seq_idx=[L // 4, L // 2 + 1], keep=False))
    if J >= 32:
        cfg.pose_invers = NS(prob_threshold=0.5, seq_idx=[L // 3, L - 1], keep=True)
    return cfg


def check_shape(device, shape, seed=7):
    """device against the restatement on fresh draws of a real generator (the bounds of every interval matter), eleven steps"""
    from cistgcn_amd.environment import RobustnessTest
    B, L, J, input_n = shape
    g = np.random.RandomState(seed)
    raw = (50 + 350 * g.randn(B, L, J, 3)).astype(np.float32)
    cfg = chain_section(L, J)
    rt = RobustnessTest(cfg)
    assert len(rt.steps) == (11 if J >= 32 else 10)
    r1, r2 = np.random.RandomState(seed + 1), np.random.RandomState(seed + 1)
    out = rt(torch.from_numpy(raw).to(device), input_n, rt.draw(B, r1, joints=J), keep_processed=True)
    steps = R.steps_of(cfg)
    items = [R.item_tensors(R.perturb_one(raw[b], steps, r2), input_n) for b in range(B)]
    assert r1.uniform() == r2.uniform(), "the host side and the restatement consumed different numbers of draws"
    compare(out, {k: np.stack([it[k] for it in items]) for k in KEYS}, "x".join(str(v) for v in shape))


def check_equivalence_with_old_kernel(device):
    """a section of random_* entries only: the step-list kernel on whole-sequence, constant steps in the old kernel's order gives
    the bits of cg_augment_sequences on the same draws"""
    from cistgcn_amd.environment import DeviceAugmentation, RobustnessTest
    cfg = NS(random_scale=NS(x=[0.95, 1.05], y=[0.90, 1.10], z=[0.95, 1.05]), random_noise=0.02, random_flip=NS(x=True, y="", z=True),
             random_rotation=NS(x=[-5, 5], y=[-180, 180], z=[-5, 5]), random_translation=NS(x=[-0.10, 0.10], y=[-0.10, 0.10], z=[-0.10, 0.10]))
    B, L, J, input_n = 8, 35, 22, 10
    g = np.random.RandomState(21)
    raw = torch.from_numpy((50 + 350 * g.randn(B, L, J, 3)).astype(np.float32)).to(device)
    old, new = DeviceAugmentation(cfg), RobustnessTest(cfg)
    r1, r2 = np.random.RandomState(22), np.random.RandomState(22)
    p_old, p_new = old.draw(B, r1, joints=J), new.draw(B, r2, joints=J)
    assert r1.uniform() == r2.uniform()
    applied = p_new["params"][:, :, 0]
    assert applied.any(0).all() and not applied.all(0).any(), "every step should be applied for one sample and skipped for another"
    a, b = old(raw, input_n, p_old, keep_processed=True), new(raw, input_n, p_new, keep_processed=True)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), "%s: %.3e" % (k, float((a[k] - b[k]).abs().max()))


def check_no_steps(device):
    from cistgcn_amd.environment import RobustnessTest
    g = np.random.RandomState(3)
    raw = (50 + 350 * g.randn(3, 12, 5, 3)).astype(np.float32)
    for cfg in (None, "", NS(random_flip="", random_noise="", random_rotation=NS(x="", y="", z=""))):
        rt = RobustnessTest(cfg)
        assert rt.steps == [] and not rt.needs_joints
        params = rt.draw(3, R.Replay([]))
        assert params.shape == (3, 0, 4)
        out = rt(torch.from_numpy(raw).to(device), 8, params, keep_processed=True)
        assert np.array_equal(out["processed"].cpu().numpy(), raw)
        assert np.array_equal(out["sample"].cpu().numpy(), raw[:, :8]) and np.array_equal(out["target"].cpu().numpy(), raw[:, 8:])
        compare(out, {k: np.stack([R.item_tensors(r, 8)[k] for r in raw]) for k in KEYS}, "no steps")


def check_inputs_untouched_and_reproducible(device):
    """an inversion-only section (the reference swaps the joints inside the dataset's array then): raw keeps its bits, the output
    is the permuted input, and a second call gives the same bits"""
    from cistgcn_amd.environment import RobustnessTest
    g = np.random.RandomState(4)
    host = (50 + 350 * g.randn(3, 12, 32, 3)).astype(np.float32)
    raw = torch.from_numpy(host.copy()).to(device)
    rt = RobustnessTest(NS(pose_invers=NS(prob_threshold=0.0, seq_idx=[3, 7], keep=False)))
    params = rt.draw(3, np.random.RandomState(5), joints=32)
    assert params.shape == (3, 1, 4) and (params[:, 0, 0] == 1).all()
    out = rt(raw, 8, params, keep_processed=True)
    assert np.array_equal(raw.cpu().numpy(), host)
    want = host.copy()
    for x, y in R.INVERSE_PAIRS:
        want[:, 3:7, [x, y]] = want[:, 3:7, [y, x]]
    assert np.array_equal(out["processed"].cpu().numpy(), want) and not np.array_equal(want, host)
    # ... and with every other kind in the list
    cfg = chain_section(12, 32)
    rt = RobustnessTest(cfg)
    params = rt.draw(3, np.random.RandomState(6), joints=32)
    a = rt(raw, 8, params, keep_processed=True)
    b = rt(raw, 8, params, keep_processed=True)
    assert np.array_equal(raw.cpu().numpy(), host)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(IndexError):                       # the 32-joint pairs on 22 joints: IndexError in the reference, and here
        rt(torch.zeros(2, 12, 22, 3).to(device), 8)


def check_prefetcher(device):
    """DevicePrefetcher takes the new class unchanged: the same batches as direct calls on the same global draws"""
    from cistgcn_amd.environment import DevicePrefetcher, RobustnessTest
    g = np.random.RandomState(8)
    batches = [(50 + 350 * g.randn(2, 12, 5, 3)).astype(np.float32) for _ in range(3)]
    rt = RobustnessTest(chain_section(12, 5))
    state = np.random.get_state()
    try:
        np.random.seed(99)
        direct = [rt(torch.from_numpy(b).to(device), 8, rt.draw(2, joints=5)) for b in batches]
        np.random.seed(99)
        got = list(DevicePrefetcher(batches, rt, input_n=8, device=device))
    finally:
        np.random.set_state(state)
    assert len(got) == 3
    for a, b in zip(direct, got):
        assert sorted(a) == sorted(b) == sorted(k for k in KEYS if k != "processed")
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(got[0]["sample"].cpu(), torch.from_numpy(batches[0][:, :8]))


def check_interface_errors(device):
    from cistgcn_amd import _lib
    from cistgcn_amd.environment import RobustnessTest
    L = 12
    raw = torch.zeros(2, L, 5, 3).to(device)
    sec = lambda seq_idx: NS(scale=NS(x=1.2, y=0.8, z=1.1, prob_threshold=0.0, seq_idx=seq_idx, continuous=True, keep=True))
    for seq_idx in ([3, L + 2], [3, L + 1], [7, 3], [5, 5], [-1, 4]):          # the reference raises for [3, L + 2]
        with pytest.raises(ValueError):
            RobustnessTest(sec(seq_idx))(raw, 8)
    RobustnessTest(sec([3, L]))(raw, 8)
    ok = RobustnessTest(sec([3, 7]))
    for bad in (np.zeros((2, 2, 4), np.float32), np.zeros((3, 1, 4), np.float32), np.zeros((2, 4), np.float32), np.zeros((2, 24), np.float32)):
        with pytest.raises(ValueError):
            ok(raw, 8, bad)
    with pytest.raises(ValueError):
        ok(raw[0], 8)
    with pytest.raises(ValueError):                                            # a noise step without its draws
        RobustnessTest(NS(random_noise=0.1))(raw, 8, np.zeros((2, 1, 4), np.float32))
    many = RobustnessTest(sec([3, 7]))
    many.steps = many.steps * 17                                               # a section has eleven names: the limit guards the table
    with pytest.raises(ValueError):
        many.draw(2, R.Replay([0.9] * 200))
    with pytest.raises(ValueError):
        many(raw, 8, np.zeros((2, 17, 4), np.float32))
    many.steps = many.steps[:16]
    many(raw, 8, many.draw(2, R.Replay([0.9] * 200)))
    # the C ABI itself: status codes, nothing launched (the pointers are never followed)
    fn = _lib.lib().cg_perturb_sequences
    p = ctypes.c_void_p(64)
    row = lambda *v: (ctypes.c_int * 6)(*v)

    def status(steps, n_steps, raw_=p, params=p, noise=p, perm=p, Ls=L, J=5, n_noise=1):
        return fn(raw_, steps, params, noise, perm, p, p, p, p, None, None, 2, Ls, J, 8, n_steps, n_noise, None)

    good = row(_lib.LIMITS["CG_PERTURB_SCALE"], 3, 7, 1, 1, 0)
    assert status(good, 17) == -2 and status(good, -1) == -2
    assert status(good, 1, raw_=None) == -1 and status(good, 1, params=None) == -1 and status(None, 1) == -1
    assert status(row(6, 3, 7, 0, 0, 0), 1) == -2 and status(row(-1, 3, 7, 0, 0, 0), 1) == -2          # unknown kind
    for s0, s1 in ((3, L + 1), (7, 3), (5, 5), (-1, 4)):
        assert status(row(_lib.LIMITS["CG_PERTURB_SCALE"], s0, s1, 0, 0, 0), 1) == -2
    noise_row = row(_lib.LIMITS["CG_PERTURB_NOISE"], 0, L, 0, 1, 1)
    assert status(noise_row, 1) == -2 and status(noise_row, 1, n_noise=2, noise=None) == -1            # slot past n_noise; no table
    inv2 = (ctypes.c_int * 12)(_lib.LIMITS["CG_PERTURB_INVERT"], 0, L, 0, 1, 0, _lib.LIMITS["CG_PERTURB_SCALE"], 0, L, 0, 1, 0)
    assert status(inv2, 2) == -2 and status(inv2, 1, perm=None) == -1                                  # inversion must come last
    assert status(good, 1, Ls=200, J=65) == -2                                                         # 156000 bytes: past the LDS bound
    assert _lib.LIMITS["CG_PERTURB_MAX_STEPS"] == 16


def check_host_tensors_refused():
    """without the shim there is no CPU path: refused before anything is launched"""
    from cistgcn_amd import _lib
    from cistgcn_amd.environment import RobustnessTest
    was = _lib._host_pointers_ok
    _lib._host_pointers_ok = False
    try:
        with pytest.raises(ValueError):
            RobustnessTest(None)(torch.zeros(2, 12, 5, 3), 8)
    finally:
        _lib._host_pointers_ok = was
