"""Checks of forward kinematics (cg_forward_kinematics), the window gather (cg_gather_windows) and the motion bank, shared by the
shim run on the CPU box (tests/test_emu_kinematics.py) and the run on the MI355X (tests/test_gpu_kinematics.py).

Yardsticks.  tests/golden/aug_kinematics.npz (tools/gen_golden_kinematics.py) holds the reference's own fp32 results and, per
forward-kinematics case, `ref_err`: the reference's max abs error against the fp64 restatement of tests/kinematics_ref.py.
  fixture cases   the kernel's max abs error against the restatement is at most 4 x ref_err of the case (the bound the feature
                  was specified with: a different operation order over chains ~10 deep), and so it is within 5 x ref_err of the
                  recorded reference output.
  loop shapes     against the restatement alone.  The kernel composes in f64 and rounds each coordinate to fp32 once, so
                  |out - ref| <= 2^-24 |ref| (half an ulp; an ulp is at most 2^-23 |x|) + 1e-10 max|ref| (f64 rounding of a
                  composition of up to 63 levels at the magnitude of the largest coordinate, ~1e-13 relative, with room for a
                  different libm).  FK_ULPS below is that half ulp with 20 % slack for the additive term at small coordinates.
  gather          bit-exact where no flip applies (copy, joint selection, IEEE fp32 `(v - mean) / std`); a flipped window's y within
                  4 ulp of its largest |y| (f64 centroid, one fp32 rounding, one subtraction), its x and z bit-exact.
  bank readers    like the fixture cases, with the reference's error taken on the recorded `target` itself against the restatement
                  of the whole pipeline.

Measured ratios (kernel error / ref_err; the bound is 4).  The shim run (x86-64, g++ -O1) and the MI355X give the same figures: the
composition is f64 on both and the result is rounded once.
  chain_h36m 0.380   chain_cmu 0.286   smpl_smpl24_p24 0.160   smpl_smpl24_p30 0.270   smpl_smplh52_p52 0.119
  h36m_bank target 0.335   amass_bank target, per file 0.436 / 0.251 / 0.353
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import kinematics_ref as KR

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aug_kinematics.npz"))
CASES = [str(c) for c in FIX["fk/cases"]]
FK_ULPS = 0.6            # of 2^-23 |ref|: see the module docstring
_F32_EPS = 2.0 ** -23


def tree(name):
    return [int(v) for v in FIX["tree/%s/parent" % name]], FIX["tree/%s/rest" % name]


def run_fk(device, angles, parent, rest, convention, select=None, scale=1.0):
    from cistgcn_amd import ops
    out = ops.forward_kinematics(torch.from_numpy(np.ascontiguousarray(angles)).to(device), parent, torch.from_numpy(rest).to(device),
                                 convention=convention, select=select, scale=scale)
    return out.cpu().numpy()


def restate(angles, parent, rest, convention, select=None, scale=1.0):
    return (KR.fk_chain if convention == "expmap_chain" else KR.fk_smpl)(angles, parent, rest, select=select, scale=scale)


def _case(name):
    g = lambda k: FIX["fk/%s/%s" % (name, k)]
    parent, rest = tree(str(g("tree")))
    return parent, rest, str(g("convention")), g("angles"), g("out"), float(g("scale")), float(g("ref_err"))


# ---- forward kinematics: the fixture -------------------------------------------------------------------------------------------------
def check_fk_fixture(device, name):
    parent, rest, conv, angles, ref32, scale, ref_err = _case(name)
    out = run_fk(device, angles, parent, rest, conv, scale=scale)
    assert out.dtype == np.float32 and out.shape == ref32.shape
    ref64 = restate(angles, parent, rest, conv, scale=scale)
    err = float(np.abs(out.astype(np.float64) - ref64).max())
    print("fk %s: kernel error %.3e, reference fp32 error %.3e, ratio %.3f (bound 4)" % (name, err, ref_err, err / ref_err))
    assert err <= 4.0 * ref_err
    assert float(np.abs(out.astype(np.float64) - ref32.astype(np.float64)).max()) <= 5.0 * ref_err


def check_restatement(name):
    """the restatement against the recorded reference: the recorded error is reproduced, and it is fp32 rounding (a misread
    convention - the quirk of the chain included - would be off by whole bone lengths)"""
    parent, rest, conv, angles, ref32, scale, ref_err = _case(name)
    ref64 = restate(angles, parent, rest, conv, scale=scale)
    err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    assert abs(err - ref_err) <= 1e-9 * np.abs(ref64).max()
    assert 0 < err <= 16 * _F32_EPS * np.abs(ref64).max()


def fixture_covers_the_issue():
    for name in CASES:
        parent, rest, conv, angles, ref32, scale, ref_err = _case(name)
        J = len(parent)
        r = angles[:, 3:].reshape(len(angles), J, 3) if conv == "expmap_chain" else angles
        nrm = np.linalg.norm(r.astype(np.float64), axis=-1)
        assert (nrm == 0).any() and ((nrm > 0) & (nrm < 3e-3)).any() and (nrm > 0.1).any(), name
        if conv == "expmap_chain":
            assert (nrm[:, 0] > 0).all(), name                  # joint 0 rotates: the quirk is exercised
        else:
            assert not ((nrm > 0) & (nrm < 1e-4)).any(), name
    assert [len(tree(t)[0]) for t in ("h36m", "cmu", "smpl24", "smplh52")] == [32, 38, 24, 52]
    inv = FIX["h36m/inverted"]
    assert inv.any() and (~inv).any() and len(FIX["h36m/files"]) == 10
    assert sorted(float(FIX["amass/rate/%d" % i]) for i in range(3)) == [50.0, 100.0, 120.0]


# ---- forward kinematics: loop shapes against the restatement ---------------------------------------------------------------------------
def _seeded_tree(g, J, kind):
    if kind == "line":
        parent = [-1] + list(range(J - 1))
    elif kind == "star":
        parent = [-1] + [0] * (J - 1)
    else:
        parent = [-1] + [int(g.randint(0, i)) for i in range(1, J)]
    rest = g.uniform(-1.0, 1.0, size=(J, 3)).astype(np.float32)
    return parent, rest


def _limits():
    from cistgcn_amd import _lib
    return _lib.LIMITS["CG_FK_MAX_BLOCKS"], _lib.LIMITS["CG_FK_THREADS"] // 64


def fk_shapes():
    """(convention, tree kind, J, N, select kind, scale).  N = "pass2" / "pass1": past one full pass of the capped grid with two
    frames / one frame per wavefront."""
    shapes, Ns, sels = [], (1, 3, 65, 130), (None, "subset", "repeats")
    for i, J in enumerate((1, 2, 31, 32, 33, 38, 52, 64)):
        for c, conv in enumerate(("expmap_chain", "smpl")):
            shapes.append((conv, "random", J, Ns[(i + c) % 4], sels[(i + 2 * c) % 3], (1.0, 1000.0)[(i + c) % 2]))
    shapes += [("expmap_chain", "line", 64, 3, None, 1.0), ("smpl", "line", 64, 65, "repeats", 1000.0),
               ("expmap_chain", "star", 20, 65, None, 1000.0), ("smpl", "star", 20, 3, "subset", 1.0),
               ("expmap_chain", "h36m", 32, 130, "subset", 1.0), ("smpl", "h36m", 32, 1, None, 1.0),
               ("expmap_chain", "random", 2, "pass2", None, 1.0), ("smpl", "random", 33, "pass1", "subset", 1000.0)]
    return shapes


def shape_id(s):
    return "-".join(str(v) for v in s)


def check_fk_shape(device, shape):
    conv, kind, J, N, sel_kind, scale = shape
    g = np.random.RandomState(sum(ord(c) for c in shape_id(shape)))
    blocks, waves = _limits()
    if N == "pass2":
        N = blocks * waves * 2 + 11
    elif N == "pass1":
        N = blocks * waves + 5
    parent, rest = tree("h36m") if kind == "h36m" else _seeded_tree(g, J, kind)
    if kind == "h36m":
        rest = (rest / 100).astype(np.float32)
    select = None if sel_kind is None else [int(v) for v in (g.permutation(J)[:max(1, J // 2)] if sel_kind == "subset" else g.randint(0, J, size=min(64, J + 3)))]
    J_pose = J + (3 if J < 60 else 0)
    if conv == "expmap_chain":
        angles = g.uniform(-1.2, 1.2, size=(N, 3 + 3 * J)).astype(np.float32)
    else:
        angles = g.uniform(-1.2, 1.2, size=(N, J_pose, 3)).astype(np.float32)
    angles.reshape(N, -1)[::3, 6:12] = 0                       # some exact zeros
    out = run_fk(device, angles, parent, rest, conv, select=select, scale=scale)
    ref = restate(angles, parent, rest, conv, select=select, scale=scale)
    assert out.shape == ref.shape and out.dtype == np.float32
    bound = FK_ULPS * _F32_EPS * np.abs(ref) + 1e-10 * np.abs(ref).max()
    over = np.abs(out.astype(np.float64) - ref) - bound
    assert over.max() <= 0, "%s: %.3e over the bound at %s" % (shape_id(shape), over.max(), np.unravel_index(over.argmax(), over.shape))


def _rest_pose(parent, rest, conv):
    """what identity rotations give: SMPL the rest positions themselves; the chain the offsets summed down the tree (a joint below
    joint 0 starts a new sum: the reference's `if parent[i] > 0`), in f64 - sums of a few fp32 numbers, exact - rounded once"""
    if conv == "smpl":
        return rest
    p = rest.astype(np.float64)
    for i in range(1, len(parent)):
        if parent[i] > 0:
            p[i] = rest[i].astype(np.float64) + p[parent[i]]
    return p.astype(np.float32)


def check_fk_zero_rotations(device):
    """theta = 0 is the identity exactly, in both conventions: the rest pose comes out to the bit; in the chain convention joint 0's
    rotation (and the three ignored columns) reach nobody; a leaf's rotation moves nothing"""
    for name, conv in (("h36m", "expmap_chain"), ("cmu", "expmap_chain"), ("smpl24", "smpl"), ("smplh52", "smpl")):
        parent, rest = tree(name)
        J = len(parent)
        want = np.broadcast_to(_rest_pose(parent, rest, conv), (5, J, 3))
        zero = np.zeros((5, 3 + 3 * J) if conv == "expmap_chain" else (5, J, 3), dtype=np.float32)
        assert np.array_equal(run_fk(device, zero, parent, rest, conv), want), name
        leaf = J - 1
        assert leaf not in parent
        moved = zero.copy()
        if conv == "expmap_chain":
            moved[:, 0:6] = np.float32(0.7)                     # the ignored columns and joint 0
            moved[:, 3 + 3 * leaf:6 + 3 * leaf] = np.float32(-1.1)
        else:
            moved[:, leaf] = np.float32(-1.1)
        assert np.array_equal(run_fk(device, moved, parent, rest, conv), want), name
    # some joints zero, the others not: against the restatement, where theta == 0 is the identity by construction
    check_fk_shape(device, ("smpl", "random", 24, 65, None, 1.0))


def check_fk_inputs_untouched_and_reproducible(device):
    from cistgcn_amd import ops
    g = np.random.RandomState(5)
    for conv, name in (("expmap_chain", "h36m"), ("smpl", "smplh52")):
        parent, rest = tree(name)
        J = len(parent)
        a = torch.from_numpy(g.uniform(-1, 1, size=(37, 3 + 3 * J) if conv == "expmap_chain" else (37, J, 3)).astype(np.float32)).to(device)
        r = torch.from_numpy(rest).to(device)
        a0, r0 = a.clone(), r.clone()
        one = ops.forward_kinematics(a, parent, r, convention=conv, select=[3, 1, 1], scale=1000.0)
        two = ops.forward_kinematics(a, parent, r, convention=conv, select=[3, 1, 1], scale=1000.0)
        assert torch.equal(one, two) and torch.equal(a, a0) and torch.equal(r, r0)
        assert one.shape == (37, 3, 3) and torch.equal(one[:, 1], one[:, 2])


def check_fk_interface_errors(device):
    from cistgcn_amd import _lib, ops
    parent, rest = tree("smpl24")
    J = len(parent)
    rest_t = torch.from_numpy(rest).to(device)
    chain, pose = torch.zeros(4, 3 + 3 * J).to(device), torch.zeros(4, J, 3).to(device)
    fk = ops.forward_kinematics
    for bad in ([-1, 1] + parent[2:], [-1, 0, 3] + parent[3:], [0] + parent[1:], [-1, -2] + parent[2:]):      # parent[i] >= i, root, < -1
        with pytest.raises(ValueError):
            fk(pose, bad, rest_t, convention="smpl")
    with pytest.raises(ValueError):
        fk(torch.zeros(4, 3).to(device), [], torch.zeros(0, 3).to(device))                     # J = 0
    with pytest.raises(ValueError):
        fk(torch.zeros(4, 3 + 3 * 65).to(device), [-1] + list(range(64)), torch.zeros(65, 3).to(device))      # J > 64
    fk(torch.zeros(4, 3 + 3 * 64).to(device), [-1] + list(range(63)), torch.zeros(64, 3).to(device))
    for bad in (torch.zeros(4, 3 * J).to(device), torch.zeros(4, 4 + 3 * J).to(device), pose):               # wrong angle width
        with pytest.raises(ValueError):
            fk(bad, parent, rest_t)
    with pytest.raises(ValueError):
        fk(pose[:, :J - 1], parent, rest_t, convention="smpl")                                    # J_pose < J
    with pytest.raises(ValueError):
        fk(chain, parent, rest_t, convention="smpl")
    with pytest.raises(ValueError):
        fk(chain, parent, rest_t, convention="euler")
    with pytest.raises(ValueError):
        fk(chain, parent, rest_t[:J - 1])
    for bad in ([J], [-1], [0, 1, J + 5]):                                                          # select out of range
        with pytest.raises(IndexError):
            fk(chain, parent, rest_t, select=bad)
    with pytest.raises(ValueError):
        fk(chain, parent, rest_t, select=[])
    with pytest.raises(TypeError):
        fk(chain.double(), parent, rest_t)
    with pytest.raises(TypeError):
        fk(chain, parent, rest_t.double())
    with pytest.raises(ValueError):
        fk(chain.clone().requires_grad_(True), parent, rest_t)
    # strided operands are handled as by the neighbouring operators: copied by a kernel
    g = np.random.RandomState(9)
    wide = torch.from_numpy(g.uniform(-1, 1, size=(6, 2 * (3 + 3 * J))).astype(np.float32)).to(device)
    assert torch.equal(fk(wide[:, ::2], parent, rest_t), fk(wide[:, ::2].contiguous(), parent, rest_t))
    assert fk(chain[:0], parent, rest_t).shape == (0, J, 3)
    # the C ABI itself: status codes, nothing launched (device pointers are never followed)
    fn = _lib.lib().cg_forward_kinematics
    p = 64

    def block(J=3, J_out=3, conv=0, J_pose=3, N=1, par=(-1, 0, 1), angles=p, rest=p, out=p, select=None):
        a = _lib.ForwardKinematics()
        a.convention, a.J, a.J_pose, a.J_out, a.N, a.scale = conv, J, J_pose, J_out, N, 1.0
        a.host_parent = (ctypes.c_int * len(par))(*par)         # kept alive by the block
        a.angles, a.parent, a.rest, a.out, a.select = angles, ctypes.cast(a.host_parent, ctypes.c_void_p), rest, out, select
        return a
    for kw in (dict(angles=None), dict(rest=None), dict(out=None)):
        assert fn(ctypes.byref(block(**kw)), None) == -1
    a = block()
    a.parent = None
    assert fn(ctypes.byref(a), None) == -1
    for kw in (dict(J=0), dict(J=65), dict(J_out=0), dict(J_out=65, select=p), dict(conv=2), dict(conv=1, J_pose=2), dict(N=-1), dict(J_out=2),
               dict(par=(0, 0, 1)), dict(par=(-1, 1, 1)), dict(par=(-1, 0, 2)), dict(par=(-1, -2, 0))):
        assert fn(ctypes.byref(block(**kw)), None) == -2, kw
    assert fn(ctypes.byref(block(N=0)), None) == 0


def check_host_tensors_refused():
    """without the shim there is no CPU path: refused before anything is launched"""
    from cistgcn_amd import _lib, ops
    was = _lib._host_pointers_ok
    _lib._host_pointers_ok = False
    try:
        with pytest.raises(RuntimeError):
            ops.forward_kinematics(torch.zeros(2, 9), [-1, 0], torch.zeros(2, 3))
        with pytest.raises(RuntimeError):
            ops.gather_windows(torch.zeros(8, 2, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 4)
    finally:
        _lib._host_pointers_ok = was


# ---- window gather ---------------------------------------------------------------------------------------------------------------------
def _sequences(g, J_src, lengths, up_src=None):
    """seeded sequences with coordinates of the loaders' magnitude; with `up_src` = (hi, lo) source joints the first frame of about half
    of all windows is upside down"""
    seqs = []
    for F in lengths:
        s = (g.randn(F, J_src, 3) * 300).astype(np.float32)
        if up_src is not None:
            sign = np.where(g.uniform(size=F) < 0.5, -1.0, 1.0)
            s[:, up_src[0], 1] = s[:, up_src[1], 1] + (sign * g.uniform(1, 50, size=F)).astype(np.float32)
        seqs.append(s)
    return seqs


GATHER_SHAPES = [(B, L, sel, norm) for B, L, sel, norm in
                 ((1, 5, "32to22", False), (3, 35, "22to18", True), (70, 75, None, False), (70, 5, "32to22", True), (3, 75, "32to22", False),
                  (1, 35, None, True), (70, 35, "22to18", False))]


def _gather_setup(device, sel_kind, L, seed=3):
    from cistgcn_amd.environment import MotionBank
    g = np.random.RandomState(seed)
    J_src, select = {"32to22": (32, [j for j in range(32) if j not in (0, 1, 6, 11, 16, 20, 23, 24, 28, 31)]),
                     "22to18": (22, list(range(4, 22))), None: (7, None)}[sel_kind]
    up = (3, 5)                                                # in the selected numbering
    up_src = tuple((select or list(range(J_src)))[j] for j in up)
    seqs = _sequences(g, J_src, (L + 9, L, L + 30), up_src)
    # a window with equal heights on its first frame (sequence 0, frame 2): strictly `< 0`, so it is not mirrored
    seqs[0][2, up_src[0], 1] = seqs[0][2, up_src[1], 1]
    bank = MotionBank.from_sequences([torch.from_numpy(s).to(device) for s in seqs], ["a", "b", "c"], L, select=select, up_joints=up)
    return bank, np.concatenate(seqs, 0)


def check_gather_shape(device, shape):
    B, L, sel_kind, norm = shape
    bank, frames = _gather_setup(device, sel_kind, L)
    if norm:
        bank.mean, bank.std = 12.5, 310.0
    W = len(bank)
    assert W == 10 + 1 + 31 and bank.starts[10] == L + 9 and bank.starts[-1] + L == len(frames)       # overlapping, stride 1
    g = np.random.RandomState(B)
    _, all_flipped = KR.gather(frames, bank.starts, np.arange(W), L, select=bank.select, mean=bank.mean, std=bank.std, up_joints=bank.up_joints)
    # first: the equal-heights window (2), an upside-down one, the last window of the bank, of sequence 0, the one-window sequence
    items = np.concatenate([[2, int(np.where(all_flipped)[0][0]), W - 1, 9, 10], g.randint(0, W, size=B)])[:B] if B > 1 else np.array([W - 1])
    raw = bank.windows(torch.from_numpy(items.astype(np.int32)).to(device)).cpu().numpy()
    ref, flipped = KR.gather(frames, bank.starts, items, L, select=bank.select, mean=bank.mean, std=bank.std, up_joints=bank.up_joints)
    assert raw.shape == ref.shape == (B, L, len(bank.select) if bank.select else frames.shape[1], 3) and raw.dtype == np.float32
    if B >= 3:
        assert flipped.any() and (~flipped).any()
        assert 2 in items and not flipped[list(items).index(2)]
    assert np.array_equal(raw[~flipped], ref[~flipped].astype(np.float32))
    assert np.array_equal(raw[flipped][..., 0::2], ref[flipped][..., 0::2].astype(np.float32))
    for b in np.where(flipped)[0]:
        ulp = float(np.spacing(np.float32(np.abs(ref[b, :, :, 1]).max())))
        assert np.abs(raw[b, :, :, 1].astype(np.float64) - ref[b, :, :, 1]).max() <= 4 * ulp
    # the same windows without the check: the plain copy
    bank.up_joints = None
    plain = bank.windows(items.tolist()).cpu().numpy()
    ref_plain, _ = KR.gather(frames, bank.starts, items, L, select=bank.select, mean=bank.mean, std=bank.std)
    assert np.array_equal(plain, ref_plain.astype(np.float32))


def check_gather_inputs_untouched_and_reproducible(device):
    bank, _ = _gather_setup(device, "32to22", 35)
    bank.mean, bank.std = -3.0, 77.0
    frames0, starts0 = bank.frames.clone(), bank.starts_dev.clone()
    items = torch.arange(len(bank), dtype=torch.int32).to(device)
    one, two = bank.windows(items), bank.windows(items)
    assert torch.equal(one, two) and torch.equal(bank.frames, frames0) and torch.equal(bank.starts_dev, starts0)
    assert torch.equal(items, torch.arange(len(bank), dtype=torch.int32).to(device))
    assert torch.equal(bank.windows(items.long()), one)


def check_gather_clamps_device_ids(device):
    """a device id is trusted and clamped by the kernel: out-of-range ids read the first / last window, nothing out of bounds"""
    bank, _ = _gather_setup(device, None, 5)
    W = len(bank)
    got = bank.windows(torch.tensor([-7, W, W + 1000, 3], dtype=torch.int32).to(device))
    want = bank.windows([0, W - 1, W - 1, 3])
    assert torch.equal(got, want)


def check_gather_errors(device):
    from cistgcn_amd import _lib, ops
    from cistgcn_amd.environment import MotionBank
    bank, _ = _gather_setup(device, "22to18", 5)
    W = len(bank)
    for bad in ([0, W], [-1], np.array([W + 3]), torch.tensor([W]) if device != "cpu" else [W]):
        with pytest.raises(IndexError):
            bank.windows(bad)
    with pytest.raises(TypeError):
        bank.windows([0.5])
    seqs = [torch.zeros(9, 4, 3).to(device), torch.zeros(6, 4, 3).to(device)]
    MotionBank.from_sequences(seqs, ["a", "b"], 5, starts=[[0, 4], [1]])
    for bad in ([[0, 5], [1]], [[0], [2]], [[-1], [0]], [[8], [0]]):      # a window crossing into the next sequence / out of the bank
        with pytest.raises(ValueError):
            MotionBank.from_sequences(seqs, ["a", "b"], 5, starts=bad)
    with pytest.raises(ValueError):
        MotionBank.from_sequences(seqs, ["a"], 5)
    assert len(MotionBank.from_sequences(seqs, ["a", "b"], 7)) == 3      # the short sequence holds no window
    fr, st, it = bank.frames, bank.starts_dev, torch.zeros(2, dtype=torch.int32).to(device)
    with pytest.raises(TypeError):
        ops.gather_windows(fr.double(), st, it, 5)
    with pytest.raises(TypeError):
        ops.gather_windows(fr, st.float(), it, 5)
    with pytest.raises(ValueError):
        ops.gather_windows(fr[0], st, it, 5)
    with pytest.raises(ValueError):
        ops.gather_windows(fr, st, it, fr.shape[0] + 1)
    with pytest.raises(ValueError):
        ops.gather_windows(fr, st, it, 5, std=0.0)
    with pytest.raises(IndexError):
        ops.gather_windows(fr, st, it, 5, select=[0, 22])
    with pytest.raises(IndexError):
        ops.gather_windows(fr, st, it, 5, select=[0, 1], up_joints=(0, 2))
    wide = torch.cat([fr, fr], 2)
    assert torch.equal(ops.gather_windows(wide[:, :, :3], st, it, 5), ops.gather_windows(fr, st, it, 5))      # strided: copied by a kernel
    fn = _lib.lib().cg_gather_windows
    p = 64

    def block(**kw):
        a = _lib.GatherWindows()
        a.B, a.L, a.J_src, a.J, a.W, a.up_hi, a.up_lo, a.F, a.mean, a.std = 2, 5, 4, 4, 3, -1, -1, 9, 0.0, 1.0
        a.frames = a.starts = a.items = a.raw = p
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for k in ("frames", "starts", "items", "raw"):
        assert fn(ctypes.byref(block(**{k: None})), None) == -1
    for kw in (dict(B=0), dict(L=0), dict(J=0), dict(J_src=0), dict(W=0), dict(F=4), dict(std=0.0), dict(J=3), dict(up_hi=0), dict(up_hi=4, up_lo=0),
               dict(up_hi=0, up_lo=-1), dict(up_hi=-2, up_lo=-2)):
        assert fn(ctypes.byref(block(**kw)), None) == -2, kw


# ---- bank and readers ------------------------------------------------------------------------------------------------------------------
def _write_h36m(root, files):
    for name, a in files.items():
        path = os.path.join(str(root), name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savetxt(path, a, fmt="%.9g", delimiter=",")


def _against_reference(what, got, ref64, ref32):
    """the FK tolerance on a loader's output: the kernel's error against the fp64 restatement of the pipeline is at most 4 x the
    reference's own (its recorded `target` against the same restatement)"""
    ref_err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print("%s: kernel error %.3e, reference fp32 error %.3e, ratio %.3f (bound 4)" % (what, err, ref_err, err / ref_err))
    assert 0 < ref_err <= 16 * _F32_EPS * np.abs(ref64).max()
    assert err <= 4.0 * ref_err


def check_h36m_bank(device, tmp_path):
    from cistgcn_amd.environment import h36m_bank
    files = {str(n): FIX["h36m/file/" + str(n)] for n in FIX["h36m/files"]}
    _write_h36m(tmp_path, files)
    parent, rest = tree("h36m")
    input_n, output_n = int(FIX["h36m/input_n"]), int(FIX["h36m/output_n"])
    up = tuple(int(v) for v in FIX["h36m/up_joints"])
    bank = h36m_bank(tmp_path, [str(FIX["h36m/action"])], input_n, output_n, "train", tree=(parent, rest), up_joints=up, device=device)
    target = FIX["h36m/target"]
    assert len(bank) == len(target) and bank.select == [int(v) for v in FIX["h36m/dim_used"]]
    assert list(bank.labels) == [str(c) for c in FIX["h36m/class_seq"]]
    assert list(bank.labels_of([0, len(bank) - 1])) == [str(FIX["h36m/class_seq"][0]), str(FIX["h36m/class_seq"][-1])]
    got = bank.windows(np.arange(len(bank))).cpu().numpy()
    assert got.shape == target.shape
    # the pipeline restated in fp64 end to end: files in the loader's order -> zeroed columns, every second frame -> chain -> windows -> fix
    seqs = []
    for name in FIX["h36m/files"]:
        a = files[str(name)].copy()
        a[:, 0:6] = 0
        seqs.append(KR.fk_chain(a[::2], parent, rest))
    L = input_n + output_n
    starts = np.concatenate([np.arange(len(s) - L + 1) + sum(len(q) for q in seqs[:i]) for i, s in enumerate(seqs)])
    assert np.array_equal(starts, bank.starts)
    ref64, flipped = KR.gather(np.concatenate(seqs, 0), starts, np.arange(len(starts)), L, select=bank.select, up_joints=up)
    assert np.array_equal(flipped, FIX["h36m/inverted"]) and flipped.any() and (~flipped).any()
    _against_reference("h36m_bank", got, ref64, target)
    # per window, the mirrored ones among them: the same bound
    for b in np.where(flipped)[0]:
        assert np.abs(got[b].astype(np.float64) - target[b]).max() <= 5.0 * np.abs(target.astype(np.float64) - ref64).max()


def check_amass_bank(device, tmp_path):
    from cistgcn_amd.environment import amass_bank
    parent, p3d0 = FIX["amass/parents"], FIX["amass/p3d0"]
    np.savez(os.path.join(str(tmp_path), "smpl_skeleton.npz"), p3d0=p3d0, parents=parent)
    rels = [str(f) for f in FIX["amass/files"]]
    for i, rel in enumerate(rels):
        os.makedirs(os.path.dirname(os.path.join(str(tmp_path), rel)), exist_ok=True)
        np.savez(os.path.join(str(tmp_path), rel), poses=FIX["amass/poses/%d" % i].astype(np.float64), mocap_framerate=FIX["amass/rate/%d" % i])
    np.savez(os.path.join(str(tmp_path), os.path.dirname(rels[0]), "shape.npz"), betas=np.zeros(16))       # no `poses`: skipped
    input_n, output_n = int(FIX["amass/input_n"]), int(FIX["amass/output_n"])
    bank = amass_bank(tmp_path, ["ACCAD"], input_n, output_n, "train", device=device)
    target, classes = FIX["amass/target"], np.array([str(c) for c in FIX["amass/class_seq"]])
    assert len(bank) == len(target) and bank.select == list(range(4, 22))
    got = bank.windows(np.arange(len(bank))).cpu().numpy()
    # the reference reads the files in the order of its directory scan: compare file by file, windows in order inside a file
    assert sorted(set(bank.labels)) == sorted(set(classes)) and len(set(classes)) == 3
    L, par = input_n + output_n, [-1] + [int(v) for v in parent[1:]]
    for i, rel in enumerate(rels):
        label = os.path.basename(os.path.dirname(rel)) + "_" + os.path.basename(rel)[:-4]
        mine, theirs = got[bank.labels == label], target[classes == label]
        assert mine.shape == theirs.shape and len(mine) > 0
        poses = FIX["amass/poses/%d" % i][::int(float(FIX["amass/rate/%d" % i]) // 25)].reshape(-1, 52, 3).copy()
        poses[:, 0] = 0
        seq = KR.fk_smpl(poses, par, p3d0[0], select=list(range(22)), scale=1000.0)
        starts = np.arange(0, len(seq) - L + 1, 5)
        ref64, _ = KR.gather(seq, starts, np.arange(len(starts)), L, select=list(range(4, 22)))
        _against_reference("amass_bank " + label, mine, ref64, theirs)


def check_find_indices_256():
    from cistgcn_amd.environment import find_indices_256
    input_n, seq_len = int(FIX["find256/input_n"]), int(FIX["find256/seq_len"])
    for F1, F2 in ((400, 523), (1210, 987)):
        s1, s2 = find_indices_256(F1, F2, seq_len, input_n=input_n)
        assert np.array_equal(s1, FIX["find256/%d_%d/s1" % (F1, F2)]) and np.array_equal(s2, FIX["find256/%d_%d/s2" % (F1, F2)])


def check_original_test_starts(device, tmp_path):
    """`original_test`: the 2 x 128 windows of find_indices_256 as explicit starts, the second sub-action's offset by the first's frames"""
    from cistgcn_amd.environment import h36m_bank
    g = np.random.RandomState(17)
    F1, F2 = 400, 523
    _write_h36m(tmp_path, {"S5/walking_1.txt": (g.randn(2 * F1, 99) * 0.3).astype(np.float32), "S5/walking_2.txt": (g.randn(2 * F2 - 1, 99) * 0.3).astype(np.float32)})
    input_n, seq_len = int(FIX["find256/input_n"]), int(FIX["find256/seq_len"])
    bank = h36m_bank(tmp_path, "walking", input_n, seq_len - input_n, "original_test", tree=tree("h36m"), device=device)
    assert len(bank) == 256 and bank.frames.shape[0] == F1 + F2
    assert np.array_equal(bank.starts[:128], FIX["find256/400_523/s1"]) and np.array_equal(bank.starts[128:], FIX["find256/400_523/s2"] + F1)
    assert bank.windows([0, 255]).shape == (2, seq_len, 22, 3)


def check_batches(device):
    from cistgcn_amd.environment import DeviceAugmentation
    input_n = 10
    bank, frames = _gather_setup(device, "32to22", 35)
    W = len(bank)                                                # 42
    gen = torch.Generator(device=device)
    gen.manual_seed(4)
    seen, sizes = [], []
    for b in bank.batches(16, shuffle=True, generator=gen):
        assert b["raw"].shape[1:] == (35, 22, 3) and b["item"].device == bank.frames.device and b["item"].dtype == torch.int32
        assert torch.equal(b["raw"], bank.windows(b["item"]))
        seen += b["item"].cpu().tolist()
        sizes.append(len(b["item"]))
    assert sorted(seen) == list(range(W)) and seen != list(range(W)) and sizes == [16, 16, 10]
    assert [len(b["item"]) for b in bank.batches(16, shuffle=True, drop_last=True)] == [16, 16]
    plain = [b["item"].cpu().tolist() for b in bank.batches(20)]
    assert sum(plain, []) == list(range(W)) and [len(p) for p in plain] == [20, 20, 2]
    b = next(iter(bank.batches(8, shuffle=True)))
    item = DeviceAugmentation()(b["raw"], input_n)
    shapes = {k: tuple(v.shape) for k, v in item.items()}
    assert shapes == {"sample": (8, 10, 22, 3), "sample_vel": (8, 10, 22, 3), "target": (8, 25, 22, 3), "target_vel": (8, 25, 22, 3),
                      "target_gvel": (8, 25, 22, 1)}
    assert torch.equal(item["sample"], b["raw"][:, :input_n]) and torch.equal(item["target"], b["raw"][:, input_n:])
