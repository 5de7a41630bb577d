"""Checks of the evaluation metrics (ops.eval_metrics, environment.evaluation.EvalMetrics), shared by the CPU suite
(tests/test_metrics.py, the kernels of csrc/eval_metrics.hip under the HIP shim) and the MI355X suite (tests/test_gpu_metrics.py).
Every check takes the device.

Two references:
* tests/golden/eval_metrics.npz: what the real reference's `Metrics.compute` / `losses` gave on three small cases and over two
  batches, evaluated in fp64 on the fp32 inputs, with `gap` = max |reference in fp32 - reference in fp64| per tensor
  (tools/gen_golden_metrics.py);
* `restate` below: the nine metrics from their definitions in stock PyTorch, written from scratch; proven against the fixture on
  the CPU and then used where the fixture has no case (the large random shape of the GPU suite).

Tolerance, per tensor: max |got - ref64| <= FACTOR * max(gap, eps32 * max |ref64|) with FACTOR = 4.  The kernels are another fp32-in /
fp32-out evaluation of the same quantity (other summation order, other 3x3 decomposition), so their distance to fp64 is of the order
of the reference's own; 4 covers the tail of a maximum over a few thousand entries.  The floor term is one fp32 rounding of the
largest entry.
"""
import os

import numpy as np
import pytest
import torch

from cistgcn_amd import ops
from cistgcn_amd.environment import EvalMetrics
from helpers import GOLDEN_DIR

FACTOR = 4.0
EPS32 = float(np.finfo(np.float32).eps)
METRICS = ("mpjpe", "pa_mpjpe", "n_mpjpe", "mve", "w_mpjpe", "bone_l", "w_bone_l", "w_joints", "w_joints_t")
CASES = ("A", "B", "C")
MODES = {"frames": "frames", "joint": None}          # fixture tag -> `reduce`
_fixture = []


def fixture():
    if not _fixture:
        z = np.load(os.path.join(GOLDEN_DIR, "eval_metrics.npz"))
        _fixture.append({k: z[k] for k in z.files})
    return _fixture[0]


def case_inputs(name, device="cpu"):
    """(pred, target, speeds, bones) of a fixture case; fresh tensors every time"""
    fx = fixture()
    pre = "acc" if name == "second" else name
    bones = [tuple(int(v) for v in p) for p in fx[("A" if name == "second" else name) + "/bones"]]
    return tuple(torch.from_numpy(fx["%s/%s" % (pre, k)].copy()).to(device) for k in ("pred", "target", "speeds")) + (bones,)


def bound_of(ref, gap):
    ref = np.asarray(ref, dtype=np.float64)
    return FACTOR * max(float(gap), EPS32 * float(np.abs(ref).max()))


def assert_within(got, ref, gap, what):
    """prints error / bound, then asserts; returns the error"""
    if isinstance(got, torch.Tensor):
        got = got.detach().cpu().numpy()
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: not finite" % what
    err, bound = float(np.abs(got - ref).max()), bound_of(ref, gap)
    print("%-40s err %.3e  bound %.3e  (%.2f of it; gap %.2e, max|ref| %.3e)" % (what, err, bound, err / bound, float(gap), float(np.abs(ref).max())))
    assert err <= bound, "%s: max err %.3e > bound %.3e" % (what, err, bound)
    return err


# ---------------------------------------------------------------------------------------------------------
# the restatement: stock PyTorch, in the dtype of its inputs, nothing modified in place
# ---------------------------------------------------------------------------------------------------------
def restate(pred, target, speeds, bones, reduce="frames", quirk=True):
    P, X = pred, target
    B, To, J, _ = P.shape
    dt = P.dtype
    w = (torch.arange(1, To + 1, device=P.device) / To).to(dt)[None, :, None]          # fp32 weights, then the working dtype
    e = (P - X).norm(dim=-1)
    c = (X * P).sum(-1).mean(-1) / (P * P).sum(-1).mean(-1)
    n = (c[..., None, None] * P - X).norm(dim=-1)
    mve = ((P[:, 1:] - P[:, :-1]) - (X[:, 1:] - X[:, :-1])).norm(dim=-1)
    bi = torch.tensor([p[0] for p in bones], device=P.device)
    bj = torch.tensor([p[1] for p in bones], device=P.device)
    bone = ((P[:, :, bi] - P[:, :, bj]).norm(dim=-1) - (X[:, :, bi] - X[:, :, bj]).norm(dim=-1)).abs()
    sn = speeds / (speeds.max(2, keepdim=True)[0] + 1e-6)
    st = (sn + w) / (sn + w).max(0, keepdim=True)[0]
    # Procrustes per frame
    muX, muY = X.mean(2, keepdim=True), P.mean(2, keepdim=True)
    X0, Y0 = X - muX, P - muY
    if quirk:
        X0 = torch.where(X0 * X0 < 1e-6, torch.full_like(X0, 1e-3), X0)
    normX = (X0 * X0).sum((-1, -2), keepdim=True).sqrt().clamp_min(1e-3)
    normY = (Y0 * Y0).sum((-1, -2), keepdim=True).sqrt()
    H = (X0 / normX).transpose(-1, -2) @ (Y0 / normY)
    ok = torch.isfinite(H).all(-1).all(-1)
    Hs = torch.where(ok[..., None, None], H, torch.eye(3, dtype=dt, device=P.device).expand_as(H))
    # polar factor through the symmetric eigenproblem of H^T H: H = Q S, Q = U V^T, S = V diag(s) V^T
    lam, V = torch.linalg.eigh(Hs.transpose(-1, -2) @ Hs)                  # ascending: lam[..., 0] is the smallest
    s = lam.clamp_min(0).sqrt()
    Q = Hs @ V @ torch.diag_embed(1 / s) @ V.transpose(-1, -2)
    R0 = Q.transpose(-1, -2)                                                # V U^T
    sigma = torch.sign(torch.linalg.det(R0))
    R = R0.clone()
    R[..., 2, :] = R[..., 2, :] * sigma[..., None]                          # diag(1,1,sigma) V U^T
    tr = (s[..., 1] + s[..., 2] + sigma * s[..., 0])[..., None, None]
    a = tr * normX / normY
    t = muX - a * (muY @ R)
    nan = torch.full((), float("nan"), dtype=dt, device=P.device)
    a, R, t = torch.where(ok[..., None, None], a, nan), torch.where(ok[..., None, None], R, nan), torch.where(ok[..., None, None], t, nan)
    a, R, t = torch.where(a != a, torch.ones_like(a), a), torch.where(R != R, torch.zeros_like(R), R), torch.where(t != t, torch.zeros_like(t), t)
    pa = (a * (P @ R) + t - X).norm(dim=-1)
    out = {"mpjpe": e, "pa_mpjpe": pa, "n_mpjpe": n, "mve": mve, "w_mpjpe": w * e, "bone_l": bone, "w_bone_l": w * bone,
           "w_joints": sn * e, "w_joints_t": st * e}
    if reduce == "frames":
        out = {k: v.mean((0, 2)) for k, v in out.items()}
    return out


# ---------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------
_results = {}


def results(device, name, mode):
    """ops.eval_metrics on a fixture case, once per (device, case, mode); the checks read it and leave it unchanged"""
    key = (str(device), name, mode)
    if key not in _results:
        pred, target, speeds, bones = case_inputs(name, device)
        _results[key] = {k: v.cpu() for k, v in ops.eval_metrics(pred, target, speeds, bones, reduce=MODES[mode]).items()}
    return _results[key]


def check_against_fixture(device, name, mode, metric):
    fx = fixture()
    got = results(device, name, mode)
    assert sorted(got) == sorted(METRICS)
    key = "%s/%s/%s" % (name, mode, metric)
    assert got[metric].dtype == torch.float32
    assert_within(got[metric], fx[key], fx[key + "/gap"], "%s on %s" % (key, device))


def check_nan_rule_and_reflection(device):
    """what the two special samples of case A are there for, read off the recording and off the kernel alike"""
    fx = fixture()
    ref = fx["A/joint/pa_mpjpe"]
    x_norm = np.linalg.norm(fx["A/target"][2, 0].astype(np.float64), axis=-1)
    assert float(np.abs(ref[2, 0] - x_norm).max()) <= 1e-9 * float(x_norm.max()), "the recording does not show |X| on the frame whose predicted joints coincide"
    per_sample = ref.mean((1, 2))
    assert per_sample[1] > 5 * np.delete(per_sample, 1).max(), "the mirrored sample of the recording is not set apart: %s" % per_sample
    got = results(device, "A", "joint")["pa_mpjpe"].numpy().astype(np.float64)
    assert float(np.abs(got[2, 0] - x_norm).max()) <= FACTOR * EPS32 * float(x_norm.max())
    assert got.mean((1, 2))[1] > 5 * np.delete(got.mean((1, 2)), 1).max()


def check_restatement(name, mode):
    """the restatement in fp64 against the recording: both are fp64 evaluations, so the bound's floor term is what applies"""
    fx = fixture()
    pred, target, speeds, bones = case_inputs(name)
    got = restate(pred.double(), target.double(), speeds.double(), bones, MODES[mode])
    for metric in METRICS:
        key = "%s/%s/%s" % (name, mode, metric)
        assert_within(got[metric], fx[key], fx[key + "/gap"], "restatement " + key)


def check_quirk_is_detected():
    """guards the guard: without the 1e-3 replacement the restatement must miss the bound of case B's pa_mpjpe, in both modes"""
    fx = fixture()
    pred, target, speeds, bones = case_inputs("B")
    for mode in MODES:
        got = restate(pred.double(), target.double(), speeds.double(), bones, MODES[mode], quirk=False)["pa_mpjpe"].numpy()
        key = "B/%s/pa_mpjpe" % mode
        err, bound = float(np.abs(got - fx[key]).max()), bound_of(fx[key], fx[key + "/gap"])
        print("%s without the replacement: err %.3e, bound %.3e (%.0f times)" % (key, err, bound, err / bound))
        assert err > 16.0 / FACTOR * bound, "%s: the comparison would not notice a missing replacement (err %.3e, bound %.3e)" % (key, err, bound)


def check_mpjpe_matches_eval_scatter(device, name):
    """frames-mode `mpjpe` against the error vector of ops.eval_scatter_mpjpe for the same tensors (all joints predicted)"""
    fx = fixture()
    pred, target, _, _ = case_inputs(name, device)
    J = pred.shape[2]
    _, err = ops.eval_scatter_mpjpe(pred, target, list(range(J)))
    key = "%s/frames/mpjpe" % name
    got = results(device, name, "frames")["mpjpe"].numpy().astype(np.float64)
    other = err.cpu().numpy().astype(np.float64)
    err, bound = float(np.abs(got - other).max()), bound_of(fx[key], fx[key + "/gap"])
    assert err <= bound, "%s: eval_metrics and eval_scatter_mpjpe differ by %.3e (bound %.3e)" % (key, err, bound)


def check_accumulator(device, joint):
    fx = fixture()
    mode = "joint" if joint else "frames"
    acc = EvalMetrics(case_inputs("A")[3], compute_joint_error=joint)
    for name in ("A", "second"):
        pred, target, speeds, _ = case_inputs(name, device)
        acc.update(pred, target, speeds)
    res = acc.result()
    assert sorted(res) == sorted([k for m in METRICS for k in (m, m + "_seq")])
    for m in METRICS:
        assert np.ndim(res[m]) == 0
        assert_within(res[m], fx["acc/%s/%s" % (mode, m)], fx["acc/%s/%s/gap" % (mode, m)], "EvalMetrics %s %s on %s" % (mode, m, device))
        k = m + "_seq"
        ref = np.concatenate([fx["A/joint/" + m], fx["acc/joint/%s/tail" % k]]) if joint else fx["acc/frames/" + k]
        assert isinstance(res[k], np.ndarray)
        assert_within(res[k], ref, fx["acc/%s/%s/gap" % (mode, k)], "EvalMetrics %s %s on %s" % (mode, k, device))
    with pytest.raises(ValueError):
        acc.update(*[t[:, :-1] for t in case_inputs("A", device)[:3]])


def check_inputs_untouched(device):
    for mode in MODES.values():
        pred, target, speeds, bones = case_inputs("B", device)
        keep = [t.clone() for t in (pred, target, speeds)]
        ops.eval_metrics(pred, target, speeds, bones, reduce=mode)
        assert all(torch.equal(a, b) for a, b in zip(keep, (pred, target, speeds))), "eval_metrics wrote to an input"


def check_bit_reproducible(device):
    pred, target, speeds, bones = case_inputs("A", device)
    first = ops.eval_metrics(pred, target, speeds, bones)
    second = ops.eval_metrics(pred, target, speeds, bones)
    for k in METRICS:
        assert torch.equal(first[k], second[k]), "%s differs between two calls" % k
        assert torch.equal(first[k].cpu(), results(device, "A", "frames")[k])


def check_strided_inputs(device):
    """non-contiguous views are copied, not misread"""
    pred, target, speeds, bones = case_inputs("C", device)
    wide = torch.zeros(pred.shape[:3] + (5,), device=device)
    wide[..., 1:4] = pred
    got = ops.eval_metrics(wide[..., 1:4], target.transpose(1, 2).contiguous().transpose(1, 2), speeds.transpose(0, 1).contiguous().transpose(0, 1),
                           bones, reduce=None)
    for k in METRICS:
        assert torch.equal(got[k].cpu(), results(device, "C", "joint")[k]), k


def check_interface_errors(device):
    pred, target, speeds, bones = case_inputs("C", device)
    B, To, J, _ = pred.shape
    with pytest.raises(ValueError):
        ops.eval_metrics(pred, target[:, :, :-1], speeds, bones)
    with pytest.raises(ValueError):
        ops.eval_metrics(pred[..., :2], target[..., :2], speeds, bones)
    with pytest.raises(ValueError):
        big = torch.zeros(1, 2, 65, 3, device=device)
        ops.eval_metrics(big, big, torch.zeros(1, 2, 65, device=device), bones)
    with pytest.raises(ValueError):
        ops.eval_metrics(pred[:, :1], target[:, :1], speeds[:, :1], bones)
    with pytest.raises(ValueError):
        ops.eval_metrics(pred, target, speeds[..., None], bones)
    with pytest.raises(ValueError):
        ops.eval_metrics(pred, target, speeds[:, :, :-1], bones)
    with pytest.raises(ValueError):
        ops.eval_metrics(pred, target, speeds, bones, reduce="joints")
    with pytest.raises(IndexError):
        ops.eval_metrics(pred, target, speeds, bones + [(0, J)])
    with pytest.raises(IndexError):
        ops.eval_metrics(pred, target, speeds, [(-1, 0)])
    # the C ABI itself: status codes, nothing launched
    import ctypes
    from cistgcn_amd import _lib
    a = _lib.EvalMetricsArgs()
    assert _lib.lib().cg_eval_metrics(ctypes.byref(a), None) == -1
    assert _lib.lib().cg_eval_metrics_ws_doubles(1, 2, 65) == 0 and _lib.lib().cg_eval_metrics_ws_doubles(1, 1, 22) == 0
    assert _lib.lib().cg_eval_metrics_ws_doubles(3, 10, 22) == 10 * 22 + 7 * 3 * 10


def check_full_wave(device):
    """a skeleton of 64 joints (no idle lane) with more bones than lanes, one of them of length 0"""
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(2, 3, 64, 3, generator=gen)
    x = p + 0.1 * torch.randn(2, 3, 64, 3, generator=gen)
    s = torch.rand(2, 3, 64, generator=gen)
    many = [(i, (i * 7 + 1) % 64) for i in range(64)] + [(63, 0), (5, 5), (1, 62)]
    for mode in MODES.values():
        got = ops.eval_metrics(p.to(device), x.to(device), s.to(device), many, reduce=mode)
        ref, r32 = restate(p.double(), x.double(), s.double(), many, mode), restate(p, x, s, many, mode)
        for k in METRICS:
            assert_within(got[k], ref[k].numpy(), float((r32[k].double() - ref[k]).abs().max()), "J=64, 67 bones, %s %s" % (mode, k))


LARGE = (67, 25, 22)


def check_large_random(device):
    """B=67: more frames than one pass of a small grid would hold, a last workgroup that is only partly filled (67 * 25 = 1675 frames,
    4 per workgroup), and a batch reduction of more than 64 samples.  Against the restatement in fp64; `gap` is the restatement's
    own fp32 <-> fp64 distance."""
    B, To, J = LARGE
    bones = case_inputs("B")[3]
    gen = torch.Generator().manual_seed(67)
    target = 0.3 * torch.randn(B, To, J, 3, generator=gen)
    pred = target + 0.02 * torch.randn(B, To, J, 3, generator=gen)
    speeds = torch.cumsum(torch.rand(B, To, J, generator=gen) * 0.003, 1)
    for mode in MODES.values():
        got = ops.eval_metrics(pred.to(device), target.to(device), speeds.to(device), bones, reduce=mode)
        ref, r32 = restate(pred.double(), target.double(), speeds.double(), bones, mode), restate(pred, target, speeds, bones, mode)
        for k in METRICS:
            assert_within(got[k], ref[k].numpy(), float((r32[k].double() - ref[k]).abs().max()), "large %s %s" % (mode, k))
