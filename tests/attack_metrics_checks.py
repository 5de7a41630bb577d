"""Checks of the attack distortion metrics (ops.attack_metrics, `_Attack.metrics`), shared by the CPU suite
(tests/test_attack_metrics.py, the kernels of csrc/attack_metrics.hip under the HIP shim) and the MI355X suite
(tests/test_gpu_attack_metrics.py).  Every check takes the device.

Two references:
* tests/golden/eval_attack_metrics.npz: what the real reference's `ComputeAttackMetrics._get_metrics(adv, orig)` gave on three small
  cases, evaluated in fp64 on the fp32 inputs, with `gap` = max |reference in fp32 - reference in fp64| per entry, and the histogram
  counts and ranges of its fp32 run (tools/gen_golden_attack_metrics.py);
* the restatement below, stock PyTorch on the CPU, written from the definitions: `counts` in fp32 with the reference's operation order
  (a count flips on the last bit of a distance) and `restate` for everything else, in the dtype of its inputs.  Both are proven
  against the fixture and then used for the shapes the fixture has no case for.

Tolerance, per tensor, as in metrics_checks.py: max |got - ref64| <= 4 * max(gap, eps32 * max |ref64|).  Counts and ranges must match
exactly.
"""
import os

import numpy as np
import pytest
import torch

from cistgcn_amd import ops
from cistgcn_amd.environment import attacks
from helpers import GOLDEN_DIR
from metrics_checks import assert_within, bound_of

CASES = ("A", "B", "C")
KEYS = ops.ATTACK_METRICS
FAMILIES = ("sample", "temporal", "spatial")      # grouped by axis 0, 1, 2 of the (B,T,J,J) distances
HIST = ("KLD", "JSD", "KSTest")
BINS = 64
_fixture = []


def fixture():
    if not _fixture:
        z = np.load(os.path.join(GOLDEN_DIR, "eval_attack_metrics.npz"))
        _fixture.append({k: z[k] for k in z.files})
    return _fixture[0]


def case_inputs(name, device="cpu"):
    """(adv, orig) of a fixture case; fresh tensors every time"""
    fx = fixture()
    return tuple(torch.from_numpy(fx["%s/%s" % (name, k)].copy()).to(device) for k in ("adv", "orig"))


def family_key(fam, suffix):
    return "%s_sample" % suffix if fam == "sample" else "%s_%s" % (fam, suffix)


# ---------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------
def counts(adv, orig):
    """{"counts_<family>": (2,G,64) int64, "max_<family>": (G,) fp32}: fp32 distances sqrt(((dx*dx)+(dy*dy))+(dz*dz)), 65 edges
    fl32(k/64) * max per group, bin = largest k with edge_k <= x, the last edge inclusive.  The root is taken in fp64 and rounded:
    `torch.sqrt` of an fp32 CPU tensor may be off by one ulp (tools/gen_golden_attack_metrics.py)."""
    assert adv.dtype == torch.float32 and orig.dtype == torch.float32
    dev = adv.device      # the checks call it on the CPU, where every fp32 operation is rounded once; tools/bench_attack_metrics.py times it on the GPU
    ds = []
    for x in (adv, orig):
        d = x[..., :, None, :] - x[..., None, :, :]
        sq = d * d
        ds.append(torch.sqrt(((sq[..., 0] + sq[..., 1]) + sq[..., 2]).double()).float())      # the correctly rounded fp32 root
    out = {}
    for axis, fam in enumerate(FAMILIES):
        rows = [d.movedim(axis, 0).reshape(d.shape[axis], -1) for d in ds]
        mx = torch.maximum(rows[0].max(1)[0], rows[1].max(1)[0])
        edges = (torch.arange(BINS + 1, dtype=torch.float32, device=dev) / BINS)[None, :] * mx[:, None]
        cnt = []
        for r in rows:
            k = (torch.searchsorted(edges, r.contiguous(), right=True) - 1).clamp(0, BINS - 1)
            cnt.append(torch.zeros(r.shape[0], BINS, dtype=torch.int64, device=dev).scatter_add_(1, k, torch.ones_like(k)))
        out["counts_" + fam], out["max_" + fam] = torch.stack(cnt), mx
    return out


def histogram_metrics(cnt, mx):
    """(KLD, JSD, KSTest) per group in fp64 from integer counts (2,G,64) and the groups' ranges: density = count / n / width"""
    cnt, width = cnt.double(), mx.double()[:, None] / BINS
    p, q = cnt[0] / cnt[0].sum(1, keepdim=True) / width, cnt[1] / cnt[1].sum(1, keepdim=True) / width
    eps = 1e-8

    def entropy(a, b):
        return (a * (torch.log(a + eps) - torch.log(b + eps))).sum(1)

    mid = (p + q) / 2
    return entropy(p, q), (entropy(p, mid) + entropy(q, mid)) / 2, (p.cumsum(1) - q.cumsum(1)).abs().max(1)[0]


def pa_mpjpe(P, X):
    """losses.pa_mpjpe (losses/losses.py:79-144) per joint, with its replacement of small centred target coordinates.  Where H has
    rank 1 (two joints) the SVD's completion of U and V is arbitrary and so is the reference's sign(det); the proper rotation is taken
    there, which the aligned pose does not depend on."""
    muX, muY = X.mean(2, keepdim=True), P.mean(2, keepdim=True)
    X0, Y0 = X - muX, P - muY
    X0 = torch.where(X0 * X0 < 1e-6, torch.full_like(X0, 1e-3), X0)
    normX = (X0 * X0).sum((-1, -2), keepdim=True).sqrt().clamp_min(1e-3)
    normY = (Y0 * Y0).sum((-1, -2), keepdim=True).sqrt()
    U, s, Vt = torch.linalg.svd((X0 / normX).transpose(-1, -2) @ (Y0 / normY))
    V = Vt.transpose(-1, -2).clone()
    det = torch.sign(torch.linalg.det(V @ U.transpose(-1, -2)))
    rank1 = s[..., 1] <= 1e-7 * s[..., 0]
    one = torch.ones_like(det)
    U = torch.cat([U[..., :2], U[..., 2:] * torch.where(rank1, det, one)[..., None, None]], -1)
    sigma = torch.where(rank1, one, det)
    V[..., 2, :] = V[..., 2, :] * sigma[..., None]          # the last ROW of V, as the reference scales it (:117)
    R = V @ U.transpose(-1, -2)
    a = (s[..., 0] + s[..., 1] + sigma * s[..., 2])[..., None, None] * normX / normY
    t = muX - a * (muY @ R)
    return (a * (P @ R) + t - X).norm(dim=-1)


def restate(adv, orig, hist=None):
    """the 33 entries in the dtype of adv / orig (both on the CPU); `hist` = counts(...) of the fp32 inputs, else the 9 histogram
    entries are left out.  adv is `predicted`, orig is `target`."""
    A, O = adv, orig
    B, T, J, _ = A.shape
    scale = (O * A).sum(-1).mean(-1) / (A * A).sum(-1).mean(-1)
    maps = {"mpjpe": (A - O).norm(dim=-1), "n_mpjpe": (scale[..., None, None] * A - O).norm(dim=-1), "pa_mpjpe": pa_mpjpe(A, O),
            "mse": ((A - O) ** 2).mean(-1)}
    out = {}
    for k in ("mpjpe", "n_mpjpe", "pa_mpjpe"):
        out[k] = maps[k].mean()
    for k, m in maps.items():
        out["temporal_" + k], out["spatial_" + k], out[k + "_sample"] = m.mean((0, 2)), m.mean((0, 1)), m.mean((1, 2))
    h = (A[:, :, :, None, :] - O[:, :, None, :, :]).norm(dim=-1).min(-1)[0]                                   # (B,T,J): nearest joint of orig
    hb = (A.permute(1, 2, 0, 3)[:, :, :, None, :] - O.permute(1, 2, 0, 3)[:, :, None, :, :]).norm(dim=-1).min(-1)[0]      # (T,J,B): nearest sample
    out["hausdorff_mean_sample"], out["hausdorff_max_sample"] = h.mean((1, 2)), h.amax((1, 2))
    out["temporal_hausdorff_mean"], out["temporal_hausdorff_max"] = h.mean((0, 2)), h.amax((0, 2))
    out["spatial_hausdorff_mean"], out["spatial_hausdorff_max"] = hb.mean((0, 2)), hb.amax((0, 2))
    eps = 1e-6

    def cos(a, o, dim):
        return (a * o).sum(dim) / (a.norm(dim=dim).clamp_min(eps) * o.norm(dim=dim).clamp_min(eps))

    out["cosine_simil_sample"] = cos(A.reshape(B, -1), O.reshape(B, -1), 1)
    along = cos(A, O, 0)
    out["temporal_cos_simil"], out["spatial_cos_simil"] = along.mean((1, 2)), along.mean((0, 2))
    if hist is not None:
        for fam in FAMILIES:
            for k, v in zip(HIST, histogram_metrics(hist["counts_" + fam], hist["max_" + fam])):
                out[family_key(fam, k)] = v
    return out


# ---------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------
_results = {}


def results(device, name):
    """ops.attack_metrics(..., return_counts=True) on a fixture case, once per (device, case); the checks leave it unchanged"""
    key = (str(device), name)
    if key not in _results:
        adv, orig = case_inputs(name, device)
        _results[key] = {k: v.cpu() for k, v in ops.attack_metrics(adv, orig, return_counts=True).items()}
    return _results[key]


def check_against_fixture(device, name, key):
    fx = fixture()
    got = results(device, name)
    assert len(KEYS) == 33 and set(KEYS) <= set(got)
    assert got[key].dtype == torch.float32
    assert_within(got[key], fx["%s/%s" % (name, key)], fx["%s/%s/gap" % (name, key)], "%s/%s on %s" % (name, key, device))


def check_counts_against_fixture(device, name):
    fx = fixture()
    got = results(device, name)
    for fam in FAMILIES:
        c, m = got["counts_" + fam], got["max_" + fam]
        assert c.dtype == torch.int32 and m.dtype == torch.float32
        ref = fx["%s/counts_%s" % (name, fam)]
        assert c.shape == ref.shape, (c.shape, ref.shape)
        print("%s %s on %s: %d of %d counts differ" % (name, fam, device, int((c.numpy() != ref).sum()), ref.size))
        assert np.array_equal(c.numpy(), ref), "%s counts_%s" % (name, fam)
        assert np.array_equal(m.numpy(), fx["%s/max_%s" % (name, fam)]), "%s max_%s" % (name, fam)


def check_restatement(name):
    """the restatement against the recording: counts and ranges exactly, the 33 entries in fp64 within the bound"""
    fx = fixture()
    adv, orig = case_inputs(name)
    hist = counts(adv, orig)
    for fam in FAMILIES:
        assert np.array_equal(hist["counts_" + fam].numpy(), fx["%s/counts_%s" % (name, fam)]), fam
        assert np.array_equal(hist["max_" + fam].numpy(), fx["%s/max_%s" % (name, fam)]), fam
    got = restate(adv.double(), orig.double(), hist)
    assert sorted(got) == sorted(KEYS)
    for key in KEYS:
        assert_within(got[key], fx["%s/%s" % (name, key)], fx["%s/%s/gap" % (name, key)], "restatement %s/%s" % (name, key))


def check_identical_sample(device):
    """sample 1 of case A has adv == orig"""
    fx = fixture()
    assert np.array_equal(fx["A/adv"][1], fx["A/orig"][1]) and not np.array_equal(fx["A/adv"][0], fx["A/orig"][0])
    got = results(device, "A")
    for key in ("mpjpe_sample", "hausdorff_mean_sample", "hausdorff_max_sample", "mse_sample", "KLD_sample", "JSD_sample", "KSTest_sample"):
        assert float(got[key][1]) == 0.0, "%s of the unmoved sample is %r" % (key, float(got[key][1]))
        assert float(got[key][0]) > 0.0, key
    key = "A/cosine_simil_sample"
    assert abs(float(got["cosine_simil_sample"][1]) - 1.0) <= bound_of(fx[key], fx[key + "/gap"])


def check_roles(device):
    """swapping the arguments must move KLD_sample and hausdorff_mean_sample of case A by more than the bound"""
    fx = fixture()
    adv, orig = case_inputs("A", device)
    swapped = ops.attack_metrics(orig, adv)
    for key in ("KLD_sample", "hausdorff_mean_sample"):
        ref = fx["A/" + key]
        diff, bound = float(np.abs(swapped[key].cpu().numpy().astype(np.float64) - ref).max()), bound_of(ref, fx["A/%s/gap" % key])
        print("%s with the arguments swapped: off by %.3e, bound %.3e (%.0f times)" % (key, diff, bound, diff / bound))
        assert diff > bound, "%s: the comparison would not notice swapped arguments (off by %.3e, bound %.3e)" % (key, diff, bound)


# shapes at which a loop can go wrong: three batch tiles of the cross pass with the last partly filled and histogram rectangles that
# hang over both edges; a full wave; the smallest skeleton; B = T = 1; many workgroups with a partly filled last one
SHAPES = [(130, 3, 5), (3, 2, 64), (2, 3, 2), (1, 1, 7), (67, 7, 22)]


def check_shape(device, shape):
    B, T, J = shape
    gen = torch.Generator().manual_seed(1000 * B + 10 * T + J)
    orig = 0.1 + 0.3 * torch.randn(B, T, J, 3, generator=gen)
    adv = orig + 0.02 * torch.randn(B, T, J, 3, generator=gen)
    got = {k: v.cpu() for k, v in ops.attack_metrics(adv.to(device), orig.to(device), return_counts=True).items()}
    hist = counts(adv, orig)
    for fam in FAMILIES:
        assert int(got["counts_" + fam].sum()) == 2 * B * T * J * J
        assert np.array_equal(got["counts_" + fam].numpy(), hist["counts_" + fam].numpy()), "%s counts_%s" % (shape, fam)
        assert torch.equal(got["max_" + fam], hist["max_" + fam]), "%s max_%s" % (shape, fam)
    ref, r32 = restate(adv.double(), orig.double(), hist), restate(adv, orig)
    for key in KEYS:
        gap = float((r32[key].double() - ref[key]).abs().max()) if key in r32 else 0.0      # histogram entries: the same counts, fp64 formulas
        assert_within(got[key], ref[key].numpy(), gap, "%s %s on %s" % (shape, key, device))


def check_inputs_untouched_and_reproducible(device):
    adv, orig = case_inputs("A", device)
    keep = adv.clone(), orig.clone()
    first = ops.attack_metrics(adv, orig, return_counts=True)
    second = ops.attack_metrics(adv, orig, return_counts=True)
    assert torch.equal(adv, keep[0]) and torch.equal(orig, keep[1]), "attack_metrics wrote to an input"
    assert len(first) == 33 + 6
    for k in first:
        assert torch.equal(first[k], second[k]), "%s differs between two calls" % k
        assert torch.equal(first[k].cpu(), results(device, "A")[k]), k


def check_strided_inputs(device):
    """non-contiguous views are copied, not misread"""
    adv, orig = case_inputs("B", device)
    wide = torch.zeros(adv.shape[:3] + (5,), device=device)
    wide[..., 1:4] = adv
    got = ops.attack_metrics(wide[..., 1:4], orig.transpose(1, 2).contiguous().transpose(1, 2), return_counts=True)
    for k, v in results(device, "B").items():
        assert torch.equal(got[k].cpu(), v), k


def check_interface_errors(device):
    adv, orig = case_inputs("C", device)
    for bad in ((adv[:, :, :1], orig[:, :, :1]),                                          # J = 1
                (torch.zeros(1, 2, 65, 3, device=device), torch.zeros(1, 2, 65, 3, device=device)),
                (adv, orig[:, :, :-1]), (adv[..., :2], orig[..., :2]), (adv[0], orig[0]),
                (adv.double(), orig.double()), (adv, orig.half())):
        with pytest.raises(ValueError):
            ops.attack_metrics(*bad)
    # the C ABI itself: status codes, nothing launched
    import ctypes
    from cistgcn_amd import _lib
    a = _lib.AttackMetricsArgs()
    assert _lib.lib().cg_attack_metrics(ctypes.byref(a), None) == -1
    ws = _lib.lib().cg_attack_metrics_ws_doubles
    assert ws(1, 2, 65) == 0 and ws(1, 2, 1) == 0 and ws(0, 2, 22) == 0
    assert ws(3, 10, 22) == 4 * 660 + 9 * 30 + 11 * 1 * 220 + (660 + 30 + 1) // 2


def check_host_tensors_refused():
    """without the shim there is no CPU path: refused before anything is launched"""
    from cistgcn_amd import _lib
    adv, orig = case_inputs("C")
    was = _lib._host_pointers_ok
    _lib._host_pointers_ok = False
    try:
        with pytest.raises(RuntimeError):
            ops.attack_metrics(adv, orig)
    finally:
        _lib._host_pointers_ok = was


def check_attack_dictionary(device):
    """`_Attack.metrics`: the reference's 35 keys, numpy fp32, the same numbers as the operator; on all four attack classes"""
    fx = fixture()
    adv, orig = case_inputs("A", device)
    ref_keys = sorted(k[2:] for k in fx if k.startswith("A/") and k.count("/") == 1 and k[2:] not in ("adv", "orig", "seed")
                      and not k[2:].startswith(("counts_", "max_")))
    assert len(ref_keys) == 33
    for cls in (attacks.FGSM, attacks.IFGSM, attacks.MIFGSM, attacks.NoAttack):
        res = cls(typ_eval="len_y").metrics(adv, orig)
        assert sorted(res) == sorted(ref_keys + ["metric_type", "queries"]) and len(res) == 35
        assert res["metric_type"] == "len_y" and res["queries"] == 0
        for k in ref_keys:
            assert isinstance(res[k], np.ndarray) and res[k].dtype == np.float32, k
            assert np.array_equal(res[k], results(device, "A")[k].numpy()), k
            assert res[k].shape == fx["A/" + k].shape, k
    q = torch.arange(adv.shape[0], dtype=torch.int32, device=device)
    assert attacks.IFGSM().metrics(adv, orig, q)["queries"] is q


def check_end_to_end(device, graphed=False):
    """IFGSM on the smallest golden model, then the distortion of what it returned"""
    import attack_checks
    net, x, target = attack_checks.model_on(device)
    att = attacks.IFGSM(typ_eval="len_y", epsilon=0.01, iterations=3)
    if graphed:
        from cistgcn_amd import runtime
        out = runtime.GraphedAttack(net, x, target, att).run()
    else:
        out = att.apply(net, x, target)
    res = att.metrics(out["adv_inputs"], x, out["queries"])
    B, T, J, _ = x.shape
    assert len(res) == 35 and res["queries"] is out["queries"]
    assert res["mpjpe_sample"].shape == (B,) and res["temporal_KLD"].shape == (T,) and res["spatial_hausdorff_max"].shape == (J,)
    assert all(np.isfinite(res[k]).all() for k in KEYS)
    assert float(res["mpjpe"]) > 0.0 and float(res["mse_sample"].min()) > 0.0
    # every coordinate moves by at most epsilon * the y extent of an iterate: |adv - orig| <= sqrt(3) * 0.01 * extent, extent <= 2 max |x| + that
    reach = 2.0 * float(x.abs().max()) * 1.1
    assert float(res["hausdorff_max_sample"].max()) <= np.sqrt(3.0) * 0.01 * reach
