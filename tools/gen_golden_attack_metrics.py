#!/usr/bin/env python3
"""Golden vectors of the attack distortion metrics from the REAL reference
(`environment/adversarial_attacks.py::ComputeAttackMetrics._get_metrics`, called as at `environment/test.py:205`).  Build container
only, like tools/gen_golden_metrics.py: the reference is imported at generation time, this script writes arrays only.

    python tools/gen_golden_attack_metrics.py       # writes tests/golden/eval_attack_metrics.npz

(The `eval_` prefix keeps the file out of the model-fixture list of tests/helpers.py.)

Per case the file holds the fp32 inputs `<case>/adv` and `<case>/orig`, for each of the 33 numeric entries of the reference's
dictionary its value evaluated in fp64 on those fp32 inputs (`<case>/<entry>`) with `gap` = max |reference in fp32 - reference in
fp64| (`<case>/<entry>/gap`), and what the fp32 run binned: the integer histogram counts `<case>/counts_{sample,temporal,spatial}`
(2,G,64) (index 0 adv, 1 orig; taken from `torch.histogram` on the very distances and edges the reference hands it) and the last
edge of every group `<case>/max_{sample,temporal,spatial}`.

  A  (5,10,22), mm scale: orig = 50 + 350 randn, adv = orig + 0.01 len_y sign(randn) (an FGSM-sized step, len_y the y extent of the
     sample).  Sample 1 has adv == orig exactly (the epsilon-0 run of massive_test_adversarial_attacks.py), sample 2 is moved only at
     joint 3 in frames 0-4 (a joint / frame selection).
  B  (3,10,18), metre scale.
  C  (1,2,25): one sample, two frames.

A histogram count depends on the last bit of a distance, so a case is only recorded when its counts are robust.  The seed of a case
is re-drawn until, with the distances and the edges in fp64, the counts do not change when every distance is scaled by 1 - 4 eps32 or
by 1 + 4 eps32 (the group's maximum stays in the last bin); then the reference's fp32 run and its fp64 run must both have produced
exactly those counts.  Any evaluation whose distances are within 4 eps32 of the exact ones bins alike.  Case A must in addition
tell adv from orig in `hausdorff_mean_sample` (`roles_visible`), which the tests check by swapping the arguments.

As in gen_golden_metrics.py, `Tensor.cuda()` returns the tensor itself and `torch.linalg.svd` hands NaN factors back for a
non-finite matrix.  A third stand-in for the reference's device: `torch.sqrt` of an fp32 tensor is taken in fp64 and rounded, which is
the correctly rounded fp32 root that the device's `sqrtf` gives.  The vectorised CPU root of PyTorch is only faithful (0.5001 ulp): it
misrounds about 0.7 % of the distances of case A by one ulp, and although no count of these cases depends on that, a recorded range
(the largest distance of a group) would.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
torch.Tensor.cuda = lambda self, *a, **k: self
_svd = torch.linalg.svd


def _svd_nan_through(H, *a, **k):
    bad = ~torch.isfinite(H).all(-1).all(-1)
    if not bool(bad.any()):
        return _svd(H, *a, **k)
    U, s, Vt = _svd(torch.where(bad[..., None, None], torch.eye(H.shape[-1], dtype=H.dtype), H), *a, **k)
    U[bad], s[bad], Vt[bad] = float("nan"), float("nan"), float("nan")
    return U, s, Vt


torch.linalg.svd = _svd_nan_through
_sqrt = torch.sqrt


def _sqrt_correctly_rounded(x, *a, **k):
    return _sqrt(x.double(), *a, **k).float() if x.dtype == torch.float32 else _sqrt(x, *a, **k)


torch.sqrt = _sqrt_correctly_rounded
_histogram = torch.histogram
_binned = []      # (counts, last edge) of every torch.histogram call of the reference, in call order


def _histogram_recorded(x, bins, density=False):
    _binned.append((_histogram(x, bins=bins, density=False).hist.numpy().astype(np.int64), bins[-1].item()))
    return _histogram(x, bins=bins, density=density)


torch.histogram = _histogram_recorded
pkg = types.ModuleType("human_motion_prediction")
pkg.__path__ = ["/root/reference/human_motion_prediction"]
sys.modules["human_motion_prediction"] = pkg
ref_attacks = importlib.import_module("human_motion_prediction.environment.adversarial_attacks")

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "eval_attack_metrics.npz")
EPS32 = float(np.finfo(np.float32).eps)
BINS = 64
FAMILIES = ("sample", "temporal", "spatial")      # the order in which CustomKLD is called (:220-222): dim 0, 1, 2


def reference(adv, orig, dtype):
    """the reference's dictionary and what it binned: {family: (counts (2,G,64), last edges (G,))}"""
    del _binned[:]
    res = ref_attacks.ComputeAttackMetrics("len_y")._get_metrics(adv.clone().to(dtype), orig.clone().to(dtype))
    B, T, J, _ = adv.shape
    hist, at = {}, 0
    for fam, G in zip(FAMILIES, (B, T, J)):      # KLD64 comes first: G calls for `in_seq`, then G for `adv_seq`, per family
        calls = _binned[at:at + 2 * G]
        at += 2 * G
        assert all(calls[g][1] == calls[G + g][1] for g in range(G))
        hist[fam] = (np.stack([np.stack([c for c, _ in calls[:G]]), np.stack([c for c, _ in calls[G:]])]), np.array([m for _, m in calls[:G]]))
    assert len(_binned) == 3 * at, (len(_binned), at)      # JSD64 and KSTest bin the same again
    return res, hist


def robust_counts(adv, orig):
    """{family: counts (2,G,64)} if scaling the distances by 1 -+ 4 eps32 against fixed edges changes no count, else None"""
    ds = []
    for x in (adv, orig):
        x = x.double().numpy()
        ds.append(np.sqrt(((x[..., :, None, :] - x[..., None, :, :]) ** 2).sum(-1)))
    out = {}
    for axis, fam in enumerate(FAMILIES):
        rows = [np.moveaxis(d, axis, 0).reshape(d.shape[axis], -1) for d in ds]
        G = rows[0].shape[0]
        cnt = np.zeros((2, G, BINS), dtype=np.int64)
        for g in range(G):
            mx = max(rows[0][g].max(), rows[1][g].max())
            edges = np.arange(BINS + 1) / BINS * mx
            for s in range(2):
                variants = []
                for scale in (1.0, 1.0 - 4 * EPS32, 1.0 + 4 * EPS32):
                    v = np.minimum(rows[s][g] * scale, mx)
                    variants.append(np.bincount(np.minimum(np.searchsorted(edges, v, side="right") - 1, BINS - 1), minlength=BINS))
                if not (np.array_equal(variants[0], variants[1]) and np.array_equal(variants[0], variants[2])):
                    return None
                cnt[s, g] = variants[0]
        out[fam] = cnt
    return out


def hausdorff_mean_sample(a, b):
    a, b = a.double().numpy(), b.double().numpy()
    return np.sqrt(((a[:, :, :, None, :] - b[:, :, None, :, :]) ** 2).sum(-1)).min(-1).mean((1, 2))


def roles_visible(adv, orig):
    """case A must tell the two arguments apart in the Hausdorff distance too: somewhere a moved joint has to be nearer to another
    joint of the clean pose than to its own, else min_j' |adv_j - orig_j'| is the symmetric |adv_j - orig_j|"""
    fwd, bwd = hausdorff_mean_sample(adv, orig), hausdorff_mean_sample(orig, adv)
    return float(np.abs(fwd - bwd).max()) > 1e-4 * float(fwd.max())


def draw(seed, shape, centre, spread):
    gen = torch.Generator().manual_seed(seed)
    orig = centre + spread * torch.randn(*shape, 3, generator=gen)
    len_y = (orig[..., 1].amax((1, 2)) - orig[..., 1].amin((1, 2))).abs()
    step = 0.01 * len_y[:, None, None, None] * torch.sign(torch.randn(*shape, 3, generator=gen))
    adv = orig + step
    if shape[0] >= 3:
        adv[1] = orig[1]
        adv[2] = orig[2]
        adv[2, 0:5, 3] = orig[2, 0:5, 3] + step[2, 0:5, 3]
    return adv, orig


CASES = {"A": ((5, 10, 22), 50.0, 350.0, 7), "B": ((3, 10, 18), 0.0, 0.3, 1), "C": ((1, 2, 25), 50.0, 350.0, 1)}      # ..., first seed tried

rec = {}
for name, (shape, centre, spread, seed) in CASES.items():
    while True:
        adv, orig = draw(seed, shape, centre, spread)
        want = robust_counts(adv, orig)
        if want is not None and (name != "A" or roles_visible(adv, orig)):
            break
        seed += 1
    r32, h32 = reference(adv, orig, torch.float32)
    r64, h64 = reference(adv, orig, torch.float64)
    for fam in FAMILIES:
        assert np.array_equal(h32[fam][0], want[fam]) and np.array_equal(h64[fam][0], want[fam]), (name, fam)
        assert int(h32[fam][0].sum()) == 2 * int(np.prod(shape)) * shape[2]
        rec["%s/counts_%s" % (name, fam)] = h32[fam][0].astype(np.int32)
        rec["%s/max_%s" % (name, fam)] = h32[fam][1].astype(np.float32)
        assert np.array_equal(rec["%s/max_%s" % (name, fam)].astype(np.float64), h32[fam][1])
    rec[name + "/adv"], rec[name + "/orig"], rec[name + "/seed"] = adv.numpy(), orig.numpy(), np.array(seed)
    keys = sorted(k for k in r64 if k not in ("metric_type", "queries"))
    assert len(keys) == 33
    print("case %s %s seed %d" % (name, shape, seed))
    for k in keys:
        v32, v64 = np.asarray(r32[k]), np.asarray(r64[k])
        assert v64.dtype == np.float64 and v32.dtype == np.float32 and v32.shape == v64.shape, (k, v32.dtype, v64.dtype)
        assert np.isfinite(v64).all(), k
        rec["%s/%s" % (name, k)] = v64
        gap = float(np.abs(v32.astype(np.float64) - v64).max())
        rec["%s/%s/gap" % (name, k)] = np.array(gap)
        print("  %-26s gap %.2e  max|ref| %.3e  relative %.1e" % (k, gap, float(np.abs(v64).max()), gap / max(float(np.abs(v64).max()), 1e-300)))

for k in ("KLD_sample", "hausdorff_mean_sample"):      # what the swapped-arguments test relies on
    swapped = np.asarray(ref_attacks.ComputeAttackMetrics("len_y")._get_metrics(torch.from_numpy(rec["A/orig"]).double(), torch.from_numpy(rec["A/adv"]).double())[k])
    off, bound = float(np.abs(swapped - rec["A/" + k]).max()), 4 * max(float(rec["A/%s/gap" % k]), EPS32 * float(np.abs(rec["A/" + k]).max()))
    print("A/%s with the arguments swapped: off by %.3e, bound %.3e" % (k, off, bound))
    assert off > 16 * bound
np.savez_compressed(OUT, **rec)
print("wrote", os.path.normpath(OUT), "%.0f KiB" % (os.path.getsize(OUT) / 1024.0))
