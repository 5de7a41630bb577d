#!/usr/bin/env python3
"""Golden vectors of the evaluation metrics from the REAL reference (`environment/test.py::Metrics`, `losses/losses.py`).  Build
container only, like tools/gen_golden_eval.py: the reference is imported at generation time, this script writes arrays only.

    python tools/gen_golden_metrics.py       # writes tests/golden/eval_metrics.npz

(The `eval_` prefix keeps the file out of the model-fixture list of tests/helpers.py.)

Per case (A: h36m bones, mm scale, one mirrored sample and one frame whose predicted joints all coincide; B: amass bones, metre scale,
target coordinates on the frame centroid, which `pa_mpjpe` replaces by 1e-3; C: cmu bones, one sample, two frames) the file holds the
fp32 inputs, the bones, and for both reduce modes the reference's nine results evaluated in fp64 on those fp32 inputs
(`<case>/<mode>/<metric>`) with `gap` = max |reference in fp32 - reference in fp64| (`<case>/<mode>/<metric>/gap`).  `acc/...` is
`Metrics` over case A and then a second batch of three samples: what `test()` (:315-334) builds from `get_values(False)` and
`get_values(True)`.  The per-joint `*_seq` of the latter are case A's per-joint results followed by the second batch's; only that tail
is stored (`acc/joint/<key>/tail`), after checking that the head is bit-identical to `A/joint/<metric>`.
`mae` is computed by the reference along the way and not recorded.

Two things of the reference's device are stood in for, since it runs on the CPU here: `Tensor.cuda()` returns the tensor itself, and
`torch.linalg.svd` hands a matrix with non-finite entries back as NaN factors, as the device solver does, where the CPU one raises.
That is what lets the frame of case A whose predicted joints coincide (normY = 0, H = NaN) reach the reference's own NaN rule
(losses.py:126-132); the coincident point is a multiple of 0.25, so its centroid is exact in fp32 and fp64 alike.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
torch.Tensor.cuda = lambda self, *a, **k: self          # pa_mpjpe and test() call .cuda(); everything here runs on the CPU
_svd = torch.linalg.svd


def _svd_nan_through(H, *a, **k):
    bad = ~torch.isfinite(H).all(-1).all(-1)
    if not bool(bad.any()):
        return _svd(H, *a, **k)
    U, s, Vt = _svd(torch.where(bad[..., None, None], torch.eye(H.shape[-1], dtype=H.dtype), H), *a, **k)
    U[bad], s[bad], Vt[bad] = float("nan"), float("nan"), float("nan")
    return U, s, Vt


torch.linalg.svd = _svd_nan_through
pkg = types.ModuleType("human_motion_prediction")
pkg.__path__ = ["/root/reference/human_motion_prediction"]
sys.modules["human_motion_prediction"] = pkg
ref_test = importlib.import_module("human_motion_prediction.environment.test")
body_utils = importlib.import_module("human_motion_prediction.utils.body_utils")

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "eval_metrics.npz")
# result key of test() -> (LossOperator of Metrics, attribute get_values() fills)
LISTS = {"mpjpe": ("mpjpe_list", "mpjpe_seq"), "pa_mpjpe": ("pa_mpjpe_list", "pa_mpjpe_seq"), "n_mpjpe": ("n_mpjpe_list", "n_mpjpe_seq"),
         "mve": ("mve_list", "mve_seq"), "w_mpjpe": ("w_mpjpe_list", "w_mpjpe_seq"), "bone_l": ("bone_length_list", "bone_length_seq"),
         "w_bone_l": ("w_bone_length_list", "w_bone_length_seq"), "w_joints": ("w_joints_list", "w_joints_seq"),
         "w_joints_t": ("w_joints_temp_list", "w_joints_temp_seq")}
MODES = {"frames": (0, 2), "joint": None}


def evaluator(To, db, reduce_axis, dtype):
    w = torch.arange(1, To + 1)
    w = (w / w.max()).to(dtype)          # test.py:301-302: fp32; the fp64 run takes the same fp32 weights
    return ref_test.Metrics(w, reduce_axis, db)


def run(batches, db, reduce_axis, dtype):
    To = batches[0][0].shape[1]
    ev = evaluator(To, db, reduce_axis, dtype)
    for pred, target, speeds in batches:
        ev.compute(pred.clone().to(dtype), target.clone().to(dtype), speeds.clone().to(dtype))      # compute() divides speeds in place
    return ev


def poses(gen, B, To, J, centre, spread, noise):
    target = centre + spread * torch.randn(B, To, J, 3, generator=gen)
    pred = target + noise * torch.randn(B, To, J, 3, generator=gen)
    speeds = torch.cumsum(torch.rand(B, To, J, generator=gen) * spread * 0.01, 1)
    return pred, target, speeds


gen = torch.Generator().manual_seed(2024)
cases = {}
# A: h36m
pred, target, speeds = poses(gen, 5, 25, 32, 50.0, 350.0, 20.0)
pred[1, :, :, 0] = 2 * pred[1, :, :, 0].mean(1, keepdim=True) - pred[1, :, :, 0]          # mirrored in x about its own centroid
pred[2, 0] = (pred[2, 0, 0] * 4).round() / 4                                                       # every predicted joint of this frame coincides
cases["A"] = ("h36m", pred, target, speeds)
# B: amass, metre scale, x of joints 1..6 on the frame's centroid
_, target, speeds = poses(gen, 3, 10, 22, 0.0, 0.3, 0.02)
for _ in range(500):
    before = target.clone()
    target[:, :, 1:7, 0] = target[:, :, :, 0].mean(2, keepdim=True)
    if torch.equal(before, target):
        break
pred = target + 0.02 * torch.randn(3, 10, 22, 3, generator=gen)
cases["B"] = ("amass", pred, target, speeds)
# C: cmu, a single mve frame and a batch maximum over one sample
cases["C"] = ("cmu",) + poses(gen, 1, 2, 25, 50.0, 350.0, 20.0)
second = poses(gen, 3, 25, 32, 50.0, 350.0, 20.0)

rec = {}
for name, (db, pred, target, speeds) in cases.items():
    bones, _ = body_utils.get_reduced_skeleton(db)
    rec[name + "/db"] = np.array(db)
    rec[name + "/bones"] = np.asarray(bones, dtype=np.int32).reshape(-1, 2)
    rec[name + "/pred"], rec[name + "/target"], rec[name + "/speeds"] = pred.numpy(), target.numpy(), speeds.numpy()
    for mode, axis in MODES.items():
        e32, e64 = run([(pred, target, speeds)], db, axis, torch.float32), run([(pred, target, speeds)], db, axis, torch.float64)
        for key, (lst, _) in LISTS.items():
            v32, v64 = getattr(e32, lst).loss[0], getattr(e64, lst).loss[0]
            assert v64.dtype == np.float64 and v32.dtype == np.float32 and v32.shape == v64.shape, (key, v32.dtype, v64.dtype)
            rec["%s/%s/%s" % (name, mode, key)] = v64
            rec["%s/%s/%s/gap" % (name, mode, key)] = np.array(np.abs(v32.astype(np.float64) - v64).max())
    x = rec[name + "/target"]
    x0 = x - x.mean(2, keepdims=True)
    print(name, db, "bones", rec[name + "/bones"].shape, "max index", int(rec[name + "/bones"].max()), "centred target coordinates with square < 1e-6:",
          int((x0 ** 2 < 1e-6).sum()))

# accumulation over two batches, as test() reports it
db, pred, target, speeds = cases["A"]
rec["acc/pred"], rec["acc/target"], rec["acc/speeds"] = [t.numpy() for t in second]
for mode, axis in MODES.items():
    evs = {}
    for dtype in (torch.float32, torch.float64):
        ev = run([(pred, target, speeds), second], db, axis, dtype)
        ev.get_values(mode == "joint")
        evs[dtype] = ev
    for key, (lst, seq) in LISTS.items():
        for tag, get in ((key, lambda ev: np.asarray(getattr(ev, lst).mean())), (key + "_seq", lambda ev: np.asarray(getattr(ev, seq)))):
            v32, v64 = get(evs[torch.float32]), get(evs[torch.float64])
            assert v64.dtype == np.float64 and v32.shape == v64.shape
            gap = np.array(np.abs(v32.astype(np.float64) - v64).max())
            if mode == "joint" and tag.endswith("_seq"):
                head = rec["A/joint/" + key]
                assert np.array_equal(v64[:head.shape[0]], head), key
                rec["acc/joint/%s/tail" % tag] = v64[head.shape[0]:]
            else:
                rec["acc/%s/%s" % (mode, tag)] = v64
            rec["acc/%s/%s/gap" % (mode, tag)] = gap

np.savez_compressed(OUT, **rec)
a = rec["A/joint/pa_mpjpe"]
print("wrote", os.path.normpath(OUT), "%.0f KiB" % (os.path.getsize(OUT) / 1024.0))
print("A pa_mpjpe per sample:", a.mean((1, 2)).round(2).tolist())
print("A sample 2 frame 0: pa_mpjpe - |X| max", float(np.abs(a[2, 0] - np.linalg.norm(cases["A"][2][2, 0].double().numpy(), axis=-1)).max()))
for k in sorted(rec):
    if k.endswith("/gap"):
        ref = rec[k[:-4]] if k[:-4] in rec else rec[k[:-4] + "/tail"]
        print("%-32s gap %.2e  max|ref| %.3e  relative %.1e" % (k[:-4], float(rec[k]), float(np.abs(ref).max()), float(rec[k]) / float(np.abs(ref).max())))
