#!/usr/bin/env python3
"""Golden vectors of the DeepFool input attack from the REAL reference (`environment/adversarial_attacks.py::DEEPFOOL`, :668-776, on
the reference's CISTGCN).  Build container only, like tools/gen_golden_attacks.py: the reference is imported at generation time, this
script writes arrays only.

    python tools/gen_golden_deepfool.py       # writes tests/golden/eval_deepfool_h36m_c8_t10_v22.npz

Weights, input and target come from the existing `h36m_c8_t10_v22` fixture; they are not stored again.  Every configuration is run
twice: by the fp32 reference model (the recording) and, from the same clean input, by the reference model in fp64.  Per configuration
the file holds

    loss (K,B)         loss_b of iteration k (0 for a sample that was frozen by then)
    started, active    (K,B) samples optimised in iteration k / still optimised after its bookkeeping
    queries (B,)       the reference's own count
    adv_inputs         the final fp32 poses
    drift (B,)         max |adv32 - adv64| over the elements of a sample, the two full runs compared
    loss_noise         max |loss32 - loss64| over every iteration and sample of the two full runs

and at the iterates k64 = {0, K // 2, K - 1}

    x, x_next          the fp32 iterate that went into the step and the one that came out
    grad, pred         what the reference stepped with, fp32 (`seq_i.grad` and `k_i`; at k = 0 the gradient is TWICE that of the loss:
                       the call of `_init_func` in front of the loop (:739) has already been accumulated into the same leaf.  The step
                       divides by the L1 norm of what it is given, so this leaves it alone)
    r64                the same step by the fp64 model at the fp32 iterate `x`, with the recorded set of started samples
    noise (B,)         max |r32 - r64|, r32 the reference's own fp32 `r_i`

The generator asserts the `queries` the configurations were chosen for and that every improved / not improved decision of the fp32 run
has a loss gap of at least `z_factor` * loss_noise, which is what makes exact agreement of the bookkeeping a fair demand.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import gen_golden as G                                  # noqa: E402
from gen_golden_attacks import build_net, predict       # noqa: E402
from helpers import load_case                           # noqa: E402

CASE = "h36m_c8_t10_v22"
OUT = os.path.join(G.OUT_DIR, "eval_deepfool_%s.npz" % CASE)
Z_FACTOR = 30.0           # the factor of the attack fixture (tools/gen_golden_attacks.py)
MAX_BYTES = 900 * 1024
# id -> (keywords, the reference's queries)
CONFIGS = {
    "D1": (dict(iterations=10), [10, 10, 10, 10]),
    "D2": (dict(iterations=16, frames=[9], joints=[0]), [6, 16, 16, 16]),
    "D3": (dict(iterations=14, frames=[0, 3, 9], joints=[1, 2, 5, 21]), [14, 14, 14, 14]),
}


def run(adv, net, kw, x0, target):
    """The reference's DEEPFOOL.apply on `net`, in the dtype of `x0`; what went through `compute_gradient` and `_init_func`."""
    B = x0.shape[0]
    attack = adv.DEEPFOOL(typ_eval="len_y", db="h36m", **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()})
    trace = {"x": [], "grad": [], "pred": [], "r": [], "loss": [], "op": [], "x_next": []}
    inner_grad, inner_init = attack.compute_gradient, attack._init_func

    def init_func(seq, seq_vel=None, model=None, pred_func=None, params=None, reduce_axis=[]):
        outputs, loss_ = inner_init(seq, seq_vel, model, pred_func, params, reduce_axis=reduce_axis)
        trace["loss"].append(loss_.detach().numpy().copy())
        return outputs, loss_

    def compute_gradient(seq, seq_i, seq_adv, g_t, op_mask, pred):
        g, p = seq_i.grad.detach().clone(), pred.detach().clone()
        trace["x"].append(seq_i.detach().numpy().copy())
        trace["grad"].append(g.numpy().copy())
        trace["pred"].append(p.numpy().copy())
        trace["op"].append(np.asarray(op_mask).copy())
        # r_i before the selection mask, by the reference's own expression (:698-699) in the reference's dtype
        trace["r"].append((-(g[:, None, :] * p[:, :, None, :]).mean(1) / (torch.norm(g, p=1, dim=[1, 2, 3], keepdim=True) + 1e-10)).numpy())
        res = inner_grad(seq, seq_i, seq_adv, g_t, op_mask, pred)
        trace["x_next"].append(res[1].detach().numpy().copy())
        return res

    attack.compute_gradient, attack._init_func = compute_gradient, init_func
    seq = x0.clone()
    result = attack.apply(seq, seq_vel=torch.zeros_like(seq), model=net, pred_func=predict, params={"target": target.clone()})
    trace["loss"] = trace["loss"][1:]             # the call in front of the loop (:739) is no iteration
    K = len(trace["x"])
    assert len(trace["loss"]) == K
    adv_inputs = np.asarray(result["adv_inputs"])
    assert np.array_equal(adv_inputs, trace["x_next"][-1])
    # the reference's bookkeeping (:755-767) restated on the recorded losses
    best, stall, active = np.zeros(B), np.zeros(B), np.ones(B, bool)
    queries, losses, starteds, actives, gaps = np.zeros(B), [], [], [], []
    for k in range(K):
        started = active.copy()
        assert np.array_equal(np.flatnonzero(started), trace["op"][k]), k
        queries[started] += 1
        loss_full = np.zeros(B)
        loss_full[started] = trace["loss"][k]
        gaps.append(np.where(started, np.abs(loss_full - best), np.inf))
        improved = started & (loss_full > best)
        best[improved] = loss_full[improved]
        stall[started & ~improved] += 1
        active = started & (stall < 5)
        losses.append(loss_full); starteds.append(started); actives.append(active.copy())
    assert np.array_equal(queries, np.asarray(attack.queries)), (queries, attack.queries)
    trace.update(K=K, adv_inputs=adv_inputs, queries=queries.astype(np.int32), loss=np.stack(losses), started=np.stack(starteds),
                 active=np.stack(actives), gap=np.stack(gaps), stall=stall)
    return trace


def fmt(v):
    return "[" + " ".join("%.2e" % t for t in v) + "]"


def selection(T, V, kw):
    """the reference's mask (:701-711) for the recorded configurations: both keywords or neither"""
    m = np.ones((T, V))
    if "joints" in kw:
        keep = np.zeros(V); keep[kw["joints"]] = 1
        m *= keep[None, :]
    if "frames" in kw:
        keep = np.zeros(T); keep[kw["frames"]] = 1
        m *= keep[:, None]
    return m


def step64(net64, ref_losses, x, target, started, mask):
    """r_i of the fp64 model at the iterate `x`: the loss is the mean over the started samples, as the reference differentiates it"""
    xi = torch.from_numpy(x).double().requires_grad_(True)
    pred = net64(xi)[0]
    loss = ref_losses.mpjpe(pred, target.double(), reduce_axis=[1, 2])
    net64.zero_grad()
    loss[torch.from_numpy(started)].mean().backward()
    g, p = xi.grad, pred.detach()
    r = -(g[:, None, :] * p[:, :, None, :]).mean(1) / (torch.norm(g, p=1, dim=[1, 2, 3], keepdim=True) + 1e-10)
    r = r.numpy() * mask[None, :, :, None]
    r[~started] = 0.0
    return r


def main():
    ref_model, ref_losses = G.import_reference()
    adv = importlib.import_module("human_motion_prediction.environment.adversarial_attacks")
    rec = load_case(CASE)
    torch.manual_seed(0)
    x0 = torch.from_numpy(rec["x"].copy())
    target = torch.from_numpy(rec["target"].copy())
    T, V = x0.shape[1:3]
    out = {"z_factor": np.float64(Z_FACTOR)}

    for cid, (kw, want_queries) in CONFIGS.items():
        t32 = run(adv, build_net(ref_model, rec, torch.float32), kw, x0, target)
        t64 = run(adv, build_net(ref_model, rec, torch.float64), kw, x0.double(), target.double())
        K = t32["K"]
        assert t32["adv_inputs"].dtype == np.float32 and t64["adv_inputs"].dtype == np.float64
        print("%s %s: %d iterations, queries fp32 %s fp64 %s, stall counters %s" % (
            cid, kw, K, t32["queries"].tolist(), t64["queries"].tolist(), t32["stall"].astype(int).tolist()))
        assert t32["queries"].tolist() == want_queries and t64["queries"].tolist() == want_queries, cid
        assert np.array_equal(t32["started"], t64["started"]), cid
        loss_noise = float(np.abs(t32["loss"] - t64["loss"]).max())
        gap = float(t32["gap"].min())
        print("   max |loss32 - loss64| %.3e, smallest gap of a decision %.3e (%.0f times)" % (loss_noise, gap, gap / loss_noise))
        assert gap >= Z_FACTOR * loss_noise, "%s: a decision of the fp32 run is within %g times the loss noise" % (cid, Z_FACTOR)
        drift = np.abs(t32["adv_inputs"].astype(np.float64) - t64["adv_inputs"]).reshape(x0.shape[0], -1).max(1)
        moved = np.abs(t32["adv_inputs"] - rec["x"]).reshape(x0.shape[0], -1).max(1)
        print("   drift %s, moved by up to %s" % (fmt(drift), fmt(moved)))
        out[cid + "/loss"] = t32["loss"].astype(np.float32)
        out[cid + "/started"], out[cid + "/active"], out[cid + "/queries"] = t32["started"], t32["active"], t32["queries"]
        out[cid + "/adv_inputs"] = t32["adv_inputs"]
        out[cid + "/drift"], out[cid + "/loss_noise"] = drift, np.float64(loss_noise)

        ks = sorted({0, K // 2, K - 1})
        mask = selection(T, V, kw)
        net64 = build_net(ref_model, rec, torch.float64)
        r64s, noises = [], []
        for k in ks:
            started = t32["started"][k]
            r64 = step64(net64, ref_losses, t32["x"][k], target, started, mask)
            r32 = t32["r"][k].astype(np.float64) * mask[None, :, :, None]
            r32[~started] = 0.0
            # what the reference added is its r_i: the recorded iterates differ by it up to the rounding of the sum
            assert np.abs((t32["x_next"][k] - t32["x"][k]) - r32).max() <= 2.0 ** -22 * np.abs(t32["x_next"][k]).max()
            noise = np.abs(r32 - r64).reshape(x0.shape[0], -1).max(1)
            print("   k=%d  max |r64| %s  noise %s" % (k, fmt(np.abs(r64).reshape(x0.shape[0], -1).max(1)), fmt(noise)))
            r64s.append(r64); noises.append(noise)
        out[cid + "/k64"] = np.asarray(ks, dtype=np.int32)
        out[cid + "/x"] = np.stack([t32["x"][k] for k in ks]).astype(np.float32)
        out[cid + "/x_next"] = np.stack([t32["x_next"][k] for k in ks]).astype(np.float32)
        out[cid + "/grad"] = np.stack([t32["grad"][k] for k in ks]).astype(np.float32)
        out[cid + "/pred"] = np.stack([t32["pred"][k] for k in ks]).astype(np.float32)
        out[cid + "/r64"] = np.stack(r64s)
        out[cid + "/noise"] = np.stack(noises)

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("%s: %d arrays, %.1f KiB" % (OUT, len(out), size / 1024.0))
    assert size <= MAX_BYTES, "the fixture is over the %d KiB a golden part may have" % (MAX_BYTES // 1024)
    for cid in CONFIGS:
        print("%s queries %s" % (cid, out[cid + "/queries"].tolist()))


if __name__ == "__main__":
    main()
