#!/usr/bin/env python3
"""Golden vectors of the input attacks from the REAL reference (`environment/adversarial_attacks.py`: FGSM, IFGSM, MIFGSM on the
reference's CISTGCN).  Build container only, like tools/gen_golden.py: the reference is imported at generation time, this script
writes arrays only.

    python tools/gen_golden_attacks.py       # writes tests/golden/eval_attack_h36m_c8_t10_v22.npz

(The `eval_` prefix keeps the file out of the model-fixture list of tests/helpers.py, which takes every other *.npz for a model case.)

Weights, input and target come from the existing `h36m_c8_t10_v22` fixture; they are not stored again.  Per configuration the file
holds the reference's final `adv_inputs` and `queries` and, per iteration k: the iterate `x` (x[k] goes in, x[k+1] = the post-step
x_adv comes out), the fp32 gradient the reference stepped with, `loss_b`, MI-FGSM's momentum after the step and the samples that were
still active after the iteration's bookkeeping.  For the iterates the sign tests use, it also holds the gradient of the SAME weighted
loss by a second reference model in fp64, `noise` = max |g32 - g64| and the share of elements with |g64| <= 30 * noise.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import gen_golden as G          # noqa: E402
from helpers import load_case   # noqa: E402

CASE = "h36m_c8_t10_v22"
OUT = os.path.join(G.OUT_DIR, "eval_attack_%s.npz" % CASE)
Z_FACTOR, ZONE_CAP = 30.0, 0.03
# id -> (class, keywords, iterates that get an fp64 gradient; -1 = the last recorded one)
CONFIGS = {
    "F": ("FGSM", dict(epsilon=0.01), [0]),
    "I1": ("IFGSM", dict(epsilon=0.01, iterations=10), [0, 5, -1]),
    "I2": ("IFGSM", dict(epsilon=0.2, iterations=12, frames=[0, 3, 9], joints=[1, 2, 5, 21]), []),
    "M": ("MIFGSM", dict(epsilon=0.05, iterations=12, mu=0.5), [0, 5, -1]),
    "I3": ("IFGSM", dict(epsilon=1.0, iterations=14), [0, -1]),
}


def build_net(ref_model, rec, dtype):
    """A fresh reference model on the fixture's weights (a fresh config each time: the reference mutates the lists it is given)."""
    C, T, V, _ = [int(v) for v in rec["meta"]]
    net = ref_model.CISTGCN(*G.make_cfg(C, T, V))
    state = {k[len("state/"):]: torch.from_numpy(v.copy()) for k, v in rec.items() if k.startswith("state/")}
    net.load_state_dict(state)
    return net.to(dtype).eval()


def predict(model=None, inputs=None, inputs_vel=None, target=None, **_):
    return model(inputs)[0]


def grad64(net64, ref_losses, x, target, active):
    """d(mean over the active samples of loss_b)/dx by the fp64 model: the loss the reference differentiated at this iterate"""
    xi = torch.from_numpy(x).double().requires_grad_(True)
    loss = ref_losses.mpjpe(net64(xi)[0], target.double(), reduce_axis=[1, 2])
    net64.zero_grad()
    loss[torch.from_numpy(active)].mean().backward()
    return xi.grad.numpy().copy()


def main():
    ref_model, ref_losses = G.import_reference()
    adv = importlib.import_module("human_motion_prediction.environment.adversarial_attacks")
    rec = load_case(CASE)
    torch.manual_seed(0)
    net64 = build_net(ref_model, rec, torch.float64)       # built BEFORE any forward: afterwards the modules hold graph tensors
    x0 = torch.from_numpy(rec["x"].copy())
    target = torch.from_numpy(rec["target"].copy())
    B = x0.shape[0]
    out = {"z_factor": np.float64(Z_FACTOR), "zone_cap": np.float64(ZONE_CAP)}

    for cid, (cls, kw, want64) in CONFIGS.items():
        net = build_net(ref_model, rec, torch.float32)
        attack = getattr(adv, cls)(typ_eval="len_y", db="h36m", **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()})
        trace = {"x": [], "grad": [], "loss": [], "op": [], "g": []}

        inner_grad, inner_init = attack.compute_gradient, attack._init_func

        def init_func(seq, seq_vel=None, model=None, pred_func=None, params=None, reduce_axis=[]):
            outputs, loss_ = inner_init(seq, seq_vel, model, pred_func, params, reduce_axis=reduce_axis)
            trace["loss"].append(loss_.detach().numpy().copy())
            return outputs, loss_

        def compute_gradient(*args):
            if cls == "FGSM":
                seq_i, op_mask = args[0], np.arange(B)
            else:
                seq_i, op_mask = args[1], np.asarray(args[-1])
            trace["x"].append(seq_i.detach().numpy().copy())
            trace["grad"].append(seq_i.grad.numpy().copy())
            trace["op"].append(op_mask.copy())
            res = inner_grad(*args)
            if cls == "MIFGSM":
                trace["g"].append(res[2].detach().numpy().copy())
            trace["x_after"] = (res[1] if cls != "FGSM" else res).detach().numpy().copy()
            return res

        attack.compute_gradient, attack._init_func = compute_gradient, init_func
        seq = x0.clone()
        result = attack.apply(seq, seq_vel=torch.zeros_like(seq), model=net, pred_func=predict, params={"target": target.clone()})
        K = len(trace["x"])
        adv_inputs = np.asarray(result["adv_inputs"], dtype=np.float32)
        assert np.array_equal(adv_inputs, trace["x_after"])
        xs = trace["x"] + [trace["x_after"]]
        # active[k] = the samples still optimised AFTER iteration k: the reference's bookkeeping (:529-538) restated on the recorded losses
        best, stall, active, queries, actives = np.zeros(B), np.zeros(B), np.ones(B, bool), np.zeros(B), []
        for k in range(K):
            started = active.copy()
            assert np.array_equal(np.flatnonzero(started), trace["op"][k]), (cid, k)
            if cls != "FGSM":
                queries[started] += 1
                loss_full = np.zeros(B)
                loss_full[started] = trace["loss"][k]
                improved = started & (loss_full > best)
                best[improved] = loss_full[improved]
                stall[started & ~improved] += 1
                active = started & (stall < 5)
            trace["loss"][k] = (loss_full if cls != "FGSM" else trace["loss"][k]).astype(np.float32)
            actives.append(active.copy())
        if cls != "FGSM":
            assert np.array_equal(queries, np.asarray(attack.queries)), (queries, attack.queries)
        out[cid + "/adv_inputs"] = adv_inputs
        out[cid + "/queries"] = queries.astype(np.int32)
        out[cid + "/x"] = np.stack(xs).astype(np.float32)                        # (K+1,B,T,V,3)
        out[cid + "/grad"] = np.stack(trace["grad"]).astype(np.float32)          # (K,B,T,V,3), zero rows for frozen samples
        out[cid + "/loss"] = np.stack(trace["loss"])                             # (K,B)
        out[cid + "/active"] = np.stack(actives)                                 # (K,B) after the bookkeeping of iteration k
        out[cid + "/started"] = np.stack([np.isin(np.arange(B), op) for op in trace["op"]])      # (K,B) active at the start
        if cls == "MIFGSM":
            out[cid + "/g"] = np.stack(trace["g"]).astype(np.float32)
        ks, g64s, noises, shares = [], [], [], []
        for want in want64:
            # the wanted iterate, or the nearest earlier one whose near-zero zone respects the cap (the share is stored either way)
            for k in range(want % K, -1, -1):
                started = out[cid + "/started"][k]
                g64 = grad64(net64, ref_losses, xs[k], target, started)
                g32 = trace["grad"][k].astype(np.float64)
                noise = float(np.abs(g32 - g64)[started].max())
                share = float((np.abs(g64[started]) <= Z_FACTOR * noise).mean())
                print("  %s k=%d  max|g64| %.3e  median|g64| %.3e  noise %.3e  zone share %.2f %%%s" % (
                    cid, k, np.abs(g64[started]).max(), np.median(np.abs(g64[started])), noise, 100 * share, "" if np.isfinite(noise) and share <= ZONE_CAP else "  (not finite or over the cap: not used)"))
                # (large epsilons drive the reference's fp32 forward to inf / NaN - I3 from its third iteration on; such an iterate
                # has no gradient to compare signs with)
                if np.isfinite(noise) and np.isfinite(g32).all() and share <= ZONE_CAP:
                    break
            else:
                raise AssertionError("%s: no iterate at or before %d keeps the zone under %.0f %%" % (cid, want % K, 100 * ZONE_CAP))
            if k not in ks:
                ks.append(k); g64s.append(g64); noises.append(noise); shares.append(share)
        out[cid + "/k64"] = np.asarray(ks, dtype=np.int32)
        if ks:
            out[cid + "/grad64"] = np.stack(g64s)
            out[cid + "/noise"] = np.asarray(noises)
            out[cid + "/zone_share"] = np.asarray(shares)
        changed = int((adv_inputs != rec["x"]).sum())
        print("%-3s %-6s %2d iterations recorded, queries %s, %d of %d elements changed" % (cid, cls, K, queries.astype(int).tolist(), changed, adv_inputs.size))

    np.savez_compressed(OUT, **out)
    print("%s: %d arrays, %.1f KiB" % (OUT, len(out), os.path.getsize(OUT) / 1024.0))


if __name__ == "__main__":
    main()
