#!/usr/bin/env python3
"""GPU box: wall time of one DeepFool iteration (eval-mode forward, per-sample loss, backward to the input, step + bookkeeping), host
included, three ways on the same seeded model and batch:

    eager     `DEEPFOOL.iterate`: the model's launches from Python, `ops.deepfool_step` as one launch
    graph     `runtime.GraphedAttack.step()`: the same iteration replayed as a HIP graph
    stock     the same forward / loss / backward, the step and the bookkeeping written in stock torch operators on the device
              (no host synchronisation either)

A window is ITERS iterations ending in a device synchronise; the sides alternate over ROUNDS rounds after warm-up and the median
window is reported with its spread.  The step is a few microseconds of traffic beside the model's forward and backward: what the
kernel buys is one launch and an iteration that can be captured, not bandwidth.  There is no pass threshold.

    python tools/bench_deepfool.py [C B T V] [--out FILE]        # default 64 256 50 22, 25 predicted frames
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                                        # noqa: E402

from cistgcn_amd import ops, runtime                                # noqa: E402
from cistgcn_amd.environment import attacks                         # noqa: E402
from cistgcn_amd.models import CISTGCN_0                            # noqa: E402
from helpers import make_cfg                                        # noqa: E402

WARMUP, ITERS, ROUNDS, PATIENCE = 3, 10, 5, 5


def stock_step(x, grad, pred, loss, st):
    """`ops.deepfool_step` in stock torch operators, in place on x and the state tensors"""
    act = st["active"]
    n1 = grad.abs().sum((1, 2, 3), keepdim=True) + 1e-10
    r = -(grad * pred.mean(1, keepdim=True)) / n1
    x.add_(r * act[:, None, None, None])
    improved = (loss > st["best"]) & (act > 0)
    st["queries"] += act.int()
    st["best"].copy_(torch.where(improved, loss, st["best"]))
    st["stall"] += ((act > 0) & ~improved).int()
    act.copy_(((act > 0) & (st["stall"] < PATIENCE)).float())
    st["w"].copy_(act / x.shape[0])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path in args:
        args.remove(out_path)
    C, B, T, V = [int(v) for v in args] if args else (64, 256, 50, 22)
    if not torch.cuda.is_available():
        raise SystemExit("bench_deepfool: no GPU; a time measured anywhere else says nothing")
    torch.manual_seed(0)
    net = CISTGCN_0(*make_cfg(C, T, V)).cuda().eval()
    gen = torch.Generator().manual_seed(1234)
    x0 = (50 + 350 * torch.randn(B, T, V, 3, generator=gen)).cuda()
    target = (x0[:, -1:].cpu() + 20 * torch.randn(B, 25, V, 3, generator=gen)).cuda()
    att = attacks.DEEPFOOL(iterations=ITERS)

    state = ops.AttackState(B, x0.device)
    x_e = x0.clone().requires_grad_(True)
    ga = runtime.GraphedAttack(net, x0, target, att)
    x_s = x0.clone().requires_grad_(True)
    st = {}

    def arm_eager():
        state.reset()
        x_e.detach().copy_(x0)

    def arm_stock():
        st.update(active=torch.ones(B, device="cuda"), best=torch.zeros(B, device="cuda"), w=torch.full((B,), 1.0 / B, device="cuda"),
                  stall=torch.zeros(B, dtype=torch.int32, device="cuda"), queries=torch.zeros(B, dtype=torch.int32, device="cuda"))
        x_s.detach().copy_(x0)

    def one_stock():
        loss, grad, pred = attacks.loss_and_input_grad(net, x_s, target, st["w"], with_pred=True)
        with torch.no_grad():
            stock_step(x_s.detach(), grad, pred, loss, st)

    sides = {"eager": (arm_eager, lambda: att.iterate(net, x_e, x0, target, state, None, None)),
             "graph": (ga.reset, ga.step),
             "stock": (arm_stock, one_stock)}

    def window(arm, one):
        arm()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            one()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / ITERS * 1e3          # milliseconds per iteration

    # same results first: the three sides land on the same poses after ITERS iterations, up to the roundings of the step
    for arm, one in sides.values():
        for _ in range(WARMUP):
            window(arm, one)
    finals = {"eager": x_e.detach().clone(), "graph": ga.x_i.detach().clone(), "stock": x_s.detach().clone()}
    apart = {k: float((v - finals["eager"]).abs().max()) for k, v in finals.items() if k != "eager"}
    times = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, (arm, one) in sides.items():
            times[k].append(window(arm, one))
    res = {"model": "CISTGCN-%d" % C, "shape": [B, T, 25, V], "iterations_per_window": ITERS, "windows": ROUNDS,
           "max_abs_distance_to_eager_after_%d_iterations" % ITERS: apart, "largest_move": float((finals["eager"] - x0).abs().max())}
    for k, v in times.items():
        v.sort()
        res[k + "_ms_per_iteration"] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
