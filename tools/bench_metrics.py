#!/usr/bin/env python3
"""GPU box: time of one `ops.eval_metrics` call (frames mode: the nine per-frame metrics of a batch) against the same metrics from
stock PyTorch operators in fp32 on the same device (`restate` of tests/metrics_checks.py: about 80 small launches, a batched `eigh`
and a batched determinant in place of the reference's SVD and its host round trip).  Device events around windows of CALLS calls,
after warm-up, the two sides alternating over ROUNDS rounds; the median window is reported, with the spread.  There is no pass
threshold; the figures go into DESIGN.md §12.

    python tools/bench_metrics.py [B To J] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                      # noqa: E402

from cistgcn_amd import ops      # noqa: E402
import metrics_checks as M       # noqa: E402

WARMUP, CALLS, ROUNDS = 10, 500, 7


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3          # microseconds per call


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path in args:
        args.remove(out_path)
    B, To, J = [int(v) for v in args] if args else (256, 25, 32)
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: no GPU; a time measured anywhere else says nothing")
    gen = torch.Generator().manual_seed(0)
    target = 50 + 350 * torch.randn(B, To, J, 3, generator=gen)
    pred = target + 20 * torch.randn(B, To, J, 3, generator=gen)
    speeds = torch.cumsum(torch.rand(B, To, J, generator=gen) * 3.5, 1)
    bones = [(i, i + 1) for i in range(J - 1)]
    pred, target, speeds = pred.cuda(), target.cuda(), speeds.cuda()
    sides = {"eval_metrics": lambda: ops.eval_metrics(pred, target, speeds, bones, reduce="frames"),
             "stock_pytorch_fp32": lambda: M.restate(pred, target, speeds, bones, "frames")}
    # same results first: faster and different is not faster
    got, ref = sides["eval_metrics"](), M.restate(pred.double(), target.double(), speeds.double(), bones, "frames")
    worst = max(float((got[k].double() - ref[k]).abs().max() / ref[k].abs().max()) for k in M.METRICS)
    for fn in sides.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            times[k].append(window(fn))
    res = {"shape": [B, To, J], "bones": len(bones), "calls_per_window": CALLS, "windows": ROUNDS, "max_rel_err_vs_fp64": worst}
    for k, v in times.items():
        v.sort()
        res[k + "_us"] = {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}
    res["ratio"] = round(res["stock_pytorch_fp32_us"]["median"] / res["eval_metrics_us"]["median"], 1)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
