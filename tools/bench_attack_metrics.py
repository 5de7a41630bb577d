#!/usr/bin/env python3
"""GPU box: time of one `ops.attack_metrics` call (the 33 distortion entries of an attacked batch) against the same entries from stock
PyTorch operators in fp32 on the same device (`counts` + `restate` of tests/attack_metrics_checks.py: the (T,J,B,B,3) tensor of the
"spatial" Hausdorff distance, a batched SVD, `searchsorted` in place of the reference's per-row `torch.histogram` on the host).  Device
events around windows of CALLS calls, after warm-up, the two sides alternating over ROUNDS rounds; the median window is reported, with
the spread.  There is no pass threshold; the figures go into DESIGN.md §13.

    python tools/bench_attack_metrics.py [B T J] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                             # noqa: E402

from cistgcn_amd import ops             # noqa: E402
import attack_metrics_checks as AM      # noqa: E402

WARMUP, CALLS, ROUNDS = 3, 20, 7


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
    B, T, J = [int(v) for v in args] if args else (256, 50, 22)
    if not torch.cuda.is_available():
        raise SystemExit("bench_attack_metrics: no GPU; a time measured anywhere else says nothing")
    gen = torch.Generator().manual_seed(0)
    orig = 50 + 350 * torch.randn(B, T, J, 3, generator=gen)
    adv = orig + 20 * torch.sign(torch.randn(B, T, J, 3, generator=gen))
    adv, orig = adv.cuda(), orig.cuda()
    sides = {"attack_metrics": lambda: ops.attack_metrics(adv, orig),
             "stock_pytorch_fp32": lambda: AM.restate(adv, orig, AM.counts(adv, orig))}
    # same results first: faster and different is not faster (the smooth entries; the counts are compared in the test suite)
    got = sides["attack_metrics"]()
    ref = AM.restate(adv.double(), orig.double())
    worst = max(float((got[k].double() - ref[k]).abs().max() / ref[k].abs().max()) for k in ref)
    for fn in sides.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            times[k].append(window(fn))
    res = {"shape": [B, T, J], "calls_per_window": CALLS, "windows": ROUNDS, "max_rel_err_vs_fp64": worst}
    for k, v in times.items():
        v.sort()
        res[k + "_us"] = {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}
    res["ratio"] = round(res["stock_pytorch_fp32_us"]["median"] / res["attack_metrics_us"]["median"], 1)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
