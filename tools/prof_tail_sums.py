#!/usr/bin/env python3
"""GPU box: the phase kernels of the DSTD_GC tail (csrc/dstd_tail.hip) at one block shape on three routes in one process - a pass per
BatchNorm sum (`old`), the sums a phase early with separate residuals (`new`), with the shared residual of a 64 -> 64 block (`shared`) -
the program rocprofv3 --kernel-trace is pointed at; then `--summarize DIR` turns the trace into launches and warm min / median / max per
kernel and route.  Usage: prof_tail_sums.py [B C T V reps]  |  prof_tail_sums.py --summarize DIR [reps]"""
import csv
import glob
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ("old", "new", "shared")


def summarize(d, reps):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    tail = [r for r in rows if "cg_tail_" in r["Kernel_Name"] or "cg_se_gate" in r["Kernel_Name"]]
    # the routes run one after the other, `reps` forward + backward calls each; a call ends with K5 (old) or the parameter epilogue
    ends = [k for k, r in enumerate(tail) if "cg_tail_k5_kernel" in r["Kernel_Name"] or "cg_tail_params_kernel" in r["Kernel_Name"]]
    assert len(ends) == reps * len(ROUTES), (len(ends), reps)
    start = 0
    per = {}
    for n, e in enumerate(ends):
        route, rep = ROUTES[n // reps], n % reps
        for r in tail[start:e + 1]:
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            per.setdefault((route, name), []).append((rep, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        start = e + 1
    for route in ROUTES:
        total = 0.0
        print("# route %s" % route)
        for (rt, name), v in per.items():
            if rt != route:
                continue
            warm = sorted(t for rep, t in v if rep >= 2)
            n_call = len(v) // reps
            med = warm[len(warm) // 2]
            total += med * n_call
            print("%-44s launches %3d  warm min %6.1f  median %6.1f  max %6.1f us" % (name, len(v), warm[0], med, warm[-1]))
        print("# route %s: sum of the warm medians of one forward + backward call %.1f us" % (route, total))


def main():
    import torch
    import torch.nn as nn
    from cistgcn_amd import ops
    from cistgcn_amd.models.layers.SE import SELayer2d
    B, C, T, V, reps = [int(a) for a in sys.argv[1:6]] if len(sys.argv) > 5 else (256, 64, 50, 22, 6)
    dev = "cuda"
    bns = nn.ModuleList([nn.BatchNorm2d(C) for _ in range(5)]).to(dev).train()
    al = nn.ModuleList([nn.PReLU() for _ in range(5)]).to(dev)
    conv = nn.Conv2d(2 * C, C, 1, bias=False).to(dev)
    se = SELayer2d(C, reduction=8).to(dev)
    R = lambda *s: torch.randn(*s, device=dev)
    for route in ROUTES:
        for _ in range(reps):
            y1, y2, r1, r2, bres = [R(B, C, T, V).requires_grad_(True) for _ in range(5)]
            w1, w2 = [R(B, C).requires_grad_(True) for _ in range(2)]
            ops.begin_step(torch.device(dev), bump_seed=True)

            def sums(y):
                st = ops._arena(torch.device(dev, 0)).take(2 * C * 16)
                yc = y.detach().double()
                st.view(16, C, 2)[0].copy_(torch.stack((yc.sum((0, 2, 3)), (yc * yc).sum((0, 2, 3))), 1))
                return st
            out, _ = ops.dstd_tail([y1, y2], [sums(y1), sums(y2)], [r1, r1] if route == "shared" else [r1, r2], (w1, w2), list(bns), list(al),
                                   conv.weight, se, bres, True, drop_p=0.1, salts=(3, 4), emit_stats=True, tail_sums=route != "old",
                                   rs_shared=route == "shared")
            out.backward(torch.randn_like(out))
            torch.cuda.synchronize()
    print("done")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 6)
    else:
        main()
