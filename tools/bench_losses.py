#!/usr/bin/env python3
"""Time of forward + backward of the training losses on the MI355X at the headline loss shape (B, T, V) = (256, 25, 22), weights
`frame table + speed` (the YAML's `speed2_sqrt`): each kind of `ops.motion_loss` (cg_motion_loss_fwd / _bwd) next to (a) the existing
`ops.mpjpe` pair and (b) the stock-torch composition of the same formula on the device, written as the reference writes it
(losses/losses.py, train.py:62-70, on a copy of `target_gvel`: the reference divides it in place).
Two figures per side: eager calls (the host's issue of every launch included - what an `EagerStep` pays) and replays of a HIP graph of
one forward + backward (what a `GraphedStep` pays).  Device events around windows of CALLS calls after a warm-up, the sides alternating
over WINDOWS windows; prints the median [min, max] per call in microseconds and one JSON line, and checks first that the composition
and the kernels agree to 1e-4 of max|ref|."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                      # noqa: E402

from cistgcn_amd import ops       # noqa: E402
from cistgcn_amd.environment import frame_weights      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=(256, 25, 22), metavar=("B", "T", "V"))
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
B, T, V = args.shape
FACTOR = 2.0
g = torch.Generator().manual_seed(0)
target = (300 * torch.randn(B, T, V, 3, generator=g)).cuda()
pred = (target.cpu() + torch.randn(B, T, V, 3, generator=g) * torch.tensor([0.3, 3.0, 30.0])).cuda().requires_grad_(True)
gvel = torch.cumsum(3 * torch.rand(B, T, V, 1, generator=g), 1).cuda()
table = frame_weights("speed2_sqrt", T).cuda()
one = torch.ones((), device="cuda")
smooth_l1 = torch.nn.SmoothL1Loss(reduction="none")


def composition(kind):
    def f():
        w = table[None, :, None].tile(B, 1, V)
        speeds = gvel.clone()[:, :, :, 0]
        speeds /= (speeds.max(2, keepdims=True)[0] + 1e-6)
        w += speeds * FACTOR
        d = smooth_l1(pred, target) if "soft" in kind else pred - target
        e = torch.norm(d, 2, dim=-1)
        return torch.sqrt(torch.mean(e)) if kind == "rmpjpe" else torch.mean(w * e) if kind.startswith("weighted") else torch.mean(e)
    return f


def kernels(kind):
    return lambda: ops.motion_loss(kind, pred, target, frame_weights=table, speeds=gvel, speed_factor=FACTOR)


def pair(f):
    def run():
        pred.grad = None
        val = f()
        val.backward(one)
        return val.detach()        # the value only: a live grad_fn would keep this pass's AccumulateGrad nodes (and their stream) alive
    return run


sides = {"ops.mpjpe": pair(lambda: ops.mpjpe(pred, target))}
for kind in ops.LOSS_KINDS:
    sides["ops." + kind] = pair(kernels(kind))
    sides["torch " + kind] = pair(composition(kind))

agree = {}
for kind in ops.LOSS_KINDS:
    a = sides["ops." + kind]()
    ga = pred.grad.clone()
    b = sides["torch " + kind]()
    gb = pred.grad.clone()
    agree[kind] = [abs(float(a) - float(b)) / abs(float(b)), float((ga - gb).abs().max() / gb.abs().max())]

# one HIP graph per side: warm-up on a side stream, then capture one forward + backward
graphs = {}
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    for f in sides.values():
        for _ in range(3):
            f()
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()
for name, f in sides.items():
    graphs[name] = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graphs[name]):
        f()
torch.cuda.synchronize()

modes = {"eager": sides, "graph": {k: gr.replay for k, gr in graphs.items()}}
times = {m: {k: [] for k in sides} for m in modes}
for m, fs in modes.items():
    for f in fs.values():
        for _ in range(30):
            f()
torch.cuda.synchronize()
for _ in range(args.windows):
    for m, fs in modes.items():
        for name, f in fs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                f()
            e1.record()
            e1.synchronize()
            times[m][name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
res = {"shape": [B, T, V], "weights": "speed2_sqrt", "calls_per_window": args.calls, "windows": args.windows, "agreement": agree}
for m in modes:
    for name, t in times[m].items():
        print("%-6s %-30s %8.2f [%.2f, %.2f] us per forward + backward" % (m, name, statistics.median(t), min(t), max(t)))
        res["%s %s" % (m, name)] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
print(json.dumps(res))
assert all(v[0] <= 1e-4 and v[1] <= 1e-4 for v in agree.values()), agree
