#!/usr/bin/env python3
"""Time of the step-list kernel (cg_perturb_sequences, `RobustnessTest`) against the fixed-order kernel (cg_augment_sequences,
`DeviceAugmentation`) on the MI355X: the same whole-sequence section, the same draws, (B, L, J) = (128, 35, 32) by default.
Device events around windows of CALLS calls after a warm-up, the two sides alternating over WINDOWS windows; prints the median
[min, max] per call in microseconds for both and one JSON line, and checks first that the two give the same bits.
A third row times a windowed, continuous section (all six explicit kinds) through the step-list kernel alone."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace as NS

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                # noqa: E402
import torch                      # noqa: E402

from cistgcn_amd.environment import DeviceAugmentation, RobustnessTest      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=(128, 35, 32), metavar=("B", "L", "J"))
ap.add_argument("--input-n", type=int, default=10)
ap.add_argument("--calls", type=int, default=500)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--no-windowed", action="store_true", help="leave the third row out (under a kernel profiler: one kernel name per row)")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
B, L, J = args.shape
cfg = NS(random_scale=NS(x=[0.95, 1.05], y=[0.90, 1.10], z=[0.95, 1.05]), random_noise=0.02, random_flip=NS(x=True, y="", z=True),
         random_rotation=NS(x=[-5, 5], y=[-180, 180], z=[-5, 5]), random_translation=NS(x=[-0.10, 0.10], y=[-0.10, 0.10], z=[-0.10, 0.10]))
w = lambda s0, s1, cont, keep: dict(prob_threshold=0.0, seq_idx=[s0, s1], continuous=cont, keep=keep)
windowed = NS(rotation=NS(x=[-60, 60], y=45.0, z=[-10, 10], **w(3, 20, True, True)), scale=NS(x=1.3, y=[0.6, 0.9], z=1.1, **w(5, 15, True, False)),
              noise=NS(noise=0.05, **w(10, L, True, True)), translation=NS(x=0.2, y=[-0.3, 0.3], z="", **w(3, L, True, False)),
              flip=NS(x="", y=True, z=True, prob_threshold=0.0, seq_idx=[8, 20], keep=False))
if J >= 32:
    windowed.pose_invers = NS(prob_threshold=0.0, seq_idx=[10, 30], keep=True)
g = np.random.RandomState(0)
raw = torch.from_numpy((50 + 350 * g.randn(B, L, J, 3)).astype(np.float32)).cuda()
old, new, win = DeviceAugmentation(cfg), RobustnessTest(cfg), RobustnessTest(windowed)


def on_device(p):
    return {k: torch.from_numpy(v).cuda() for k, v in p.items()} if isinstance(p, dict) else torch.from_numpy(p).cuda()


p_old, p_new = on_device(old.draw(B, np.random.RandomState(1), joints=J)), on_device(new.draw(B, np.random.RandomState(1), joints=J))
p_win = on_device(win.draw(B, np.random.RandomState(2), joints=J))
a, b = old(raw, args.input_n, p_old, keep_processed=True), new(raw, args.input_n, p_new, keep_processed=True)
same = all(torch.equal(a[k], b[k]) for k in a)
sides = {"cg_augment_sequences": lambda: old(raw, args.input_n, p_old), "cg_perturb_sequences": lambda: new(raw, args.input_n, p_new),
         "cg_perturb_sequences windowed": lambda: win(raw, args.input_n, p_win)}
if args.no_windowed:
    del sides["cg_perturb_sequences windowed"]
for f in sides.values():
    for _ in range(50):
        f()
torch.cuda.synchronize()
times = {k: [] for k in sides}
for _ in range(args.windows):
    for name, f in sides.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            f()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
res = {"shape": [B, L, J], "input_n": args.input_n, "same_bits": same, "calls_per_window": args.calls, "windows": args.windows}
for name, t in times.items():
    print("%-32s %8.2f [%.2f, %.2f] us per call (host issue included)" % (name, statistics.median(t), min(t), max(t)))
    res[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
print(json.dumps(res))
assert same, "the two kernels disagree on a whole-sequence section"
