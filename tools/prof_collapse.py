#!/usr/bin/env python3
"""GPU box: the collapsing convolutions (csrc/collapse_rows.hip) at the three shapes of the headline step (CISTGCN-64, B = 256, T = 50,
V = 22), forward + backward, a few repetitions: the program rocprofv3 is pointed at.  Usage: prof_collapse.py [B T V reps]
  rows gate   C = 64, O = 64   (K = C * T = 3200)
  rows tower  C = 32, O = 32   (K = 1600)
  cols tower  C = 32, O = 32   (K = C * V = 704)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cistgcn_amd import ops

B, T, V, reps = [int(a) for a in sys.argv[1:5]] if len(sys.argv) > 4 else (256, 50, 22, 5)
dev = "cuda"
torch.manual_seed(0)
R = lambda *s: torch.randn(*s, device=dev)
cases = (("rows gate", ops.collapse_rows, 64, 64, T), ("rows tower", ops.collapse_rows, 32, 32, T), ("cols tower", ops.collapse_cols, 32, 32, V))
for name, fn, C, O, kw in cases:
    x, w = R(B, C, T, V).requires_grad_(True), (0.2 * R(O, C, kw)).requires_grad_(True)
    for _ in range(reps):
        x.grad = w.grad = None
        ops.begin_step(torch.device(dev), bump_seed=True)
        y, _st = fn(x, w, want_stats=True)
        y.backward(torch.randn_like(y))
    torch.cuda.synchronize()
    print("%s: B%d C%d T%d V%d O%d  |dx| %.6g  |dW| %.6g" % (name, B, C, T, V, O, float(x.grad.abs().sum()), float(w.grad.abs().sum())))
print("done")
