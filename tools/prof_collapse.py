#!/usr/bin/env python3
"""GPU box: the collapsing convolutions (csrc/collapse_rows.hip) at the shapes of the headline step (CISTGCN-64, B = 256, T = 50,
V = 22), forward + backward, a few repetitions: the program rocprofv3 is pointed at.  Usage: prof_collapse.py [B T V reps [nosums]]
  rows gate   C = 64, O = 64   (K = C * T = 3200)
  tower       the first tower level of a DSTD_GC block as the model runs it: ops.tower_maps(defer=True) of x (B, 64, T, V) into four raw
              maps of 32 channels, each consumed by its collapsing convolution with the BatchNorm + PReLU applied on load -
              rows tower  C = 32, O = 32   (K = 1600), twice
              cols tower  C = 32, O = 32   (K = C * V = 704), twice
              backward: cols | rows | cols | rows, [cg_norm_act_bwd_reduce_many], cg_pointwise_maps_bwd
  nosums      the collapsing backward does not form the channel sums of the towers' BatchNorm backward (`fuse_sums` False in the transform
              records): they come from cg_norm_act_bwd_reduce_many"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from torch import nn
from cistgcn_amd import ops

B, T, V, reps = [int(a) for a in sys.argv[1:5]] if len(sys.argv) > 4 else (256, 50, 22, 5)
fuse = "nosums" not in sys.argv[5:]
dev = "cuda"
torch.manual_seed(0)
R = lambda *s: torch.randn(*s, device=dev)

x, w = R(B, 64, T, V).requires_grad_(True), (0.2 * R(64, 64, T)).requires_grad_(True)
for _ in range(reps):
    x.grad = w.grad = None
    ops.begin_step(torch.device(dev), bump_seed=True)
    y, _st = ops.collapse_rows(x, w, want_stats=True)
    y.backward(torch.randn_like(y))
torch.cuda.synchronize()
print("rows gate: B%d C64 T%d V%d O64  |dx| %.6g  |dW| %.6g" % (B, T, V, float(x.grad.abs().sum()), float(w.grad.abs().sum())))

C, M, O = 64, 32, 32
maps = [(0.2 * R(M, C)).requires_grad_(True) for _ in range(4)]
bns = [nn.BatchNorm2d(M).to(dev).train() for _ in range(4)]
prelus = [nn.PReLU().to(dev) for _ in range(4)]
cws = [(0.2 * R(O, M, T if k % 2 == 0 else V)).requires_grad_(True) for k in range(4)]
x = R(B, C, T, V).requires_grad_(True)
for _ in range(reps):
    for p in [x] + maps + cws + [q for m in bns + prelus for q in m.parameters()]:
        p.grad = None
    ops.begin_step(torch.device(dev), bump_seed=True)
    ys, trs = ops.tower_maps(x, maps, bns, prelus, True, defer=True)
    outs = []
    for k in range(4):
        trs[k]["fuse_sums"] = fuse
        outs.append((ops.collapse_rows if k % 2 == 0 else ops.collapse_cols)(ys[k], cws[k], want_stats=True, transform=trs[k])[0])
    torch.autograd.backward(outs, [torch.randn_like(o) for o in outs])
torch.cuda.synchronize()
print("tower (%s): B%d C%d 4 x M%d T%d V%d O%d  |dx| %.6g  |dW rows| %.6g  |dW cols| %.6g  |dgamma| %.6g  |dalpha| %.6g"
      % ("sums in the collapsing backward" if fuse else "sums from the reduction pass", B, C, M, T, V, O, float(x.grad.abs().sum()),
         float(cws[0].grad.abs().sum()), float(cws[1].grad.abs().sum()), float(bns[0].weight.grad.abs().sum()), float(prelus[0].weight.grad.abs().sum())))
print("done")
