#!/usr/bin/env python3
"""GPU box: `ops.block_mid` (csrc/block_mid.hip) at the items of a 64 -> 64 block of the headline step (CISTGCN-64, B = 256, T = 50,
V = 22), forward + backward, a few repetitions: the program rocprofv3 is pointed at.  Usage: prof_block_mid.py [B T V reps [gates|towers]]
  gates    two full items       C = 32, L = V, O = 64        as channel ranges of one (B, 64, V) tensor
  towers   four pointwise items C = 32, L = V, O = T  |  C = 32, L = T, O = V   (time_compress / joint_compress of both domains)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from torch import nn
from cistgcn_amd import _lib, ops

B, T, V, reps = [int(a) for a in sys.argv[1:5]] if len(sys.argv) > 4 else (256, 50, 22, 12)
which = sys.argv[5] if len(sys.argv) > 5 else "all"
dev = torch.device("cuda")
torch.manual_seed(0)
R = lambda *s: torch.randn(*s, device=dev)
M, O, NR = 32, 64, _lib.STAT_REPLICAS


def sums(x):
    st = torch.zeros(NR, x.shape[1], 2, dtype=torch.float64, device=dev)
    st[0, :, 0], st[0, :, 1] = x.double().sum((0, 2)), x.double().pow(2).sum((0, 2))
    return st


items, leaves = [], []
if which in ("all", "gates"):
    xg = R(B, 2 * M, V).requires_grad_(True)
    sg = sums(xg.detach())
    leaves.append(xg)
    for i in range(2):
        items.append(dict(kind=0, x=xg[:, i * M:(i + 1) * M], bn=nn.BatchNorm2d(M).to(dev), prelu=nn.PReLU().to(dev),
                          weight=(0.1 * R(O, M, V)).requires_grad_(True), salt=3 + i, stats=(sg, i * M, 2 * M)))
if which in ("all", "towers"):
    for k in range(4):
        L, Ok = (V, T) if k % 2 == 0 else (T, V)
        x = R(B, M, L).requires_grad_(True)
        leaves.append(x)
        items.append(dict(kind=1, x=x, bn=nn.BatchNorm2d(M).to(dev), prelu=None, weight=(0.1 * R(Ok, M)).requires_grad_(True), salt=7 + k,
                          stats=(sums(x.detach()), 0, M)))
ops.manual_seed(1, dev)
for _ in range(reps):
    ops.begin_step(dev, bump_seed=True)
    ys = ops.block_mid(items, True, drop_p=0.1)
    torch.autograd.backward(ys, [torch.ones_like(y) for y in ys])
torch.cuda.synchronize()
print("block_mid %s: B%d T%d V%d  %s  |y| %.6g  |dx| %.6g" % (which, B, T, V, " | ".join("%s C%d L%d O%d" % ("pw" if it["kind"] else "full", it["x"].shape[1], it["x"].shape[2],
      it["weight"].shape[0]) for it in items), float(sum(y.abs().sum() for y in ys)), float(sum(x.grad.abs().sum() for x in leaves))))
print("done")
