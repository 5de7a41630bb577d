#!/usr/bin/env python3
"""Times of forward kinematics and of the window gather on the MI355X against the same work written as device torch ops (the
reference's route: `fkl_torch` / `ang2joint` are dozens of small torch ops, `the_sequence[fs_sel][:, :, dim_used]` an index op):
  chain FK   260 000 frames x 32 joints (H3.6M after the loader's subsampling), the H3.6M-shaped tree
  SMPL FK    --smpl-frames frames x 52 joints, scale 1000
  gather     B = 256 windows of L = 35 frames, 32 -> 22 joints, out of a bank of 260 000 frames
Device events around windows of CALLS calls after a warm-up, the two sides alternating over WINDOWS windows; prints the median
[min, max] per call and, for the kernels, the bytes the algorithm has to move (inputs read once + outputs written once) over that time
next to the HBM peak (8 TB/s).  The bank (100 MB) fits the 256 MiB Infinity Cache, so the gather's rate is a cache rate; the FK inputs
and outputs together (chain: 203 MB) do not fit it twice over.  Checks first that both sides agree.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                # noqa: E402
import torch                      # noqa: E402

from cistgcn_amd import ops       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chain-frames", type=int, default=260000)
ap.add_argument("--smpl-frames", type=int, default=260000)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
HBM_PEAK = 8.0e12
dev = "cuda"
g = np.random.RandomState(0)

# a 32-joint tree of the H3.6M kind (five chains off the root, depth <= 8) and a 52-joint SMPL-H-like one, seeded: tools/ holds no skeleton tables
chain_parent = [-1, 0, 1, 2, 3, 4, 0, 6, 7, 8, 9, 0, 11, 12, 13, 14, 12, 16, 17, 18, 19, 20, 19, 22, 12, 24, 25, 26, 27, 28, 27, 30]
chain_rest = torch.from_numpy((g.randn(32, 3) * 150).astype(np.float32)).to(dev)
smpl_parent = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19]
for wrist in (20, 21):
    for _ in range(5):
        first = len(smpl_parent)
        smpl_parent += [wrist, first, first + 1]
smpl_rest = torch.from_numpy(np.cumsum(g.uniform(-0.25, 0.25, size=(52, 3)), 0).astype(np.float32)).to(dev)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
angles = (torch.rand(args.chain_frames, 99, device=dev, generator=gen) - 0.5) * 2.4
pose = (torch.rand(args.smpl_frames, 52, 3, device=dev, generator=gen) - 0.5) * 2.4


def skew(k):
    K = torch.zeros(k.shape[:-1] + (3, 3), device=k.device)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -k[..., 2], k[..., 1], -k[..., 0]
    return K - K.transpose(-1, -2)


def torch_chain(angles, parent, rest):
    N, J = angles.shape[0], len(parent)
    r = angles[:, 3:].reshape(N, J, 3)
    th = r.norm(dim=-1)
    K = skew(r / (th[..., None] + 1e-7))
    R = torch.eye(3, device=r.device) + torch.sin(th)[..., None, None] * K + (1 - torch.cos(th))[..., None, None] * (K @ K)
    p = rest[None].repeat(N, 1, 1)
    for i in range(1, J):
        if parent[i] > 0:
            R[:, i] = R[:, i] @ R[:, parent[i]]
            p[:, i] = rest[i] @ R[:, parent[i]] + p[:, parent[i]]
    return p


def torch_smpl(pose, parent, rest, scale):
    th = pose.norm(dim=-1)
    k = pose / th.clamp_min(1e-30)[..., None]
    c = torch.cos(th)[..., None, None]
    R = c * torch.eye(3, device=pose.device) + (1 - c) * (k[..., :, None] * k[..., None, :]) + torch.sin(th)[..., None, None] * skew(k)
    Rg, t = [R[:, 0]], [rest[0].expand(pose.shape[0], 3)]
    for i in range(1, len(parent)):
        q = parent[i]
        t.append((Rg[q] @ (rest[i] - rest[q])[:, None])[..., 0] + t[q])
        Rg.append(Rg[q] @ R[:, i])
    return torch.stack(t, 1) * scale


fk_chain = ops.forward_kinematics(angles, chain_parent, chain_rest)
fk_smpl = ops.forward_kinematics(pose, smpl_parent, smpl_rest, convention="smpl", scale=1000.0)
agree = {"chain": float((fk_chain - torch_chain(angles, chain_parent, chain_rest)).abs().max()),
         "smpl": float((fk_smpl - torch_smpl(pose, smpl_parent, smpl_rest, 1000.0)).abs().max())}
dim_used = [j for j in range(32) if j not in (0, 1, 6, 11, 16, 20, 23, 24, 28, 31)]
L = 35
starts = torch.arange(0, fk_chain.shape[0] - L + 1, dtype=torch.int32, device=dev)
items = torch.randint(0, starts.shape[0], (args.batch,), device=dev, generator=gen).to(torch.int32)
sel, steps = torch.tensor(dim_used, device=dev), torch.arange(L, device=dev)


def torch_gather():
    return fk_chain[starts[items.long()].long()[:, None] + steps[None, :]][:, :, sel]


same_gather = torch.equal(ops.gather_windows(fk_chain, starts, items, L, select=dim_used), torch_gather())
sides = {
    "chain FK  cg_forward_kinematics": (lambda: ops.forward_kinematics(angles, chain_parent, chain_rest), angles.numel() * 4 + fk_chain.numel() * 4),
    "chain FK  torch ops": (lambda: torch_chain(angles, chain_parent, chain_rest), None),
    "SMPL FK   cg_forward_kinematics": (lambda: ops.forward_kinematics(pose, smpl_parent, smpl_rest, convention="smpl", scale=1000.0),
                                        pose.numel() * 4 + fk_smpl.numel() * 4),
    "SMPL FK   torch ops": (lambda: torch_smpl(pose, smpl_parent, smpl_rest, 1000.0), None),
    "gather    cg_gather_windows": (lambda: ops.gather_windows(fk_chain, starts, items, L, select=dim_used), args.batch * L * 22 * 3 * 4 * 2),
    "gather    torch index ops": (torch_gather, None),
}
for f, _ in sides.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
times = {k: [] for k in sides}
for _ in range(args.windows):
    for name, (f, _) in sides.items():
        calls = args.calls * (50 if name.startswith("gather") else 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            f()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
res = {"chain_frames": args.chain_frames, "smpl_frames": args.smpl_frames, "batch": args.batch, "max_abs_diff_vs_torch": agree,
       "gather_same_bits": same_gather, "calls_per_window": args.calls, "windows": args.windows}
for name, t in times.items():
    med, nbytes = statistics.median(t), sides[name][1]
    rate = "" if nbytes is None else "  %.1f MB moved -> %.2f TB/s (%.0f %% of the 8 TB/s HBM peak)" % (nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / med * 1e6 / HBM_PEAK)
    print("%-34s %10.1f [%.1f, %.1f] us per call (host issue included)%s" % (name, med, min(t), max(t), rate))
    res[name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "bytes": nbytes}
print(json.dumps(res))
assert same_gather, "the gather kernel and the torch index ops disagree"
assert agree["chain"] < 0.05 and agree["smpl"] < 0.5, agree      # fp32 torch ops against the f64-composed kernels at coordinates of ~1500 / ~3000
