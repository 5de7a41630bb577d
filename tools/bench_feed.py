#!/usr/bin/env python3
"""What it costs to get from "the window ids of the batch are known" to "the static batch of the training step is ready" on the MI355X,
at B = 256 and B = 16 with L = 35 (10 -> 25 frames) and 22 of 32 joints, for two sides:
  host draws     the path without the device draws: `bank.windows(ids)` + `DeviceAugmentation.draw` (a Python loop over the samples,
                 np.random) + the upload of the table + `cg_augment_sequences` + copies into the buffers of a `GraphedStep`
  in-graph feed  `BankStep` replay time minus `GraphedStep` replay time on the same model and batch size: seed advance, gather at the
                 device cursor, `cg_draw_augmentation`, `cg_augment_sequences` and the cursor advance as nodes of the step's graph
and, as a cross-check of that difference of two much larger numbers, the same five launches captured in a graph of their own.
Device events around windows of CALLS calls after a warm-up, the sides alternating over WINDOWS windows, host issue included; prints the
median [min, max] per call.  The model is the small one (--channels 8): the feed does not depend on it, the difference is the clearer
the shorter the step.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace as NS

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                # noqa: E402
import torch                      # noqa: E402

from cistgcn_amd import ops       # noqa: E402
from cistgcn_amd.environment import DeviceAugmentation, MotionBank, TrainingLoss      # noqa: E402
from cistgcn_amd.models import CISTGCN_0      # noqa: E402
from cistgcn_amd.runtime import BankStep, GraphedStep      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[256, 16])
ap.add_argument("--channels", type=int, default=8)
ap.add_argument("--frames", type=int, default=100000)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
dev, T, To, V = "cuda", 10, 25, 22
L = T + To
dim_used = [j for j in range(32) if j not in (0, 1, 6, 11, 16, 20, 23, 24, 28, 31)]
gen = torch.Generator(device=dev)
gen.manual_seed(0)
bank = MotionBank.from_sequences([300 * torch.randn(args.frames, 32, 3, device=dev, generator=gen)], ["bench"], L, select=dim_used)
# the augmentations of the reference's training YAML: flip, rotation, scale, noise, translation on every axis
aug = DeviceAugmentation(NS(random_flip=NS(x=True, y=True, z=True), random_rotation=NS(x=[-180, 180], y=[-180, 180], z=[-180, 180]),
                            random_scale=NS(x=[0.8, 1.2], y=[0.8, 1.2], z=[0.8, 1.2]), random_noise=0.01,
                            random_translation=NS(x=[-0.1, 0.1], y=[-0.1, 0.1], z=[-0.1, 0.1])))
arch = NS(model_params=NS(input_n=T, output_n=To, joints=V, n_txcnn_layers=4, txc_kernel_size=3, reduction=8, hidden_dim=64, clipping=15,
                          input_gcn=NS(model_complexity=[args.channels] * 4, interpretable=[True] * 5),
                          output_gcn=NS(model_complexity=[3], interpretable=[True])))
loss_cfg = NS(loss=NS(type="w_mpjpe_soft", weights="speed2_sqrt"))


def timed(f, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


res = {"channels": args.channels, "frames": args.frames, "L": L, "joints": V, "calls_per_window": args.calls, "windows": args.windows}
for B in args.batches:
    torch.manual_seed(0)
    net = CISTGCN_0(arch, NS(dropout=0.1)).to(dev).train()
    loss_fn = TrainingLoss(loss_cfg, To, dev)
    feed = bank.feed(B, shuffle=True, generator=gen)
    assert len(feed) >= args.calls + 3
    bank_step = BankStep(net, feed, aug, T, loss=loss_fn, warmup=3)
    bank_step.replay()
    b = bank_step.batch
    plain = GraphedStep(net, b["sample"], b["target"], warmup=3, loss=loss_fn, target_gvel=b["target_gvel"])
    # the five feed launches in a graph of their own, on buffers of their own
    raw, draws = feed.gather(), aug.draw_device(B, joints=V, device=dev)
    item = aug(raw, T, params=draws)

    def feed_launches():
        ops.advance_seed(dev)
        feed.gather(out=raw)
        aug.draw_device(B, joints=V, device=dev, out=draws)
        aug(raw, T, params=draws, out=item)
        ops.cursor_advance(feed.cursor, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        feed_launches()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    feed_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(feed_graph):
        feed_launches()
    at = [0]

    def host_path():
        ids = feed.order[at[0]:at[0] + B]                  # "ids known": a view, nothing is launched
        at[0] += B
        got = aug(bank.windows(ids), T, aug.draw(B, joints=V))
        plain.x.copy_(got["sample"])
        plain.target.copy_(got["target"])
        plain.target_gvel.copy_(got["target_gvel"])

    def epoch():
        feed.start_epoch()
        at[0] = 0
    sides = {"host draws + upload + augment + copies": host_path, "BankStep replay": bank_step.replay, "GraphedStep replay": plain.replay,
             "feed launches as a graph": feed_graph.replay}
    times = {k: [] for k in sides}
    for name, f in sides.items():
        epoch()
        timed(f, 3)
    for _ in range(args.windows):
        for name, f in sides.items():
            epoch()
            torch.cuda.synchronize()
            times[name].append(timed(f, args.calls))
    out = {}
    for name, t in times.items():
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
        print("B = %3d  %-40s %10.1f [%.1f, %.1f] us per call (host issue included)" % (B, name, out[name]["median_us"], min(t), max(t)))
    diff = [a - c for a, c in zip(times["BankStep replay"], times["GraphedStep replay"])]
    out["in-graph feed (BankStep - GraphedStep)"] = {"median_us": statistics.median(diff), "min_us": min(diff), "max_us": max(diff)}
    print("B = %3d  %-40s %10.1f [%.1f, %.1f] us per call (window by window)" % (B, "in-graph feed (BankStep - GraphedStep)", statistics.median(diff), min(diff), max(diff)))
    res["B%d" % B] = out
    del bank_step, plain, feed_graph
print(json.dumps(res))
