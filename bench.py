#!/usr/bin/env python3
"""Headline benchmark: sequences/sec of forward + MPJPE + backward of CIST-GCN on synthetic
H3.6M-shaped poses (BASELINE.json metric), one process per GPU.

    python bench.py --gpus 1 --steps 80 --warmup 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path over one batch resident in HBM: forward, loss, backward and, for
N > 1, the weighted gather of all gradients into the flat buffer plus its RCCL all-reduce (two buckets,
the first one overlapped with the rest of the backward pass).  No optimizer, no logging, no H2D
(SURVEY.md §8d).  Rank 0 prints ONE JSON line.

N = 1 times BASELINE.json configs[2] (CISTGCN-64, B=256, 50->25 frames, 22 joints: the largest
single-GPU configuration and the one the %HBM metric is quoted on) as the headline.  A plain run does
only that: set up, warm up, time --steps steps, print the line.  --full adds, at N = 1, the eval-mode
forward, the block / family rooflines, configs[1] (CISTGCN-8, B=16) under "secondary" and the
configs[4] shape, the CPU baselines timed on this box's host cores and the data-parallel overhead.

--dump-outputs DIR writes what the last timed step computed (loss, gradients, BatchNorm running
statistics) as DIR/*.npy; with the same arguments the inputs are the same from run to run.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from types import SimpleNamespace as NS

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# name -> (C, B per GPU, T_in, V); T_out = 25 everywhere
WORKLOADS = {
    "cistgcn8_b16_t50_v22": (8, 16, 50, 22),      # BASELINE.json configs[1]
    "cistgcn64_b256_t50_v22": (64, 256, 50, 22),  # configs[2] (headline) / per-GPU shard of configs[3]
    "cistgcn32_b256_t50_v25": (32, 256, 50, 25),  # configs[4] shape
    "cistgcn8_b16_t10_v22": (8, 16, 10, 22),      # reference-YAML frames
    "cistgcn64_b256_t10_v22": (64, 256, 10, 22),
    "cistgcn32_b256_t10_v18": (32, 256, 10, 18),  # reference AMASS joints
}
HEADLINE, SECONDARY, AMASS25 = "cistgcn64_b256_t50_v22", "cistgcn8_b16_t50_v22", "cistgcn32_b256_t50_v25"
MIXED_BATCHES = (64, 128, 256, 512)   # configs[4]: per-GPU batch of rank r = MIXED_BATCHES[r % 4]
REAL_STDOUT = 1
HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
F32_PEAK_TFLOPS = 157.3    # same guide: fp32 vector = fp32-input MFMA peak


def make_cfg(C, T, V, dropout):
    arch = NS(model_params=NS(input_n=T, output_n=25, joints=V, n_txcnn_layers=4, txc_kernel_size=3, reduction=8,
                              hidden_dim=64, clipping=15,
                              input_gcn=NS(model_complexity=[C] * 4, interpretable=[True] * 5),
                              output_gcn=NS(model_complexity=[3], interpretable=[True])))
    return arch, NS(dropout=dropout)


def synth(B, T, V, rank, base=1234):
    g = torch.Generator().manual_seed(base + rank)
    x = 50 + 350 * torch.randn(B, T, V, 3, generator=g)
    tgt = x[:, -1:] + 20 * torch.randn(B, 25, V, 3, generator=g)
    return x, tgt


def block_shapes(C, T, V, To=25):
    """(Cin, Cout, T, V) of the six DSTD_GC invocations of one forward (CISTGCN.py:520-524, 549-553)."""
    w = [10, C, C, C, C, 10]
    return [(w[i], w[i + 1], T, V) for i in range(5)] + [(3, 3, V, To)]


def block_bytes(ci, co, t, v):
    """SURVEY 8(d) algorithmic bytes of ONE DSTD_GC invocation per sample: forward = read x, write out, write both
    adjacency maps, write the gates; backward = read x, dOut, both maps, write dx."""
    fwd = 4 * (ci * t * v + co * t * v + v * t * t + t * v * v + 2 * co)
    bwd = 4 * (ci * t * v + co * t * v + v * t * t + t * v * v + ci * t * v)
    return fwd, bwd


def model_bytes_per_sequence(C, T, V, To=25):
    """ALGORITHMIC HBM bytes of one sequence through the six DSTD_GC blocks + model I/O, forward and backward."""
    fb = [block_bytes(*s) for s in block_shapes(C, T, V, To)]
    io = 4 * (3 * T * V + 10 * T * V + 2 * 10 * To * V + 4 * 3 * To * V)
    return sum(f for f, _ in fb) + io, sum(b for _, b in fb) + io


# ---------------------------------------------------------------------------------------------------------------------
# live per-entry-point timing: HIP events (on the stream the library launches on) around every C-ABI call of one
# eager training step, with the ALGORITHMIC bytes of each call computed from its arguments
# ---------------------------------------------------------------------------------------------------------------------
# Kernel families: forward AND backward entry points of one stage form one family everywhere (round-2 review: a stage split in two
# next to stages counted whole made "the dominant family" an artefact of the grouping).  Each family names the device kernels
# rocprofv3 reports for it, so profiles/*kernel_stats.csv can be summed the same way.
FAM_STGCN = "fused ST-GCN stage (cg_stgcn_domain_fwd/bwd)"
FAM_TAIL = "DSTD_GC tail phases (cg_dstd_tail_fwd/bwd)"
FAM_CONTRACT = "contraction (cg_contract_many)"
FAM_ADJ = "Map2Adj tail phases (cg_map2adj_tail_fwd/bwd)"
FAM_ROWS = "row kernels (cg_norm_act_fwd/bwd, cg_chan_stats)"
FAM_PWM = "stacked tower maps (cg_pointwise_maps_fwd/bwd)"
FAM_ROWSCONV = "frame- / joint-collapsing convolutions (cg_collapse_rows_fwd/bwd, cg_collapse_cols_fwd/bwd)"
FAM_FPN = "time-extrapolator convolutions (cg_fpn_conv_fwd/bwd)"
FAM_STATS = "block input: global_norm + statistics (cg_block_input_fwd/bwd, cg_dstd_stats_fwd/bwd)"
FAM_CTX = "ContextLayer heads (cg_context_heads_fwd/bwd)"
FAM_GATE = "gate paths behind their (1,V) convolutions (cg_gate_head_fwd/bwd)"
FAMILY_KERNELS = {          # device-kernel name prefixes of each family, as rocprofv3 --kernel-trace reports them
    FAM_STGCN: ("cg_stgcn_", "cg_dom_fold"),
    FAM_TAIL: ("cg_tail_",),
    FAM_CONTRACT: ("cg_contract",),
    FAM_ADJ: ("cg_adj_",),
    FAM_ROWS: ("cg_norm_act_", "cg_chan_stats"),
    FAM_PWM: ("cg_pwm_",),
    FAM_ROWSCONV: ("cg_rows_", "cg_cols_"),
    FAM_FPN: ("cg_fpn_",),
    FAM_STATS: ("cg_bin_", "cg_dstd_stats"),
    FAM_CTX: ("cg_ctx_",),
    FAM_GATE: ("cg_gate_",),
}
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r04_traffic.json")      # HBM bytes per family / per block from rocprofv3 PMC passes (tools/collect_profiles_r04.py)


def _numel(v):
    return int(v.n[0]) * int(v.n[1]) * int(v.n[2]) * int(v.n[3])


def _call_bytes(name, args):
    """(family, algorithmic bytes) of one C-ABI call: every operand and result counted once."""
    from cistgcn_amd import _lib
    if name == "cg_contract_many":
        arr, n = args[0], args[1]
        total = 0
        for i in range(n):
            d = arr[i]
            total += 4 * (d.G * d.M * d.K + d.G * d.K * d.N + d.G * d.M * d.N)
        return FAM_CONTRACT, total
    if name in ("cg_norm_act_fwd_many", "cg_norm_act_bwd_many"):
        arr, n = args[0], args[-2] if name.endswith("bwd_many") else args[1]
        total = 0
        for i in range(n):
            a = arr[i]
            e = _numel(a.xv)
            if name == "cg_norm_act_fwd_many":
                total += 4 * e * (2 + (1 if a.add else 0))                      # x (+ add) -> y
            else:
                total += 4 * e * (2 + (1 if a.dx else 0) + (1 if (a.add and not a.add_post) else 0) + (1 if a.dadd else 0))
        return FAM_ROWS, total
    if name == "cg_chan_stats_many":
        return FAM_ROWS, sum(4 * _numel(args[0][i].xv) for i in range(args[1]))
    if name in ("cg_stgcn_domain_fwd", "cg_stgcn_domain_bwd"):
        B, ci, co, T, V, dom = args[-7:-1] if name.endswith("fwd") else args[-8:-2]
        ng, j = (V, T) if dom == 0 else (T, V)
        x, y, adj = B * ci * T * V, B * co * T * V, B * ng * j * j
        if name.endswith("fwd"):
            return FAM_STGCN, 4 * (x + adj + y + co * ci + co)
        return FAM_STGCN, 4 * (2 * x + 2 * adj + y + 2 * co * ci)
    if name in ("cg_dstd_tail_fwd", "cg_dstd_tail_bwd"):
        import ctypes
        t = ctypes.cast(args[0], ctypes.POINTER(_lib.DstdTail)).contents
        n = 4 * t.B * t.C * t.T * t.V                    # one (B,C,T,V) tensor
        # tensor passes of each phase (section 4 of DESIGN.md): F1 y,r x2 | F2 y,r x2 -> h0 | F3 h0 | F4 h0,bres -> out;
        # K1 dout,h0 | K2 dout,h0 | K3 dout,h0,y,r x2 -> gp x2 | K4 y,r,gp x2 -> dr x2 | K5 y,dr x2 -> dy x2
        passes = {1: 4, 2: 5, 3: 1, 4: 3} if name.endswith("fwd") else {1: 2, 2: 2, 3: 8, 4: 8, 5: 6}
        return FAM_TAIL, n * passes.get(args[1], 0)
    if name in ("cg_map2adj_tail_fwd", "cg_map2adj_tail_bwd"):
        items, n, phase = args[0], args[1], args[2]
        e = sum(4 * items[i].B * items[i].Kc * items[i].J * items[i].J for i in range(n))      # one (B,Kc,J,J) tensor per tower
        passes = {1: 1, 2: 2} if name.endswith("fwd") else {1: 3, 2: 2}
        return FAM_ADJ, e * passes.get(phase, 0)
    if name in ("cg_pointwise_maps_fwd", "cg_pointwise_maps_bwd"):
        import ctypes
        t = ctypes.cast(args[0], ctypes.POINTER(_lib.PwMaps)).contents
        x, ys = 4 * t.B * t.Cin * t.P, sum(4 * t.B * t.M[i] * t.P for i in range(t.n))
        return FAM_PWM, (x + ys) if name.endswith("fwd") else (2 * x + ys)
    if name in ("cg_collapse_rows_fwd", "cg_collapse_rows_bwd", "cg_collapse_cols_fwd", "cg_collapse_cols_bwd"):
        import ctypes
        t = ctypes.cast(args[0], ctypes.POINTER(_lib.RowsConv)).contents
        x = 4 * t.B * t.C * t.T * t.V
        return FAM_ROWSCONV, x if name.endswith("fwd") else 2 * x
    if name in ("cg_fpn_conv_fwd", "cg_fpn_conv_bwd"):
        import ctypes
        t = ctypes.cast(args[0], ctypes.POINTER(_lib.FpnConv)).contents
        x, y = 4 * t.B * t.C * t.H * t.W, 4 * t.B * t.O * t.H * t.W
        return FAM_FPN, (x + t.n * y) if name.endswith("fwd") else (3 * x + 2 * t.n * y)
    if name in ("cg_dstd_stats_fwd", "cg_dstd_stats_bwd"):
        B, C, T, V = args[-5:-1]
        return FAM_STATS, 4 * B * C * T * V * (1 if name.endswith("fwd") else 3)
    if name in ("cg_block_input_fwd", "cg_block_input_bwd"):
        import ctypes
        t = ctypes.cast(args[0], ctypes.POINTER(_lib.BlockInput)).contents
        n = 4 * t.B * t.C * t.T * t.V
        # forward: x -> xn; backward: the consumers' gradients and x -> dx (the stored sum G travels twice more: not algorithmic)
        return FAM_STATS, 2 * n if name.endswith("fwd") else (sum(1 for i in range(t.ng) if t.g[i]) + 2) * n
    if name in ("cg_gate_head_fwd", "cg_gate_head_bwd"):
        import ctypes
        t = ctypes.cast(args[0], ctypes.POINTER(_lib.GateHead)).contents
        per = 4 * t.B * (2 * t.C + t.S) + 4 * t.C * (2 * t.C + t.S)          # z, statistics, gate; both weight matrices
        return FAM_GATE, t.n * per * (1 if name.endswith("fwd") else 2)
    if name in ("cg_context_heads_fwd", "cg_context_heads_bwd"):
        import ctypes
        t = ctypes.cast(args[0], ctypes.POINTER(_lib.CtxHeads)).contents
        return FAM_CTX, 4 * t.B * (t.P + 4 * t.C) * (1 if name.endswith("fwd") else 2)
    return "other (%s)" % name, 0


class CallProbe:
    """Context manager: wraps cistgcn_amd._lib.call for the duration of one eager step."""

    def __init__(self):
        self.rows = []

    def __enter__(self):
        from cistgcn_amd import _lib
        self._lib, self._orig = _lib, _lib.call

        def call(name, *args):
            fam, nbytes = _call_bytes(name, args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._orig(name, *args)
            e1.record()
            self.rows.append((fam, nbytes, e0, e1))

        _lib.call = call
        return self

    def __exit__(self, *exc):
        self._lib.call = self._orig
        return False

    def families(self):
        torch.cuda.synchronize()
        fam = {}
        for name, nbytes, e0, e1 in self.rows:
            f = fam.setdefault(name, {"launches": 0, "us": 0.0, "algorithmic_bytes": 0})
            f["launches"] += 1
            f["us"] += e0.elapsed_time(e1) * 1e3
            f["algorithmic_bytes"] += nbytes
        for f in fam.values():
            f["GBps"] = f["algorithmic_bytes"] / max(f["us"], 1e-9) / 1e3
            f["frac"] = f["GBps"] / HBM_PEAK_GBS
        return fam


def family_rooflines(net, x, tgt, reps=3):
    """One eager (un-graphed) training step per repetition with every library call bracketed by HIP events.
    Kernels are long at the headline size, so the brackets see kernel time, not launch gaps."""
    from cistgcn_amd.runtime import EagerStep
    step = EagerStep(net, x, tgt)
    for _ in range(2):
        step.replay()
    torch.cuda.synchronize()
    acc = None
    for _ in range(reps):
        with CallProbe() as probe:
            step.replay()
        fam = probe.families()
        if acc is None:
            acc = fam
        else:
            for k, f in fam.items():
                for kk in ("launches", "us", "algorithmic_bytes"):
                    acc[k][kk] += f[kk]
    other = {"launches": 0, "us": 0.0, "algorithmic_bytes": 0}
    out = {}
    for k, f in acc.items():
        for kk in ("launches", "us", "algorithmic_bytes"):
            f[kk] = f[kk] / reps
        if k.startswith("other"):
            for kk in other:
                other[kk] += f[kk]
            continue
        f["GBps"] = f["algorithmic_bytes"] / max(f["us"], 1e-9) / 1e3
        f["frac"] = f["GBps"] / HBM_PEAK_GBS
        f["kernels"] = [pre + "*" for pre in FAMILY_KERNELS.get(k, ())]
        out[k] = f
    out["other entry points (cat / sum / zero copies, SE gates, pooling, MPJPE, feature lift)"] = other
    return out


def attach_traffic(fams, workload):
    """HBM bytes per step of every family from the committed rocprofv3 PMC passes (separate FETCH_SIZE / WRITE_SIZE runs of this
    very workload, corrected as MI355X_MICROARCH.md prescribes: FETCH_SIZE doubled for wide streaming reads); null when the
    profile of this round has not been collected."""
    rec = {}
    if os.path.exists(TRAFFIC_FILE):
        rec = json.load(open(TRAFFIC_FILE)).get(workload, {})
    for k, f in fams.items():
        t = rec.get(k)                       # bytes per training step, all launches of the family
        f["traffic_per_step"] = t
        f["traffic_over_algorithmic"] = (t / f["algorithmic_bytes"]) if (t and f.get("algorithmic_bytes")) else None


def block_roofline(C, B, T, V, device, dropout, reps=5):
    """SURVEY 8(d) bytes of ONE DSTD_GC invocation (C -> C on (T,V): three of the six blocks, and the bulk of the step)
    divided by the summed time of all its kernels, forward and backward: HIP events around every library call of the eager block."""
    from cistgcn_amd import ops
    from cistgcn_amd.models import CISTGCN_0
    torch.manual_seed(0)
    net = CISTGCN_0(*make_cfg(C, T, V, dropout)).to(device).train()
    blk = net.st_gcnns[1]
    x = torch.randn(B, C, T, V, device=device, requires_grad=True)
    tf = tb = 0.0
    nf = nb = 0
    for r in range(reps + 2):
        ops.begin_step(device, bump_seed=False)
        net._site = 0
        x.grad = None
        # every library call of the block bracketed by HIP events on its stream, the brackets summed: kernel time.  (Events around the
        # whole eager block measured the host as well: ~45 launches of a few tens of microseconds of Python each are as long as the
        # block's kernels since round 4 - the figure moved with the box's CPU, not with the kernels.)
        with CallProbe() as pf:
            y = net._block_staged(blk, x)
            y = y[0] if isinstance(y, tuple) else y
        with CallProbe() as pb:
            y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
        if r >= 2:
            tf += sum(e0.elapsed_time(e1) for _, _, e0, e1 in pf.rows) * 1e-3
            tb += sum(e0.elapsed_time(e1) for _, _, e0, e1 in pb.rows) * 1e-3
            nf, nb = len(pf.rows), len(pb.rows)
    tf, tb = tf / reps, tb / reps
    bf, bb = block_bytes(C, C, T, V)
    flops = 2.0 * B * (C * V * T * T + C * T * V * V + 2 * C * C * T * V + 2 * C * C * T * V)   # both graph products, both tcn, compressor
    return {"block": "DSTD_GC %d->%d on (T=%d, V=%d), B=%d, train mode, eager launches" % (C, C, T, V, B), "bound": "hbm",
            "library_calls_fwd": nf, "library_calls_bwd": nb, "timing": "sum of the HIP-event brackets of every library call",
            "algorithmic_bytes_fwd": B * bf, "algorithmic_bytes_bwd": B * bb, "fwd_us": tf * 1e6, "bwd_us": tb * 1e6,
            "achieved": B * (bf + bb) / (tf + tb) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": B * (bf + bb) / (tf + tb) / 1e9 / HBM_PEAK_GBS,
            "fwd_frac": B * bf / tf / 1e9 / HBM_PEAK_GBS, "bwd_frac": B * bb / tb / 1e9 / HBM_PEAK_GBS,
            "dense_gflop_fwd": flops / 1e9, "f32_frac_fwd": flops / tf / 1e12 / F32_PEAK_TFLOPS}


# ---------------------------------------------------------------------------------------------------------------------
# CPU baseline (oracle = stock-PyTorch restatement pinned to the reference), child process with fixed thread count
# ---------------------------------------------------------------------------------------------------------------------
def cpu_baseline_worker(C, B, T, V, dropout, budget_s, max_steps, min_steps=3):
    from oracle import cistgcn_ref as O
    torch.manual_seed(0)
    net = O.CISTGCN(*make_cfg(C, T, V, dropout)).train()
    x, tgt = synth(B, T, V, 0)

    def step():
        net.zero_grad(set_to_none=True)
        pred, = net(x)
        O.mpjpe(pred, tgt).backward()

    step()
    n, t0 = 0, time.perf_counter()
    while True:
        step()
        n += 1
        el = time.perf_counter() - t0
        if n >= min(min_steps, max_steps) and (el >= budget_s or n >= max_steps):      # at least three timed steps
            break
    print(json.dumps({"rate": B * n / el, "steps": n, "seconds": el, "threads": torch.get_num_threads()}))


def cpu_baseline(C, B, T, V, dropout, thread_counts, budget_s, max_steps=30):
    """The CPU oracle timed on this box's host cores on the same workload (forward + MPJPE + backward), one child process
    per thread count (OMP_NUM_THREADS fixed); the BEST count is reported.  PyTorch's intra-op threading does not scale on
    ~1.5 k small ops per step, so more threads are not always faster."""
    import subprocess
    ncpu = os.cpu_count() or 1
    counts = sorted({min(ncpu, c) for c in thread_counts})
    tried, best = [], None
    for nt in counts:
        env = dict(os.environ, OMP_NUM_THREADS=str(nt), MKL_NUM_THREADS=str(nt), HIP_VISIBLE_DEVICES="")
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", str(C), str(B), str(T), str(V), str(dropout),
               str(budget_s / len(counts)), str(max_steps)]
        print("bench.py: cpu baseline C=%d B=%d with %d threads ..." % (C, B, nt), file=sys.stderr, flush=True)
        try:
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            r = json.loads(res.stdout.strip().splitlines()[-1])
        except Exception as e:        # a failed trial must not take the GPU result down with it
            tried.append("%d thr: failed (%s)" % (nt, type(e).__name__))
            continue
        tried.append("%d thr: %.2f seq/s (%d steps, %.1f s)" % (nt, r["rate"], r["steps"], r["seconds"]))
        if best is None or r["rate"] > best[0]:
            best = (r["rate"], nt)
    if best is None:
        return {"value": None, "unit": "sequences/sec", "cores": 0, "kind": "port", "sample": "; ".join(tried)}
    return {"value": best[0], "unit": "sequences/sec", "cores": best[1], "kind": "port",
            "sample": "fwd+bwd steps of the same workload (C=%d, B=%d, T=%d, V=%d) on the host (%d logical CPUs), torch %s CPU, "
                      "1 warm-up step, best of: %s" % (C, B, T, V, ncpu, torch.__version__, "; ".join(tried))}


def headline_cpu_baseline(C, B, T, V, dropout):
    """Large workloads: the thread count is chosen on a bounded sample (a quarter of the batch, >= 3 timed steps per count, 16 / 32 /
    64 / 128 threads), then the FULL batch is timed with the best count for >= 3 steps; `value` is the full-batch rate.  Small
    workloads: the whole sweep runs at full size."""
    if B * C < 4096:
        return cpu_baseline(C, B, T, V, dropout, (8, 16, 32), 12.0)
    Bs = max(16, B // 4)
    sweep = cpu_baseline(C, Bs, T, V, dropout, (16, 32, 64, 128), 48.0, max_steps=3)
    nt = sweep["cores"] or 16
    full = cpu_baseline(C, B, T, V, dropout, (nt,), 40.0, max_steps=3)
    full["thread_sweep"] = {"batch": Bs, "best_threads": nt, "rates": sweep["sample"]}
    return full


def cpu_forward_worker(C, B, T, V, budget_s, max_steps):
    """BASELINE configs[0]: eval-mode forward only (no_grad) of the CPU oracle."""
    from oracle import cistgcn_ref as O
    torch.manual_seed(0)
    net = O.CISTGCN(*make_cfg(C, T, V, 0.0)).eval()
    x, _ = synth(B, T, V, 0)
    with torch.no_grad():
        net(x)
        n, t0 = 0, time.perf_counter()
        while True:
            net(x)
            n += 1
            el = time.perf_counter() - t0
            if el >= budget_s or n >= max_steps:
                break
    print(json.dumps({"rate": B * n / el, "steps": n, "seconds": el, "threads": torch.get_num_threads()}))


def cpu_forward_baseline(C, B, T, V, thread_counts=(8, 16, 32), budget_s=9.0):
    import subprocess
    ncpu = os.cpu_count() or 1
    tried, best = [], None
    for nt in sorted({min(ncpu, c) for c in thread_counts}):
        env = dict(os.environ, OMP_NUM_THREADS=str(nt), MKL_NUM_THREADS=str(nt), HIP_VISIBLE_DEVICES="")
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-forward-worker", str(C), str(B), str(T), str(V), str(budget_s / 3), "200"]
        try:
            r = json.loads(subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
        except Exception as e:
            tried.append("%d thr: failed (%s)" % (nt, type(e).__name__))
            continue
        tried.append("%d thr: %.1f seq/s (%d forwards, %.1f s)" % (nt, r["rate"], r["steps"], r["seconds"]))
        if best is None or r["rate"] > best[0]:
            best = (r["rate"], nt)
    return {"value": best[0] if best else None, "unit": "sequences/sec", "cores": best[1] if best else 0, "kind": "port",
            "sample": "eval-mode forward of the same workload (C=%d, B=%d, T=%d, V=%d, no_grad) on the host (%d logical CPUs), 1 warm-up, "
                      "best of: %s" % (C, B, T, V, ncpu, "; ".join(tried))}


def dp_overhead(net, device, reps=20):
    """What data parallelism adds to a step besides waiting for other ranks, timed on this one GPU: the weighted gather of all
    gradients into the flat buffer, an RCCL all-reduce of that buffer in a ONE-rank communicator (launch + kernel cost, no wire)
    and the 1/world scale.  HIP events on the launch stream."""
    import torch.distributed as dist
    from cistgcn_amd import ops, _lib
    from cistgcn_amd.runtime import FlatGrads
    own = False
    try:
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
            own = True
        params = [p for p in net.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.zeros_like(p)
        flat = FlatGrads(params, device)
        def once():
            flat.gather(scale=1.0)
            dist.all_reduce(flat.flat)
            _lib.call("cg_scale", ops._ptr(flat.flat), flat.flat.numel(), 1.0, ops._stream(flat.flat))
        for _ in range(3):
            once()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            once()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        for p in params:
            p.grad = None
        return {"ms": ms, "bytes": 4 * flat.numel, "tensors": len(params), "what": "gather + one-rank RCCL all-reduce + scale of the flat gradient buffer"}
    except Exception as e:           # a missing RCCL must not take the throughput line down
        return {"ms": None, "error": "%s: %s" % (type(e).__name__, e)}
    finally:
        if own and dist.is_initialized():
            dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------------
def dump_outputs(out_dir, step, net, world):
    """What the last timed step handed its caller, as float32 .npy files: the loss, the gradient of every trainable
    parameter (in net.parameters() order, flattened and concatenated; for N > 1 the averaged flat buffer) and the
    BatchNorm running statistics the step updated.  About 8 MB at C = 64."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    if world > 1:
        grads = step.flat.flat
    else:
        grads = torch.cat([p.grad.reshape(-1) for p in net.parameters() if p.requires_grad])
    stats = torch.cat([b.reshape(-1) for b in net.buffers() if b.is_floating_point()])
    for name, t in (("loss", step.loss), ("param_grads", grads), ("bn_running_stats", stats)):
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


def timed_training(workload, args, device, rank, world, steps, warmup, batch=None, dump_dir=None):
    """Builds the model and the captured step for `workload`, runs `warmup` untimed and exactly `steps` timed steps
    bracketed by barrier + synchronize; returns (result dict, net, x, tgt) - the step object is released.  `dump_dir`:
    rank 0 writes the outputs of the last timed step there (dump_outputs)."""
    import torch.distributed as dist
    from cistgcn_amd import ops
    from cistgcn_amd.models import CISTGCN_0
    from cistgcn_amd.runtime import DataParallelStep, EagerStep, GraphedStep
    C, B, T, V = WORKLOADS[workload]
    B = batch or B
    torch.manual_seed(0)
    net = CISTGCN_0(*make_cfg(C, T, V, args.dropout)).to(device).train()
    ops.manual_seed(args.data_seed + rank, device)
    x, tgt = synth(B, T, V, rank, args.data_seed)
    x, tgt = x.to(device), tgt.to(device)
    if world > 1:
        step = DataParallelStep(net, x, tgt, graph=not args.no_graph, cut_block=None if args.buckets > 1 else -1)
    elif args.no_graph:
        step = EagerStep(net, x, tgt)
    else:
        step = GraphedStep(net, x, tgt, warmup=3, branches=args.branches, tries=args.capture_tries)
    for _ in range(warmup):
        step.replay()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.replay()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    total_b = B
    if world > 1:
        t = torch.tensor([el, float(B)], device=device, dtype=torch.float64)
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        el, total_b = float(tmax[0].item()), int(round(float(t[1].item())))
    loss = float(step.loss.item())
    if not (loss == loss):
        raise SystemExit("bench.py: loss is NaN on rank %d for %s" % (rank, workload))
    res = {"workload": workload, "value": total_b * steps / el, "ms_per_step": el / steps * 1e3, "steps": steps, "seconds": el,
           "loss": loss, "capture_ms": getattr(step, "capture_ms", None), "global_batch": total_b, "per_gpu_batch": B,
           "shard_weight": getattr(step, "weight", None),
           "buckets": len(step.flat.buckets) if world > 1 else None,
           "bucket_bytes": [4 * int(step.flat.bucket_view(k).numel()) for k in range(len(step.flat.buckets))] if world > 1 else None,
           "per_rank": None, "overlap_probe": getattr(step, "overlap_probe", None) if world > 1 else None}
    if world > 1:          # per-GPU batch and gradient weight of every rank (mixed batches: B_r * world / sum B)
        per = [None] * world
        dist.all_gather_object(per, {"rank": rank, "batch": B, "shard_weight": getattr(step, "weight", None)})
        res["per_rank"] = per
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, step, net, world)
    del step
    for p in net.parameters():
        p.grad = None
    torch.cuda.synchronize()
    return res, net, x, tgt


def eval_forward(net, x, steps, warmup):
    from cistgcn_amd.runtime import GraphedForward
    net.eval()
    fwd = GraphedForward(net, x)
    for _ in range(warmup):
        fwd.replay()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(steps):
        fwd.replay()
    torch.cuda.synchronize()
    ef = (time.perf_counter() - t1) / steps
    net.train()
    del fwd
    return {"value": x.shape[0] / ef, "unit": "sequences/sec", "ms_per_batch": ef * 1e3, "graph": True}


def step_roofline(C, T, V, seq_per_s):
    bf, bb = model_bytes_per_sequence(C, T, V)
    gbs = (bf + bb) * seq_per_s / 1e9
    return {"bound": "hbm", "algorithmic_bytes_per_sequence_fwd": bf, "algorithmic_bytes_per_sequence_bwd": bb,
            "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-baseline-worker":
        C, B, T, V = [int(v) for v in sys.argv[2:6]]
        return cpu_baseline_worker(C, B, T, V, float(sys.argv[6]), float(sys.argv[7]), int(sys.argv[8]))
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-forward-worker":
        C, B, T, V = [int(v) for v in sys.argv[2:6]]
        return cpu_forward_worker(C, B, T, V, float(sys.argv[6]), int(sys.argv[7]))
    # exactly ONE line on stdout: RCCL prints a version banner on stdout when a communicator is created (and libraries may print
    # more); everything but the result line goes to stderr from here on
    global REAL_STDOUT
    sys.stdout.flush()
    REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=80, help="timed steps of the headline workload (80 x ~30 ms > 2 s)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default=HEADLINE, choices=sorted(WORKLOADS))
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of HIP-graph replay")
    ap.add_argument("--branches", action="store_true", help="(default at N = 1) capture independent branches - the ContextLayer beside the output block - on forked streams")
    ap.add_argument("--no-branches", action="store_true", help="capture the step on one stream")
    ap.add_argument("--full", action="store_true",
                    help="N=1: after the headline, also the eval forward, rooflines, CPU baselines, secondary workloads and the "
                         "data-parallel overhead (each can be left out with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the loss, parameter gradients and BatchNorm running statistics of the last timed step as DIR/*.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the block / family rooflines")
    ap.add_argument("--no-eval", action="store_true", help="--full: skip the eval-mode forward-only timing")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the configs[1] (CISTGCN-8, B=16) and configs[4]-shape lines")
    ap.add_argument("--no-dp-overhead", action="store_true", help="--full: skip the one-GPU timing of gather + one-rank RCCL all-reduce + scale")
    ap.add_argument("--capture-tries", type=int, default=3,
                    help="graphs captured before the run; the MEDIAN one is kept (buffer placement moves the step by +-3 %%)")
    ap.add_argument("--data-seed", type=int, default=1234, help="base seed of the synthetic batch (rank is added)")
    ap.add_argument("--buckets", type=int, default=2, help="N>1: 2 = two-phase backward with the first bucket's all-reduce overlapped, 1 = one bucket")
    ap.add_argument("--mixed-batches", action="store_true", help="N>1: per-GPU batch of rank r = (64,128,256,512)[r %% 4] (BASELINE configs[4])")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="collective backend for N>1: nccl (= RCCL over xGMI, the real path) or gloo (rehearsal of the "
                         "multi-rank code path on a box with fewer GPUs than ranks)")
    args = ap.parse_args()
    # one-stream capture measured 20.78 ms, forked capture 20.40 ms on the headline workload (round 4, same box, 60 steps each)
    args.branches = not args.no_branches and os.environ.get("CISTGCN_BRANCHES", "1") != "0"

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run for N>1)" % (args.gpus, world))
    if args.backend == "gloo":
        local = local % max(1, torch.cuda.device_count())     # rehearsal: ranks may share a GPU
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    from cistgcn_amd import _lib
    _lib.lib()   # fail loudly if the HIP library is missing

    C, B, T, V = WORKLOADS[args.workload]
    batch = MIXED_BATCHES[rank % len(MIXED_BATCHES)] if (args.mixed_batches and world > 1) else None
    res, net, x, tgt = timed_training(args.workload, args, device, rank, world, args.steps, args.warmup, batch, args.dump_outputs)
    out = {
        "metric": "sequences/sec (fwd+bwd) H3.6M 22-joint 50->25" if (T, V) == (50, 22) else "sequences/sec (fwd+bwd)",
        "value": res["value"], "unit": "sequences/sec", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": res["ms_per_step"], "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": args.workload, "C": C, "per_gpu_batch": res["per_gpu_batch"], "global_batch": res["global_batch"],
                   "T_in": T, "T_out": 25, "V": V, "dropout": args.dropout, "parallelism": "dp%d" % world, "graph": not args.no_graph,
                   "graph_branches": bool(args.branches and not args.no_graph), "timed_seconds": res["seconds"],
                   "capture_probe_ms": res["capture_ms"], "capture_kept": "median" if res["capture_ms"] else None,
                   "collective": ("rccl" if args.backend == "nccl" else "gloo") if world > 1 else None,
                   "gradient_buckets": res["buckets"], "gradient_bucket_bytes": res["bucket_bytes"], "per_rank": res["per_rank"],
                   "side_stream_probe": res["overlap_probe"],
                   "mixed_batches": bool(batch), "loss": res["loss"]},
    }
    if rank == 0 and world == 1:
        out["step_roofline"] = step_roofline(C, T, V, out["value"])
    if rank == 0 and world == 1 and args.full:
        if not args.no_eval:
            out["eval_forward"] = eval_forward(net, x, args.steps, args.warmup)
        if not args.no_roofline:
            fams = family_rooflines(net, x, tgt)
            attach_traffic(fams, args.workload)
            dom = max((k for k in fams if not k.startswith("other")), key=lambda k: fams[k]["us"])
            f = fams[dom]
            del net
            torch.cuda.synchronize()
            blk = block_roofline(C, B, T, V, device, args.dropout)
            blk_traffic = None
            if os.path.exists(TRAFFIC_FILE):
                blk_traffic = (json.load(open(TRAFFIC_FILE)).get(args.workload, {}).get("_block") or {}).get("bytes")
            # `roofline` is SURVEY 8(d)'s quantity (round-3 review): the unit is ONE DSTD_GC invocation (64 -> 64 on (T, V): three of the six
            # blocks and the bulk of the step), its algorithmic bytes (read x, write out, both adjacency maps, the gates; backward: x, dOut,
            # the maps, dx - times the batch) over the summed duration of ALL its kernels, forward + backward, HIP events on the launch stream.
            # `traffic`: HBM bytes of one such invocation from the PMC passes over tools/prof_block.py (profiles/r04_traffic.json).
            out["roofline"] = {"bound": "hbm", "achieved": blk["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": blk["frac"],
                               "traffic": blk_traffic,
                               "kernel": "every kernel of one DSTD_GC block invocation, forward + backward (cg_bin_*, cg_pwm_*, cg_rows_*, cg_cols_*, cg_contract*, "
                                         "cg_norm_act_*, cg_adj_*, cg_stgcn_*, cg_tail_*, cg_se_gate_*)",
                               "unit_of_work": blk["block"],
                               "algorithmic_bytes_per_launch": blk["algorithmic_bytes_fwd"] + blk["algorithmic_bytes_bwd"],
                               "avg_us": blk["fwd_us"] + blk["bwd_us"], "fwd_us": blk["fwd_us"], "bwd_us": blk["bwd_us"],
                               "traffic_over_algorithmic": (blk_traffic / (blk["algorithmic_bytes_fwd"] + blk["algorithmic_bytes_bwd"])) if blk_traffic else None,
                               "f32_mfma_frac_fwd": blk["f32_frac_fwd"],
                               "how": "SURVEY 8(d) bytes of one block invocation x batch / summed time of all its kernels (eager launches, HIP events); "
                                      "the whole step by the same rule is `step_roofline`",
                               # the largest kernel family of the step on its OWN operand bytes (every operand / result of each call once): how well
                               # the kernels stream what they are given, not a SURVEY 8(d) figure
                               "dominant_family": {"family": dom, "kernel": ", ".join(f["kernels"]), "achieved": f["GBps"], "frac_of_peak_on_operand_bytes": f["frac"],
                                                   "launches_per_step": f["launches"], "avg_us": f["us"] / max(1, f["launches"]), "us_per_step": f["us"],
                                                   "traffic_per_launch": (f["traffic_per_step"] / max(1, f["launches"])) if f["traffic_per_step"] else None},
                               "per_family": fams}
            out["block_roofline"] = blk
        else:
            del net
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = headline_cpu_baseline(C, B, T, V, args.dropout)
        if not args.no_secondary and args.workload != SECONDARY:
            torch.cuda.empty_cache()
            C2, B2, T2, V2 = WORKLOADS[SECONDARY]
            r2, net2, x2, _ = timed_training(SECONDARY, args, device, rank, world, 400, 20)
            sec = {"config": "BASELINE configs[1]: %s" % SECONDARY, "value": r2["value"], "unit": "sequences/sec", "ms_per_step": r2["ms_per_step"],
                   "steps": 400, "timed_seconds": r2["seconds"], "capture_probe_ms": r2["capture_ms"], "loss": r2["loss"],
                   "step_roofline": step_roofline(C2, T2, V2, r2["value"])}
            if not args.no_eval:
                sec["eval_forward"] = eval_forward(net2, x2, 400, 20)
                if not args.no_cpu_baseline:       # BASELINE configs[0]: the same forward on the reference's CPU path
                    sec["eval_forward"]["cpu_baseline"] = cpu_forward_baseline(C2, B2, T2, V2)
            del net2
            if not args.no_cpu_baseline:
                sec["cpu_baseline"] = cpu_baseline(C2, B2, T2, V2, args.dropout, (8, 16, 32), 12.0)
            out["secondary"] = sec
            # BASELINE configs[4]'s per-GPU workload (CISTGCN-32, 25 joints) at one of its batch sizes, on this one GPU
            torch.cuda.empty_cache()
            r3, net3, _, _ = timed_training(AMASS25, args, device, rank, world, 60, 10)
            out["other_workloads"] = [{"config": "BASELINE configs[4] shape on one GPU: %s" % AMASS25, "value": r3["value"], "unit": "sequences/sec",
                                       "ms_per_step": r3["ms_per_step"], "steps": 60, "timed_seconds": r3["seconds"], "loss": r3["loss"],
                                       "step_roofline": step_roofline(*[WORKLOADS[AMASS25][i] for i in (0, 2, 3)], r3["value"])}]
            del net3
        if not args.no_dp_overhead:
            torch.cuda.empty_cache()
            from cistgcn_amd.models import CISTGCN_0
            torch.manual_seed(0)
            out["dp_overhead"] = dp_overhead(CISTGCN_0(*make_cfg(C, T, V, args.dropout)).to(device), device)
            out["dp_overhead_ms"] = out["dp_overhead"].get("ms")
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        sys.stdout.flush()
        os.write(REAL_STDOUT, (json.dumps(out) + "\n").encode())


if __name__ == "__main__":
    main()
