"""Constant rows, channels and samples in the block statistics (DSTD_GC._get_stats_, CISTGCN.py:360-371): the two kernel families that
compute them, ops.dstd_stats (csrc/stages.hip) and ops.block_input (csrc/block_input.hip), and the whole model on a batch with a dead
coordinate or a padded sample.  At a standard deviation of exactly 0 the function has a kink; torch's std_backward takes the sub-gradient
0 there and its Welford update gives exactly 0 on equal values, so float64 autograd on the same float32 values is finite and is the
reference throughout.  The constants are non-dyadic on purpose: the sum of 22 copies of 0.7f is not 22 x 0.7f, and a kernel that divides
a plain sum sees a std of 1e-8 where the reference sees 0.
Device-agnostic like tests/checks.py: "cpu" runs the kernels through the shim (tests/test_emu_degenerate.py), "cuda" on the MI355X
(tests/test_gpu_degenerate.py).  tests/MUTANTS.md, "Constant rows, channels and samples", has the measured figures."""
import torch
import torch.nn as nn

import checks
from checks import _gen, _leaf, _rand, _run, assert_within_stock
from cistgcn_amd import ops
from helpers import assert_close
from oracle import cistgcn_ref as O

# (B, C, T, V): small case | the first block's shape | one wave per row | rows wider than a wave (strided tail of cg_stats_rows) | the 16-wave workgroup
DSTD_SHAPES = ((3, 4, 5, 6), (2, 10, 10, 22), (2, 3, 4, 40), (2, 3, 2, 70), (2, 8, 50, 22))


class _Stds:
    """the four standard deviations inside block_stats, in the type of x"""

    def __init__(self, x):
        self.row = x.std(3)              # (B, C, T)
        self.ch = x.std((3, 2))          # (B, C)
        self.t = self.row.std(1)         # (B, T): over c of the row stds
        self.g = self.ch.std(1)          # (B,): over c of the channel stds


def _dstd_patterns(C, T, V):
    """name -> (edit of sample 0 in place, the stds that are exactly 0 afterwards, the stds that stay positive).  Every other sample
    keeps its dense noise."""
    c1, t1, c2, t2 = C - 1, T - 1, 1, 0

    def rows(x, g):
        x[0, c1, t1] = 0.7
        x[0, c2, t2] = 0.0

    def channel(x, g):
        x[0, c2] = 0.3

    def zero_sample(x, g):
        x[0] = 0.0

    def constant_channels(x, g):
        x[0] = (0.1 + 0.37 * torch.arange(C, dtype=torch.float32)).view(C, 1, 1)

    def equal_rows(x, g):
        x[0, :, t1] = x[0, 0, t1].clone()

    def copied_channels(x, g):
        x[0] = x[0, 0].clone()

    def near_row(x, g):
        x[0, c1, t1] = 0.7 + 1e-6 * _rand(g, V)

    everything = lambda s: [s.row[0], s.ch[0], s.t[0], s.g[0]]
    return (
        ("a constant rows", rows, lambda s: [s.row[0, c1, t1], s.row[0, c2, t2]], lambda s: [s.t[0], s.g[0]]),
        ("b constant channel", channel, lambda s: [s.ch[0, c2], s.row[0, c2]], lambda s: [s.t[0], s.g[0]]),
        ("c zero sample", zero_sample, everything, lambda s: []),
        ("c constant channels", constant_channels, everything, lambda s: []),
        ("d equal rows at one t", equal_rows, lambda s: [s.t[0, t1]], lambda s: [s.row[0, :, t1], s.g[0]]),
        ("e copied channels", copied_channels, lambda s: [s.g[0], s.t[0]], lambda s: [s.row[0], s.ch[0]]),
        ("f nearly constant row", near_row, None, lambda s: [s.row[0, c1, t1]]),
    )


def _assert_reference_zeros(x, zeros, positive, what):
    """the preconditions: exact zeros at the degenerate places in float64 AND float32 torch, the rest alive"""
    for dt in (torch.float64, torch.float32):
        s = _Stds(x.to(dt))
        for z in (zeros(s) if zeros else []):
            assert z.numel() and bool((z == 0).all()), "%s: precondition: the reference's own std (%s) is not exactly 0 there: %s" % (what, dt, z.flatten()[:4])
        for p in positive(s):
            assert p.numel() and bool((p > 0).all()), "%s: precondition: a std that should be alive is 0 in the reference (%s)" % (what, dt)


def _assert_exact_zeros(y, ref, T, what, expect_some):
    """every std entry of the statistics that is exactly 0.0 in the reference is exactly 0.0 from the kernel"""
    got, r = y.detach().cpu()[:, 1 + T:], ref.detach()[:, 1 + T:]
    zero = r == 0
    assert bool(zero.any()) == expect_some, "%s: the reference has %d zero std outputs" % (what, int(zero.sum()))
    assert bool((got[zero] == 0).all()), "%s: %d std outputs are exactly 0 in the reference and not in the kernel (largest %.3e)" % (
        what, int((got[zero] != 0).sum()), float(got[zero].abs().max()))


def check_dstd_stats_degenerate(device, shapes=DSTD_SHAPES, patterns="abcdef"):
    """ops.dstd_stats against float64 autograd of the oracle's block_stats, one pattern per call in sample 0.  a-e: the family's bound
    (checks._run, rel 2e-5) on the output and on dx (NaN fails it), exact zeros where the reference has them.  f: the row is alive and
    ill-conditioned: dx is held to checks.assert_within_stock (4 x stock float32, half-ulp floor), the output to the family's bound."""
    for shape in shapes:
        B, C, T, V = shape
        for i, (name, edit, zeros, positive) in enumerate(_dstd_patterns(C, T, V)):
            if name[0] not in patterns:
                continue
            g = _gen(7000 + 10 * sum(shape) + i)
            x = _rand(g, *shape)
            edit(x, g)
            what = "dstd_stats %s %s" % (shape, name)
            _assert_reference_zeros(x, zeros, positive, what)
            x64 = _leaf(x.double(), "cpu")
            r64 = O.CISTGCN.block_stats(x64)
            gy = _rand(_gen(99), *r64.shape)
            if zeros is not None:
                r64.backward(gy.double())
                assert bool(torch.isfinite(x64.grad).all()), "%s: precondition: the reference gradient is not finite" % what
                _run(ops.dstd_stats, O.CISTGCN.block_stats, [x], device, what=what, ref_dtype=torch.float64)
                with torch.no_grad():
                    ops.begin_step(device)
                    y = ops.dstd_stats(x.to(device))
                _assert_exact_zeros(y, r64, T, what, expect_some=name[0] in "cde")
                continue

            def run(xl, dtype):
                y = (O.CISTGCN.block_stats if dtype is not None else ops.dstd_stats)(xl)
                y.backward(gy.to(y.device, y.dtype))
                return {"y": y, "dx": xl.grad}

            def kernel():
                ops.begin_step(device)
                return run(_leaf(x, device), None)

            assert_within_stock(what, kernel, lambda dtype, ratios: run(_leaf(x.to(dtype), "cpu"), dtype),
                                lambda n, refs: 2e-5 * max(1.0, float(refs[n].detach().abs().max())) if n == "y" else float("inf"))


# ---- block input ---------------------------------------------------------------------------------------------------------------
BLOCK_INPUT_SHAPES = ((3, 5, 4, 6, 3), (2, 10, 10, 22, 7))          # (B, C, T, V, n aliases)
# the issue's five, and one more: with the five alone the masks of the two stds over c never decide anything in this family (wherever
# those stds are 0 the channel and row stds are 0 too), and the centred mean over c meets nothing but zeros.  "copied channels": every
# channel of x a copy of channel 0 under a BatchNorm whose channels share one set of parameters, so that xn has equal, live channels
BLOCK_INPUT_PATTERNS = ("zero channel", "constant channel", "gamma 0", "zero sample", "constant row", "copied channels")


def check_block_input_degenerate(device, shapes=BLOCK_INPUT_SHAPES, patterns=BLOCK_INPUT_PATTERNS):
    """ops.block_input against nn.BatchNorm2d(...).double() + the oracle's block_stats on inputs whose normalised form has constant rows,
    channels or samples; gradient layout and bounds of checks.check_block_input, the floor of the dx bound taken per channel (a dead
    channel's dx carries 1 / sqrt(eps) = 316: one floor over the tensor would hold the live channels 300 x looser than their own check)."""
    g = _gen(73)
    for (B, C, T, V, n) in shapes:
        cd, cl, bz, tr = 2, C - 1, B - 1, T - 1          # the dead channel (z of (x, y, z)), a live one, the padded sample, the row
        for pattern in patterns:
            for train in (True, False):
                for given_stats in ((False, True) if train else (False,)):
                    def make(dt=torch.float32):
                        gg = _gen(400 + C)
                        bn = nn.BatchNorm2d(C)
                        with torch.no_grad():
                            bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=gg)); bn.bias.copy_(0.3 * torch.randn(C, generator=gg))
                            bn.running_mean.copy_(0.2 * torch.randn(C, generator=gg)); bn.running_var.copy_(0.5 + torch.rand(C, generator=gg))
                            if pattern == "gamma 0":
                                bn.weight[cl] = 0.0
                            if pattern == "copied channels":
                                for p in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
                                    p.copy_(p[:1].expand(C).clone())
                        return bn.to(dt)
                    x0 = 0.7 + 2.0 * _rand(g, B, C, T, V)
                    if pattern == "zero channel":
                        x0[:, cd] = 0.0
                    elif pattern == "constant channel":
                        x0[:, cd] = 0.7
                    elif pattern == "zero sample":
                        x0[bz] = 0.0
                    elif pattern == "constant row":
                        x0[0, cl, tr] = 0.7
                    elif pattern == "copied channels":
                        x0 = x0[:, :1].expand(B, C, T, V).contiguous()
                    gxs = [_rand(g, B, C, T, V) if i != 1 else None for i in range(n)]          # one consumer without a gradient
                    gst = [_rand(g, B, 2 + 2 * T), _rand(g, B, 7 + 2 * T)[:, 3:5 + 2 * T]]         # the second one: a column slice (the gate inputs' gradient)
                    what = "block_input %s B%d C%d T%d V%d %s%s" % (pattern, B, C, T, V, "train" if train else "eval", " (sums given)" if given_stats else "")
                    # reference in fp64
                    ref = make(torch.float64).train(train)
                    xr = _leaf(x0.double(), "cpu")
                    xnr = ref(xr)
                    sr = O.CISTGCN.block_stats(xnr)
                    s = _Stds(xnr.detach())
                    dead = {"zero channel": [s.ch[:, cd]], "constant channel": [s.ch[:, cd]], "gamma 0": [s.ch[:, cl]],
                            "zero sample": [s.row[bz], s.ch[bz], s.t[bz], s.g[bz]], "constant row": [s.row[0, cl, tr]], "copied channels": [s.t, s.g]}[pattern]
                    for z in dead:
                        assert bool((z == 0).all()), "%s: precondition: the reference's own std is not exactly 0 at the degenerate place" % what
                    if pattern == "copied channels":
                        assert bool((s.row > 0).all()) and bool((s.ch > 0).all()), "%s: precondition: the rows and channels are alive" % what
                    torch.autograd.backward([xnr, sr], [sum(t.double() for t in gxs if t is not None), (gst[0] + gst[1]).double()])
                    assert bool(torch.isfinite(xr.grad).all()), "%s: precondition: the reference gradient is not finite" % what
                    # HIP
                    bn = make().to(device).train(train)
                    xd = _leaf(x0, device)
                    ops.begin_step(device)
                    stats = None
                    if given_stats:
                        stats = ops._arena(device).take(2 * C * ops._lib.STAT_REPLICAS)
                        xc = x0.double()
                        stats.view(ops._lib.STAT_REPLICAS, C, 2)[3] = torch.stack((xc.sum((0, 2, 3)), (xc * xc).sum((0, 2, 3))), 1).to(device)
                    xs, (sa, sb) = ops.block_input(xd, bn, train, n, stats=stats)
                    outs = [t for t, gg_ in zip(xs, gxs) if gg_ is not None] + [sa, sb]
                    torch.autograd.backward(outs, [gg_.to(device) for gg_ in gxs if gg_ is not None] + [t.to(device) for t in gst])
                    for t in xs:
                        assert_close(t, xnr, what + " xn", rel=2e-5)
                    assert_close(sa, sr, what + " statistics", rel=2e-5)
                    assert_close(sb, sr, what + " statistics (2)", rel=2e-5)
                    for st, name in ((sa, " statistics"), (sb, " statistics (2)")):
                        _assert_exact_zeros(st, sr, T, what + name, expect_some=pattern in ("zero sample", "copied channels"))
                    for c in range(C):
                        assert_close(xd.grad[:, c], xr.grad[:, c], "%s dx channel %d" % (what, c), rel=5e-5, floor=max(1e-3, float(xr.grad[:, c].abs().max())))
                    if pattern == "gamma 0":
                        assert bool((xd.grad[:, cl] == 0).all()), "%s: dx of the channel with gamma = 0 is not exactly 0" % what
                    assert_close(bn.weight.grad, ref.weight.grad, what + " dgamma", rel=5e-5)
                    assert_close(bn.bias.grad, ref.bias.grad, what + " dbeta", rel=5e-5)
                    for (k, ba), (_, bb) in zip(bn.named_buffers(), ref.named_buffers()):
                        assert_close(ba.float(), bb.float(), "%s buffer %s" % (what, k), rel=1e-5)


# ---- whole model ---------------------------------------------------------------------------------------------------------------
def _dead_z(x):
    x[..., 2] = 0
    return x


def _padded_sample(x):
    x[x.shape[0] - 1] = 0
    return x


MODEL_EDITS = {"z=0": _dead_z, "padded-sample": _padded_sample}
MODEL_CASES = [(edit, fused, mode) for edit in MODEL_EDITS for fused in (True, False) for mode in ("train", "eval")]


def check_model_degenerate(device, edit, fused, mode):
    """CISTGCN-8 (T = 10, V = 22, B = 4), kink-free: every gradient as accurate against the float64 oracle as the float32 oracle is (x 8:
    the rule of checks.check_model_vs_oracle(smooth=True)), on a planar batch (z = 0) and on a batch whose last sample is padding"""
    checks.check_model_vs_oracle(device, 8, 10, 22, 4, mode, fused=fused, smooth=True, edit=MODEL_EDITS[edit])


KERNEL_CHECKS = (check_dstd_stats_degenerate, check_block_input_degenerate)
