"""Channels far off centre (|mean| / std = 30 and 300, checks.OFF_CENTRE) in every operator that sums BatchNorm statistics or hands sums to
a later BatchNorm.  The library forms every train-mode statistic as E[x^2] - E[x]^2 (csrc/cg_bn.h), safe only while squares and sums are
carried in float64 per element; the families' own data is centred and an f32 partial sum passes there.  One case per family at its
smallest shape and at the small shape whose lanes or waves visit the most tiles, train mode everywhere and eval mode where the family
has it (eval forms no sums: it pins `v - mean`).  Bound: checks.assert_within_stock - 4 x the error of stock float32 PyTorch against
float64 on the same float32 values, on top of the family's own bound, and stock float32 inside the family's bound before the kernel runs.
Device-agnostic like tests/checks.py: "cpu" runs the kernels through the shim (tests/test_emu_audit.py), "cuda" on the MI355X
(tests/test_gpu_audit.py).  tests/MUTANTS.md, "Off-centre channels and non-finite gradients", has the measured ratios."""
import contextlib
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import checks
import loop_shapes as L
from audit_checks import PlanSpy
from checks import (OFF_CENTRE, _chan_sums, _gen, _leaf, _off_centre_input, _off_centre_rows, _off_centre_running, _rand, _ratio_ok,
                    assert_within_stock)
from cistgcn_amd import _lib, ops
from oracle import cistgcn_ref as O

F64 = torch.float64

# the second ratio a family runs at: -300 unless stock float32 itself leaves the family's bound there (the precondition of
# assert_within_stock), then -100; tests/MUTANTS.md lists the families stepped down and the figure that did it
SECOND_RATIO = {"collapse_cols": -100.0, "context_heads": -100.0, "gate_head": -100.0, "map2adj_tail": -100.0, "dstd_tail": -100.0, "tower_maps": -100.0, "tower_collapse": -100.0}


def _ratios(family):
    return (OFF_CENTRE[0], SECOND_RATIO.get(family, OFF_CENTRE[1]))


def _rel(rel, floor=1.0):
    """the bound of helpers.assert_close: rel * max(floor, max|ref|)"""
    return lambda ref: rel * max(floor, float(ref.abs().max()) if ref.numel() else 0.0)


def _moments(sums, cnt):
    """(mean, biased variance) per channel from the [C * 2] f64 {sum, sum of squares}: what a BatchNorm that consumes the sums forms"""
    s = sums.detach().cpu().double().view(-1, 2)
    mean = s[:, 0] / cnt
    return mean, s[:, 1] / cnt - mean * mean


def _stat_dims(y):
    return tuple(d for d in range(y.dim()) if d != 1)


def _stock_moments(y):
    d = _stat_dims(y)
    return y.mean(d), y.var(d, unbiased=False)


# the moments a later BatchNorm derives from emitted sums end in its running buffers: held to the bound of those buffers in every family
_MOMENT_BOUND = _rel(1e-5)


@contextlib.contextmanager
def _planes(planes):
    """the kernel generation of ops.stgcn_domain pinned as in checks.check_stgcn_domain: True the plane kernels, None the tile / matrix-core
    kernels, False the default switch"""
    lib = _lib.lib()
    prev = lib.cg_stgcn_domain_planes_min_workgroups((1 << 40) if planes is None else 1 if planes else -1)
    if planes is None or planes:
        assert lib.cg_stgcn_domain_planes_min_workgroups(-1) == ((1 << 40) if planes is None else 1), "the kernel-generation switch is locked: run the tests with CISTGCN_ABLATION=1"
    try:
        yield
    finally:
        lib.cg_stgcn_domain_planes_min_workgroups(prev)


# ---- operators that hand {sum, sum of squares} to a later BatchNorm: output, mean and biased variance from the sums -------------------
def _emitter_case(device, what, family, build, run_dev, run_ref, y_bound):
    """build(ratios) -> float32 operands of the case; run_dev(operands on the device) -> (y, f64 sums); run_ref(operands in a dtype) -> y"""
    def stock(dtype, ratios):
        y = run_ref([t.to(dtype) for t in build(ratios)])
        mean, var = _stock_moments(y)
        return {"y": y, "mean": mean, "var": var}

    def kernel():
        ops.begin_step(device)
        y, st = run_dev([t.to(device) for t in build(_ratios(family))])
        mean, var = _moments(_chan_sums(st), y.numel() // y.shape[1])
        return {"y": y, "mean": mean, "var": var}

    assert_within_stock(what, kernel, stock, lambda name, refs: (y_bound if name == "y" else _MOMENT_BOUND)(refs[name].detach()), _ratios(family))


def check_stgcn_stats(device, variant):
    """ops.stgcn_domain(want_stats=True), both domains; the bias carries the offset (the stage's own input stays as generated)"""
    shapes, planes = {"tile": (((3, 10, 8, 5, 7),) + L.STGCN_TILE, None), "mfma1": (((2, 16, 16, 3, 70),), None),
                      "mfma2": (((2, 18, 16, 5, 7),) + L.STGCN_MFMA, None), "planes": ((checks.PLANE_SHAPES[-2],) + L.STGCN_PLANES, True)}[variant]
    g = _gen(307)
    with _planes(planes):
        for (B, Cin, Cout, T, V) in shapes:
            for domain in (0, 1):
                x = _rand(g, B, Cin, T, V)
                adj = _rand(g, B, V, T, T, scale=0.3) if domain == 0 else _rand(g, B, T, V, V, scale=0.3)
                w, b0 = _rand(g, Cout, Cin, scale=0.3), _rand(g, Cout)
                spec = "bctv,bvtq->bcqv" if domain == 0 else "bctv,btvw->bctw"
                ref = lambda ts: torch.einsum("oc,bchw->bohw", ts[2], torch.einsum(spec, ts[0], ts[1])) + ts[3].view(1, -1, 1, 1)
                y0 = ref([t.double() for t in (x, adj, w, torch.zeros(Cout))])

                def build(ratios):
                    b = b0.clone()
                    for c, r in enumerate(ratios):
                        b[c] = r * float(y0[:, c].std(unbiased=False))
                    for c, r in enumerate(ratios):
                        _ratio_ok(ref([t.double() for t in (x, adj, w, b)])[:, c], r, "stgcn_domain output channel %d" % c)
                    return [x, adj, w, b]

                _emitter_case(device, "stgcn_stats off centre %s B%d Cin%d Cout%d T%d V%d dom%d" % (variant, B, Cin, Cout, T, V, domain), "stgcn_" + variant,
                              build, lambda ts: ops.stgcn_domain(ts[0], ts[1], ts[2], ts[3], domain, want_stats=True), ref, _rel(5e-5))


def check_contract_stats(device):
    """ops.contract_stats without a bias (constants on two input channels) and with one: the thin and the matrix-core tile of the tiled
    kernel, and a position count that takes the streaming kernel"""
    g = _gen(311)
    for (B, C, Oc, H, W), stream in (((3, 6, 5, 5, 7), False), ((3, 12, 40, 5, 7), False), ((2, 6, 10, 16, 40), True)):
        x0, w = _rand(g, B, C, H, W), _rand(g, Oc, C, scale=0.3)
        for biased in (False, True):
            conv = nn.Conv2d(C, Oc, 1, bias=biased)
            with torch.no_grad():
                conv.weight.copy_(w.view(Oc, C, 1, 1))

            def build(ratios):
                x = _off_centre_rows(conv, ratios=ratios, x=x0)
                return [conv.weight.detach().view(Oc, C).clone(), x] + ([conv.bias.detach().clone()] if biased else [])

            def dev(ts):
                saved = (ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N)
                if stream:
                    ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N = 0, 64
                try:
                    with PlanSpy() as spy:
                        y, st = ops.contract_stats("oc,bchw->bohw", ts[0], ts[1], ts[2] if biased else None, "o" if biased else None)
                finally:
                    ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N = saved
                assert st is not None and spy.plans[0].mode == (1 if stream else 0), "the plan has mode %d%s" % (spy.plans[0].mode, "" if st is not None else " and no sums")
                return y, st

            ref = lambda ts: torch.einsum("oc,bchw->bohw", ts[0], ts[1]) + (ts[2].view(1, -1, 1, 1) if biased else 0.0)
            _emitter_case(device, "contract_stats off centre B%d C%d O%d H%d W%d%s%s" % (B, C, Oc, H, W, " +bias" if biased else "", " stream" if stream else ""),
                          "contract_stats", build, dev, ref, _rel(2e-5))


def check_pointwise_stats(device):
    """ops.pointwise_maps(want_stats=True): biases on every map carry the offsets"""
    g = _gen(313)
    for (B, C, Ms, T, V) in (checks.check_pointwise_maps.__defaults__[0][0],) + L.POINTWISE_MAPS[:1]:
        x0 = _rand(g, B, C, T, V)
        convs = [nn.Conv2d(C, M, 1) for M in Ms]
        for conv in convs:
            with torch.no_grad():
                conv.weight.copy_(0.3 * _rand(g, *conv.weight.shape))
        for k in range(len(Ms)):
            def build(ratios):
                for conv in convs:
                    _off_centre_rows(conv, ratios=ratios, x=x0)
                return [x0] + [c.weight.detach().view(c.out_channels, C).clone() for c in convs] + [c.bias.detach().clone() for c in convs]

            n = len(Ms)
            dev = lambda ts: ops.pointwise_maps(ts[0], ts[1:1 + n], want_stats=True, biases=ts[1 + n:])[k]
            ref = lambda ts: torch.einsum("oc,bchw->bohw", ts[1 + k], ts[0]) + ts[1 + n + k].view(1, -1, 1, 1)
            _emitter_case(device, "pointwise_maps off centre B%d C%d M%s T%d V%d map %d" % (B, C, Ms, T, V, k), "pointwise_maps", build, dev, ref, _rel(2e-5))


def check_collapse_stats(device, cols):
    """ops.collapse_rows / collapse_cols(want_stats=True): no bias - constants on two input channels"""
    g = _gen(317)
    first = (checks.check_collapse_cols if cols else checks.check_collapse_rows).__defaults__[0][0]
    for (B, C, T, V, Oc) in (first,) + (L.COLLAPSE_COLS if cols else L.COLLAPSE_ROWS)[:1]:
        x0 = _rand(g, B, C, T, V)
        conv = nn.Conv2d(C, Oc, (1, V) if cols else (T, 1), bias=False)
        with torch.no_grad():
            conv.weight.copy_(0.2 * _rand(g, *conv.weight.shape))

        def build(ratios):
            return [_off_centre_rows(conv, ratios=ratios, x=x0), conv.weight.detach().clone()]

        def dev(ts):
            w = ts[1].view(Oc, C, -1)
            assert (ops.collapse_cols_ok if cols else ops.collapse_rows_ok)(ts[0], w)
            return (ops.collapse_cols if cols else ops.collapse_rows)(ts[0], w, want_stats=True)

        ref = lambda ts: F.conv2d(ts[0], ts[1]).squeeze(3 if cols else 2)
        _emitter_case(device, "collapse_%s off centre B%d C%d T%d V%d O%d" % ("cols" if cols else "rows", B, C, T, V, Oc), "collapse_cols" if cols else "collapse_rows", build, dev, ref, _rel(2e-5))


def check_norm_act_emit(device):
    """ops.norm_act(emit_stats=True): the sums of the OUTPUT, which the next BatchNorm consumes - the gated residual form of the DSTD_GC tail
    (x * pre + add behind it), the addend off centre"""
    g = _gen(331)
    for (B, C, T, V) in ((4, 6, 5, 7),) + L.NORM_ACT_ROWS:
        x0, pre, add0 = _rand(g, B, C, T, V), _rand(g, B, C), _rand(g, B, C, T, V)
        y0 = x0.double() * pre.double()[:, :, None, None] + add0.double()

        def build(ratios):
            add = add0.clone()
            for c, r in enumerate(ratios):
                add[:, c] = (add0[:, c].double() + r * float(y0[:, c].std(unbiased=False))).float()
                _ratio_ok(x0[:, c].double() * pre.double()[:, c, None, None] + add[:, c].double(), r, "norm_act output channel %d" % c)
            return [x0, pre, add]

        _emitter_case(device, "norm_act emit off centre B%d C%d T%d V%d" % (B, C, T, V), "norm_act_emit", build,
                      lambda ts: ops.norm_act(ts[0], pre=ts[1], add=ts[2], add_post=True, emit_stats=True),
                      lambda ts: ts[0] * ts[1][:, :, None, None] + ts[2], _rel(2e-5))


def check_dstd_stats(device):
    """ops.dstd_stats (means and standard deviations of a block's input, no BatchNorm sums: two passes over a row in LDS): output and
    gradient on off-centre channels.  The family's own gradient bound is already max(2e-5, 4 x stock float32) (glue_checks.check_dstd_stats:
    statistics over a few channels are ill-conditioned in float32), so the stock bound stands alone there."""
    import glue_shapes as G
    g = _gen(337)
    for shape in ((3, 5, 6, 7), G.DSTD_STATS_LDS):
        x0 = _rand(g, *shape)
        gy = _rand(g, shape[0], 2 + 2 * shape[2])

        def run(x, dtype):
            y = (O.CISTGCN.block_stats if dtype is not None else ops.dstd_stats)(x)
            y.backward(gy.to(y.device, y.dtype))
            return {"y": y, "dx": x.grad}

        stock = lambda dtype, ratios: run(_leaf(_off_centre_input(x0, ratios=ratios).to(dtype), "cpu"), dtype)
        kernel = lambda: run(_leaf(_off_centre_input(x0, ratios=_ratios("dstd_stats")), device), None)
        assert_within_stock("dstd_stats off centre %s" % (shape,), kernel, stock, lambda name, refs: _rel(2e-5)(refs[name].detach()) if name == "y" else float("inf"),
                            _ratios("dstd_stats"))


# ---- families that apply a BatchNorm: outputs, every gradient, running buffers -------------------------------------------------------
PARAM_FACTOR_AT_SIZE = 8.0


def _chain_case(device, what, family, train, make, forward_ref, forward_dev, gouts, bound, at_size=False):
    """at_size (the loop shapes, B > 64): every parameter gradient is one sum over 20 000 .. 1 000 000 terms, which stock PyTorch adds
    pairwise and the kernels in the order of their tiles and atomics; the project's factor for such sums against stock float32 is 8
    (checks._assert_tail_grads, test_gradients_as_accurate_as_cpu_fp32), measured here: tower_maps dgamma 4.4 x, dstd_tail dgamma 5.1 x,
    both inside the family's own bound.
    make(ratios) -> (nn.Module on the CPU in float32, [float32 inputs]) of the case; forward_ref(module, leaves) / forward_dev(module,
    leaves) -> list of outputs (stock modules | the operator), differentiated with `gouts`; compared: every output, the gradient of every
    input and parameter, every buffer.  bound(name, refs) -> the family's own absolute bound."""
    def collect(mod, leaves, outs):
        torch.autograd.backward(list(outs), [g_.to(o.device, o.dtype) for g_, o in zip(gouts, outs)])
        res = {"out %d" % i: o for i, o in enumerate(outs)}
        res.update({"d input %d" % i: t.grad for i, t in enumerate(leaves) if t.grad is not None})
        res.update({"grad " + k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
        res.update({"buffer " + k: b for k, b in mod.named_buffers()})
        return {k: v.detach().cpu().clone() for k, v in res.items()}

    def stock(dtype, ratios):
        mod, ins = make(ratios)
        mod = mod.to(dtype).train(train)
        leaves = [_leaf(t.to(dtype), "cpu") for t in ins]
        return collect(mod, leaves, forward_ref(mod, leaves))

    def kernel():
        mod, ins = make(_ratios(family))
        mod = mod.to(device).train(train)
        leaves = [_leaf(t, device) for t in ins]
        ops.begin_step(device)
        return collect(mod, leaves, forward_dev(mod, leaves))

    factors = None
    if at_size:
        mod, _ = make(_ratios(family))
        factors = {"grad " + k: PARAM_FACTOR_AT_SIZE for k, _ in mod.named_parameters()}
    assert_within_stock(what, kernel, stock, bound, _ratios(family), factors)


def _std_bound(out_rel=2e-5, grad_rel=5e-5, buf_rel=1e-5, gamma_floor=None, alone=False):
    """the bounds the families share: outputs out_rel * max(1, max|ref|), gradients grad_rel * max(1e-3, max|ref|), buffers buf_rel *
    max(1, max|ref|); gamma_floor(name) -> the name of the BatchNorm weight whose gradient is the floor of a gradient in front of that
    train-mode BatchNorm (the remainder of cancelling sums, as in the families' own checks).  alone: the map in front of the BatchNorm has
    no bias, so its INPUT carries the offset and its weight gradient is the remainder of sums of terms 30 .. 300 times the size of the
    data's: stock float32 itself misses the family's bound there at either ratio (gate_head: 2.2e-2 against 4.7e-4; map2adj_tail: 2.8e-2
    against 1.2e-3), and the quantity is held to 4 x stock float32 alone."""
    def bound(name, refs):
        ref = refs[name].double()
        if name.startswith("out"):
            return _rel(out_rel)(ref)
        if name.startswith("buffer"):
            return _rel(buf_rel)(ref)
        floor = max(1e-3, float(ref.abs().max()))
        other = gamma_floor(name) if gamma_floor else None
        if other is not None and alone:
            return None
        if other is not None:
            floor = max(floor, float(refs[other].abs().max()))
        return grad_rel * floor
    return bound


def _bn_init(bn, gg):
    C = bn.num_features
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=gg)); bn.bias.copy_(0.3 * torch.randn(C, generator=gg))
        bn.running_mean.copy_(0.2 * torch.randn(C, generator=gg)); bn.running_var.copy_(0.5 + torch.rand(C, generator=gg))
    return bn


def check_norm_act(device):
    """ops.norm_act: the row kernels sum their own statistics (csrc/rowops.hip); plain, and with the gate factor and an addend"""
    for (B, C, T, V) in ((4, 6, 5, 7), (4, 6, 4, 6)) + L.NORM_ACT_ROWS:          # odd rows: scalar path | rows of 24 floats: float4 path | several samples per workgroup
        g = _gen(341)
        x0, pre, add = _rand(g, B, C, T, V, scale=3.0) + 1.5, 1.0 + 0.1 * _rand(g, B, C), _rand(g, B, C, T, V)
        gy = [_rand(g, B, C, T, V)]
        for train in (True, False):
            for gated in (False, True):
                def make(ratios):
                    mod = nn.ModuleList([_bn_init(nn.BatchNorm2d(C), _gen(343)), nn.PReLU(C)])
                    with torch.no_grad():
                        mod[1].weight.copy_(torch.linspace(0.1, 0.4, C))
                    x = _off_centre_input(x0, ratios=ratios)
                    if not train:
                        _off_centre_running(mod[0], ratios, x.double() * pre.double()[:, :, None, None] if gated else x)
                    return mod, [x] + ([pre, add] if gated else [])

                ref = lambda m, ts: [m[1](m[0](ts[0] * ts[1][:, :, None, None]) + ts[2]) if gated else m[1](m[0](ts[0]))]
                dev = lambda m, ts: [ops.norm_act(ts[0], bn=m[0], train=train, prelu=m[1], **(dict(pre=ts[1], add=ts[2]) if gated else {}))]
                _chain_case(device, "norm_act off centre B%d C%d T%d V%d %s%s" % (B, C, T, V, "train" if train else "eval", " gated" if gated else ""),
                            "norm_act", train, make, ref, dev, gy, _std_bound(2e-5, 2e-5, 2e-5), at_size=B > 64)


def check_norm_act_many(device):
    """three row problems of different shapes in one launch (as audit_checks._low_var_norm_act_many)"""
    g = _gen(347)
    shapes = [(4, 6, 4, 7), (4, 3, 1, 9), (6, 5)]
    xs0 = [_rand(g, *sh, scale=2.0) + 0.5 for sh in shapes]
    gy = [_rand(g, *sh) for sh in shapes]
    for train in (True, False):
        def make(ratios):
            gg = _gen(349)
            bns = [_bn_init(bn, gg) for bn in (nn.BatchNorm2d(6), nn.BatchNorm2d(3), nn.BatchNorm1d(5))]
            xs = [_off_centre_input(x, ratios=ratios) for x in xs0]
            if not train:
                for bn, x in zip(bns, xs):
                    _off_centre_running(bn, ratios, x)
            return nn.ModuleList(bns + [nn.PReLU(), nn.PReLU(5)]), xs

        ref = lambda m, ts: [m[3](m[0](ts[0])), m[1](ts[1]), m[4](m[2](ts[2]))]
        dev = lambda m, ts: ops.norm_act_many([dict(x=ts[0], bn=m[0], train=train, prelu=m[3]), dict(x=ts[1], bn=m[1], train=train),
                                               dict(x=ts[2], bn=m[2], train=train, prelu=m[4])])
        _chain_case(device, "norm_act_many off centre %s" % ("train" if train else "eval"), "norm_act_many", train, make, ref, dev, gy, _std_bound(2e-5, 2e-5, 2e-5))


def check_block_input(device):
    """ops.block_input: the BatchNorm of a block's input sums its own statistics (csrc/block_input.hip) and hands the normalised planes'
    means and deviations on"""
    for (B, C, T, V, n) in (checks.check_block_input.__defaults__[0][0],) + L.BLOCK_INPUT[:1]:
        g = _gen(353)
        x0 = 0.7 + 2.0 * _rand(g, B, C, T, V)
        gouts = [_rand(g, B, C, T, V) for _ in range(n)] + [_rand(g, B, 2 + 2 * T), _rand(g, B, 2 + 2 * T)]
        for train in (True, False):
            def make(ratios):
                bn = _bn_init(nn.BatchNorm2d(C), _gen(359))
                x = _off_centre_input(x0, ratios=ratios)
                if not train:
                    _off_centre_running(bn, ratios, x)
                return bn, [x]

            def ref(bn, ts):
                xn = bn(ts[0])
                s = O.CISTGCN.block_stats(xn)
                return [xn] * n + [s, s]

            def dev(bn, ts):
                xs, (sa, sb) = ops.block_input(ts[0], bn, train, n)
                return list(xs) + [sa, sb]

            _chain_case(device, "block_input off centre B%d C%d T%d V%d %s" % (B, C, T, V, "train" if train else "eval"), "block_input", train, make, ref, dev,
                        gouts, _std_bound(2e-5, 5e-5, 1e-5), at_size=B > 64)


def check_context_heads(device):
    """ops.context_heads: Conv2d(1, C, 1) without a bias, so every channel of w[c] * x has the |mean| / std of x itself and the sign of
    w[c]; x goes off centre (ratio 30, then the family's second ratio), the channels split by sign"""
    from cistgcn_amd.models.CISTGCN.CISTGCN import Stage, _conv
    for (B, H, W, C) in checks.check_context_heads.__defaults__[0][:2]:
        g = _gen(367)
        x0 = 3.0 * _rand(g, B, 1, H, W)
        gouts = [_rand(g, B, C), _rand(g, B, C)]
        for which in (0, 1):
            for train in (True, False):
                def make(ratios):
                    gg = _gen(373)
                    heads = []
                    for k in range(2):
                        hd = Stage(s0=_conv(1, C, 1), s1=_bn_init(nn.BatchNorm2d(C), gg), s2=nn.PReLU())
                        with torch.no_grad():
                            hd[0].weight.copy_(torch.randn(hd[0].weight.shape, generator=gg) * 0.7)
                            hd[2].weight.fill_(0.15 + 0.2 * k)
                        heads.append(hd)
                    x = x0.double()
                    x = (x + ratios[which] * float(x.std(unbiased=False))).float()
                    _ratio_ok(x, ratios[which], "context_heads input")
                    if not train and ratios[which]:
                        with torch.no_grad():
                            for hd in heads:          # the running statistics of w[c] * x: the channels they meet
                                w = hd[0].weight.detach().double().view(C)
                                hd[1].running_var.copy_(w * w * float(x.double().var(unbiased=False)))
                                hd[1].running_mean.copy_(ratios[which] * torch.sign(w) * hd[1].running_var.double().sqrt())
                    return nn.ModuleList(heads), [x]

                ref = lambda m, ts: [m[0][2](m[0][1](m[0][0](ts[0]))).max(-1)[0].max(-1)[0], m[1][2](m[1][1](m[1][0](ts[0]))).mean((2, 3))]
                dev = lambda m, ts: list(ops.context_heads(ts[0], m[0], m[1], train))
                # the weight in front of a train-mode BatchNorm: stock alone (_std_bound; here 2.9e-4 against 2.1e-4 even at ratio 10)
                gf = (lambda name: "grad %s.1.weight" % name.split()[1][0] if name.endswith(".0.weight") else None) if train else None
                bound = _std_bound(2e-5, 5e-5, 1e-5, gf, alone=True)
                _chain_case(device, "context_heads off centre B%d H%d W%d C%d ratio %d %s" % (B, H, W, C, which, "train" if train else "eval"), "context_heads", train, make, ref,
                            dev, gouts, bound)


def _tower(C, Ms, gg, col=None, linear=False):
    """maps of a tower level, every one with a bias (it carries the offset): Conv2d(C, M, 1) -> BatchNorm2d -> PReLU [-> collapsing conv].
    linear (the loop shapes): PReLU slopes of 1 - among 200 000 and more pre-activations float32 and float64 take different branches
    (checks.BranchLog) and stock float32 is 0.1 .. 0.2 off in dx for that reason alone; with slope 1 a branch changes nothing, and the sums
    under test sit in front of the PReLU."""
    mods = []
    for k, M in enumerate(Ms):
        conv, bn, pr = nn.Conv2d(C, M, 1, bias=True), _bn_init(nn.BatchNorm2d(M), gg), nn.PReLU()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gg) * 0.4)
            conv.bias.copy_(0.3 * torch.randn(M, generator=gg))
            pr.weight.fill_(1.0 if linear else 0.1 + 0.1 * k)
        seq = [conv, bn, pr]
        if col is not None:
            T, V, Oc = col
            cc = nn.Conv2d(M, Oc, (T, 1) if k % 2 == 0 else (1, V), bias=False)
            with torch.no_grad():
                cc.weight.copy_(torch.randn(cc.weight.shape, generator=gg) * 0.2)
            seq.append(cc)
        mods.append(nn.Sequential(*seq))
    return nn.ModuleList(mods)


def _tower_gamma_floor(train):
    return (lambda name: "grad %s.1.weight" % name.split()[1].split(".")[0] if (name.endswith(".0.weight") or name.endswith(".0.bias")) else None) if train else None


def check_tower_maps(device):
    """ops.tower_maps: pointwise maps whose epilogue sums the statistics of their BatchNorm (csrc/tower_maps.hip)"""
    for (B, C, Ms, T, V) in (checks.check_tower_maps.__defaults__[0][0],) + L.TOWER_MAPS:
        g = _gen(379)
        x0 = 0.3 + _rand(g, B, C, T, V)
        gouts = [_rand(g, B, M, T, V) for M in Ms]
        for train in (True, False):
            def make(ratios):
                net = _tower(C, Ms, _gen(383), linear=B > 64)
                for m in net:
                    _off_centre_rows(m[0], ratios=ratios, x=x0)
                    if not train:
                        _off_centre_running(m[1], ratios, F.conv2d(x0.double(), m[0].weight.detach().double(), m[0].bias.detach().double()))
                return net, [x0]

            ref = lambda net, ts: [m(ts[0]) for m in net]
            dev = lambda net, ts: ops.tower_maps(ts[0], [m[0].weight.view(m[0].out_channels, C) for m in net], [m[1] for m in net], [m[2] for m in net], train,
                                                 biases=[m[0].bias for m in net])
            _chain_case(device, "tower_maps off centre B%d C%d M%s T%d V%d %s" % (B, C, Ms, T, V, "train" if train else "eval"), "tower_maps", train, make, ref, dev, gouts,
                        _std_bound(2e-5, 5e-5, 1e-5, _tower_gamma_floor(train)), at_size=B > 64)


def check_tower_collapse(device):
    """the tower level deferred into its collapsing convolutions (ops.tower_maps(defer=True) + ops.collapse_rows / collapse_cols with the
    BatchNorm + PReLU applied on load)"""
    for (B, C, Ms, T, V, Oc) in (checks.check_tower_collapse.__defaults__[0][0],) + L.TOWER_COLLAPSE:
        g = _gen(389)
        x0 = 0.3 + _rand(g, B, C, T, V)
        gouts = [_rand(g, B, Oc, 1, V) if k % 2 == 0 else _rand(g, B, Oc, T, 1) for k in range(len(Ms))]
        for train in (True, False):
            def make(ratios):
                net = _tower(C, Ms, _gen(397), col=(T, V, Oc), linear=B > 64)
                for m in net:
                    _off_centre_rows(m[0], ratios=ratios, x=x0)
                    if not train:
                        _off_centre_running(m[1], ratios, F.conv2d(x0.double(), m[0].weight.detach().double(), m[0].bias.detach().double()))
                return net, [x0]

            def dev(net, ts):
                ys, trs = ops.tower_maps(ts[0], [m[0].weight.view(m[0].out_channels, C) for m in net], [m[1] for m in net], [m[2] for m in net], train,
                                         biases=[m[0].bias for m in net], defer=True)
                outs = []
                for k, m in enumerate(net):
                    w = m[3].weight.view(Oc, m[3].in_channels, -1)
                    if k % 2 == 0:
                        outs.append(ops.collapse_rows(ys[k], w, transform=trs[k])[0].unsqueeze(2))
                    else:
                        outs.append(ops.collapse_cols(ys[k], w, transform=trs[k])[0].unsqueeze(3))
                return outs

            _chain_case(device, "tower_collapse off centre B%d C%d M%s T%d V%d O%d %s" % (B, C, Ms, T, V, Oc, "train" if train else "eval"), "tower_collapse", train, make,
                        lambda net, ts: [m(ts[0]) for m in net], dev, gouts, _std_bound(3e-5, 5e-5, 1e-5, _tower_gamma_floor(train)), at_size=B > 64)


def check_block_mid(device):
    import block_mid_checks
    block_mid_checks.check_off_centre(device)


def check_gate_head(device):
    """ops.gate_head: BatchNorm2d on z (the input goes off centre), BatchNorm1d behind a Linear without a bias, whose input is cat(h2,
    statistics): constants on the statistics' columns - the one input of that map the case owns - put rows 0 and 1 of every path on the
    ratios (minimum-norm solution over all columns, one system for all paths: they share the statistics)"""
    from cistgcn_amd.models.CISTGCN.CISTGCN import Stage
    for (B, C, S, n) in (checks.check_gate_head.__defaults__[0][0], checks.check_gate_head.__defaults__[0][1]):
        g = _gen(401)
        z0 = [0.5 + 1.5 * _rand(g, B, C) for _ in range(n)]
        wide0 = _rand(g, B, S + 5)
        gouts = [_rand(g, B, C) for _ in range(n)]
        for train in (True, False):
            def first_half(mod, zs):
                return [mod[0][k][7](mod[0][k][5](z.view(B, C, 1, 1)).view(B, C)) for k, z in enumerate(zs)]

            def make(ratios):
                gg = _gen(409)
                convs, maps = [], []
                for k in range(n):
                    conv = Stage(s5=_bn_init(nn.BatchNorm2d(C), gg), s7=nn.PReLU())
                    mp = Stage(s0=nn.Linear(C + S, C, bias=False), s1=_bn_init(nn.BatchNorm1d(C), gg), s3=nn.PReLU(), s4=nn.Linear(C, C, bias=False))
                    with torch.no_grad():
                        mp[0].weight.copy_(torch.randn(mp[0].weight.shape, generator=gg) * 0.3); mp[4].weight.copy_(torch.randn(C, C, generator=gg) * 0.3)
                        conv[7].weight.fill_(0.1 + 0.1 * k); mp[3].weight.fill_(0.3 - 0.1 * k)
                    convs.append(conv); maps.append(mp)
                mod = nn.ModuleList([nn.ModuleList(convs), nn.ModuleList(maps)])
                zs = [_off_centre_input(z, ratios=ratios) for z in z0]
                if not train:
                    for k in range(n):
                        _off_centre_running(convs[k][5], ratios, zs[k])
                wide = wide0.clone()
                if any(ratios):
                    m64 = copy.deepcopy(mod).double().train(train)
                    with torch.no_grad():
                        h2 = first_half(m64, [z.double() for z in zs])
                        rows, tgt = [], []
                        for k in range(n):
                            y = F.linear(torch.cat((h2[k], wide.double()[:, 2:2 + S]), 1), m64[1][k][0].weight)
                            for c in range(2):
                                rows.append(m64[1][k][0].weight[c, C:])
                                tgt.append(ratios[c] * float(y[:, c].std(unbiased=False)) - float(y[:, c].mean()))
                        A, t = torch.stack(rows), torch.tensor(tgt, dtype=F64)
                        d = A.t() @ torch.linalg.solve(A @ A.t(), t)
                        wide[:, 2:2 + S] = (wide.double()[:, 2:2 + S] + d).float()
                        for k in range(n):
                            y = F.linear(torch.cat((h2[k], wide.double()[:, 2:2 + S]), 1), m64[1][k][0].weight)
                            for c in range(2):
                                _ratio_ok(y[:, c], ratios[c], "gate_head path %d Linear row %d" % (k, c))
                            if not train:
                                _off_centre_running(maps[k][1], ratios, y)
                return mod, zs + [wide]

            def ref(mod, ts):
                h2 = first_half(mod, ts[:n])
                return [mod[1][k][4](mod[1][k][3](mod[1][k][1](mod[1][k][0](torch.cat((h2[k], ts[n][:, 2:2 + S]), 1))))) for k in range(n)]

            dev = lambda mod, ts: ops.gate_head(ts[:n], [ts[n][:, 2:2 + S]] * n, list(mod[0]), list(mod[1]), train, drop_p=0.0, salts=[(3 + k, 11 + k) for k in range(n)])
            gf = (lambda name: "grad 1.%s.1.weight" % name.split()[1].split(".")[1] if (name.startswith("grad 1.") and name.endswith(".0.weight")) else None) if train else None
            _chain_case(device, "gate_head off centre B%d C%d S%d x%d %s" % (B, C, S, n, "train" if train else "eval"), "gate_head", train, make, ref, dev, gouts,
                        _std_bound(3e-5, 5e-5, 1e-5, gf, alone=True))


def check_map2adj_tail(device):
    """ops.map2adj_tail: the expansors' first convolution has no bias and its input is the rank-1 seed the kernel forms itself, so a constant
    input channel k is s[:, k, :] = d, q[:, :, k] = 1 (space tower; the time tower alike): the two channels of checks._off_centre_pair become
    constants that put channels 0 and 1 of the BatchNorm on the ratios.  Second shape: (131, 50, 3), the longest `for (w ...)` loop of a wave
    in the M1 phase (eight tiles of 256 positions per workgroup: sixteen rounds per wave), over which the per-lane sums run.  There the
    PReLU slopes are 1: among a million pre-activations float32 and float64 take different branches (checks.BranchLog) and stock float32 is
    1.3 off in the input gradients for that reason alone; with slope 1 a branch changes nothing, and the sums under test sit in front of it."""
    from cistgcn_amd.models.CISTGCN.CISTGCN import Stage, _conv
    for (B, T, V) in (checks.check_map2adj_tail.__defaults__[0][0], L.MAP2ADJ_TAIL[-1]):
        g = _gen(419)
        data0 = [_rand(g, B, V, T), _rand(g, B, T, V), _rand(g, B, V, T), _rand(g, B, T, V)]
        gouts = [_rand(g, B, V, T, T), _rand(g, B, T, V, V)]
        seeds = lambda ts: (torch.einsum("bvt,bxv->bvtx", ts[0], ts[1]), torch.einsum("bvt,btw->btvw", ts[2], ts[3]))
        for train in (True, False):
            def make(ratios):
                gg = _gen(421)
                exps = []
                for ch in (V, T):
                    e = Stage(s0=_conv(ch, ch), s1=_bn_init(nn.BatchNorm2d(ch), gg), s3=nn.PReLU(), s4=_conv(ch, ch))
                    with torch.no_grad():
                        e[0].weight.copy_(0.4 * torch.randn(e[0].weight.shape, generator=gg)); e[4].weight.copy_(0.4 * torch.randn(e[4].weight.shape, generator=gg))
                        e[3].weight.fill_(1.0 if B > 64 else 0.2 + 0.1 * len(exps))
                    exps.append(e)
                data = [t.clone() for t in data0]
                for i, e in enumerate(exps):
                    s, q = data[2 * i], data[2 * i + 1]
                    k0, _, k1, _ = checks._off_centre_pair(e[0], seeds(data)[i], ratios)
                    for k in (k0, k1):          # the two channels empty first: their constants are then the whole channel
                        if i == 0:
                            s[:, k, :] = 0.0; q[:, :, k] = 1.0
                        else:
                            s[:, :, k] = 0.0; q[:, k, :] = 1.0
                    _, d0, _, d1 = checks._off_centre_pair(e[0], seeds(data)[i], ratios, pair=(k0, k1))
                    for k, d in ((k0, d0), (k1, d1)):
                        if i == 0:
                            s[:, k, :] = d
                        else:
                            s[:, :, k] = d
                    y = F.conv2d(seeds([t.double() for t in data])[i], e[0].weight.detach().double())
                    for c in range(2):
                        _ratio_ok(y[:, c], ratios[c], "map2adj_tail tower %d channel %d" % (i, c))
                    if not train:
                        _off_centre_running(e[1], ratios, y)
                return nn.ModuleList(exps), data

            ref = lambda mod, ts: [e[4](e[3](e[1](e[0](o)))) for e, o in zip(mod, seeds(ts))]
            dev = lambda mod, ts: list(ops.map2adj_tail([(0, ts[0], ts[1]), (1, ts[2], ts[3])], list(mod), train, drop_p=0.0, salts=(5, 6)))
            gf = (lambda name: "grad %s.1.weight" % name.split()[1][0] if name.endswith(".0.weight") else None) if train else None
            if B > 64:          # every parameter gradient is one sum over a million terms: the family's own check holds those to a multiple of
                gf = lambda name: "grad 0.1.weight" if name.startswith("grad") else None          # stock float32 at this size (checks._assert_tail_grads)
            _chain_case(device, "map2adj_tail off centre B%d T%d V%d %s" % (B, T, V, "train" if train else "eval"), "map2adj_tail", train, make, ref, dev, gouts,
                        _std_bound(2e-5, 5e-5, 1e-5, gf, alone=True), at_size=B > 64)


def check_dstd_tail(device):
    """ops.dstd_tail, all five BatchNorms.  tcn1 / tcn2 (sums handed over by the producer): y1 / y2 go off centre.  prelu1 / prelu2 (the
    kernel sums w * x itself): the residual addends r1 / r2 carry the offset through the PReLU in front (one branch for the whole channel)
    and the gate columns 0 and 1 are 1 + 1e-4 n (a gate of unit spread would turn the offset into spread).  compressor (no bias, summed in
    the matrix phase): the constants of checks._off_centre_pair on two of its input channels are the betas of prelu1 / prelu2 there - a
    parameter in front of the map, not its input; a negative constant flips the sign of its weight column instead, so that the PReLU in
    between passes it.  The slopes of the two PReLUs whose input carries the offset (keys 5 and 6) are sums of terms 30 .. 300 times the
    data's size: stock float32 misses the family's bound on them at either ratio (1.7e-2 against 3.6e-4 at -100) - stock alone.
    Second shape: (523, 16, 6, 13), three and four tiles per workgroup in the matrix phases.  It puts 650 000 elements through five
    PReLUs, where stock float32 takes other branches than float64 (checks.BranchLog) and is 0.4 off in the input gradients for that reason
    alone: the slopes are 1 at that shape - a branch changes nothing then, and every sum under test sits in front of a PReLU."""
    from cistgcn_amd.models.layers.SE import SELayer2d
    for (B, C, T, V) in (checks.check_dstd_tail.__defaults__[0][0], (4, 16, 6, 6), L.DSTD_TAIL[1]):          # (4, 16, 6, 6): T V % 4 == 0, the float4 row path
        g = _gen(431)
        data0 = [_rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C), _rand(g, B, C), _rand(g, B, C, T, V)]
        for w in data0[4:6]:
            w[:, :2] = 1.0 + 1e-4 * w[:, :2]
        gouts = [_rand(g, B, C, T, V)]
        for train in (True, False):
            def pre(m, ts, i):
                return m[i](ts[i]) + ts[2 + i]

            def acts(m, ts):
                return torch.cat([m[7 + i](m[2 + i](ts[4 + i][:, :, None, None] * m[5 + i](pre(m, ts, i)))) for i in range(2)], 1)

            def ref(m, ts):
                h = m[9](m[4](m[10](acts(m, ts))))
                gate = torch.sigmoid(F.linear(F.relu(F.linear(h.mean((2, 3)), m[11].w1)), m[11].w2))
                return [h * gate[:, :, None, None] + ts[6]]

            def make(ratios):
                gg = _gen(433)
                bns = [_bn_init(nn.BatchNorm2d(C), gg) for _ in range(5)]
                al = [nn.PReLU() for _ in range(5)]
                conv, se = nn.Conv2d(2 * C, C, 1, bias=False), SELayer2d(C, reduction=8)
                with torch.no_grad():
                    for i, a in enumerate(al):
                        a.weight.fill_(1.0 if B > 64 else 0.1 + 0.07 * i)
                    conv.weight.copy_(0.3 * torch.randn(conv.weight.shape, generator=gg))
                    se.w1.copy_(0.5 * torch.randn(se.w1.shape, generator=gg)); se.w2.copy_(0.5 * torch.randn(se.w2.shape, generator=gg))
                mod = nn.ModuleList(bns + al + [conv, se])
                data = [t.clone() for t in data0]
                data[0], data[1] = _off_centre_input(data[0], ratios=ratios), _off_centre_input(data[1], ratios=ratios)
                f64 = lambda: (copy.deepcopy(mod).double().train(train), [t.double() for t in data])
                with torch.no_grad():
                    for i in range(2):
                        if not train:
                            _off_centre_running(bns[i], ratios, data[i])
                        u = pre(*f64(), i)
                        for c, r in enumerate(ratios):
                            data[2 + i][:, c] = (data[2 + i][:, c].double() + r * float(u[:, c].std(unbiased=False))).float()
                        m, ts = f64()
                        wx = ts[4 + i][:, :, None, None] * m[5 + i](pre(m, ts, i))
                        for c, r in enumerate(ratios):
                            _ratio_ok(wx[:, c], r, "dstd_tail gated activation %d channel %d" % (i, c))
                        if not train:
                            _off_centre_running(bns[2 + i], ratios, wx)
                    if any(ratios):
                        cand = [k for k in range(2 * C) if k % C >= 2]
                        pair = None
                        for _ in range(3):
                            m, ts = f64()
                            k0, d0, k1, d1 = checks._off_centre_pair(conv, acts(m, ts), ratios, cand, pair)
                            pair = (k0, k1)
                            for k, d in ((k0, d0), (k1, d1)):
                                beta = bns[2 + k // C].bias
                                beta[k % C] += d
                                if float(beta[k % C]) < 0:
                                    beta[k % C] = -beta[k % C]
                                    conv.weight[:, k] = -conv.weight[:, k]
                    m, ts = f64()
                    h0 = m[10](acts(m, ts))
                    for c, r in enumerate(ratios):
                        _ratio_ok(h0[:, c], r, "dstd_tail compressor output channel %d" % c)
                    if not train:
                        _off_centre_running(bns[4], ratios, h0)
                return mod, data

            def dev(m, ts):
                def sums(y):
                    st = ops._arena(torch.device(device)).take(2 * C * _lib.STAT_REPLICAS)
                    yc = y.detach().double()
                    st.view(_lib.STAT_REPLICAS, C, 2)[0].copy_(torch.stack((yc.sum((0, 2, 3)), (yc * yc).sum((0, 2, 3))), 1))
                    return st
                out, _ = ops.dstd_tail([ts[0], ts[1]], [sums(ts[0]), sums(ts[1])] if train else [None, None], [ts[2], ts[3]], (ts[4], ts[5]), list(m[:5]), list(m[5:10]),
                                       m[10].weight, m[11], ts[6], train, drop_p=0.0, salts=(7, 9), emit_stats=train)
                return [out]

            slopes = ("grad 5.weight", "grad 6.weight")          # their input carries the offset, in eval mode too
            gf = lambda name: "grad 4.weight" if (name in slopes or (train and name == "grad 10.weight")) else None
            if B > 64:          # as in check_map2adj_tail: sums over 650 000 terms, held to stock float32 by the family's own check at this size
                gf = lambda name: "grad 4.weight" if name.startswith("grad") else None
            _chain_case(device, "dstd_tail off centre B%d C%d T%d V%d %s" % (B, C, T, V, "train" if train else "eval"), "dstd_tail", train, make, ref, dev, gouts,
                        _std_bound(2e-5, 5e-5, 1e-5, gf, alone=True), at_size=B > 64)


# name -> check(device): the families of audit_checks.LOW_VARIANCE, then the operators that hand sums to a later BatchNorm
OFF_CENTRE_CASES = (
    ("norm_act", check_norm_act),
    ("norm_act_many", check_norm_act_many),
    ("dstd_tail", check_dstd_tail),
    ("map2adj_tail", check_map2adj_tail),
    ("block_input", check_block_input),
    ("gate_head", check_gate_head),
    ("block_mid", check_block_mid),
    ("tower_maps", check_tower_maps),
    ("tower_collapse", check_tower_collapse),
    ("context_heads", check_context_heads),
    ("stgcn_stats_tile", lambda device: check_stgcn_stats(device, "tile")),
    ("stgcn_stats_mfma1", lambda device: check_stgcn_stats(device, "mfma1")),
    ("stgcn_stats_mfma2", lambda device: check_stgcn_stats(device, "mfma2")),
    ("stgcn_stats_planes", lambda device: check_stgcn_stats(device, "planes")),
    ("contract_stats", check_contract_stats),
    ("pointwise_stats", check_pointwise_stats),
    ("collapse_rows_stats", lambda device: check_collapse_stats(device, False)),
    ("collapse_cols_stats", lambda device: check_collapse_stats(device, True)),
    ("dstd_stats", check_dstd_stats),
    ("norm_act_emit", check_norm_act_emit),
)


def check_off_centre(device, name):
    dict(OFF_CENTRE_CASES)[name](device)
