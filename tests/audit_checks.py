"""Operator checks that came out of seeding value errors into cistgcn_amd/csrc (tools/mutants.py, tests/MUTANTS.md): launch-plan
branches of the generic contraction that no other operator check reaches, equal maxima in the fused context heads, and the drivers of
the cases other families gained (channels whose variance is comparable to eps: `low_var=True` of the families' checks, LOW_VARIANCE
below; the dropout mask against its host restatement: checks.check_dropout(mask=True)), and rows wider than a wave in the ST-GCN stage.  Device-agnostic like tests/checks.py: "cpu" runs the kernels through the shim
(tests/test_emu_audit.py), "cuda" on the MI355X (tests/test_gpu_audit.py).  References: stock PyTorch in float64 on the same float32
values; bounds: the ones of check_contract / check_contract_kred / check_context_heads."""
import torch
import torch.nn as nn

import checks
from checks import _gen, _leaf, _rand, _run
from cistgcn_amd import ops
from helpers import assert_close

F64 = torch.float64
_DESC_FIELDS = ("G", "M", "N", "K", "splitk", "x_vec", "mode", "chain", "accumulate")


class PlanSpy:
    """records, while active, every launch plan the contractions ask for (ops._plan) and every descriptor that reaches cg_contract_many"""

    def __enter__(self):
        self.plans, self.descs, self.launches = [], [], []
        self._plan, self._call = ops._plan, ops._lib.call

        def plan(*a, **k):
            p = self._plan(*a, **k)
            self.plans.append(p)
            return p

        def call(name, *a):
            if name == "cg_contract_many":
                ds = [{f: getattr(a[0][i], f) for f in _DESC_FIELDS} for i in range(a[1])]
                self.descs += ds
                self.launches.append(ds)
            return self._call(name, *a)

        ops._plan, ops._lib.call = plan, call
        return self

    def __exit__(self, *exc):
        ops._plan, ops._lib.call = self._plan, self._call
        return False


def _forward_case(device, what, fn, inputs, expect, desc=None, rel=2e-5):
    """fn(contract, *leaves) -> y with contract = ops.contract (device run) or an einsum (+ bias) in float64 (reference): output and every
    input gradient at `rel` (gradients against max(1e-3, max|ref grad|): checks._run); `expect`: attributes of the launch plan of the
    FORWARD contraction (the first plan asked for), `desc`: fields of the descriptor that reached the launcher."""
    spy = PlanSpy()

    def dev(*ts):
        with spy:
            return fn(ops.contract, *ts)

    def ref_contract(spec, a, x, bias=None, bias_label=None):
        y = torch.einsum(spec, a, x)
        if bias is not None:
            shape = [1] * y.dim()
            shape[spec.split("->")[1].index(bias_label)] = -1
            y = y + bias.view(shape)
        return y

    _run(dev, lambda *ts: fn(ref_contract, *ts), inputs, device, rel=rel, what=what, ref_dtype=F64)
    p = spy.plans[0]
    for k, v in expect.items():
        got = getattr(p, k)
        assert (v(got) if callable(v) else got == v), "%s: the launch plan has %s = %r" % (what, k, got)
    for k, v in (desc or {}).items():
        assert spy.descs[0][k] == v, "%s: the descriptor has %s = %r" % (what, k, spy.descs[0][k])


def check_contract_edges(device):
    """Branches of the launch plan (ops._plan) and of the launcher (csrc/contract.hip) that the other operator checks do not reach; every case
    asserts the plan it was written for (mode, splitk, K, x_vec), so that a moved threshold fails here instead of testing something else."""
    g = _gen(101)
    many = lambda v: v > 1
    # split-K with a bias, thin (M <= 16) and matrix-core tile: the bias belongs to the first split only
    for O in (5, 40):
        _forward_case(device, "edges split-K + bias O=%d" % O, lambda c, w, x, b: c("oi,bi->bo", w, x, b, "o"),
                      [_rand(g, O, 300, scale=0.3), _rand(g, 3, 300), _rand(g, O)], dict(mode=0, splitk=many, K=300, M=O), rel=3e-5)
    # the shape that takes this path in the model at T = 50: 3x3 convolutions on an odd plane, K = 9 * 50 with a bias
    with PlanSpy() as spy:
        checks.check_dilated_convs(device, shapes=((2, 50, 25, 5, 5),))
    assert any(p.mode == 0 and p.K == 450 and p.splitk > 1 and p.M == 25 for p in spy.plans), "dilated convolutions: no split-K plan with K = 450"
    # a K range per workgroup above CG_KT = 2048: the k-offset tables are read from global memory (splitk == 1 needs >= 512 output tiles)
    _forward_case(device, "edges k tables in memory, thin", lambda c, a, x: c("gk,gk->g", a, x),
                  [_rand(g, 512, 2100, scale=0.2), _rand(g, 512, 2100)], dict(mode=0, splitk=1, K=2100, G=512, M=1))
    _forward_case(device, "edges k tables in memory, wide", lambda c, a, x: c("gmk,gkn->gmn", a, x),
                  [_rand(g, 512, 17, 2100, scale=0.2), _rand(g, 512, 2100, 3)], dict(mode=0, splitk=1, K=2100, G=512, M=17, N=3))
    # 31 splits of 65 -> the launcher rounds the chunk to 80: the last six splits start past K
    _forward_case(device, "edges empty trailing splits", lambda c, a, x: c("bko,bkc->oc", a, x),
                  [_rand(g, 1, 2000, 7, scale=0.2), _rand(g, 1, 2000, 5)], dict(mode=0, splitk=31, K=2000), rel=3e-5)
    # operands 4 bytes past a 16-byte boundary: the plan (tables only) says float4, the descriptor must not
    wv, xv = _rand(g, 40, 12, scale=0.3), _rand(g, 5, 12, 4, 8)
    pad = lambda t: torch.cat((torch.zeros(1), t.reshape(-1)))

    def x_off(c, w, buf):
        x = buf[1:].view(5, 12, 4, 8)
        assert buf.dtype != torch.float32 or (buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4)
        return c("oc,bchw->bohw", w, x)

    def w_off(c, buf, x):
        w = buf[1:].view(40, 12)
        assert buf.dtype != torch.float32 or w.data_ptr() % 16 == 4
        return c("oc,bchw->bohw", w, x)

    _forward_case(device, "edges x off alignment", x_off, [wv, pad(xv)], dict(mode=0, x_vec=1, M=40), desc=dict(x_vec=0))
    _forward_case(device, "edges w off alignment", w_off, [pad(wv), xv], dict(mode=0, x_vec=1, M=40), desc=dict(x_vec=1))
    # operands with a storage offset (channel slices of wider tensors)
    ws, xs = _rand(g, 40, 20, scale=0.3), _rand(g, 4, 20, 6, 8)
    _forward_case(device, "edges x slice", lambda c, w, x: c("oc,bchw->bohw", w, x[:, 4:16]), [wv, xs], dict(mode=0, K=12))
    _forward_case(device, "edges w slice", lambda c, w, x: c("oc,bchw->bohw", w[:, 3:15], x), [ws, _rand(g, 4, 12, 6, 8)], dict(mode=0, K=12))
    _forward_case(device, "edges both slices", lambda c, w, x: c("oc,bchw->bohw", w[:, 3:15], x[:, 4:16]), [ws, xs], dict(mode=0, K=12))
    # tile edges: a second tile of one row and one column; one column; one input / one output channel
    _forward_case(device, "edges 65x33x65", lambda c, a, x: c("mk,kn->mn", a, x), [_rand(g, 65, 33, scale=0.3), _rand(g, 33, 65)],
                  dict(mode=0, splitk=1, M=65, N=65, K=33))
    _forward_case(device, "edges 17x5x1", lambda c, a, x: c("mk,kn->mn", a, x), [_rand(g, 17, 5), _rand(g, 5, 1)], dict(mode=0, M=17, N=1, K=5))
    _forward_case(device, "edges C=1", lambda c, w, x: c("oc,bchw->bohw", w, x), [_rand(g, 9, 1), _rand(g, 3, 1, 5, 7)], dict(mode=0, K=1, M=9))
    _forward_case(device, "edges O=1", lambda c, w, x: c("oc,bchw->bohw", w, x), [_rand(g, 1, 10), _rand(g, 3, 10, 5, 7)], dict(mode=0, K=10, M=1))
    _check_many_chunks(device, g, (2, 6, 5, 7), stream=False)
    _check_many_chunks(device, g, (2, 6, 10, 16), stream=True)


def _check_many_chunks(device, g, xshape, stream):
    """19 pointwise maps of one shared input in one ops.contract_many (CG_MAX_BATCH = 16 problems per launch): outputs, every weight
    gradient, the accumulated input gradient.  stream: the large-tensor plan of check_contract_chain (no atomics into a shared buffer,
    streaming kernel from 64 positions on) - the 19 input gradients are chained streaming problems and a chain must end at the boundary of
    a launch (`same_chunk` in ops._contract_launch): 38 gradient problems, the input gradients at the odd places -> chains of 8, 8 and 3."""
    n = 19
    C = xshape[1]
    x0 = _rand(g, *xshape)
    ws = [_rand(g, 3 + (5 * i) % 11, C, scale=0.4) for i in range(n)]
    gys = [_rand(g, xshape[0], w.shape[0], *xshape[2:]) for w in ws]
    assert n > ops._MAX_CONTRACT_BATCH
    saved = (ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N)
    if stream:
        ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N = 0, 64
    try:
        xd, wd = _leaf(x0, device), [_leaf(w, device) for w in ws]
        ops.begin_step(device)
        with PlanSpy() as fwd:
            ys = [o[0] for o in ops.contract_many([("oc,bchw->bohw", w, xd, None, None, None) for w in wd])]
        with PlanSpy() as bwd:
            torch.autograd.backward(ys, [t.to(device) for t in gys])
    finally:
        ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N = saved
    what = "edges %d maps in one call%s" % (n, " (chained streams)" if stream else "")
    assert [len(l) for l in fwd.launches] == [16, 3], "%s: forward launches of %s problems" % (what, [len(l) for l in fwd.launches])
    assert [len(l) for l in bwd.launches] == [16, 16, 6], "%s: backward launches of %s problems" % (what, [len(l) for l in bwd.launches])
    assert all(d["mode"] == (1 if stream else 0) for d in fwd.descs), what + ": forward plan"
    links = [sum(1 for d in l if d["chain"]) for l in bwd.launches]
    if stream:
        assert links == [7, 7, 2], "%s: chain links per launch %s" % (what, links)
        assert all(d["mode"] == 1 for l in bwd.launches for d in l[1::2]), what + ": the input gradients do not stream"
    else:
        assert links == [0, 0, 0] and all(d["accumulate"] for l in bwd.launches for d in l[1::2]), what + ": the input gradients do not share one buffer"
    xr, wr = _leaf(x0.double(), "cpu"), [_leaf(w.double(), "cpu") for w in ws]
    yr = [torch.einsum("oc,bchw->bohw", w, xr) for w in wr]
    torch.autograd.backward(yr, [t.double() for t in gys])
    rel = 3e-5 if stream else 2e-5
    for i in range(n):
        assert_close(ys[i], yr[i], "%s y[%d]" % (what, i), rel=rel)
        assert_close(wd[i].grad, wr[i].grad, "%s dW[%d]" % (what, i), rel=rel, floor=max(1e-3, float(wr[i].grad.abs().max())))
    assert_close(xd.grad, xr.grad, what + " dx", rel=rel, floor=max(1e-3, float(xr.grad.abs().max())))


def tie_positions(P, b=0):
    """positions of the four maxima and the four minima of sample b among P positions, by the slices of ceil(P / 16) positions a wave of
    cg_ctx_heads_fwd_kernel scans: maxima - two inside one slice, then a pair on both sides of a later slice boundary; minima - a pair on
    both sides of the FIRST slice boundary (P = 1650: positions 103 and 104), then two inside a later slice.  The first maximum is the first
    of a pair inside a slice, the first minimum the last position of a slice."""
    per = (P + 15) // 16
    s = 2 + b % 3
    return ((s * per + 1, s * per + 3, 7 * per - 1, 7 * per), (per - 1, per, 11 * per, 11 * per + 1))


def check_context_ties(device, shapes=((3, 5, 12, 7), (2, 25, 66, 64))):
    """ops.context_heads with equal maxima: torch's nested .max(-1)[0].max(-1)[0] sends the gradient to the first maximum in flat order and
    the kernel promises the same (first arg-max inside a slice, slices merged in position order).  Every sample's maximum and minimum occur
    four times (tie_positions); head 0 has channels of both signs of w * gamma, so some channels peak at the maximum of x and some at its
    minimum.  Against the float64 modules at the bounds of checks.check_context_heads.  shapes: (B, H, W, C)."""
    from cistgcn_amd.models.CISTGCN.CISTGCN import Stage, _conv
    g = _gen(131)
    for (B, H, W, C) in shapes:
        P = H * W
        x0 = 1.5 + 3.0 * _rand(g, B, 1, H, W)
        flat = x0.view(B, P)
        for b in range(B):
            hi, lo = tie_positions(P, b)
            assert len(set(hi + lo)) == 8 and max(hi + lo) < P and len({p // W for p in hi}) > 1 and len({p // W for p in lo}) > 1
            top, bottom = flat[b].max() + 1.0, flat[b].min() - 1.0
            flat[b, list(hi)] = top
            flat[b, list(lo)] = bottom
        g0, g1 = _rand(g, B, C), _rand(g, B, C)

        def make():
            gg = _gen(900 + C)
            heads = []
            for k in range(2):
                hd = Stage(s0=_conv(1, C, 1), s1=nn.BatchNorm2d(C), s2=nn.PReLU())
                with torch.no_grad():
                    w = (0.3 + torch.rand(C, generator=gg)) * torch.tensor([1.0 if c % 2 == 0 else -1.0 for c in range(C)])
                    hd[0].weight.copy_(w.view(hd[0].weight.shape))
                    hd[1].weight.copy_(0.7 + 0.6 * torch.rand(C, generator=gg)); hd[1].bias.copy_(0.3 * torch.randn(C, generator=gg))
                    hd[1].running_mean.copy_(0.2 * torch.randn(C, generator=gg)); hd[1].running_var.copy_(0.5 + torch.rand(C, generator=gg))
                    hd[2].weight.fill_(0.15 + 0.2 * k)
                heads.append(hd)
            return nn.ModuleList(heads)

        for train in (True, False):
            what = "context ties B%d H%d W%d C%d %s" % (B, H, W, C, "train" if train else "eval")
            ref = make().double().train(train)
            xr = _leaf(x0.double(), "cpu")
            z0 = ref[0][2](ref[0][1](ref[0][0](xr)))
            r0, r1 = z0.max(-1)[0].max(-1)[0], ref[1][2](ref[1][1](ref[1][0](xr))).mean((2, 3))
            torch.autograd.backward([r0, r1], [g0.double(), g1.double()])
            # the reference's own arg-max is the first of the four in flat order, at the maximum or the minimum of x by the sign of w * gamma
            first = z0.detach().view(B, C, P).argmax(-1)
            for b in range(B):
                hi, lo = tie_positions(P, b)
                assert {int(first[b, c]) for c in range(0, C, 2)} == {hi[0]} and {int(first[b, c]) for c in range(1, C, 2)} == {lo[0]}, what
            net = make().to(device).train(train)
            xd = _leaf(x0, device)
            ops.begin_step(device)
            y0, y1 = ops.context_heads(xd, net[0], net[1], train)
            torch.autograd.backward([y0, y1], [g0.to(device), g1.to(device)])
            assert_close(y0, r0, what + " max", rel=2e-5)
            assert_close(y1, r1, what + " mean", rel=2e-5)
            assert_close(xd.grad, xr.grad, what + " dx", rel=5e-5, floor=max(1e-3, float(xr.grad.abs().max())))
            for (k, pa), (_, pb) in zip(net.named_parameters(), ref.named_parameters()):
                floor = max(1e-3, float(pb.grad.abs().max()))
                if train and k.endswith("0.weight"):          # in front of a train-mode BatchNorm: the remainder of cancelling sums (check_context_heads)
                    floor = max(floor, float(ref[int(k[0])][1].weight.grad.abs().max()))
                assert_close(pa.grad, pb.grad, "%s grad %s" % (what, k), rel=5e-5, floor=floor)


# ---- channels whose variance is comparable to eps: one small case per family that applies a BatchNorm ------------------------------
def _low_var_norm_act(device):
    checks._check_norm_act_shape(device, True, 5, 7, low_var=True)          # odd rows: scalar path
    checks._check_norm_act_shape(device, True, 4, 6, low_var=True)          # float4 rows


def _low_var_norm_act_many(device):
    """three row problems of different shapes in one launch (as check_batched_ops), channels 0 and 1 of each at LOW_VAR_BATCH, train and
    eval mode, against float64 modules"""
    g = _gen(141)
    shapes = [(4, 6, 4, 7), (4, 3, 1, 9), (6, 5)]
    xs = [checks._low_var_input(_rand(g, *sh, scale=2.0) + 0.5) for sh in shapes]
    gy = [_rand(g, *sh) for sh in shapes]
    for train in (True, False):
        bns_ref = [nn.BatchNorm2d(6), nn.BatchNorm2d(3), nn.BatchNorm1d(5)]
        prs_ref = [nn.PReLU(), None, nn.PReLU(5)]
        for bn in bns_ref:
            with torch.no_grad():
                bn.weight.copy_(1 + 0.3 * _rand(g, bn.num_features)); bn.bias.copy_(0.3 * _rand(g, bn.num_features))
                bn.running_mean.copy_(0.2 * _rand(g, bn.num_features))
            checks._low_var_running(bn)
        bns_dev = [type(b)(b.num_features) for b in bns_ref]
        prs_dev = [None if p is None else type(p)(p.num_parameters).to(device) for p in prs_ref]
        for a, b in zip(bns_dev, bns_ref):
            a.load_state_dict(b.state_dict())
            a.to(device).train(train); b.double().train(train)
        prs_ref = [None if p is None else p.double() for p in prs_ref]
        xd, xr = [_leaf(t, device) for t in xs], [_leaf(t.double(), "cpu") for t in xs]
        ops.begin_step(device)
        yd = ops.norm_act_many([dict(x=xd[i], bn=bns_dev[i], train=train, prelu=prs_dev[i]) for i in range(3)])
        yr = [(prs_ref[i](bns_ref[i](xr[i])) if prs_ref[i] is not None else bns_ref[i](xr[i])) for i in range(3)]
        torch.autograd.backward(yd, [t.to(device) for t in gy])
        torch.autograd.backward(yr, [t.double() for t in gy])
        for i in range(3):
            what = "norm_act_many low variance %s %d" % ("train" if train else "eval", i)
            assert_close(yd[i], yr[i], what + " y", rel=2e-5)
            assert_close(xd[i].grad, xr[i].grad, what + " dx", rel=2e-5, floor=max(1e-3, float(xr[i].grad.abs().max())))
            assert_close(bns_dev[i].weight.grad, bns_ref[i].weight.grad, what + " dgamma", rel=2e-5, floor=max(1e-3, float(bns_ref[i].weight.grad.abs().max())))
            assert_close(bns_dev[i].running_var, bns_ref[i].running_var, what + " running_var", rel=2e-5)


def _low_var_block_mid(device):
    import block_mid_checks
    block_mid_checks.check_low_variance(device)


LOW_VARIANCE = (
    ("norm_act", _low_var_norm_act),
    ("norm_act_many", _low_var_norm_act_many),
    ("dstd_tail", lambda device: checks.check_dstd_tail(device, shapes=((3, 20, 7, 9),), low_var=True)),
    ("map2adj_tail", lambda device: checks.check_map2adj_tail(device, shapes=((3, 7, 9),), low_var=True)),
    ("block_input", lambda device: checks.check_block_input(device, shapes=((3, 5, 4, 6, 3), (2, 6, 5, 5, 2)), low_var=True)),
    ("gate_head", lambda device: checks.check_gate_head(device, shapes=((5, 8, 10, 2),), low_var=True)),
    ("block_mid", _low_var_block_mid),
    ("tower_maps", lambda device: checks.check_tower_maps(device, shapes=((3, 10, (5, 5, 5, 5), 7, 8),), low_var=True)),
    ("tower_collapse", lambda device: checks.check_tower_collapse(device, shapes=((3, 10, (8, 8, 8, 8), 6, 8, 5),), low_var=True)),
    ("context_heads", lambda device: checks.check_context_heads(device, shapes=((3, 5, 12, 7),), low_var=True)),
)


def check_low_variance(device, family):
    dict(LOW_VARIANCE)[family](device)


def check_stgcn_wide_rows(device):
    """ops.stgcn_domain with rows of 70 joints and 16 channels: the second-generation matrix-core kernels (csrc/stgcn_domain_mfma.hip) refuse
    rows wider than a wave, so the time-domain forward falls to the first-generation matrix-core kernel of csrc/stgcn_domain.hip, which no
    other operator check reaches (tools/mutants.py, row stgcn-mfma1-bias-sign: the sign of its bias could be flipped unnoticed).  The
    smallest such shape, both domains, forward and every gradient, at the bounds of checks.check_stgcn_domain."""
    checks.check_stgcn_domain(device, shapes=((2, 16, 16, 3, 70),), planes=None)
