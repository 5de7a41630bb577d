"""Checks of the glue operators: (A) the operand contract of the public wrappers in cistgcn_amd/ops.py and (B) the glue kernels on
the shapes of tests/glue_shapes.py against stock PyTorch on the CPU in float64.  Device-agnostic like tests/checks.py: "cpu" runs the
kernel sources through the CPU shim (tests/test_emu_glue.py), "cuda" the real library on the MI355X (tests/test_gpu_glue.py).

Bounds are those of tests/checks.py (outputs 2e-5, the SE gate 3e-5, gradients against max(1e-3, max|ref grad|)); the exceptions are
derived where they are used."""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import glue_shapes as G
import loop_shapes as L
from checks import _gen, _leaf, _rand, _run
from cistgcn_amd import _lib, ops
from helpers import assert_close
from oracle import cistgcn_ref as O
from oracle import eval_ref as E

F64 = torch.float64


# =====================================================================================================================
# A. operand contract: a tensor operand a wrapper cannot read as it is (float64, a strided view, an expanded or transposed upstream
#    gradient) either raises TypeError / ValueError before anything is launched, or gives the bits of the contiguous float32 call
# =====================================================================================================================
class Case:
    """one small valid call: `tensors` are its float32 operands in the order `call` takes them (a list of device tensors -> output or
    tuple of outputs); `f64` names the operands whose native type is float64 (their wrong type is float32); `index` holds
    integer-list operands, passed to `call` as a second argument"""

    def __init__(self, name, tensors, call, f64=(), index=None, backward=True):
        self.name, self.tensors, self.call, self.f64, self.index, self.backward = name, tensors, call, set(f64), index, backward


def _bn(C, device, seed):
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * _rand(_gen(seed), C))
        bn.bias.copy_(0.2 * _rand(_gen(seed + 1), C))
    return bn.to(device)


def _prelu(C, device):
    pr = nn.PReLU(C)
    with torch.no_grad():
        pr.weight.copy_(torch.linspace(0.1, 0.4, C))
    return pr.to(device)


def _sums(x):
    """replicated f64 channel sums of x (B,C,H,W), as the contraction epilogues emit them"""
    st = torch.zeros(_lib.STAT_REPLICAS, x.shape[1], 2, dtype=F64)
    st[0, :, 0] = x.double().sum((0, 2, 3))
    st[0, :, 1] = (x.double() ** 2).sum((0, 2, 3))
    return st.reshape(-1)


def contract_cases():
    """B = 2 everywhere: where a kernel adds one float per sample or workgroup onto zeroed memory, two terms commute and the bits do not
    depend on the order the workgroups arrive in.  Odd rows (15 positions): every call takes the scalar row path, with and without a
    strided operand."""
    g = _gen(31)
    sh = (2, 3, 3, 5)
    x = _rand(g, *sh)

    def norm_act(ts, _, **kw):
        dev = ts[0].device
        return ops.norm_act(ts[0], bn=_bn(3, dev, 5), train=True, prelu=_prelu(3, dev), **kw)

    def many(ts, _):
        outs = ops.contract_many([("oc,bchw->bohw", ts[0], ts[1], ts[2], "o", "o"), ("oc,bchw->bohw", ts[3], ts[1], ts[4], "o", None)])
        return outs[0][0], outs[1][0]

    return [
        Case("se_gate", [_rand(g, 2, 6), _rand(g, 2, 6), _rand(g, 6, 2)], lambda ts, _: ops.se_gate(*ts)),
        Case("cumsum_time", [_rand(g, *sh)], lambda ts, _: ops.cumsum_time(ts[0])),
        Case("dstd_stats", [_rand(g, *sh)], lambda ts, _: ops.dstd_stats(ts[0])),
        Case("cat_channels", [_rand(g, *sh), _rand(g, 2, 2, 3, 5), _rand(g, 2, 2)], lambda ts, _: ops.cat_channels(ts, bcast=(False, False, True))),
        Case("add3", [_rand(g, 2, 2, 3, 5), _rand(g, 2, 2, 3, 5), _rand(g, 2, 1, 3, 5)], lambda ts, _: ops.add3(*ts)),
        Case("norm_act add pre", [x, _rand(g, 2, 3), _rand(g, *sh)], lambda ts, _: norm_act(ts, _, pre=ts[1], add=ts[2])),
        Case("norm_act stats", [x, _sums(x)], lambda ts, _: norm_act(ts, _, stats=ts[1]), f64=(1,)),
        Case("norm_act_many", [x, _rand(g, *sh), _rand(g, 2, 3)],
             lambda ts, _: tuple(ops.norm_act_many([dict(x=ts[0], bn=_bn(3, ts[0].device, 7), train=True, add=ts[1], add_post=True),
                                                    dict(x=ts[1], pre=ts[2], prelu=_prelu(3, ts[0].device))]))),
        Case("contract", [_rand(g, 4, 3), _rand(g, *sh), _rand(g, 4)], lambda ts, _: ops.contract("oc,bchw->bohw", ts[0], ts[1], ts[2], "o")),
        Case("contract_stats", [_rand(g, 4, 3), _rand(g, *sh), _rand(g, 4)], lambda ts, _: ops.contract_stats("oc,bchw->bohw", ts[0], ts[1], ts[2], "o")[0]),
        Case("contract_many", [_rand(g, 4, 3), _rand(g, *sh), _rand(g, 4), _rand(g, 5, 3), _rand(g, 5)], many),
        Case("fanout", [_rand(g, *sh)], lambda ts, _: ops.fanout(ts[0], 3)),
        Case("split_channels", [_rand(g, 2, 6, 3, 5)], lambda ts, _: ops.split_channels(ts[0], (2, 3, 1))),
        Case("mean_bc", [_rand(g, *sh)], lambda ts, _: ops.mean_bc(ts[0])),
        Case("max_bc", [_rand(g, *sh)], lambda ts, _: ops.max_bc(ts[0])),
        Case("feature_lift", [50 + 350 * _rand(g, 2, 4, 5, 3)], lambda ts, _: ops.feature_lift(ts[0])),
        Case("rank1_adj", [_rand(g, 2, 5, 4), _rand(g, 2, 4, 5), _rand(g, 2, 5, 4), _rand(g, 2, 4, 5)],
             lambda ts, _: tuple(ops.rank1_adj([(0, ts[0], ts[1]), (1, ts[2], ts[3])]))),
        Case("gather_joints", [_rand(g, 2, 3, 6, 3)], lambda ts, ix: ops.gather_joints(ts[0], ix[0]), index=[[4, 0, 2]], backward=False),
        Case("eval_scatter_mpjpe", [_rand(g, 2, 3, 4, 3), _rand(g, 2, 3, 6, 3)], lambda ts, ix: ops.eval_scatter_mpjpe(ts[0], ts[1], *ix),
             index=[[5, 0, 3, 1], [2], [1]], backward=False),
        Case("mpjpe", [_rand(g, 2, 3, 4, 3), _rand(g, 2, 3, 4, 3)], lambda ts, _: ops.mpjpe(*ts)),
        Case("mpjpe_per_sample", [_rand(g, 2, 3, 4, 3), _rand(g, 2, 3, 4, 3)], lambda ts, _: ops.mpjpe_per_sample(*ts)),
    ]


def _strided_views(t):
    """the values of t (already on its device) as non-contiguous views that stay inside their own storage: [..., ::2] of doubled
    storage, and a transpose of transposed storage"""
    views = []
    if t.dim() >= 1 and t.shape[-1] > 1:
        views.append(("[..., ::2]", t.repeat_interleave(2, -1)[..., ::2]))
    if t.dim() >= 2 and t.shape[-1] > 1 and t.shape[-2] > 1:
        views.append(("transposed", t.transpose(-1, -2).contiguous().transpose(-1, -2)))
    for _, v in views:
        assert not v.is_contiguous() and torch.equal(v, t)
    return views


def _tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _attempt(case, operands, index, upstream, device):
    """one forward + backward of the case; returns ("raised", exception name) when the call refused its operands - before any launch of
    the pass that refused - or ("ran", outputs, gradients)"""
    ops.begin_step(device)
    with L.counted_calls() as launched:
        try:
            outs = _tuple(case.call(operands, index))
        except (TypeError, ValueError) as e:
            assert not launched, "%s: raised %r after launching %s" % (case.name, e, dict(launched))
            return ("raised", type(e).__name__)
    grads = None
    if case.backward:
        with L.counted_calls() as launched:
            try:
                upstream(outs)
            except (TypeError, ValueError) as e:
                assert not launched, "%s backward: raised %r after launching %s" % (case.name, e, dict(launched))
                return ("raised", type(e).__name__)
        grads = [None if t.grad is None else t.grad.detach().cpu() for t in operands]
    return ("ran", [o.detach().cpu() for o in outs], grads)


def _same(case, what, got, base):
    assert got[0] == "ran"
    for i, (a, b) in enumerate(zip(got[1], base[1])):
        assert a.dtype == torch.float32 and torch.equal(a, b), "%s, %s: output %d differs from the contiguous float32 call by %.3e" % (
            case.name, what, i, float((a.double() - b.double()).abs().max()))
    if base[2] is not None:
        for i, (a, b) in enumerate(zip(got[2], base[2])):
            assert (a is None) == (b is None), "%s, %s: gradient %d %s" % (case.name, what, i, "missing" if a is None else "unexpected")
            if a is not None:
                assert torch.equal(a.double(), b.double()), "%s, %s: gradient %d differs from the contiguous float32 call by %.3e" % (
                    case.name, what, i, float((a.double() - b.double()).abs().max()))


def check_operand_contract(device, case, report=None):
    report = {} if report is None else report
    gs = None

    def plain(outs):                    # contiguous float32 upstream gradients
        torch.autograd.backward(outs, [g.to(device) for g in gs])

    def transposed(outs):               # the same values through a transposed view: a non-contiguous gradient reaches the operator
        ys = [o.transpose(-1, -2) if o.dim() >= 2 else o for o in outs]
        torch.autograd.backward(ys, [(g.transpose(-1, -2).contiguous() if g.dim() >= 2 else g).to(device) for g in gs])

    def summed(outs):                   # d (c * y.sum()) / dy: an expanded gradient, every stride 0
        torch.autograd.backward([o.sum() for o in outs], [torch.tensor(0.25 * (i + 1), device=device) for i in range(len(outs))])

    def leaves(swap=None, view=None):
        ts = []
        for k, t in enumerate(case.tensors):
            t = view if k == swap else t.to(device)
            ts.append(t.detach().requires_grad_(case.backward))
        return ts

    ops.begin_step(device)
    probe = _tuple(case.call(leaves(), case.index))
    gs = [torch.randn(o.shape, generator=_gen(60 + i)) for i, o in enumerate(probe)]
    base = _attempt(case, leaves(), case.index, plain, device)
    assert base[0] == "ran", "%s: the valid call raised %s" % (case.name, base[1])
    for k, t in enumerate(case.tensors):
        wrong = t.float() if k in case.f64 else t.double()
        subs = [("operand %d as %s" % (k, wrong.dtype), wrong.to(device))] + [("operand %d %s" % (k, n), v) for n, v in _strided_views(t.to(device))]
        for what, v in subs:
            ts = leaves(k, v)
            assert ts[k].dtype == v.dtype and ts[k].is_contiguous() == v.is_contiguous() and ts[k].data_ptr() == v.data_ptr()
            got = _attempt(case, ts, case.index, plain, device)
            report[what] = got[0] if got[0] == "ran" else got[1]
            if k in case.f64 and v.dtype == torch.float32:
                assert got[0] == "raised", "%s, %s: float32 memory was read as float64" % (case.name, what)
            if got[0] == "ran":
                _same(case, what, got, base)
    if case.index is not None:          # integer lists as int64 tensors and arrays: converted on the host
        for conv, what in ((lambda ix: torch.tensor(ix, dtype=torch.int64), "int64 tensor"), (lambda ix: np.asarray(ix, dtype=np.int64), "int64 array")):
            got = _attempt(case, leaves(), [conv(ix) for ix in case.index], plain, device)
            report["indices as " + what] = got[0] if got[0] == "ran" else got[1]
            if got[0] == "ran":
                _same(case, "indices as " + what, got, base)
    if case.backward:
        if any(o.dim() >= 2 and o.shape[-1] > 1 and o.shape[-2] > 1 for o in probe):
            got = _attempt(case, leaves(), case.index, transposed, device)
            report["transposed upstream"] = got[0] if got[0] == "ran" else got[1]
            if got[0] == "ran":
                _same(case, "transposed upstream gradient", got, base)
        gs = [torch.full(o.shape, 0.25 * (i + 1)) for i, o in enumerate(probe)]
        base = _attempt(case, leaves(), case.index, plain, device)
        got = _attempt(case, leaves(), case.index, summed, device)
        report["expanded upstream"] = got[0] if got[0] == "ran" else got[1]
        if got[0] == "ran":
            _same(case, "expanded upstream gradient", got, base)
    return report


def check_issue_table(device):
    """the calls that returned wrong numbers without an exception: each one raises, or is exact"""
    g = _gen(32)
    x = _rand(g, 2, 3, 3, 5).to(device)
    pooled, w1, w2 = _rand(g, 2, 6), _rand(g, 2, 6), _rand(g, 6, 2)
    gate = ops.se_gate(pooled.to(device), w1.to(device), w2.to(device)).cpu()

    def exact_or_raises(what, fn, ref):
        try:
            out = fn()
        except (TypeError, ValueError):
            return
        assert out.dtype == torch.float32 and torch.equal(out.cpu(), ref), "%s: max abs error %.3e" % (what, float((out.cpu().double() - ref.double()).abs().max()))

    exact_or_raises("se_gate(pooled.t())", lambda: ops.se_gate(pooled.t().contiguous().to(device).t(), w1.to(device), w2.to(device)), gate)
    exact_or_raises("se_gate(pooled[:, ::2])", lambda: ops.se_gate(pooled.repeat_interleave(2, 1).to(device)[:, ::2], w1.to(device), w2.to(device)), gate)
    exact_or_raises("se_gate(transposed w1)", lambda: ops.se_gate(pooled.to(device), w1.t().contiguous().to(device).t(), w2.to(device)), gate)
    exact_or_raises("se_gate(float64)", lambda: ops.se_gate(pooled.double().to(device), w1.double().to(device), w2.double().to(device)), gate)
    exact_or_raises("cumsum_time(float64)", lambda: ops.cumsum_time(x.double()), ops.cumsum_time(x).cpu())
    exact_or_raises("dstd_stats(float64)", lambda: ops.dstd_stats(x.double()), ops.dstd_stats(x).cpu())
    exact_or_raises("cat_channels([x, float64])", lambda: ops.cat_channels([x, x.double()]), ops.cat_channels([x, x]).cpu())
    exact_or_raises("add3(x, float64)", lambda: ops.add3(x, x.double()), ops.add3(x, x).cpu())
    exact_or_raises("norm_act(add=float64)", lambda: ops.norm_act(x, add=x.double()), ops.norm_act(x, add=x).cpu())
    w, bias = _rand(g, 4, 3).to(device), _rand(g, 4)
    y = ops.contract("oc,bchw->bohw", w, x, bias.to(device), "o").cpu()
    exact_or_raises("contract(bias[::2])", lambda: ops.contract("oc,bchw->bohw", w, x, bias.repeat_interleave(2).to(device)[::2], "o"), y)
    exact_or_raises("contract(bias float64)", lambda: ops.contract("oc,bchw->bohw", w, x, bias.double().to(device), "o"), y)


# =====================================================================================================================
# B. the glue kernels past their first pass, against float64
# =====================================================================================================================
def check_mpjpe(device):
    """more points than one grid of cg_mpjpe_fwd: every thread of the first 356 runs a second iteration.  Loss bound: the loss is a
    float32 sum of `blocks` = 1024 positive partial sums (one atomic per workgroup; each partial is an f64 sum rounded once, 2^-24
    relative, which the 1023 roundings of the additions dominate): |error| <= blocks * 2^-24 * |loss|.  Measured: 1.3e-7 and 5.4e-7
    of the loss on the MI355X (contiguous, permuted), 1.3e-7 and 5.4e-8 on the CPU shim."""
    g = _gen(41)
    shape = G.MPJPE_SHAPE
    N = shape[0] * shape[1] * shape[2]
    pred, tgt = _rand(g, *shape), _rand(g, *shape)
    flat_t = tgt.view(N, 3)
    flat_t[G.MPJPE_GRID:] += 300.0                                   # the second pass carries a share of the loss no bound forgives
    flat_t[1234] = pred.view(N, 3)[1234]                            # pred == target: gradient 0
    dist = (pred.double() - tgt.double()).norm(dim=-1).reshape(-1)
    share = float(dist[G.MPJPE_GRID:].sum() / dist.sum())
    assert share >= G.MPJPE_TAIL_SHARE, "the points past one grid carry only %.3f of the error" % share
    B, T, V, _ = shape
    stored = pred.view(B, T, V, 3).permute(0, 2, 1, 3).contiguous()   # (B, V, T, 3) storage of the same prediction
    for what, base, view in (("contiguous", pred, lambda t: t), ("permuted", stored, lambda t: t.permute(0, 2, 1, 3))):
        pd, pr = _leaf(base, device), _leaf(base.double(), "cpu")
        assert what == "contiguous" or not view(pd).is_contiguous()
        ld = ops.mpjpe(view(pd), tgt.to(device))
        lr = torch.linalg.vector_norm(view(pr) - tgt.double(), dim=-1).mean()
        err = abs(ld.item() - lr.item())
        print("mpjpe %s, %d points (%.1f %% of the error past one grid): loss error %.3e = %.3e of the loss, bound %.3e" % (
            what, N, 100 * share, err, err / lr.item(), G.MPJPE_BLOCKS * 2.0 ** -24))
        assert_close(ld, lr, "mpjpe %s loss" % what, rel=G.MPJPE_BLOCKS * 2.0 ** -24, floor=0.0)
        ld.backward(); lr.backward()
        assert float(view(pr.grad).reshape(N, 3)[1234].abs().max()) == 0.0 and float(view(pd.grad).reshape(N, 3)[1234].abs().max()) == 0.0
        assert_close(pd.grad, pr.grad, "mpjpe %s grad" % what, rel=1e-5, floor=float(pr.grad.abs().max()))


def check_flat_adam(device):
    """cg_adam_flat on more parameters than one grid covers, the gradient gather on a tensor of 257 chunks, cg_scale past one grid"""
    from cistgcn_amd.runtime import FlatAdam
    torch.manual_seed(5)
    ref = nn.Linear(*G.ADAM_LINEAR)
    dev = nn.Linear(*G.ADAM_LINEAR)
    dev.load_state_dict(ref.state_dict())
    ref.double(); dev.to(device)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-4)
    opt_dev = FlatAdam(dev, lr=1e-2, weight_decay=1e-4)
    g = _gen(42)
    for step in range(2):
        for pr, pd in zip(ref.parameters(), dev.parameters()):
            gr = torch.randn(pr.shape, generator=g)
            pr.grad, pd.grad = gr.double(), gr.clone().to(device)
        opt_ref.step(); opt_dev.step()
        for (k, pr), pd in zip(ref.named_parameters(), dev.parameters()):
            assert_close(pd, pr, "adam step %d %s" % (step, k), rel=1e-5)
    x = _rand(g, G.SCALE_N)
    xd = x.clone().to(device)
    s = 1.0 / 3.0
    _lib.call("cg_scale", ops._ptr(xd), xd.numel(), s, ops._stream(xd))
    assert torch.equal(xd.cpu(), x * s), "cg_scale"


ADAM_CLIPS, ADAM_SCALES = (0.0, 0.5), (1.0, 0.5)
ADAM_SPECIALS = (float("nan"), float("inf"), float("-inf"))


def _adam_clip_places(n_weight, n_bias):
    """(tensor, flat index) of the first element of the flat buffer, of one past the first grid stride of cg_adam_flat_kernel and of the
    last element; the weight of G.ADAM_LINEAR alone is longer than one grid (G.assert_properties)"""
    grid = G.glue_geometry()["flat_grid"]
    assert n_weight > grid + 101
    return ((0, 0), (0, grid + 101), (1, n_bias - 1))


def _adam_clip_run(device, clip, gscale, grads, special):
    """two steps of FlatAdam (lr 1e-2, weight decay 0.5) on G.ADAM_LINEAR; grads[step][tensor]: float32 CPU gradients; special: {(tensor,
    flat index): value} written into the gradients of the first step.  -> after every step, per tensor, (p, exp_avg, exp_avg_sq) on the CPU"""
    from cistgcn_amd.runtime import FlatAdam
    torch.manual_seed(5)
    dev = nn.Linear(*G.ADAM_LINEAR).to(device)
    opt = FlatAdam(dev, lr=1e-2, weight_decay=0.5, clip_value=clip)
    out = []
    for step in range(2):
        for t, pd in enumerate(dev.parameters()):
            gr = grads[step][t].clone()
            if step == 0:
                for (tt, i), v in special.items():
                    if tt == t:
                        gr.view(-1)[i] = v
            pd.grad = gr.view(pd.shape).to(device)
        opt.step(grad_scale=gscale)
        state = []
        for pd, off in zip(opt.params, opt.grads.offsets[:-1]):
            n, off = pd.numel(), int(off)
            state.append(tuple(t.detach().cpu().reshape(-1).clone() for t in (pd, opt.exp_avg[off:off + n], opt.exp_avg_sq[off:off + n])))
        out.append(state)
    return out


def _adam_clip_ref(clip, gscale, grads, special):
    """the same two steps by torch.optim.Adam in float64: the gradient scaled, then torch.nn.utils.clip_grad_value_, then the step"""
    torch.manual_seed(5)
    ref = nn.Linear(*G.ADAM_LINEAR).double()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=0.5)
    out = []
    for step in range(2):
        for t, pr in enumerate(ref.parameters()):
            gr = grads[step][t].clone()
            if step == 0:
                for (tt, i), v in special.items():
                    if tt == t:
                        gr.view(-1)[i] = v
            pr.grad = gr.view(pr.shape).double() * gscale
        if clip > 0:
            torch.nn.utils.clip_grad_value_(ref.parameters(), clip)
        opt.step()
        out.append([tuple(t.detach().reshape(-1).clone() for t in (pr, opt.state[pr]["exp_avg"], opt.state[pr]["exp_avg_sq"])) for pr in ref.parameters()])
    return out


def check_flat_adam_clip(device):
    """cg_adam_flat with clip_grad_value_ and the gradient pre-scale on values random gradients never hold: gradients exactly at +-clip, one
    float32 step beyond, and at +-clip / grad_scale (scaled first, clipped second); one NaN, one +Inf and one -Inf in the gradient of the
    first of two steps, at the first element of the flat buffer, the last one and one past the first grid stride, every value at every
    place in turn.  torch.nn.utils.clip_grad_value_ is clamp_: a NaN stays a NaN and reaches the parameter, +-Inf is clipped.  Against
    torch.optim.Adam in float64 on the same values: the same NaN, +Inf and -Inf positions in p, exp_avg and exp_avg_sq, every finite
    element at the rel = 1e-5 of check_flat_adam (1 - beta2 in float32 is 4.7e-5 off 0.001, so exp_avg_sq has no tighter bound of its own),
    and every element that had no special gradient bit for bit what a run
    without the special values gives."""
    n_in, n_out = G.ADAM_LINEAR
    sizes = (n_in * n_out, n_out)
    places = _adam_clip_places(*sizes)
    g = _gen(421)
    grads = [[torch.randn(n, generator=g) for n in sizes] for _ in range(2)]
    one = torch.tensor(1.0)
    for gscale in ADAM_SCALES:           # the boundary values of every (clip, scale) pair stand in every run; 0.5 is the only clip > 0
        c = torch.tensor(0.5)
        vals = [c, torch.nextafter(c, one), c / gscale, torch.nextafter(c / gscale, 2 * one / gscale)]
        vals = [float(s * v) for v in vals for s in (1.0, -1.0)]
        base = 16 if gscale == 1.0 else 48
        for step in range(2):
            for t, n in enumerate(sizes):
                for k, v in enumerate(vals):
                    grads[step][t][base + k] = v if step == 0 else -v
                    grads[step][t][n - 8 - base - k] = v
    for clip in ADAM_CLIPS:
        for gscale in ADAM_SCALES:
            plain = _adam_clip_run(device, clip, gscale, grads, {})
            for turn in range(3):
                special = {places[k]: ADAM_SPECIALS[(k + turn) % 3] for k in range(3)}
                what = "adam clip=%g scale=%g turn %d" % (clip, gscale, turn)
                got, ref = _adam_clip_run(device, clip, gscale, grads, special), _adam_clip_ref(clip, gscale, grads, special)
                for step in range(2):
                    for t in range(2):
                        touched = torch.zeros(sizes[t], dtype=torch.bool)
                        for (tt, i), v in special.items():
                            if tt == t:
                                touched[i] = True
                        for name, a, r, b in zip(("p", "exp_avg", "exp_avg_sq"), got[step][t], ref[step][t], plain[step][t]):
                            w = "%s step %d tensor %d %s" % (what, step, t, name)
                            for kind, f in (("NaN", torch.isnan), ("+Inf", torch.isposinf), ("-Inf", torch.isneginf)):
                                assert torch.equal(f(a), f(r)), "%s: %s at %s, the reference has it at %s" % (
                                    w, kind, f(a).nonzero().flatten().tolist()[:8], f(r).nonzero().flatten().tolist()[:8])
                            for (tt, i), v in special.items():
                                if tt != t:
                                    continue
                                if v != v:
                                    assert bool(torch.isnan(a[i])), "%s: a NaN gradient at %d gave %r" % (w, i, float(a[i]))
                                elif clip > 0:
                                    assert bool(torch.isfinite(a[i])), "%s: an infinite gradient at %d was not clipped: %r" % (w, i, float(a[i]))
                            fin = torch.isfinite(r)
                            zero = torch.zeros((), dtype=a.dtype)
                            assert_close(torch.where(fin, a, zero), torch.where(fin, r, zero.double()), w, rel=1e-5)
                            same = (a.view(torch.int32) == b.view(torch.int32)) | touched
                            assert bool(same.all()), "%s: %d elements without a special gradient differ from the run without special values, first at %d" % (
                                w, int((~same).sum()), int((~same).nonzero()[0]))


def check_se_gate(device):
    g = _gen(43)
    for B, C, H in G.SE_GATE:
        _run(ops.se_gate, lambda p, w1, w2: torch.sigmoid(F.linear(F.relu(F.linear(p, w1)), w2)),
             [_rand(g, B, C), _rand(g, H, C) / C ** 0.5, _rand(g, C, H)], device, what="se_gate B%d C%d H%d" % (B, C, H), rel=3e-5, ref_dtype=F64)


def _reduce_input():
    x = _rand(_gen(44), *G.REDUCE_SHAPE)
    rows = x.flatten(2)
    for (b, c), pos in G.REDUCE_TIES.items():
        rows[b, c, list(pos)] = 9.0 + b + c
    rows[G.REDUCE_CONSTANT_ROW[0], G.REDUCE_CONSTANT_ROW[1]] = 0.5
    return x


def check_reduce_bc(device):
    """256 threads, three iterations, the last one partial; the maximum stands at several positions of a row (in one thread's
    iterations, in different threads and waves, in a constant row): value and gradient go to the first, as `flatten(2).max(-1)` has it"""
    x = _reduce_input()
    _run(ops.max_bc, lambda t: t.flatten(2).max(-1)[0], [x], device, what="max_bc ties", ref_dtype=F64)
    xd = _leaf(x, device)
    y = ops.max_bc(xd)
    assert torch.equal(y.detach().cpu(), x.flatten(2).max(-1)[0])
    y.backward(torch.ones_like(y))
    hit = xd.grad.cpu().flatten(2)
    want = torch.zeros_like(hit)
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            row = x.flatten(2)[b, c]
            first = int((row == row.max()).nonzero()[0])
            expect = min(G.REDUCE_TIES[(b, c)]) if (b, c) in G.REDUCE_TIES else 0 if (b, c) == G.REDUCE_CONSTANT_ROW else first
            assert first == expect
            want[b, c, first] = 1.0
    assert torch.equal(hit, want), "max_bc: the gradient does not go to the first maximum"
    _run(lambda t: ops.max_bc(t.permute(0, 2, 3, 1)), lambda t: t.permute(0, 2, 3, 1).flatten(2).max(-1)[0], [x], device, what="max_bc permuted", ref_dtype=F64)
    _run(ops.mean_bc, lambda t: t.mean((2, 3)), [x], device, what="mean_bc", ref_dtype=F64)
    B, _, H, W = G.REDUCE_SHAPE                # kind 2: the sum behind a broadcast input of cat_channels
    g = _gen(45)
    _run(lambda a, m: ops.cat_channels([a, m], bcast=(False, True)), lambda a, m: torch.cat((a, m[:, :, None, None].expand(-1, -1, H, W)), 1),
         [_rand(g, B, 2, H, W), _rand(g, B, 3)], device, what="cat broadcast P%d" % (H * W), ref_dtype=F64)


def check_cumsum(device):
    g = _gen(46)
    for shape, perm in G.CUMSUM:
        view = (lambda t, perm=perm: t.permute(*perm)) if perm is not None else (lambda t: t)
        _run(lambda t: ops.cumsum_time(view(t)), lambda t: view(t).cumsum(1), [_rand(g, *shape)], device, what="cumsum %s %s" % (shape, perm), ref_dtype=F64)


def check_feature_lift(device):
    g = _gen(47)
    for B, T, V in G.FEATURE_LIFT:
        x = 50 + 350 * _rand(g, B, T, V, 3)
        x[0, T - 1, 0] = 0.0                   # vel[T-1] = x[T-1] = 0: the sub-gradient of |vel| is 0
        if T >= 2:
            x[1, 1] = x[1, 0]                  # two equal frames: vel[0] = 0
        _run(ops.feature_lift, lambda t: O.CISTGCN.feature_lift(t).contiguous(), [x], device, rel=1e-5, what="feature_lift B%d T%d V%d" % (B, T, V), ref_dtype=F64)


def check_dstd_stats(device):
    """Gradient bound: statistics over two to seven channels are ill-conditioned in float32 (stock float32 PyTorch is 5.5e-5 of max|grad|
    away from float64 on (3, 2, 5, 129)), so the bound is max(2e-5 * floor, 4 x the error of float32 CPU PyTorch against float64 on the
    same input), floor = max(1e-3, max|ref grad|); the factor 4 covers the kernel's other order of summation."""
    g = _gen(48)
    worst = (0.0, None)
    for shape in G.DSTD_STATS:
        x = _rand(g, *shape) + (0.5 if shape[1] > 8 else 0.0)
        xd, x32, x64 = _leaf(x, device), _leaf(x, "cpu"), _leaf(x.double(), "cpu")
        y, y32, y64 = ops.dstd_stats(xd), O.CISTGCN.block_stats(x32), O.CISTGCN.block_stats(x64)
        assert_close(y, y64, "dstd_stats %s output" % (shape,), rel=2e-5)
        up = _rand(_gen(99), *y64.shape)
        y.backward(up.to(device)); y32.backward(up); y64.backward(up.double())
        floor = max(1e-3, float(x64.grad.abs().max()))
        e32 = float((x32.grad.double() - x64.grad).abs().max())
        err = float((xd.grad.cpu().double() - x64.grad).abs().max())
        bound = max(2e-5 * floor, 4.0 * e32)
        print("dstd_stats %s: gradient error %.3e of max|grad| (kernel) against %.3e (float32 PyTorch); bound %.3e" % (shape, err / floor, e32 / floor, bound / floor))
        assert err <= bound, "dstd_stats %s grad: max err %.3e > bound %.3e (float32 PyTorch: %.3e)" % (shape, err, bound, e32)
        if err / bound > worst[0]:
            worst = (err / bound, shape, err / floor, e32 / floor)
    print("dstd_stats: closest to its bound %s at %.3f: kernel %.3e, float32 PyTorch %.3e of max|grad|" % (worst[1], worst[0], worst[2], worst[3]))


def check_fanout(device):
    g = _gen(49)
    for n, shape in G.FANOUT:
        with L.counted_calls() as launched:
            _run(lambda t: sum(a * (i + 1.0) for i, a in enumerate(ops.fanout(t, n))), lambda t: (n * (n + 1) / 2.0) * t, [_rand(g, *shape)], device,
                 what="fanout %d %s" % (n, shape), ref_dtype=F64)
        assert launched.get("cg_sum_many") == (n + 5) // 7, "fanout %d: %s launches of cg_sum_many" % (n, launched.get("cg_sum_many"))


def check_cat_split(device):
    g = _gen(50)
    H, W = G.CAT_POSITIONS
    ins = [_rand(g, 2, -c) if c < 0 else _rand(g, 2, c, H, W) for c in G.CAT_CHANNELS]
    bcast = tuple(c < 0 for c in G.CAT_CHANNELS)
    with L.counted_calls() as launched:
        _run(lambda *ts: ops.cat_channels(list(ts), bcast=bcast),
             lambda *ts: torch.cat([t[:, :, None, None].expand(-1, -1, H, W) if bc else t for t, bc in zip(ts, bcast)], 1), ins, device, what="cat six", ref_dtype=F64)
    assert launched.get("cg_copy_many") == 2, "cat of six inputs: %s copy launches" % launched.get("cg_copy_many")
    x = _rand(g, *G.SPLIT_SHAPE)
    with L.counted_calls() as launched:       # pieces consumed through sum(): every piece receives an expanded gradient
        _run(lambda t: torch.stack([p.sum() * (i + 1.0) for i, p in enumerate(ops.split_channels(t, G.SPLIT_SIZES))]),
             lambda t: torch.stack([p.sum() * (i + 1.0) for i, p in enumerate(torch.split(t, G.SPLIT_SIZES, 1))]), [x], device, what="split expanded", ref_dtype=F64)
    assert launched.get("cg_copy_many") == 2, "split into five pieces: %s copy launches" % launched.get("cg_copy_many")
    _run(lambda t: torch.cat([p * (i + 1.0) for i, p in enumerate(ops.split_channels(t, G.SPLIT_SIZES))], 1),
         lambda t: torch.cat([p * (i + 1.0) for i, p in enumerate(torch.split(t, G.SPLIT_SIZES, 1))], 1), [x], device, what="split", ref_dtype=F64)


def _zero(buf, start, n):
    _lib.call("cg_zero", ctypes.c_void_p(buf.data_ptr() + start), n, ops._stream(buf))


def check_zero(device):
    """cg_zero on a byte buffer of 0xA5: the range is zero, every byte outside it untouched"""
    slot = 1072                                                     # 16 guard bytes + offset + 1000 bytes + guard, a multiple of 16
    cases = [(o, n) for o in G.ZERO_OFFSETS for n in G.ZERO_LENGTHS]
    buf = torch.full((len(cases) * slot + 32,), 0xA5, dtype=torch.uint8, device=device)
    a0 = (-buf.data_ptr()) % 16
    want = np.full(buf.numel(), 0xA5, dtype=np.uint8)
    for i, (o, n) in enumerate(cases):
        start = a0 + i * slot + 16 + o
        assert (buf.data_ptr() + start) % 16 == o % 16 and o + n + 16 < slot
        _zero(buf, start, n)
        want[start:start + n] = 0
    got = buf.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "cg_zero: byte %d of case (offset, length) = %s is %#x" % (bad[0], cases[min((bad[0] - a0) // slot, len(cases) - 1)], got[bad[0]])
    n, o = G.ZERO_BIG
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=device)
    start = (-buf.data_ptr()) % 16 + 16 + o
    _zero(buf, start, n)
    got = buf.cpu()
    assert not bool(got[start:start + n].any()), "cg_zero: a fill of %d bytes left %d bytes set" % (n, int((got[start:start + n] != 0).sum()))
    assert bool((got[:start] == 0xA5).all()) and bool((got[start + n:] == 0xA5).all()), "cg_zero: a fill of %d bytes wrote outside its range" % n


def check_norm_act_alignment(device):
    """the same rows read as float4, scalar and float2: the vector width of the row kernels follows the base address of the input"""
    shape = G.NORM_ACT_ALIGN_SHAPE
    n = int(np.prod(shape))
    g = _gen(51)
    x, up = _rand(g, *shape, scale=2.0) + 0.5, _rand(g, *shape)
    runs = []
    for off in G.NORM_ACT_ALIGN_OFFSETS:
        store = torch.zeros(n + 8, device=device)
        a0 = ((-store.data_ptr()) % 16) // 4 + off
        xd = store[a0:a0 + n].view(shape)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4 * off
        xd.requires_grad_(True)
        bn, pr = _bn(shape[1], device, 9), _prelu(shape[1], device)
        ops.manual_seed(77, device)
        ops.begin_step(device)
        y = ops.norm_act(xd, bn=bn, train=True, drop_p=0.3, salt=5, prelu=pr)
        y.backward(up.to(device))
        runs.append((y.detach().cpu(), xd.grad.cpu(), bn.weight.grad.cpu(), pr.weight.grad.cpu()))
    base = runs[0]
    dropped = base[0] == 0
    assert 0.15 < float(dropped.float().mean()) < 0.45
    for off, r in zip(G.NORM_ACT_ALIGN_OFFSETS[1:], runs[1:]):
        assert torch.equal(r[0] == 0, dropped), "norm_act at float offset %d: another dropout mask" % off
        assert_close(r[0], base[0], "norm_act offset %d y" % off, rel=2e-6)
        assert_close(r[1], base[1], "norm_act offset %d dx" % off, rel=2e-6, floor=max(1e-3, float(base[1].abs().max())))
        assert_close(r[2], base[2], "norm_act offset %d dgamma" % off, rel=2e-6, floor=max(1e-3, float(base[2].abs().max())))
        assert_close(r[3], base[3], "norm_act offset %d dalpha" % off, rel=2e-6, floor=max(1e-3, float(base[3].abs().max())))


def check_eval_scatter(device):
    B, To, J32, J22 = G.EVAL_SCATTER
    g = _gen(52)
    pred, tgt = 50 + 350 * _rand(g, B, To, J22, 3), 50 + 350 * _rand(g, B, To, J32, 3)
    perm = torch.randperm(J32, generator=g).tolist()
    used, rest = perm[:J22], perm[J22:]
    rep32, rep22 = rest[:2], [5, J22 - 1]
    full, frames = ops.eval_scatter_mpjpe(pred.to(device), tgt.to(device), used, rep32, rep22)
    ref = E.scatter_prediction(pred, tgt, used, rep32, rep22)
    assert torch.equal(full.cpu(), ref), "scattered prediction"
    assert_close(frames, E.mpjpe_frames(ref.double(), tgt.double()), "per-frame MPJPE J32=%d" % J32, rel=1e-5)


KERNEL_CHECKS = (check_mpjpe, check_flat_adam, check_flat_adam_clip, check_se_gate, check_reduce_bc, check_cumsum, check_feature_lift, check_dstd_stats, check_fanout,
                 check_cat_split, check_zero, check_norm_act_alignment, check_eval_scatter)
