"""Helpers of the tail-sums tests (CPU shim and MI355X): the backward of ops.dstd_tail on the route that forms its BatchNorm sums a phase
early (csrc/dstd_tail.hip: the compressor sums from row sums of K1, the tcn sums from moments of F1 and K3, K4 and K5 as one pass, the
shared residual gradient), against fp64 stock PyTorch (checks._dstd_tail_ref) and against the route with a pass per sum.

Bounds.  Gradients: exactly those of checks.check_dstd_tail / _assert_tail_grads - rel 5e-5 of max(1e-3, max |ref|), the compressor
weight in train mode with the floor of its BatchNorm weight's gradient.  Sums: per channel |got - ref| <= 16 * 2^-24 * sum |term| as in
tower_sums_checks, the terms being the products of the formula the kernel evaluates, summed in absolute value over the elements:
  compressor   g_c = dout gate s + dpooled / P s                 (times hhat for the second sum, times u / s' on the slope branch)
  tcn          g_t = scale_p q g_p - scale_p m1 q - scale_p m2 q zhat     (times yhat for the second sum)
Each product is formed in f32 with a handful of roundings and summed in f32 over at most a few quads per lane (row sums) or a few tiles
(K3), everything above is f64.  The reference takes the PReLU branches the kernel's forward took (BranchLog), so no sum holds a kink term."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import checks
from checks import BranchLog, _dstd_tail_ref, _gen, _leaf, _rand, _ref_keep, _ref_state
from helpers import assert_close
from cistgcn_amd import _lib, ops
import loop_shapes as L

EPS = 2.0 ** -24
BOUND = 16 * EPS
P_DROP, SALTS = 0.25, (7, 9)

# (B, C, T, V)
MERGED = (
    (5, 20, 6, 6),       # P = 36: two K3 tiles, the second with 4 positions; the run-time K3 instantiation
    (3, 8, 13, 24),      # P = 312: a lane's second quad iteration in the row kernels; K3 <1, 1>
    (2, 16, 4, 5),       # K3 <1, 2>
    (3, 32, 5, 8),       # K3 <2, 4>
    (5, 64, 6, 12),      # K3 <4, 8>
    (67, 16, 4, 4),      # row phases: two samples per workgroup, the last group one (the shapes above keep one sample per workgroup); K3: 2 tiles
)
FALLBACK = ((3, 20, 7, 9), (2, 8, 6, 11))      # P = 63, 66: rows that are no whole quads keep K4 and K5
SHAPES = MERGED + FALLBACK


def ident(shape):
    return "-".join(str(s) for s in shape)


def assert_properties():
    """the loop properties the shapes are chosen for, asked from the library's own geometry query"""
    ragged = False
    for shape in SHAPES:
        g = L.dstd_tail_geometry(*shape)
        print("dstd_tail geometry %s: %s" % (shape, g))
        ragged |= g["rows"] >= 2 and g["row_last"] < g["rows"]
    assert ragged, "no shape gives the row phases several samples per workgroup and a short last group"
    g = L.dstd_tail_geometry(*MERGED[0])
    assert g["K3"]["tps"] == 2 and (MERGED[0][2] * MERGED[0][3]) % g["K3"]["PT"] == 4, g
    g = L.dstd_tail_geometry(*MERGED[5])
    assert g["rows"] >= 2 and g["row_last"] < g["rows"] and (MERGED[5][2] * MERGED[5][3]) % 4 == 0, g
    assert MERGED[1][2] * MERGED[1][3] > 256                    # a second quad iteration of a lane
    assert all((s[2] * s[3]) % 4 == 0 for s in MERGED) and all((s[2] * s[3]) % 4 != 0 for s in FALLBACK)
    assert sorted(s[1] for s in MERGED[:5]) == [8, 16, 20, 32, 64]   # <1,1> <1,2> run-time <2,4> <4,8>


class _Capture(BranchLog):
    """BranchLog that keeps the pre-activations of the five PReLUs (in call order: d_1, p_1, d_2, p_2, c) with their gradients"""

    def __init__(self):
        super().__init__()
        self.pre = []

    def prelu(self, u, weight, dev_out, add=None):
        u.retain_grad()
        self.pre.append(u)
        return super().prelu(u, weight, dev_out, add)


def _make(C, device, seed):
    from cistgcn_amd.models.layers.SE import SELayer2d
    gg = _gen(seed)
    bns = [nn.BatchNorm2d(C) for _ in range(5)]
    for bn in bns:
        with torch.no_grad():
            bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=gg)); bn.bias.copy_(0.3 * torch.randn(C, generator=gg))
            bn.running_mean.copy_(0.2 * torch.randn(C, generator=gg)); bn.running_var.copy_(0.5 + torch.rand(C, generator=gg))
    al = [nn.PReLU() for _ in range(5)]
    for i, a in enumerate(al):
        with torch.no_grad():
            a.weight.fill_(0.1 + 0.07 * i)
    conv = nn.Conv2d(2 * C, C, 1, bias=False)
    se = SELayer2d(C, reduction=8)
    with torch.no_grad():
        conv.weight.copy_(0.3 * torch.randn(conv.weight.shape, generator=gg))
        se.w1.copy_(0.5 * torch.randn(se.w1.shape, generator=gg)); se.w2.copy_(0.5 * torch.randn(se.w2.shape, generator=gg))
    return nn.ModuleList(bns + al + [conv, se]).to(device)


def _inputs(shape):
    B, C, T, V = shape
    g = _gen(31 + B + 3 * C + T)
    data = [_rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C), _rand(g, B, C), _rand(g, B, C, T, V)]
    return data, _rand(g, B, C, T, V)


def run(device, shape, train, shared, tail_sums):
    """one forward + backward of ops.dstd_tail.  shared: r1 is r2 (the data of r1) and rs_shared=True.  Returns out, the gradients (inputs
    y1 y2 r1 [r2] w1 w2 bres, then the parameters in named_parameters() order), the PReLU taps, the sums the backward left, the seed word."""
    B, C, T, V = shape
    data, gout = _inputs(shape)
    mods = _make(C, device, 100 + B + C)
    mods.train(train)
    y1, y2, r1, r2, w1, w2, bres = [_leaf(t, device) for t in data]
    ops.manual_seed(1234, device)
    ops.begin_step(device)
    seed = int(ops.seed_state(device)[0].item())

    def sums(y):
        st = ops._arena(torch.device(device)).take(2 * C * 16)
        yc = y.detach().double()
        st.view(16, C, 2)[0].copy_(torch.stack((yc.sum((0, 2, 3)), (yc * yc).sum((0, 2, 3))), 1))
        return st
    taps, tap = [], {}
    out, _ = ops.dstd_tail([y1, y2], [sums(y1), sums(y2)] if train else [None, None], [r1, r1] if shared else [r1, r2], (w1, w2), list(mods[:5]),
                           list(mods[5:10]), mods[10].weight, mods[11], bres, train, drop_p=P_DROP, salts=SALTS, emit_stats=train, taps=taps,
                           tail_sums=tail_sums, rs_shared=shared, sums_tap=tap)
    out.backward(gout.to(device))
    leaves = [y1, y2, r1] + ([] if shared else [r2]) + [w1, w2, bres]
    grads = [t.grad.detach().cpu() for t in leaves] + [p.grad.detach().cpu() for p in mods.parameters()]
    tap = {k: ([t.cpu() for t in v] if isinstance(v, list) else (v.cpu() if torch.is_tensor(v) else v)) for k, v in tap.items()}
    return dict(out=out.detach().cpu(), grads=grads, taps=[t.detach().cpu() for t in taps], tap=tap, seed=seed, mods=mods, data=data, gout=gout)


def reference(res, shape, train, shared):
    """fp64 stock PyTorch on the branches of the run `res`: gradients in the order of run(), and the captured pre-activations"""
    rparams, rbufs = _ref_state(_make(shape[1], "cpu", 100 + shape[0] + shape[1]))
    rleaves = [_leaf(t.double(), "cpu") for t in res["data"]]
    if shared:
        rleaves[3] = _leaf(res["data"][2].double(), "cpu")          # r2 carries the values of r1
    log = _Capture()
    rout = _dstd_tail_ref(rleaves, rparams, rbufs, train, P_DROP, SALTS, res["seed"], log, res["taps"])
    rout.backward(res["gout"].double())
    log.settle("tail sums %s" % (shape,))
    g = [t.grad for t in rleaves]
    grads = g[:2] + ([g[2] + g[3]] if shared else g[2:4]) + g[4:] + [rparams[k].grad for k in rparams]
    names = ["y1", "y2"] + (["r1 (= r1 + r2)"] if shared else ["r1", "r2"]) + ["w1", "w2", "bres"] + list(rparams)
    return dict(out=rout.detach(), grads=grads, names=names, params=rparams, bufs=rbufs, pre=log.pre, leaves=rleaves)


def _floors(ref, train):
    """the floors of checks._assert_tail_grads"""
    floors = []
    for k, b in zip(ref["names"], ref["grads"]):
        floor = max(1e-3, float(b.abs().max()))
        if train and k == "10.weight":
            floor = max(floor, float(ref["params"]["4.weight"].grad.abs().max()))
        floors.append(floor)
    return floors


def _within(got, ref, mag, what):
    err = (got.double() - ref).abs()
    lim = BOUND * mag
    worst = float((err / lim.clamp_min(1e-300)).max())
    print("%s: max |got - ref| / (16 * 2^-24 * sum |term|) = %.3g" % (what, worst))
    assert bool((err <= lim).all()), "%s: error %.3g of the bound (got %s, ref %s)" % (what, worst, got.flatten()[:4].tolist(), ref.flatten()[:4].tolist())


def _compressor_sums(res, ref, shape, what):
    """red_c against the sums of g_c = dout gate s + dpooled / P s formed in fp64 from the reference's tensors"""
    B, C, T, V = shape
    P = T * V
    pr = ref["params"]
    u = ref["pre"][4].detach()
    pos = res["taps"][4].double() > 0
    alpha = float(pr["9.weight"].detach())
    s = torch.where(pos, torch.ones_like(u), torch.full_like(u, alpha))
    h = u * s
    hh = (u - pr["4.bias"].detach().view(1, C, 1, 1)) / pr["4.weight"].detach().view(1, C, 1, 1)
    pooled = h.mean((2, 3)).requires_grad_(True)
    gate = torch.sigmoid(F.linear(F.relu(F.linear(pooled, pr["11.excitation.0.weight"].detach())), pr["11.excitation.2.weight"].detach()))
    dout = res["gout"].double()
    dpooled, = torch.autograd.grad(gate, pooled, (dout * h).sum((2, 3)))
    t1, t2 = dout * gate.detach()[:, :, None, None] * s, (dpooled / P)[:, :, None, None] * s
    gc = t1 + t2
    assert_close(gc, ref["pre"][4].grad, what + ": g_c rebuilt from the reference's tensors", rel=1e-9)
    mag = t1.abs() + t2.abs()
    neg = ~pos
    red = res["tap"]["red_c"].double()
    ax = (0, 2, 3)
    _within(red[:2 * C:2], gc.sum(ax), mag.sum(ax), what + " red_c sum g_c")
    _within(red[1:2 * C:2], (gc * hh).sum(ax), (mag * hh.abs()).sum(ax), what + " red_c sum g_c hhat")
    # slope: sum over the second branch of dh u, dh = g_c / alpha
    _within(red[2 * C:].sum().view(1), (gc / alpha * u)[neg].sum().view(1), (mag / alpha * u.abs())[neg].sum().view(1), what + " red_c slope words")


def _tcn_sums(res, ref, shape, what):
    """red_t[2c], red_t[2c + 1] as the last pass stores them (train mode) against sum g_t, sum g_t yhat in fp64"""
    B, C, T, V = shape
    pr, bufs = ref["params"], ref["bufs"]
    ax = (0, 2, 3)
    for i in range(2):
        pre_d, pre_p = ref["pre"][2 * i], ref["pre"][2 * i + 1]
        keep = _ref_keep(res["seed"], SALTS[i], P_DROP, pre_d.shape).double()
        gt = pre_d.grad * keep                                     # gradient behind the tcn BatchNorm
        y = ref["leaves"][i].detach()
        yhat = (y - y.mean(ax, keepdim=True)) / torch.sqrt(y.var(ax, unbiased=False, keepdim=True) + 1e-5)
        assert_close(gt.sum(ax), pr["%d.bias" % i].grad, what + ": sum g_t is d beta_t", rel=1e-9)
        assert_close((gt * yhat).sum(ax), pr["%d.weight" % i].grad, what + ": sum g_t yhat is d gamma_t", rel=1e-9)
        sd = torch.where(res["taps"][i].double() > 0, torch.ones_like(keep), torch.full_like(keep, float(pr["%d.weight" % (5 + i)].detach())))
        q = keep * sd * ref["leaves"][4 + i].detach()[:, :, None, None]
        gam, bet = pr["%d.weight" % (2 + i)].detach().view(1, C, 1, 1), pr["%d.bias" % (2 + i)].detach().view(1, C, 1, 1)
        zhat = (pre_p.detach() - bet) / gam
        gp = pre_p.grad
        z = ref["leaves"][4 + i].detach()[:, :, None, None] * torch.where(res["taps"][i].double() > 0, pre_d.detach(), float(pr["%d.weight" % (5 + i)].detach()) * pre_d.detach())
        scale = gam / torch.sqrt(z.var(ax, unbiased=False, keepdim=True) + 1e-5)
        m1, m2 = gp.mean(ax, keepdim=True), (gp * zhat).mean(ax, keepdim=True)
        mag = (scale * q * gp).abs() + (scale * m1 * q).abs() + (scale * m2 * q * zhat).abs()
        red = res["tap"]["red_t"][i].double()
        _within(red[:2 * C:2], gt.sum(ax), mag.sum(ax), what + " red_t[%d] sum g_t" % i)
        _within(red[1:2 * C:2], (gt * yhat).sum(ax), (mag * yhat.abs()).sum(ax), what + " red_t[%d] sum g_t yhat" % i)


def check(device, shape, train, shared):
    """checks 1 - 5 of one shape in one mode on one form of the residuals"""
    B, C, T, V = shape
    merged = (T * V) % 4 == 0
    what = "tail sums %s %s %s" % (shape, "train" if train else "eval", "shared residual" if shared else "separate residuals")
    new = run(device, shape, train, shared, True)
    assert new["tap"]["last_pass"] == merged and new["tap"]["shared"] == (merged and shared), new["tap"]
    ref = reference(new, shape, train, shared)
    floors = _floors(ref, train)
    # 1. every gradient against fp64
    assert_close(new["out"], ref["out"], what + " out", rel=2e-5)
    assert len(new["grads"]) == len(ref["grads"])
    for g, r, fl, k in zip(new["grads"], ref["grads"], floors, ref["names"]):
        assert_close(g, r, "%s grad fp64 %s" % (what, k), rel=5e-5, floor=fl)
    # 2. the derived tcn sums
    if train and merged:
        _tcn_sums(new, ref, shape, what)
    # 3. the compressor sums from the row sums, and the same bits twice
    _compressor_sums(new, ref, shape, what)
    again = run(device, shape, train, shared, True)
    assert torch.equal(new["tap"]["red_c"], again["tap"]["red_c"]), what + ": red_c differs between two runs"
    names = ref["names"]
    for k in ("4.weight", "4.bias", "9.weight"):
        j = names.index(k)
        assert torch.equal(new["grads"][j], again["grads"][j]), "%s: gradient of %s differs between two runs" % (what, k)
    # 4. the routes agree
    old = run(device, shape, train, shared, False)
    assert not old["tap"]["last_pass"] and not old["tap"]["shared"]
    for g, o, fl, k in zip(new["grads"], old["grads"], floors, names):
        assert_close(g, o, "%s grad new | old route %s" % (what, k), rel=5e-5, floor=fl)


def check_shared_bookkeeping(device, shape=MERGED[0]):
    """5. the shared form never writes dr[1], and the entry point refuses the flag on two different residuals"""
    import ctypes
    B, C, T, V = shape
    res = run(device, shape, True, True, True)
    assert res["tap"]["shared"] and res["tap"]["dr1"] is None        # ops hands the kernels no second buffer at all
    f32, f64 = torch.float32, torch.float64
    big = lambda: torch.randn(B, C, T, V, dtype=f32, device=device)
    keepalive = []

    def buf(*s, dtype=f32, fill=None):
        x = torch.zeros(*s, dtype=dtype, device=device) if fill is None else torch.full(s, fill, dtype=dtype, device=device)
        keepalive.append(x)
        return x
    t = _lib.DstdTail()
    t.B, t.C, t.T, t.V, t.train = B, C, T, V, 0                      # eval mode: phase 4 needs no statistics of a forward
    y, r, gp = [big(), big()], big(), [big(), big()]
    w = [torch.randn(B, C, device=device) for _ in range(2)]
    t.y[0], t.y[1], t.r[0], t.r[1], t.w[0], t.w[1] = y[0].data_ptr(), y[1].data_ptr(), r.data_ptr(), r.data_ptr(), w[0].data_ptr(), w[1].data_ptr()
    save = buf(5, 2, C, fill=1.0)
    gam, bet, alp = buf(C, fill=1.1), buf(C, fill=0.1), buf(1, fill=0.2)
    for k, bn in enumerate((t.bn_t[0], t.bn_t[1], t.bn_p[0], t.bn_p[1], t.bn_c)):
        bn.gamma, bn.beta, bn.save, bn.momentum, bn.eps = gam.data_ptr(), bet.data_ptr(), save[k].data_ptr(), 0.1, 1e-5
    t.alpha_d[0] = t.alpha_d[1] = t.alpha_p[0] = t.alpha_p[1] = t.alpha_c = alp.data_ptr()
    t.Wc, t.h0 = buf(C, 2 * C).data_ptr(), big().data_ptr()
    keepalive.extend([y, r, gp, w])
    dout, gate = big(), buf(B, C, fill=0.5)
    t.dout, t.gate = dout.data_ptr(), gate.data_ptr()
    SENT = 12345.0
    dr = [buf(B, C, T, V, fill=SENT), buf(B, C, T, V, fill=SENT)]
    dy, dw = [buf(B, C, T, V), buf(B, C, T, V)], [buf(B, C), buf(B, C)]
    red = [buf(2 * C + _lib.ALPHA_SLOTS, dtype=f64) for _ in range(4)]
    redq = buf(2, _lib.STAT_REPLICAS * 2 * C, dtype=f64)
    for i in range(2):
        t.gp[i], t.dr[i], t.dy[i], t.dw[i], t.red_p[i], t.red_t[i], t.red_q[i] = (gp[i].data_ptr(), dr[i].data_ptr(), dy[i].data_ptr(), dw[i].data_ptr(),
                                                                                  red[i].data_ptr(), red[2 + i].data_ptr(), redq[i].data_ptr())
    t.rs_shared = 1
    stream = ops._stream(dout)
    _lib.call("cg_dstd_tail_bwd", ctypes.byref(t), 4, stream)
    d0, d1 = dr[0].cpu().clone(), dr[1].cpu().clone()
    assert bool((d1 == SENT).all()), "the shared form wrote dr[1]"
    assert bool((d0 != SENT).all()) and bool(torch.isfinite(d0).all())
    # the same launch on separate residual gradients: dr[0] of the shared form is their sum
    t.rs_shared = 0
    _lib.call("cg_dstd_tail_bwd", ctypes.byref(t), 4, stream)
    s0, s1 = dr[0].cpu(), dr[1].cpu()
    assert_close(d0, s0.double() + s1.double(), "shared residual gradient = dr[0] + dr[1]", rel=2.0 ** -22, floor=float((s0.abs() + s1.abs()).max()))
    # the flag on two different residuals is a bad argument
    r2 = big()
    t.r[1], t.rs_shared = r2.data_ptr(), 1
    rc = int(_lib.lib().cg_dstd_tail_bwd(ctypes.byref(t), 4, stream))
    assert rc == -1, "rs_shared with r[0] != r[1] returned %d, expected CG_EARG (-1)" % rc
