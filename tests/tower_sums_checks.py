"""Helpers of the tower-sums tests (CPU shim and MI355X): the channel sums of the producer's BatchNorm / PReLU backward as the collapsing
backward kernels form them on the way (CgRowsConv.sums / red, csrc/collapse_rows.hip), checked directly.

Reference: an fp64 PyTorch evaluation on the CPU of the same f32 inputs - the raw map, the dx tensor THE KERNEL wrote, `save`, gamma, beta,
the slope.  Bound, per channel: |got - ref| <= 16 * 2^-24 * sum |term| (each term is formed in f32 with at most four roundings, the f32
partial over one sample's values of a row adds at most about ten more, everything above is f64).  cg_norm_act_bwd_reduce_many has to meet
the same bound on the same inputs: the new route and the consumer mean the same quantity.

One flipped PReLU branch moves a sum by ~1e-5 of sum |term|, far above the bound, so the inputs keep away from the kinks: the raw map is
+-(0.5 + |n|) with random signs, gamma in [0.7, 1.3], beta in [-0.2, 0.2], and the reference asserts min |u| >= 0.04."""
import ctypes

import torch

from cistgcn_amd import _lib, ops
from loop_shapes import _geom

EPS = 2.0 ** -24
BOUND = 16 * EPS
GUARD = 32           # elements of NaN around every output and scratch buffer: nothing is written outside, nothing has to be zeroed

# (B, M, T, V, O): the map x is (B, M, T, V), the convolution collapses T (frame axis) or V (joint axis) into O outputs
FRAME = (
    (805, 6, 14, 7, 5),      # two K ranges, the last short; three samples per slice, short last slice; channel 4 straddles the ranges; channels change inside a wave's 16 rows
    (5, 4, 1, 16, 16),       # T = 1: every row its own channel
    (5, 3, 72, 6, 8),        # a channel longer than a range, spread over two ranges
    (3, 8, 16, 32, 64),      # the limits: V = 32, O = 64
)
JOINT = (
    (805, 12, 5, 6, 5),      # two ranges, channel 10 straddles; planes of 30 floats: 8-byte aligned
    (3, 4, 3, 5, 3),         # planes of 15 floats: 4-byte aligned
    (3, 6, 33, 22, 20),      # three ranges, T = 33
    (2, 8, 64, 16, 64),      # the limits: T = 64, O = 64
)


def ident(shape):
    return "-".join(str(s) if not isinstance(s, tuple) else "x".join(map(str, s)) for s in shape)


def assert_properties():
    """the loop properties the shapes are chosen for, asked from the library's own geometry query"""
    def geom(shape, cols):
        B, M, T, V, O = shape
        return _geom("cg_collapse_geometry", B, M, T, V, O, 1 if cols else 0, n=3)
    B, M, T, V, O = FRAME[0]
    kranges, slices, per = geom(FRAME[0], False)
    assert kranges == 2 and (M * T) % 64 != 0 and per >= 3 and B - (slices - 1) * per < per, (kranges, slices, per)
    assert 4 * T < 64 < 5 * T and T < 16                       # channel 4 straddles; several channels in a wave's 16 rows
    assert FRAME[1][2] == 1
    assert FRAME[2][2] > 64 and geom(FRAME[2], False)[0] >= 2
    assert geom(FRAME[3], False)[0] >= 2 and FRAME[3][3] == 32 and FRAME[3][4] == 64
    B, M, T, V, O = JOINT[0]
    kranges, slices, per = geom(JOINT[0], True)
    assert kranges == 2 and per >= 3 and B - (slices - 1) * per < per and 10 * V < 64 < 11 * V, (kranges, slices, per)
    assert (T * V) % 4 == 2 and (JOINT[1][2] * JOINT[1][3]) % 2 == 1
    assert geom(JOINT[2], True)[0] == 3 and JOINT[2][2] == 33
    assert JOINT[3][2] == 64 and JOINT[3][4] == 64


def _guarded(n, dtype, device, fill=float("nan")):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, what):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    assert bool(torch.isnan(g).all()), "%s: written outside the buffer" % what


def make_inputs(shape, cols, train, seed):
    """CPU f32 operands: raw map, collapsing weight, dy, save (mean, rstd), gamma, beta, slope"""
    B, M, T, V, O = shape
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(B, M, T, V, generator=g) < 0.5, -1.0, 1.0)
    x = (sign * (0.5 + torch.randn(B, M, T, V, generator=g).abs())).float()
    w = (0.2 * torch.randn(O, M, V if cols else T, generator=g)).float()
    dy = torch.randn(B, O, T if cols else V, generator=g).float()
    gamma = (0.7 + 0.6 * torch.rand(M, generator=g)).float()
    beta = (-0.2 + 0.4 * torch.rand(M, generator=g)).float()
    alpha = torch.tensor([0.25])
    if train:        # batch statistics, as the forward saves them
        xd = x.double()
        mean = xd.mean((0, 2, 3))
        rstd = 1.0 / torch.sqrt(xd.var((0, 2, 3), unbiased=False) + 1e-5)
    else:            # running statistics, as the forward hands them out in eval mode
        mean = -0.03 + 0.06 * torch.rand(M, generator=g).double()
        rstd = 1.0 / torch.sqrt(1.0 + 0.6 * torch.rand(M, generator=g).double() + 1e-5)
    save = torch.stack([mean, rstd]).float().contiguous()
    return dict(x=x, w=w, dy=dy, gamma=gamma, beta=beta, alpha=alpha, save=save, cols=cols, train=train)


def run_kernel(device, inp, want_sums=True):
    """the collapsing backward with the sums asked for: dx, dW, red, (dgamma, dbeta, dalpha) - every buffer between NaN guards"""
    d = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in inp.items()}
    x, w = d["x"], d["w"]
    B, M, T, V = x.shape
    O, cols = w.shape[0], d["cols"]
    t = _lib.RowsConv()
    t.B, t.C, t.T, t.V, t.O = B, M, T, V, O
    t.x, t.W, t.dy = x.data_ptr(), w.data_ptr(), d["dy"].data_ptr()
    t.in_on, t.in_train = 1, 1 if d["train"] else 0
    t.in_bn.gamma, t.in_bn.beta, t.in_bn.save = d["gamma"].data_ptr(), d["beta"].data_ptr(), d["save"].data_ptr()
    t.in_bn.momentum, t.in_bn.eps = 0.1, 1e-5
    t.in_alpha = d["alpha"].data_ptr()
    lib = _lib.lib()
    n_ws = int(lib.cg_collapse_cols_ws_floats(M, V, O) if cols else lib.cg_collapse_rows_ws_floats(M, T, O))
    n_sums = int(lib.cg_collapse_sums_ws_floats(M, V if cols else T))
    assert n_sums % 2 == 0
    f32, f64 = torch.float32, torch.float64
    bufs = {"dx": _guarded(x.numel(), f32, device), "dW": _guarded(w.numel(), f32, device), "ws": _guarded(n_ws, f32, device),
            "sums": _guarded(n_sums // 2, f64, device), "red": _guarded(2 * M + _lib.ALPHA_SLOTS, f64, device), "small": _guarded(3 * M, f32, device)}
    t.dx, t.dW, t.ws = bufs["dx"][1].data_ptr(), bufs["dW"][1].data_ptr(), bufs["ws"][1].data_ptr()
    if want_sums:
        small = bufs["small"][1]
        t.sums, t.red = bufs["sums"][1].data_ptr(), bufs["red"][1].data_ptr()
        t.dgamma, t.dbeta, t.dalpha = small[:M].data_ptr(), small[M:2 * M].data_ptr(), small[2 * M:].data_ptr()
    _lib.call("cg_collapse_cols_bwd" if cols else "cg_collapse_rows_bwd", ctypes.byref(t), ops._stream(x))
    for k, (buf, _) in bufs.items():
        _guards_intact(buf.cpu(), k)
    out = {k: v[1].cpu() for k, v in bufs.items()}
    out["dx"] = out["dx"].view(B, M, T, V)
    assert bool(torch.isfinite(out["dx"]).all()) and bool(torch.isfinite(out["dW"]).all())
    if want_sums:
        assert bool(torch.isfinite(out["red"]).all()), "red holds words the fold did not write"
        assert bool(torch.isfinite(out["small"][:2 * M + 1]).all())
    return out


def run_reduce(device, inp, dx):
    """cg_norm_act_bwd_reduce_many on the same operands (the raw map and the kernel's dx): red, small (3, M)"""
    d = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in inp.items()}
    x, dh = d["x"], dx.to(device)
    M = x.shape[1]
    arr = (_lib.NormAct * 1)()
    a = arr[0]
    a.x, a.xv, a.dy, a.dyv = x.data_ptr(), ops._view4(x), dh.data_ptr(), ops._view4(dh)
    a.bn_mode = 1 if d["train"] else 2
    a.gamma, a.beta = d["gamma"].data_ptr(), d["beta"].data_ptr()
    a.momentum, a.eps = 0.1, 1e-5
    a.save_mean, a.save_rstd = d["save"][0].data_ptr(), d["save"][1].data_ptr()
    a.alpha, a.alpha_n = d["alpha"].data_ptr(), 1
    red = torch.zeros(2 * M + _lib.ALPHA_SLOTS, dtype=torch.float64, device=device)
    small = torch.zeros(3, M, dtype=torch.float32, device=device)
    a.red, a.dgamma, a.dbeta, a.dalpha = red.data_ptr(), small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr()
    _lib.call("cg_norm_act_bwd_reduce_many", arr, 1, ops._stream(x))
    return red.cpu(), small.cpu()


def reference(inp, dx):
    """fp64 on the CPU: (s1, s2 per channel, sa) and the sums of |term| the bound is built from"""
    x, dh = inp["x"].double(), dx.double()
    M = x.shape[1]
    mean, rstd = inp["save"][0].double().view(1, M, 1, 1), inp["save"][1].double().view(1, M, 1, 1)
    gamma, beta, alpha = inp["gamma"].double().view(1, M, 1, 1), inp["beta"].double().view(1, M, 1, 1), float(inp["alpha"][0])
    u = (x - mean) * (gamma * rstd) + beta
    assert float(u.abs().min()) >= 0.04, "an input sits at a PReLU kink: min |u| = %g" % float(u.abs().min())
    pos = u > 0
    gh = torch.where(pos, dh, alpha * dh)
    xhat = (x - mean) * rstd
    t2 = gh * xhat
    ta = torch.where(pos, torch.zeros_like(dh), dh * u)
    ax = (0, 2, 3)
    return dict(s1=gh.sum(ax), s2=t2.sum(ax), sa=ta.sum(), a1=gh.abs().sum(ax), a2=t2.abs().sum(ax), aa=ta.abs().sum())


def _within(got, ref, mag, what):
    err = (got.double() - ref).abs()
    lim = BOUND * mag
    worst = float((err / lim.clamp_min(1e-300)).max())
    print("%s: max |got - ref| / (16 * 2^-24 * sum |term|) = %.3g" % (what, worst))
    assert bool((err <= lim).all()), "%s: error %.3g of the bound (got %s, ref %s)" % (what, worst, got.flatten()[:4].tolist(), ref.flatten()[:4].tolist())


def compare(red, small, ref, M, what):
    """red: [2M + slots] f64; small: dgamma | dbeta | dalpha"""
    small = small.reshape(-1)
    _within(red[:2 * M:2], ref["s1"], ref["a1"], what + " red sum gh")
    _within(red[1:2 * M:2], ref["s2"], ref["a2"], what + " red sum gh xhat")
    _within(red[2 * M:].sum().view(1), ref["sa"].view(1), ref["aa"].view(1), what + " red slope words")
    _within(small[:M], ref["s2"], ref["a2"], what + " dgamma")
    _within(small[M:2 * M], ref["s1"], ref["a1"], what + " dbeta")
    _within(small[2 * M:2 * M + 1], ref["sa"].view(1), ref["aa"].view(1), what + " dalpha")


def check_sums(device, shape, cols, train, seed=11):
    """the sums of the collapsing backward and of cg_norm_act_bwd_reduce_many against fp64, and twice the same bits"""
    inp = make_inputs(shape, cols, train, seed)
    what = "tower sums %s %s %s" % ("joint" if cols else "frame", shape, "train" if train else "eval")
    M = shape[1]
    out = run_kernel(device, inp)
    ref = reference(inp, out["dx"])
    compare(out["red"], out["small"], ref, M, what)
    red2, small2 = run_reduce(device, inp, out["dx"])
    compare(red2, small2, ref, M, what + " (cg_norm_act_bwd_reduce_many)")
    again = run_kernel(device, inp)
    for k in ("red", "small", "dx", "dW"):
        assert torch.equal(out[k][:2 * M + 1] if k == "small" else out[k], again[k][:2 * M + 1] if k == "small" else again[k]), "%s: %s differs between two runs" % (what, k)
    plain = run_kernel(device, inp, want_sums=False)            # with the new pointers null the entry point behaves as before
    assert torch.equal(plain["dx"], out["dx"]) and torch.equal(plain["dW"], out["dW"]), what + ": dx / dW depend on the sums switch"
    assert bool(torch.isnan(plain["red"]).all()) and bool(torch.isnan(plain["sums"]).all())


def _tower(device, shape, fuse, train=True):
    """ops.tower_maps(defer=True) + collapsing convolutions (frame / joint alternating) forward and backward; fuse[k] False: map k's sums
    come from cg_norm_act_bwd_reduce_many.  Returns the transform records and [dx, every parameter gradient]."""
    from torch import nn
    B, C, Ms, T, V, O = shape
    g = torch.Generator().manual_seed(23)
    mods = []
    for k, M in enumerate(Ms):
        conv, bn, pr = nn.Conv2d(C, M, 1, bias=False), nn.BatchNorm2d(M), nn.PReLU()
        col = nn.Conv2d(M, O, (T, 1) if k % 2 == 0 else (1, V), bias=False)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.4)
            col.weight.copy_(torch.randn(col.weight.shape, generator=g) * 0.2)
            bn.weight.copy_(1 + 0.3 * torch.randn(M, generator=g)); bn.bias.copy_(0.3 * torch.randn(M, generator=g))
            pr.weight.fill_(0.1 + 0.1 * k)
        mods.append(nn.Sequential(conv, bn, pr, col))
    net = nn.ModuleList(mods).to(device).train(train)
    x = (0.3 + torch.randn(B, C, T, V, generator=g)).to(device).requires_grad_(True)
    gs = [torch.randn(B, O, 1, V, generator=g) if k % 2 == 0 else torch.randn(B, O, T, 1, generator=g) for k in range(len(Ms))]
    ops.begin_step(device)
    ys, trs = ops.tower_maps(x, [m[0].weight.view(m[0].out_channels, C) for m in net], [m[1] for m in net], [m[2] for m in net], train, defer=True)
    outs = []
    for k, m in enumerate(net):
        trs[k]["fuse_sums"] = bool(fuse[k])
        w = m[3].weight.view(O, m[3].in_channels, -1)
        if k % 2 == 0:
            outs.append(ops.collapse_rows(ys[k], w, transform=trs[k])[0].unsqueeze(2))
        else:
            outs.append(ops.collapse_cols(ys[k], w, transform=trs[k])[0].unsqueeze(3))
    torch.autograd.backward(outs, [t.to(device) for t in gs])
    names = ["dx"] + [k for k, _ in net.named_parameters()]
    grads = [x.grad.cpu()] + [p.grad.cpu() for _, p in net.named_parameters()]
    return trs, names, grads


def check_routes_agree(device, shape, fuse):
    """dx and every gradient of the route `fuse` against the route through cg_norm_act_bwd_reduce_many for all maps: equal to
    2^-20 max |grad| per tensor (only the last bits of the f32 casts of the channel means m1, m2 may differ)"""
    n = len(shape[2])
    trs, names, got = _tower(device, shape, fuse)
    for k in range(n):
        assert ("red" in trs[k]) == bool(fuse[k]), "map %d: sums %s" % (k, "missing" if fuse[k] else "formed although not asked for")
    trs0, _, ref = _tower(device, shape, [False] * n)
    assert not any("red" in tr for tr in trs0)
    for name, a, b in zip(names, got, ref):
        lim = 2.0 ** -20 * float(b.abs().max())
        err = float((a - b).abs().max())
        print("routes %s %s: max |diff| = %.3g, 2^-20 max |grad| = %.3g" % (shape, name, err, lim))
        assert err <= lim, "%s: %s differs by %.3g (limit %.3g)" % (shape, name, err, lim)
