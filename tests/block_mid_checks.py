"""Helpers of the block mid-section tests (CPU shim and MI355X): `ops.block_mid` (csrc/block_mid.hip) against the chain it replaces and
against fp64.

Per item  x (B,C,L) -> BatchNorm2d -> Dropout [-> PReLU] = h,  then  full: z[b,o] = sum_{c,l} W[o,c,l] h[b,c,l]  or  pointwise:
y[b,o,l] = sum_c W[o,c] h[b,c,l].  The composite route is `ops.norm_act_many` + `ops.contract_many` as CISTGCN._block_staged calls them when
the new route is off.  Both routes run on the same f32 inputs, parameters, seed and site ids; the reference is an fp64 evaluation on the CPU
with the keep masks `ops.norm_act_many` draws on a constant tensor.

Condition, per tensor (every output, input gradient and parameter gradient): err = max |got - ref| / max |ref|, and
err(new) <= 2 * err(composite): the yardstick is the code path the new one replaces, the factor two covers a different summation order.
Both figures are printed.

One flipped PReLU branch moves an output far above either error, so the inputs keep away from the kinks as in tower_sums_checks.py: x is
+-(0.6 + |n|) with random signs, centred per channel (the batches here are small), gamma in [0.7, 1.3], beta in [-0.2, 0.2]; the reference
asserts min |u| >= KINK on the kept elements."""
import ctypes

import torch
from torch import nn

from cistgcn_amd import _lib, ops
from loop_shapes import _geom

GUARD = 32
KINK = 0.02
FULL, PW = 0, 1

# name -> (B, items); an item is (kind, C, L, O, with PReLU).  Items 0 and 1 of a case marked `stacked` are channel ranges of one
# (B, 2C, L) tensor with one sums buffer, as the stacked gate convolution of a block hands them over.
CASES = {
    # one item; five slices of eight samples, the last one short (5); C*L = 110: no multiple of 4; O = 10: two rows of the third group of four unused
    "one": (37, [(FULL, 5, 22, 10, True)], False),
    # six mixed items, the gates as channel ranges; pointwise slices of 3 / 2 / 8 / 8 samples; O = 50, 22, 10: no multiples of 16; C*L = 125
    "six": (37, [(FULL, 6, 22, 50, True), (FULL, 6, 22, 50, True), (PW, 32, 22, 50, False), (PW, 32, 50, 22, False), (PW, 5, 25, 10, False), (PW, 6, 22, 22, True)], True),
    # B = 2; the two kinds at different sizes; C*L = 1250: two passes of the full backward over the columns, the second one short
    "two": (2, [(FULL, 25, 50, 22, True), (PW, 3, 7, 5, False)], False),
    # L = 1 and C = 1
    "thin": (5, [(FULL, 4, 1, 5, True), (PW, 1, 9, 4, False), (FULL, 1, 64, 3, True), (PW, 7, 1, 64, False)], False),
    # the limits C = L = O = 64: slices of two samples (full) and one sample (pointwise), all sixteen waves busy with output rows, four passes over the columns
    "limits": (3, [(FULL, 64, 64, 64, True), (PW, 64, 64, 64, False)], False),
}
MODES = {"train-drop": (True, 0.1), "train": (True, 0.0), "eval-drop": (False, 0.1)}
# channels 0 and 1 of both items with a variance comparable to eps (checks.LOW_VAR_BATCH / LOW_VAR_RUNNING): check_low_variance
LOW_VAR_CASE = (37, [(FULL, 5, 22, 10, True), (PW, 6, 22, 22, True)], False)


def geometry(B, item):
    kind, C, L, O, _ = item
    return _geom("cg_block_mid_geometry", B, kind, C, L, O, n=8)


def assert_properties():
    """the loop edges the cases are chosen for, asked from the library's own geometry query"""
    B, items, _ = CASES["one"]
    sb, ns, _, _, part, wpart, og, kp = geometry(B, items[0])
    assert sb == 8 and ns >= 3 and B % sb != 0 and B - (ns - 1) * sb < sb and (items[0][1] * items[0][2]) % 4 != 0 and og == 1 and kp == 1, (sb, ns, og, kp)
    assert part == ns * (2 * 5 + 1) and wpart == ns * 10 * 110
    B, items, _ = CASES["six"]
    g = [geometry(B, it) for it in items]
    assert len(items) == 6 and [x[0] for x in g] == [8, 8, 3, 2, 8, 8] and all(x[1] >= 3 for x in g), g
    assert g[0][6] == 1 and items[0][3] % 16 != 0 and items[0][3] % 4 != 0 and (5 * 25) % 4 != 0        # O = 50: thirteen waves, the last group of four rows half used
    assert all(B % x[0] != 0 for x in g)
    B, items, _ = CASES["two"]
    g = [geometry(B, it) for it in items]
    assert B == 2 and g[0][7] == 2 and (25 * 50) % 1024 != 0 and g[0][1] == 1 and g[1][1] == 1
    B, items, _ = CASES["thin"]
    assert items[0][2] == 1 and items[3][2] == 1 and items[1][1] == 1 and items[2][1] == 1
    B, items, _ = CASES["limits"]
    g = [geometry(B, it) for it in items]
    assert g[0][0] == 2 and g[0][1] == 2 and g[0][6] == 1 and g[0][7] == 4 and g[1][0] == 1 and g[1][1] == 3, g
    assert max(g[0][3], g[1][3]) > 64 * 1024                  # the backward's LDS image is above the default limit
    lib = _lib.lib()
    assert lib.cg_block_mid_supported(3, 0, 65, 4, 4) == 0 and lib.cg_block_mid_supported(3, 1, 4, 65, 4) == 0 and lib.cg_block_mid_supported(3, 1, 4, 4, 65) == 0
    assert lib.cg_block_mid_supported(3, 2, 4, 4, 4) == 0 and lib.cg_block_mid_supported(0, 0, 4, 4, 4) == 0


def make_inputs(name, seed=5, low_var=False):
    """CPU f32 operands of a case (a name of CASES or a case itself).  low_var: channels 0 and 1 of every x centred and scaled to the
    variances checks.LOW_VAR_BATCH, their running variances checks.LOW_VAR_RUNNING, their beta 0 (|u| stays above KINK)."""
    B, items, stacked = CASES[name] if isinstance(name, str) else name
    g = torch.Generator().manual_seed(seed)
    data = []
    for kind, C, L, O, act in items:
        sign = torch.where(torch.rand(B, C, L, generator=g) < 0.5, -1.0, 1.0)
        x = sign * (0.6 + torch.randn(B, C, L, generator=g).abs())
        x = x - x.mean((0, 2), keepdim=True)           # a small batch moves a channel's mean by ~0.15: centred, every |x| stays above 0.4
        d = dict(kind=kind, act=act, x=x.float(),
                 w=(0.3 * torch.randn(O, C, L, generator=g) if kind == FULL else 0.3 * torch.randn(O, C, generator=g)).float(),
                 dy=(torch.randn(B, O, generator=g) if kind == FULL else torch.randn(B, O, L, generator=g)).float(),
                 gamma=(0.7 + 0.6 * torch.rand(C, generator=g)).float(), beta=(-0.2 + 0.4 * torch.rand(C, generator=g)).float(),
                 rm=(-0.03 + 0.06 * torch.rand(C, generator=g)).float(), rv=(1.0 + 0.6 * torch.rand(C, generator=g)).float(),
                 alpha=torch.tensor([0.25]))
        if low_var:
            import checks
            d["x"] = checks._low_var_input(d["x"])
            d["rv"][:2] = torch.tensor(checks.LOW_VAR_RUNNING)
            d["rm"][:2] *= 1e-3
            d["beta"][:2] = 0.0
        data.append(d)
    return B, data, stacked


def producer_sums(x):
    """f64 {sum, sum of squares} per channel of x (B,C,L) in the layout the collapse kernels leave: [replicas][C][2], sample b in replica b mod R"""
    R = _lib.STAT_REPLICAS
    B, C, L = x.shape
    st = torch.zeros(R, C, 2, dtype=torch.float64)
    xd = x.double()
    for r in range(R):
        st[r, :, 0] = xd[r::R].sum((0, 2))
        st[r, :, 1] = xd[r::R].pow(2).sum((0, 2))
    return st


def _modules(data, device):
    mods = []
    for d in data:
        C = d["x"].shape[1]
        bn = nn.BatchNorm2d(C, momentum=1.0)          # momentum 1: the running statistics afterwards ARE the batch statistics the forward saved
        pr = nn.PReLU() if d["act"] else None
        with torch.no_grad():
            bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["rm"]); bn.running_var.copy_(d["rv"])
            if pr is not None:
                pr.weight.copy_(d["alpha"])
        w = nn.Parameter(d["w"].clone())
        mods.append((bn.to(device), pr.to(device) if pr is not None else None, w.to(device).detach().requires_grad_(True)))
    return mods


def run_route(device, B, data, stacked, new, train, p, salts, seed=1234):
    """forward + backward of one route; per item a dict of CPU tensors"""
    mods = _modules(data, device)
    for bn, pr, _ in mods:
        bn.train(train)
    xs, leaves, sums = [], [], []
    if stacked:                      # items 0 and 1: channel ranges of one tensor
        both = torch.cat([data[0]["x"], data[1]["x"]], 1).to(device).requires_grad_(True)
        C = data[0]["x"].shape[1]
        st = producer_sums(both.detach().cpu()).to(device)
        xs += [both[:, :C], both[:, C:]]
        leaves += [both, None]
        sums += [(st, 0, 2 * C), (st, C, 2 * C)]
    for d in data[len(xs):]:
        x = d["x"].clone().to(device).requires_grad_(True)
        xs.append(x); leaves.append(x)
        sums.append((producer_sums(d["x"]).to(device), 0, d["x"].shape[1]))
    ops.manual_seed(seed, torch.device(device))
    ops.begin_step(torch.device(device))
    taps = []
    if new:
        items = [dict(kind=d["kind"], x=x, bn=bn, prelu=pr, weight=w, salt=s, stats=st if train else None)
                 for d, x, (bn, pr, w), s, st in zip(data, xs, mods, salts, sums)]
        ys = ops.block_mid(items, train, drop_p=p, taps=taps)
        hs = [None] * len(data)
    else:
        # as CISTGCN._block_staged: the gates' sums come from the row kernel's own pass, the towers' from the collapse kernels
        calls = [dict(x=(x.unsqueeze(2), None if d["kind"] == FULL or not train else st[0]), bn=bn, train=train, drop_p=p, salt=s, prelu=pr)
                 for d, x, (bn, pr, w), s, st in zip(data, xs, mods, salts, sums)]
        hs = ops.norm_act_many(calls)
        citems = [("ocw,bchw->boh", w, h, None, None, None) if d["kind"] == FULL else ("oc,bchw->bohw", w, h, None, None, None)
                  for d, h, (bn, pr, w) in zip(data, hs, mods)]
        ys = [y for y, _ in ops.contract_many(citems)]
        taps = [h.detach() if d["act"] else None for d, h in zip(data, hs)]
    torch.autograd.backward(ys, [d["dy"].to(device).view(y.shape) for d, y in zip(data, ys)])
    out = []
    for i, (d, y, (bn, pr, w)) in enumerate(zip(data, ys, mods)):
        C = d["x"].shape[1]
        if stacked and i < 2:
            dx = leaves[0].grad[:, i * C:(i + 1) * C]
        else:
            dx = leaves[i].grad
        r = dict(y=y.detach().reshape(d["dy"].shape), dx=dx, dgamma=bn.weight.grad, dbeta=bn.bias.grad, dW=w.grad,
                 rm=bn.running_mean, rv=bn.running_var, nbt=bn.num_batches_tracked)
        if pr is not None:
            r["dalpha"] = pr.weight.grad
            r["tap"] = taps[i].reshape(d["x"].shape)
        if hs[i] is not None:
            r["h"] = hs[i].detach().reshape(d["x"].shape)
        out.append({k: v.detach().cpu().clone() for k, v in r.items()})
    return out


def keep_masks(device, B, data, p, salts, seed=1234):
    """the keep factors (0 or 1/(1-p)) the row kernels draw at the sites `salts`: norm_act_many on a constant tensor"""
    ops.manual_seed(seed, torch.device(device))
    ops.begin_step(torch.device(device))
    ones = [torch.ones(B, d["x"].shape[1], 1, d["x"].shape[2], device=device) for d in data]
    ks = ops.norm_act_many([dict(x=o, train=True, drop_p=p, salt=s) for o, s in zip(ones, salts)])
    return [k.cpu().reshape(d["x"].shape).double() for k, d in zip(ks, data)]


def reference(d, keep, train, dtype=torch.float64):
    """fp64 on the CPU: outputs and gradients of one item (dtype: the same chain in float32, the yardstick of check_off_centre)"""
    x = d["x"].detach().clone().to(dtype).requires_grad_(True)
    gamma, beta = d["gamma"].detach().clone().to(dtype).requires_grad_(True), d["beta"].detach().clone().to(dtype).requires_grad_(True)
    alpha, w = d["alpha"].detach().clone().to(dtype).requires_grad_(True), d["w"].detach().clone().to(dtype).requires_grad_(True)
    C = x.shape[1]
    if train:
        mean, var = x.mean((0, 2)), x.var((0, 2), unbiased=False)
    else:
        mean, var = d["rm"].to(dtype), d["rv"].to(dtype)
    u = ((x - mean.view(1, C, 1)) / torch.sqrt(var.view(1, C, 1) + 1e-5) * gamma.view(1, C, 1) + beta.view(1, C, 1)) * keep.to(dtype)
    if d["act"]:
        live = u.detach().abs()[keep > 0]
        assert float(live.min()) >= KINK, "an input sits at a PReLU kink: min |u| = %g" % float(live.min())
        h = torch.where(u > 0, u, alpha * u)
    else:
        h = u
    y = torch.einsum("ocl,bcl->bo", w, h) if d["kind"] == FULL else torch.einsum("oc,bcl->bol", w, h)
    (y * d["dy"].to(dtype)).sum().backward()
    r = dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dW=w.grad, mean=mean.detach(), var=var.detach())
    if d["act"]:
        r["dalpha"] = alpha.grad
        r["tap"] = h.detach()
    return r


def _err(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def check_operator(device, name, mode):
    """tests 1, 2 and 4: both routes against fp64, the factor-two condition, masks and taps element for element, running statistics"""
    train, p = MODES[mode]
    B, data, stacked = make_inputs(name)
    salts = [11 + 3 * i for i in range(len(data))]
    new = run_route(device, B, data, stacked, True, train, p, salts)
    old = run_route(device, B, data, stacked, False, train, p, salts)
    if train and p > 0:
        keeps = keep_masks(device, B, data, p, salts)
    else:
        keeps = [torch.ones(d["x"].shape, dtype=torch.float64) for d in data]
    failures = []
    for i, d in enumerate(data):
        ref = reference(d, keeps[i], train)
        what = "block_mid %s %s item %d (%s C%d L%d O%d)" % (name, mode, i, "full" if d["kind"] == FULL else "pw", d["x"].shape[1], d["x"].shape[2], d["w"].shape[0])
        for k in ("y", "dx", "dgamma", "dbeta", "dalpha", "dW"):
            if k not in ref:
                continue
            assert bool(torch.isfinite(new[i][k]).all()), what + ": " + k + " not finite"
            en, eo = _err(new[i][k].reshape(ref[k].shape), ref[k]), _err(old[i][k].reshape(ref[k].shape), ref[k])
            print("%s %-6s err new %.3e  composite %.3e  ratio %.2f" % (what, k, en, eo, en / eo if eo > 0 else float("inf") if en > 0 else 0.0))
            if not en <= 2 * eo:
                failures.append("%s %s: new %.3e > 2 x composite %.3e" % (what, k, en, eo))
        # masks and branches: element for element
        if d["act"]:
            assert torch.equal(new[i]["tap"] == 0, old[i]["tap"] == 0), what + ": dropped positions of the tap differ"
            assert torch.equal(new[i]["tap"] > 0, old[i]["tap"] > 0), what + ": PReLU branches differ"
            lim = 2.0 ** -20 * float(ref["tap"].abs().max())
            assert float((new[i]["tap"].double() - ref["tap"]).abs().max()) <= lim and float((old[i]["tap"].double() - ref["tap"]).abs().max()) <= lim, what + ": tap"
        # dropped positions: the input gradient vanishes exactly where the mask says so (in eval mode and with p = 0 nowhere)
        dropped = keeps[i] == 0
        if train:
            assert bool((new[i]["dx"].double() - old[i]["dx"].double()).abs().max() <= 1e-3 * max(1.0, float(ref["dx"].abs().max())))
        if "h" in old[i]:
            assert torch.equal(old[i]["h"] == 0, dropped) or not (train and p > 0), what + ": composite mask"
        if not train:
            assert torch.equal(new[i]["dx"] == 0, old[i]["dx"] == 0), what + ": zero pattern of dx"
        # batch statistics as saved (momentum 1: running = batch) and the running statistics' bookkeeping
        for k in ("rm", "rv"):
            a, b = new[i][k].double(), old[i][k].double()
            assert bool(((a - b).abs() <= 2.0 ** -21 * b.abs().clamp_min(1e-3)).all()), "%s: %s differs from the composite route: %s vs %s" % (what, k, a[:4].tolist(), b[:4].tolist())
        assert int(new[i]["nbt"]) == int(old[i]["nbt"]) == (1 if train else 0)
        if train:
            assert bool(((new[i]["rm"].double() - ref["mean"]).abs() <= 2.0 ** -20 * ref["mean"].abs().clamp_min(1e-2)).all()), what + ": batch mean"
    assert not failures, "\n".join(failures)


def check_low_variance(device):
    """two BatchNorm channels whose variance is comparable to eps (make_inputs(low_var=True)), both item kinds, train and eval mode.  The
    condition of check_operator compares two routes that share csrc/cg_bn.h, so a wrong eps passes it; here the new route is held to the
    fp64 evaluation itself: the PReLU taps (BatchNorm + PReLU, element for element) to the 2^-20 * max |tap| of check_operator, outputs to
    2e-5 * max(1, max |ref|), gradients to 5e-5 * max(1e-3, max |ref|) - the bounds of the other fused BatchNorm families (tests/checks.py)."""
    from helpers import assert_close
    B, data, stacked = make_inputs(LOW_VAR_CASE, low_var=True)
    salts = [11 + 3 * i for i in range(len(data))]
    for mode in ("train", "eval-drop"):
        train, p = MODES[mode]
        new = run_route(device, B, data, stacked, True, train, p, salts)
        for i, d in enumerate(data):
            ref = reference(d, torch.ones(d["x"].shape, dtype=torch.float64), train)
            what = "block_mid low variance %s item %d" % (mode, i)
            if train:
                var = ref["var"][:2].tolist()
                assert 0.8e-5 < var[0] < 1.0e-5 and 0.08e-5 < var[1] < 0.12e-5, var
            assert float((new[i]["tap"].double() - ref["tap"]).abs().max()) <= 2.0 ** -20 * float(ref["tap"].abs().max()), what + ": tap"
            assert_close(new[i]["y"].reshape(ref["y"].shape), ref["y"], what + " y", rel=2e-5)
            for k in ("dx", "dgamma", "dbeta", "dalpha", "dW"):
                assert_close(new[i][k].reshape(ref[k].shape), ref[k], "%s %s" % (what, k), rel=5e-5, floor=max(1e-3, float(ref[k].abs().max())))


OFF_CENTRE_CASES = (LOW_VAR_CASE, (37, [(FULL, 6, 22, 50, True), (PW, 32, 50, 22, False)], False))


def check_off_centre(device):
    """channels 0 and 1 of every item far off centre (checks.OFF_CENTRE), both item kinds, train and eval mode.  As in check_low_variance the
    new route is held to the fp64 evaluation itself (both routes of check_operator share csrc/cg_bn.h); the bound is
    checks.assert_within_stock: 4 x the error of `reference` in float32, on top of the bounds of check_low_variance.  The forward takes the
    producer's f64 sums; the backward forms dgamma / dbeta and the two means of the BatchNorm backward itself.  Cases: the one of
    check_low_variance, and the widest full item with the pointwise item of the longest rows of CASES["six"]."""
    import checks
    for case in OFF_CENTRE_CASES:
        B, base, stacked = make_inputs(case)
        salts = [11 + 3 * i for i in range(len(base))]
        for mode in ("train", "eval-drop"):
            train, p = MODES[mode]

            def build(ratios):
                data = []
                for d in base:
                    d = dict(d)
                    d["x"] = checks._off_centre_input(d["x"], ratios=ratios)
                    d["rm"], d["rv"] = d["rm"].clone(), d["rv"].clone()
                    for c, r in enumerate(ratios):
                        if r:
                            d["rv"][c] = float(d["x"][:, c].double().var(unbiased=False))
                            d["rm"][c] = r * float(d["rv"][c].double().sqrt())
                    data.append(d)
                return data

            def stock(dtype, ratios):
                res = {}
                for i, d in enumerate(build(ratios)):
                    ref = reference(d, torch.ones(d["x"].shape, dtype=torch.float64), train, dtype)
                    res.update({"item %d %s" % (i, k): ref[k] for k in ("y", "dx", "dgamma", "dbeta", "dalpha", "dW", "tap") if k in ref})
                    if train:
                        res["item %d mean" % i] = ref["mean"]
                return res

            def kernel():
                data = build(checks.OFF_CENTRE)
                new = run_route(device, B, data, stacked, True, train, p, salts)
                res = {}
                for i, d in enumerate(data):
                    res.update({"item %d %s" % (i, k): new[i][k].reshape(d["dy"].shape if k == "y" else new[i][k].shape) for k in ("y", "dx", "dgamma", "dbeta", "dalpha", "dW", "tap") if k in new[i]})
                    if train:
                        res["item %d mean" % i] = new[i]["rm"]          # momentum 1: the running mean is the batch mean the forward saved
                return res

            def family(name, refs):
                ref = refs[name].double()
                k = name.split()[-1]
                if k == "tap":          # 2^-20 * max|tap| in check_low_variance: a float32 mean of a channel at 300 std is itself 2^-24 * 300 std off, 9e-6 here - stock alone
                    return None
                if k in ("y", "mean"):
                    return 2e-5 * max(1.0, float(ref.abs().max()))
                return 5e-5 * max(1e-3, float(ref.abs().max()))

            checks.assert_within_stock("block_mid off centre B%d %s %s" % (B, [it[:4] for it in case[1]], mode), kernel, stock, family)


def _guarded(n, dtype, device):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def run_direct(device, B, data, train, p, salts, seed=1234):
    """the entry points called directly with every output and scratch buffer between NaN guards; returns per item the CPU tensors"""
    dev = torch.device(device)
    ops.manual_seed(seed, dev)
    ops.begin_step(dev)
    f32, f64 = torch.float32, torch.float64
    t = _lib.BlockMid()
    t.B, t.train, t.n, t.drop_p = B, 1 if train else 0, len(data), p if train else 0.0
    if train and p > 0:
        t.seed = ops.seed_state(dev).data_ptr()
    hold, bufs = [], []
    for i, d in enumerate(data):
        C, L, O = d["x"].shape[1], d["x"].shape[2], d["w"].shape[0]
        geo = geometry(B, (d["kind"], C, L, O, d["act"]))
        dd = {k: d[k].to(device).contiguous() for k in ("x", "w", "dy", "gamma", "beta", "rm", "rv", "alpha")}
        st = producer_sums(d["x"]).to(device)
        nbt = torch.zeros(1, dtype=torch.int64, device=device)
        hold += [dd, st, nbt]
        b = {"y": _guarded(d["dy"].numel(), f32, device), "tap": _guarded(B * C * L, f32, device), "save": _guarded(2 * C, f32, device),
             "dx": _guarded(B * C * L, f32, device), "dW": _guarded(d["w"].numel(), f32, device), "small": _guarded(3 * C, f32, device),
             "g": _guarded(B * C * L, f32, device), "part": _guarded(geo[4], f64, device), "wpart": _guarded(geo[5], f32, device)}
        bufs.append(b)
        q = t.it[i]
        q.kind, q.C, q.L, q.O = d["kind"], C, L, O
        q.x, q.x_ld, q.W, q.salt = dd["x"].data_ptr(), C * L, dd["w"].data_ptr(), salts[i]
        q.bn.stats, q.stats_ld = (st.data_ptr() if train else None), C
        q.bn.gamma, q.bn.beta, q.bn.running_mean, q.bn.running_var = dd["gamma"].data_ptr(), dd["beta"].data_ptr(), dd["rm"].data_ptr(), dd["rv"].data_ptr()
        q.bn.num_batches_tracked = nbt.data_ptr() if train else None
        q.bn.momentum, q.bn.eps, q.bn.save = 1.0, 1e-5, b["save"][1].data_ptr()
        q.alpha = dd["alpha"].data_ptr() if d["act"] else None
        q.y, q.tap = b["y"][1].data_ptr(), (b["tap"][1].data_ptr() if d["act"] else None)
        q.dy, q.dx, q.dW, q.g, q.part, q.wpart = dd["dy"].data_ptr(), b["dx"][1].data_ptr(), b["dW"][1].data_ptr(), b["g"][1].data_ptr(), b["part"][1].data_ptr(), b["wpart"][1].data_ptr()
        small = b["small"][1]
        q.dgamma, q.dbeta, q.dalpha = small[:C].data_ptr(), small[C:2 * C].data_ptr(), (small[2 * C:].data_ptr() if d["act"] else None)
    x0 = hold[0]["x"]
    _lib.call("cg_block_mid_fwd", ctypes.byref(t), ops._stream(x0))
    _lib.call("cg_block_mid_bwd", ctypes.byref(t), ops._stream(x0))
    out = []
    for i, (d, b) in enumerate(zip(data, bufs)):
        C = d["x"].shape[1]
        for k, (buf, _) in b.items():
            g = torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu()
            assert bool(torch.isnan(g).all()), "item %d: written outside %s" % (i, k)
        r = {k: v[1].cpu().clone() for k, v in b.items()}
        for k in ("y", "save", "dx", "dW", "g", "part", "wpart"):
            assert bool(torch.isfinite(r[k]).all()), "item %d: %s holds words nobody wrote" % (i, k)
        assert bool(torch.isfinite(r["small"][:2 * C + (1 if d["act"] else 0)]).all())
        assert bool(torch.isfinite(r["tap"]).all()) == bool(d["act"])
        r["rm"], r["rv"] = hold[3 * i]["rm"].cpu().clone(), hold[3 * i]["rv"].cpu().clone()
        out.append(r)
    return out


def check_guards_and_determinism(device, name, mode):
    """tests 2 and 3: nothing is written outside the buffers, every word of them is written, and two runs - one through `ops`, one through
    the entry points - give the same bits in every output and gradient"""
    train, p = MODES[mode]
    B, data, _ = make_inputs(name)
    salts = [11 + 3 * i for i in range(len(data))]
    a = run_direct(device, B, data, train, p, salts)
    b = run_direct(device, B, data, train, p, salts)
    via_ops = run_route(device, B, data, False, True, train, p, salts)
    for i, d in enumerate(data):
        C = d["x"].shape[1]
        for k in ("y", "dx", "dW", "save", "part", "wpart", "g"):
            assert torch.equal(a[i][k], b[i][k]), "item %d: %s differs between two runs" % (i, k)
        assert torch.equal(a[i]["small"][:2 * C], b[i]["small"][:2 * C])
        o = via_ops[i]
        assert torch.equal(a[i]["y"], o["y"].reshape(-1)) and torch.equal(a[i]["dx"], o["dx"].reshape(-1)) and torch.equal(a[i]["dW"], o["dW"].reshape(-1)), "item %d: ops route differs" % i
        assert torch.equal(a[i]["small"][:C], o["dgamma"]) and torch.equal(a[i]["small"][C:2 * C], o["dbeta"])
        if d["act"]:
            assert torch.equal(a[i]["small"][2 * C:2 * C + 1], o["dalpha"].reshape(1)) and torch.equal(a[i]["tap"], o["tap"].reshape(-1))
        if train:                # save = (mean, rstd) against the running statistics at momentum 1
            assert torch.equal(a[i]["save"][:C], a[i]["rm"]), "item %d: saved mean" % i
    if train and p > 0:          # test 4 for the items without a tap: the gradient in front of the BatchNorm vanishes exactly where the row kernels drop
        keeps = keep_masks(device, B, data, p, salts)
        for i, d in enumerate(data):
            assert torch.equal(a[i]["g"].view(d["x"].shape) == 0, keeps[i] == 0), "item %d: dropped positions differ from the row kernels'" % i


def check_model(device):
    """test 5: one forward and backward of a small model in train mode with dropout 0.1, the new route on and off.  Either run is held to
    the project's model-level bound against the fp64 oracle on the branches and masks of the run itself (checks.check_model_branch_replay:
    pred, loss, dL/dx and every gradient within 1e-4 * max(1, max |ref|), running statistics, attributes) - two fp32 runs compared with each
    other directly differ by legitimate PReLU flips - and the launch plan of the forward is counted."""
    import checks
    import loop_shapes
    C, T, V, B = 8, 10, 22, 8
    res = []
    for mid in (True, False):
        kinds, snap = [], {}
        saved = (ops.block_mid, ops.block_mid_ok)
        ops.block_mid = lambda items, *a, **k: (kinds.append(tuple(it["kind"] for it in items)), saved[0](items, *a, **k))[1]
        if not mid:
            ops.block_mid_ok = lambda B_, items: False
        try:
            with loop_shapes.counted_calls() as launches:
                r = checks.check_model_branch_replay(device, C, T, V, B, "train", grad_floor=1.0, oracle_fp64=True, stack_all=True, dropout=0.1,
                                                     after_device_run=lambda: snap.update(launches))
        finally:
            ops.block_mid, ops.block_mid_ok = saved
        print("block_mid model, route %s: worst gradient at %.3f of its bound (%s); calls %s" % ("on" if mid else "off", r["worst_grad"][0], r["worst_grad"][1], kinds))
        res.append((snap, kinds))
    (f0, k0), (f1, k1) = res
    whole = sum(1 for k in k0 if k == (FULL, FULL, PW, PW, PW, PW))            # blocks whose gates and towers all qualify
    gates_only = sum(1 for k in k0 if k == (FULL, FULL))                       # a block with fewer items: its towers keep the chain
    towers_only = sum(1 for k in k0 if k == (PW, PW, PW, PW))
    assert whole >= 1 and whole + gates_only + towers_only == len(k0) and not k1, (k0, k1)
    assert f0.get("cg_block_mid_fwd", 0) == len(k0) and f0.get("cg_block_mid_bwd", 0) == len(k0), f0      # one launch per qualifying block
    assert "cg_block_mid_fwd" not in f1 and "cg_block_mid_bwd" not in f1
    # a whole block: the gates' (1,V) convolutions and the last tower maps were one contraction launch each, forward and backward, the two
    # BatchNorm tails one row-kernel launch each; with the gates alone only their row-kernel launches go (the contractions still carry the towers)
    for name, gone in (("cg_contract_many", 2 * (2 * whole + towers_only)), ("cg_norm_act_fwd_many", 2 * whole + gates_only + towers_only),
                       ("cg_norm_act_bwd_many", 2 * whole + gates_only + towers_only)):
        print("block_mid model: %s %d -> %d launches per step" % (name, f1[name], f0.get(name, 0)))
        assert f1[name] - f0.get(name, 0) == gone, (name, f1[name], f0.get(name, 0), gone)
    for k in ("cg_collapse_rows_fwd", "cg_collapse_cols_fwd", "cg_gate_head_fwd", "cg_map2adj_tail_fwd", "cg_dstd_tail_fwd"):
        assert f0.get(k) == f1.get(k), k
