"""Device-agnostic parity checks of the HIP operators against stock-PyTorch references computed on
the CPU.  The same functions run (a) in `-m "not gpu"` through the test-only HIP shim (tests/hipemu,
device "cpu") and (b) in `-m gpu` on the MI355X through the real libcistgcn_hip.so (device "cuda").

Tolerance: fp32 north_star bound, max|a-b| <= 1e-4 * max(1, max|ref|) per tensor;
unit-scale operator tests use the tighter 2e-5.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from cistgcn_amd import ops
from helpers import assert_close, assert_grads_close, load_case, make_cfg, state_of
from oracle import cistgcn_ref as O


def _chan_sums(st):
    """fold the replicated [R][C][2] channel-sum buffer (CG_STAT_REPLICAS) into [C*2]"""
    from cistgcn_amd import _lib
    return st.detach().cpu().view(_lib.STAT_REPLICAS, -1).sum(0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _leaf(t, device):
    return t.detach().clone().to(device).requires_grad_(True)


# ---- channels whose variance is comparable to eps -------------------------------------------------------------------------------
# The families' own data has channel variances of 0.5 .. 9: against those the eps = 1e-5 of a BatchNorm is a 5e-6 effect, below every bound,
# and a kernel that drops it passes (tests/MUTANTS.md).  `low_var=True` of a family's check gives channels 0 and 1 of every BatchNorm a batch
# variance of about 0.9 eps and 0.1 eps (train) and these running variances (eval); references and bounds stay the family's.
LOW_VAR_BATCH = (0.9e-5, 0.1e-5)
LOW_VAR_RUNNING = (2e-5, 3e-6)
LOW_VAR_ROWS = (3e-3, 1e-3)          # a map of O(1) rows in front of the BatchNorm, where its output is not at hand to be measured


def _low_var_input(x, dim=1):
    """a copy of the data tensor x whose channels 0 and 1 (along `dim`) are centred (no cancellation in the float32 values) and scaled to
    the biased variances LOW_VAR_BATCH"""
    x = x.clone().movedim(dim, 0)
    for c, var in enumerate(LOW_VAR_BATCH):
        v = x[c].double()
        v = v - v.mean()
        x[c] = (v * (var / float(v.pow(2).mean())) ** 0.5).float()
    return x.movedim(0, dim).contiguous()


def _low_var_rows(weight, y=None, bias=None):
    """in place: rows 0 and 1 of the weight of a map in front of a BatchNorm (never its input) scaled so that the map's output channels get
    the variances LOW_VAR_BATCH - y: that output (channels along dim 1) with the weight as it is, in float64; without it by LOW_VAR_ROWS -
    and the bias entries with them"""
    with torch.no_grad():
        for c in range(2):
            s = LOW_VAR_ROWS[c] if y is None else (LOW_VAR_BATCH[c] / float(y.transpose(0, 1)[c].double().var(unbiased=False))) ** 0.5
            weight[c] *= s
            if bias is not None:
                bias[c] *= s


def _low_var_running(bn):
    """in place: running_var of channels 0 and 1 = LOW_VAR_RUNNING, their running_mean of the size of such a channel"""
    with torch.no_grad():
        for c, var in enumerate(LOW_VAR_RUNNING):
            bn.running_var[c] = var
            bn.running_mean[c] *= 1e-3


# ---- channels far off centre ----------------------------------------------------------------------------------------------------
# Every BatchNorm statistic of the library is E[x^2] - E[x]^2 from {sum, sum of squares} (csrc/cg_bn.h), which is safe only while both sums
# are carried in float64 per element: an f32 partial sum of squares of a channel at |mean| / std = r loses r^2 * 6e-8 of the variance.  The
# families' own data is centred (|mean| / std < 1) and cannot tell.  `off_centre` cases put channels 0 and 1 of every BatchNorm at the
# ratios OFF_CENTRE (opposite signs; every other channel stays as generated: the control) and hold the kernel to 4 x the error of stock
# float32 PyTorch against float64 on the same float32 values (assert_within_stock), on top of the family's own bound.
OFF_CENTRE = (30.0, -300.0)
OFF_CENTRE_NONE = (0.0, 0.0)          # "the same case with offsets 0": the second measurement of the stock error


def _ratio_ok(v, ratio, what):
    """precondition of a case: the float32 channel v has |mean| / std within 10 % of the target (a target of 0 asks nothing)"""
    if ratio == 0.0:
        return
    v = v.detach().double()
    got = float(v.mean()) / float(v.std(unbiased=False))
    assert abs(got - ratio) <= 0.1 * abs(ratio), "%s: mean / std = %.2f, wanted %.1f" % (what, got, ratio)


def _off_centre_input(x, dim=1, ratios=OFF_CENTRE):
    """a copy of the data tensor x with ratios[c] * std(channel c) added to channels 0 and 1 (along `dim`) in float64, rounded to float32 once"""
    x = x.clone().movedim(dim, 0)
    for c, ratio in enumerate(ratios):
        v = x[c].double()
        x[c] = (v + ratio * float(v.std(unbiased=False))).float()
        _ratio_ok(x[c], ratio, "off-centre input channel %d" % c)
    return x.movedim(0, dim).contiguous()


def _map_fwd(conv):
    w = conv.weight.detach().double()
    bias = None if conv.bias is None else conv.bias.detach().double()
    return (lambda t: F.linear(t, w, bias)) if w.dim() == 2 else (lambda t: F.conv2d(t, w, bias))


def _off_centre_pair(conv, x, ratios=OFF_CENTRE, candidates=None, pair=None):
    """(k0, d0, k1, d1): the constants d0 / d1 which, added to the input channels k0 / k1 of the bias-free map `conv` with the input x,
    put its output channels 0 and 1 on the ratios - solved in float64.  The pair (among `candidates`, default every input channel) is the
    one whose 2 x 2 matrix of weight sums over the kernel taps (the shift of output channels 0 and 1 per unit constant) has the largest
    determinant, so no column sum near zero is divided by."""
    w = conv.weight.detach().double()
    y = _map_fwd(conv)(x.double())
    s = w.flatten(2).sum(-1) if w.dim() > 2 else w          # [O, Cin]
    if pair is None:
        cand = list(range(s.shape[1])) if candidates is None else list(candidates)
        best = None
        for i, k0 in enumerate(cand):
            for k1 in cand[i + 1:]:
                det = float(s[0, k0] * s[1, k1] - s[0, k1] * s[1, k0])
                if best is None or abs(det) > abs(best[0]):
                    best = (det, k0, k1)
        pair = best[1:]
    k0, k1 = pair
    det = float(s[0, k0] * s[1, k1] - s[0, k1] * s[1, k0])
    assert abs(det) > 1e-3 * float(s[:2].abs().max()) ** 2, "no pair of input channels moves output channels 0 and 1 independently"
    t = []
    for c in range(2):
        v = y.transpose(0, 1)[c]
        t.append(ratios[c] * float(v.std(unbiased=False)) - float(v.mean()) if ratios[c] else 0.0)
    d0 = (t[0] * float(s[1, k1]) - t[1] * float(s[0, k1])) / det
    d1 = (t[1] * float(s[0, k0]) - t[0] * float(s[1, k0])) / det
    return k0, d0, k1, d1


def _off_centre_rows(conv, y=None, ratios=OFF_CENTRE, x=None, candidates=None):
    """in place, for a BatchNorm behind the map `conv` (nn.Conv2d / nn.Linear; its input is x, its output with the parameters as they are is
    y, channels along dim 1).  With a bias: bias[c] = ratios[c] * std(y channel c) in float64, the input untouched.  Without one: returns a
    copy of x with the constants of _off_centre_pair added to two input channels; the other output channels move with them.  The float32
    result is measured through the map in float64."""
    fwd = _map_fwd(conv)
    if conv.bias is not None:
        y = fwd(x.double()) if y is None else y.double()
        with torch.no_grad():
            for c in range(2):
                conv.bias[c] = ratios[c] * float(y.transpose(0, 1)[c].std(unbiased=False))
        if x is not None:
            for c in range(2):
                _ratio_ok(_map_fwd(conv)(x.double()).transpose(0, 1)[c], ratios[c], "off-centre map output channel %d" % c)
        return x
    k0, d0, k1, d1 = _off_centre_pair(conv, x, ratios, candidates)
    x = x.clone()
    x[:, k0] = (x[:, k0].double() + d0).float()
    x[:, k1] = (x[:, k1].double() + d1).float()
    for c in range(2):
        _ratio_ok(fwd(x.double()).transpose(0, 1)[c], ratios[c], "off-centre map output channel %d" % c)
    return x


def _off_centre_running(bn, ratios=OFF_CENTRE, y=None):
    """in place, for the eval passes: running_mean[c] = ratios[c] * sqrt(running_var[c]) of channels 0 and 1.  y: the tensor the BatchNorm
    normalises (channels along dim 1) - running_var[c] is then that channel's variance first, so that the running statistics describe the
    off-centre channel they meet (as after training on it) and `v - mean` cancels as it does in a trained model."""
    with torch.no_grad():
        for c, ratio in enumerate(ratios):
            if ratio:
                if y is not None:
                    bn.running_var[c] = float(y.transpose(0, 1)[c].double().var(unbiased=False))
                bn.running_mean[c] = ratio * float(bn.running_var[c].double().sqrt())
                assert abs(float(bn.running_mean[c]) / float(bn.running_var[c].double().sqrt()) - ratio) <= 0.1 * abs(ratio)


def _max_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0


STOCK_FACTOR = 4.0
# a tensor of ONE element (the gradient of a shared PReLU slope) is one draw of the kernel's error against one draw of stock's: two
# zero-mean errors of equal size are more than 4 x apart in 2 / pi * atan(1 / 4) = 16 % of all draws, more than 32 x apart in 2 %
# (measured: context_heads 5.3 x, gate_head 16 x with float64 sums throughout); the max over a tensor of many elements is no such draw
STOCK_FACTOR_ONE = 32.0
STOCK_MISSES = None        # a list: a measuring script collects every miss of every case here, and the case goes on instead of stopping


def assert_within_stock(what, kernel, stock, family, ratios=OFF_CENTRE, factors=None):
    """The bound of the off-centre cases.  stock(dtype, ratios) -> {name: tensor}: the stock PyTorch chain of the case in `dtype` on the
    float32 values of the case built with `ratios`; kernel() -> the same names from the HIP run of the case with `ratios`; family(name,
    refs) -> the absolute bound the family's own check holds that quantity to, from the float64 results `refs` of the case (None: the
    family itself holds the quantity to stock float32 alone).
    For every name: e_stock = max(stock float32 against float64 on the case, the same with ratios 0); the kernel must be within
    min(family bound, STOCK_FACTOR * e_stock) of float64 (STOCK_FACTOR_ONE for a tensor of one element), and equal where e_stock is 0.  A non-zero e_stock counts as at least half an ulp
    of the largest float32 element of the tensor: neither run can be held below the rounding of its own float32 result, a stock error
    under it is the luck of a few numbers (running_var of three channels), and a correctly rounded kernel would miss 4 x that.
    factors: {name: factor} for the quantities whose recorded cause (tests/MUTANTS.md) puts them above STOCK_FACTOR.
    Before the kernel runs: stock float32 itself is inside the family's bound on the case, or the case would test float32."""
    from helpers import WORST
    r64, r32 = stock(torch.float64, ratios), stock(torch.float32, ratios)
    z64, z32 = stock(torch.float64, OFF_CENTRE_NONE), stock(torch.float32, OFF_CENTRE_NONE)
    e_stock, fam = {}, {}
    for name, ref in r64.items():
        e_off = _max_err(r32[name], ref)
        e_stock[name] = max(e_off, _max_err(z32[name], z64[name]))
        if e_stock[name] > 0.0:
            e_stock[name] = max(e_stock[name], 2.0 ** -24 * float(ref.detach().abs().max()))
        fam[name] = family(name, r64)
        if fam[name] is None:
            fam[name] = float("inf")
        assert e_off <= fam[name], "%s %s: precondition: stock float32 is %.3e off float64, the family's bound is %.3e (ratios %s)" % (what, name, e_off, fam[name], ratios)
    got = kernel()
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    misses = []
    for name, ref in r64.items():
        err = _max_err(got[name], ref)
        if e_stock[name] == 0.0:
            if err != 0.0:
                misses.append((float("inf"), "%s %s: stock float32 is exact, the kernel is %.3e off" % (what, name, err)))
            continue
        factor = STOCK_FACTOR if ref.numel() > 1 else STOCK_FACTOR_ONE
        bound = min(fam[name], max(factor, (factors or {}).get(name, 0.0)) * e_stock[name])
        print("%s %s: kernel %.3e, stock float32 %.3e (x %.2f), family bound %.3e" % (what, name, err, e_stock[name], err / e_stock[name], fam[name]))
        if err > bound:
            misses.append((err / bound, "%s %s: max err %.3e > bound %.3e (%.1f x stock float32)" % (what, name, err, bound, err / e_stock[name])))
        elif err / bound > WORST[0]:
            WORST[:] = [err / bound, "%s %s" % (what, name), err, bound]
    if STOCK_MISSES is not None:
        STOCK_MISSES.extend(m for _, m in misses)
    elif misses:
        raise AssertionError(max(misses)[1] + ("" if len(misses) == 1 else " and %d more" % (len(misses) - 1)))


class BranchLog:
    """PReLU of a CPU reference on the branches the HIP run took, for tensors of millions of elements.

    The gradient of a PReLU jumps at 0.  Among millions of pre-activations a few lie within fp32 rounding of 0 and land on the other
    side in another implementation; there the two differentiate different piecewise-linear functions and every gradient upstream differs
    by O((1 - alpha) * dy), whatever the precision of either (the model tests meet the same fact with helpers.BranchReplay).  `prelu`
    reads the HIP run's branch off the sign of its PReLU output (slope > 0; an output of exactly 0 is the kernels' `u > 0 ? u : alpha * u`
    on its second branch) and evaluates the reference on that branch.  `add`: an addend behind the PReLU is taken off first; where the
    difference is exactly 0 - |PReLU(u)| below half an ulp of the addend - the branch cannot be read: `unknown` marks these elements and the
    caller keeps them out of the backward pass (zero upstream gradient), so that no gradient depends on a branch nobody can know.  An element where the reference's own pre-activation has the other sign is counted, and must
    be rounding-sized: `settle` holds it to the tolerance the check holds the outputs to (2e-5 * max(1, max|u|)) - an output within that
    tolerance cannot tell the branches apart there, and a kernel whose pre-activation is off by more fails here.

    Reading the branch off the forward's output is not enough on its own: the kernels form the pre-activation again in their backward
    pass, in another kernel with its own rounding (fused multiply-adds), and at an element within an ulp of 0 the backward may take the
    other branch than its own forward (seen on the MI355X, fused tail and row kernels alike: one element of 18 million with the
    gradient off by exactly the slope, everything else within 1e-6; which element changes with the order of the f64 atomics from run to
    run).  The slopes stay as they are; these elements are accounted for one by one (`kink_terms`, `assert_grads_at_kinks`): the gradient
    is linear in the derivative the PReLU takes at an element, so the other choice at element e adds d_e = J^T((alpha - 1 | 1 - alpha) *
    dy_e) to every gradient upstream - one partial backward pass of the reference from that pre-activation.  Only elements whose fp64
    pre-activation is within 1e-7 * max(1, max|u|) of 0 qualify (u is a sum of a few fp32 terms of the size of max|u|, each rounded to
    6e-8 of itself; the elements seen to do it were below 1e-8), the twelve closest to 0; a term is used only when the kernel's
    gradient contains it with a factor within 5 % of 1.  Anything else - a wrong slope, a slope on the wrong branch, a flip at a
    pre-activation that is not rounding-sized - fails at the bound it failed at before."""

    def __init__(self):
        self.flips, self.elements, self.worst, self.unknown = 0, 0, 0.0, None
        self.sites = []

    def prelu(self, u, weight, dev_out, add=None):
        alpha = weight.reshape((1, -1) + (1,) * (u.dim() - 2)) if weight.numel() > 1 else weight
        own = u > 0
        self.elements += own.numel()
        if dev_out is None or not bool((weight > 0).all()):
            return torch.where(own, u, alpha * u)
        t = dev_out.detach().cpu().to(u.dtype)
        if add is None:
            pos = t > 0
        else:
            d = t - add.detach()
            pos = torch.where(d != 0, d > 0, own)
            self.unknown = d == 0
        diff = pos != own
        n = int(diff.sum())
        if n:
            self.flips += n
            self.worst = max(self.worst, float(u.detach().abs()[diff].max()) / max(1.0, float(u.detach().abs().max())))
        out = torch.where(pos, u, alpha * u)
        if u.requires_grad:
            site = {"u": u, "pos": pos, "alpha": alpha.detach(), "dy": None}
            out.register_hook(lambda g, site=site: site.__setitem__("dy", g))
            self.sites.append(site)
        return out

    def kink_terms(self, leaves, rel=1e-7, most=12, resid=None):
        """[(description, d_e per leaf)] for the pre-activations closest to 0 (see the class comment); needs the reference's backward pass
        to have run with retain_graph=True.  resid: the difference that is to be explained, in units of its bounds, one tensor per leaf: of the
        qualifying elements those come first at whose (sample, position) a tensor of the same layout misses its bound (a term is largest at
        its own place)."""
        cands = []
        for k, site in enumerate(self.sites):
            ua = site["u"].detach().abs()
            lim = rel * max(1.0, float(ua.max()))
            for idx in (ua <= lim).nonzero():
                idx = tuple(int(v) for v in idx)
                here = 0.0
                for r in (resid or []):
                    if r.dim() == 4 and len(idx) == 4 and r.shape[0] == ua.shape[0] and r.shape[2:] == ua.shape[2:]:
                        here = max(here, float(r[idx[0], :, idx[2], idx[3]].abs().max()))
                cands.append((here <= 1.0, float(ua[idx]) / max(1.0, float(ua.max())), k, idx))
        terms = []
        for _, size, k, idx in sorted(cands)[:most]:
            site = self.sites[k]
            a = float(site["alpha"].expand_as(site["u"])[idx])
            seed = torch.zeros_like(site["u"])
            seed[idx] = ((a - 1.0) if bool(site["pos"][idx]) else (1.0 - a)) * site["dy"][idx]
            d = torch.autograd.grad(site["u"], leaves, grad_outputs=seed, retain_graph=True, allow_unused=True)
            terms.append(("PReLU %d element %s, |u| = %.1e of max(1, max|u|)" % (k, idx, size), d))
        return terms

    def settle(self, what, rel=2e-5):
        assert self.worst <= rel, "%s: a pre-activation on the other side of 0 than in the HIP run is not rounding-sized: |u| = %.2e of max(1, max|u|)" % (what, self.worst)
        if self.flips:
            print("%s: %d of %d PReLU elements within rounding of 0 (largest %.1e of max(1, max|u|)) replayed on the HIP run's branch" % (what, self.flips, self.elements, self.worst))


def assert_grads_at_kinks(got, refs, floors, names, what, log, leaves, rel=5e-5, both_ways=False):
    """got[i] against refs[i] at rel * floors[i] (refs in the order of `leaves`).  When a tensor misses and `log` (BranchLog) has
    pre-activations within rounding of 0, the reference is moved by the kink terms the kernel's gradients contain (factor 1; both_ways:
    also -1, for two fp32 runs compared with each other) and every tensor is then held to the same bound."""
    refs = kink_adjusted(got, refs, floors, what, log, leaves, rel, both_ways)
    for g, r, fl, k in zip(got, refs, floors, names):
        assert_close(g, r, "%s grad %s" % (what, k), rel=rel, floor=fl)


def kink_adjusted(got, refs, floors, what, log, leaves, rel=5e-5, both_ways=False):
    """refs (fp64, CPU) moved by the kink terms that got contains, see assert_grads_at_kinks"""
    got = [g.detach().cpu().double() for g in got]
    refs = [r.detach().cpu().double() for r in refs]
    bounds = [rel * f for f in floors]
    if log is not None and any(float((g - r).abs().max()) > b for g, r, b in zip(got, refs, bounds)):
        # greedy fit: in each round the term whose factor in what is left of the difference is closest to 1 (-1), within 5 %, is taken out
        # (terms of two elements of one PReLU overlap through the BatchNorm statistics, so the factors settle as terms are removed);
        # terms smaller than the bounds (norm below 1 in units of them) cannot make a tensor miss and are left alone
        terms = []
        for desc, d in log.kink_terms(leaves, resid=[(g - r) / b for g, r, b in zip(got, refs, bounds)]):
            den = sum(float(((t.double() / b) ** 2).sum()) for b, t in zip(bounds, d) if t is not None)
            if den > 1.0:
                terms.append((desc, d, den))
        while terms:
            best = None
            for n, (desc, d, den) in enumerate(terms):
                fac = sum(float((((g - r) / b) * (t.double() / b)).sum()) for g, r, b, t in zip(got, refs, bounds, d) if t is not None) / den
                f = max(-1 if both_ways else 0, min(1, round(fac)))
                if f and abs(fac - f) <= 0.05 and (best is None or abs(fac - f) < best[0]):
                    best = (abs(fac - f), n, f, fac)
            if best is None:
                break
            desc, d, _ = terms.pop(best[1])
            print("%s: the gradients contain the other branch at %s (factor %.3f)" % (what, desc, best[3]))
            refs = [r if t is None else r + best[2] * t.double() for r, t in zip(refs, d)]
    return refs


def _run(fn_dev, fn_ref, inputs, device, rel=2e-5, what="", ref_sees_dev_out=False, log=None, params=None, ref_dtype=None):
    """fn_dev / fn_ref map a list of leaf tensors to one output; compares output and all input grads.  ref_sees_dev_out: fn_ref also gets the
    HIP output (keyword dev_out), to take its PReLU branches (`log`, a BranchLog; elements whose branch cannot be read get no upstream gradient).
    ref_dtype: the reference runs in this type (torch.float64) on the same float32 values; default: float32 as the inputs."""
    dev_in = [_leaf(t, device) for t in inputs]
    ref_in = [_leaf(t if ref_dtype is None else t.to(ref_dtype), "cpu") for t in inputs]
    ops.begin_step(device)
    y = fn_dev(*dev_in)
    r = fn_ref(*ref_in, dev_out=y) if ref_sees_dev_out else fn_ref(*ref_in)
    assert_close(y, r, what + " output", rel=rel)
    g = _rand(_gen(99), *r.shape)
    if log is not None and log.unknown is not None:
        g = g.masked_fill(log.unknown, 0.0)
    y.backward(g.to(device))
    r.backward(g.to(r.dtype), retain_graph=log is not None)
    if log is not None:          # inputs and `params` = (device parameters, reference parameters) together, kink terms accounted for
        pairs = [(a, b) for a, b in zip(dev_in, ref_in) if b.grad is not None] + list(zip(*params))
        assert_grads_at_kinks([a.grad for a, _ in pairs], [b.grad for _, b in pairs], [max(1e-3, float(b.grad.abs().max())) for _, b in pairs],
                              range(len(pairs)), what, log, [b for _, b in pairs], rel=rel)
        return
    for i, (a, b) in enumerate(zip(dev_in, ref_in)):
        if b.grad is None:
            continue
        assert a.grad is not None, "%s: missing grad for input %d" % (what, i)
        assert_close(a.grad, b.grad, "%s grad[%d]" % (what, i), rel=rel, floor=max(1e-3, float(b.grad.abs().max())))


# ---------------------------------------------------------------------------------------------
def check_contract(device, quick=False):
    """quick=True (CPU shim): smaller tiled case; the MI355X run uses the full sizes"""
    g = _gen(1)
    B, C, O, T, V = 3, 10, 8, 5, 7
    x = _rand(g, B, C, T, V)
    cases = [
        ("oc,bchw->bohw", _rand(g, O, C), x, _rand(g, O), "o"),          # 1x1 conv + bias
        ("och,bchw->bow", _rand(g, O, C, T), x, None, None),             # (T,1) conv
        ("ocw,bchw->boh", _rand(g, O, C, V), x, None, None),             # (1,V) conv
        ("oi,bi->bo", _rand(g, O, 12), _rand(g, B, 12), None, None),      # Linear
        ("bctv,bvtq->bcqv", x, _rand(g, B, V, T, T), None, None),        # adjacency product, space
        ("bctv,btvw->bctw", x, _rand(g, B, T, V, V), None, None),        # adjacency product, time
        ("bvt,bxv->bvtx", _rand(g, B, V, T), _rand(g, B, T, V), None, None),   # rank-1 outer (space)
        ("bvt,btw->btvw", _rand(g, B, V, T), _rand(g, B, T, V), None, None),   # rank-1 outer (time)
        ("bt,bv->btv", _rand(g, B, T), _rand(g, B, V), None, None),
        ("bctv,vtq->bcqv", x, _rand(g, V, T, T), None, None),             # batch-shared adjacency
    ]
    for spec, a, xx, bias, bl in cases:
        ins = [a, xx] + ([bias] if bias is not None else [])
        def dev(a_, x_, *b_, spec=spec, bl=bl):
            return ops.contract(spec, a_, x_, b_[0] if b_ else None, bl)
        def ref(a_, x_, *b_, spec=spec):
            y = torch.einsum(spec, a_, x_)
            if b_:
                shape = [1] * y.dim()
                shape[spec.split("->")[1].index("o")] = -1
                y = y + b_[0].view(shape)
            return y
        _run(dev, ref, ins, device, what="contract " + spec)
    # strided (permuted) operand: NTCV view of an NCTV buffer, as in CISTGCN.py:582
    w = _rand(g, 6, T)
    _run(lambda w_, x_: ops.contract("oc,bchw->bohw", w_, x_.permute(0, 2, 1, 3)),
         lambda w_, x_: torch.einsum("oc,bchw->bohw", w_, x_.permute(0, 2, 1, 3)), [w, x], device, what="contract permuted")
    # many output rows/cols (several tiles, both tile shapes) and a long K (split-K path in the weight grad)
    xb = _rand(g, 6, 36, 5, 6) if quick else _rand(g, 40, 70, 9, 11)
    wb = _rand(g, 70 if quick else 130, xb.shape[1], scale=0.1)
    _run(lambda w_, x_: ops.contract("oc,bchw->bohw", w_, x_), lambda w_, x_: torch.einsum("oc,bchw->bohw", w_, x_),
         [wb, xb], device, rel=1e-4, what="contract tiled/split-K")


    # float4 operand loads (positions contiguous in aligned groups of four), both tile shapes
    xv = _rand(g, 5, 12, 4, 8)
    for O_ in ((40,) if quick else (8, 40)):
        wv = _rand(g, O_, 12, scale=0.3)
        _run(lambda w_, x_: ops.contract("oc,bchw->bohw", w_, x_), lambda w_, x_: torch.einsum("oc,bchw->bohw", w_, x_),
             [wv, xv], device, what="contract vectorised loads O=%d" % O_)


    # wide (matrix-core) tile with bias and the BatchNorm-sum epilogue, ragged N and short K
    for K_ in ((12,) if quick else (4, 12, 20)):
        xw, ww, bw = _rand(g, 3, K_, 5, 7), _rand(g, 40, K_, scale=0.3), _rand(g, 40)
        ops.begin_step(device)
        yw, st = ops.contract_stats("oc,bchw->bohw", ww.to(device), xw.to(device), bw.to(device), "o")
        rw = (torch.einsum("oc,bchw->bohw", ww, xw) + bw.view(1, -1, 1, 1)).double()
        assert_close(yw, rw, "contract wide K=%d" % K_, rel=2e-5)
        assert_close(_chan_sums(st), torch.stack((rw.sum((0, 2, 3)), (rw * rw).sum((0, 2, 3))), 1).reshape(-1), "contract wide sums K=%d" % K_, rel=1e-5)


def _check_norm_act_shape(device, quick, T, V, trains=(True, False), B=4, C=6, replay=False, low_var=False):
    """replay: the stock-PyTorch reference takes the PReLU branches of the HIP run (BranchLog; for tensors of millions of elements).
    low_var: two channels whose variance is comparable to eps (LOW_VAR_BATCH above), the reference in float64."""
    g = _gen(2)
    x = _rand(g, B, C, T, V, scale=3.0) + 1.5
    if low_var:
        x = _low_var_input(x)
    add = _rand(g, B, C, T, V)
    pre = _rand(g, B, C)

    def make_bn():
        bn = nn.BatchNorm2d(C)
        with torch.no_grad():
            bn.weight.copy_(1 + 0.3 * _rand(g, C)); bn.bias.copy_(0.3 * _rand(g, C))
            bn.running_mean.copy_(_rand(g, C)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        if low_var:
            _low_var_running(bn)
        return bn

    for train in trains:
        for use_pre in (False, True):
            for add_mode in (None, "pre", "post"):
                for alpha_n in ((1, C) if (quick and add_mode == "pre") else ((1,) if quick else (0, 1, C))):
                    bn_ref = make_bn()
                    bn_dev = nn.BatchNorm2d(C)
                    bn_dev.load_state_dict(bn_ref.state_dict())
                    bn_dev.to(device)
                    bn_ref.train(train)
                    if low_var:
                        bn_ref.double()
                    pr_ref = nn.PReLU(alpha_n) if alpha_n else None
                    pr_dev = None
                    if pr_ref is not None:
                        with torch.no_grad():
                            pr_ref.weight.copy_(0.25 + 0.2 * _rand(g, alpha_n))
                            if replay:
                                pr_ref.weight.abs_().clamp_(min=0.05)          # the branch is read off the sign of the output
                        pr_dev = nn.PReLU(alpha_n)
                        pr_dev.load_state_dict(pr_ref.state_dict())
                        pr_dev.to(device)
                        if low_var:
                            pr_ref.double()
                    ins = [x] + ([pre] if use_pre else []) + ([add] if add_mode else [])

                    def split(ts):
                        ts = list(ts)
                        x_ = ts.pop(0)
                        p_ = ts.pop(0) if use_pre else None
                        a_ = ts.pop(0) if add_mode else None
                        return x_, p_, a_

                    def dev(*ts):
                        x_, p_, a_ = split(ts)
                        return ops.norm_act(x_, bn=bn_dev, train=train, pre=p_, add=a_, add_post=add_mode == "post", prelu=pr_dev)

                    log = BranchLog()

                    def ref(*ts, dev_out=None):
                        x_, p_, a_ = split(ts)
                        v = x_ * p_[:, :, None, None] if p_ is not None else x_
                        u = bn_ref(v)
                        if add_mode == "pre":
                            u = u + a_
                        if pr_ref is not None:
                            u = log.prelu(u, pr_ref.weight, dev_out, add=a_ if add_mode == "post" else None) if replay else pr_ref(u)
                        if add_mode == "post":
                            u = u + a_
                        return u

                    what = "norm_act%s train=%s pre=%s add=%s alpha=%d" % (" low variance" if low_var else "", train, use_pre, add_mode, alpha_n)
                    dev_ps = list(bn_dev.parameters()) + (list(pr_dev.parameters()) if pr_dev is not None else [])
                    ref_ps = list(bn_ref.parameters()) + (list(pr_ref.parameters()) if pr_ref is not None else [])
                    _run(dev, ref, ins, device, what=what, ref_sees_dev_out=True, log=log if replay else None, params=(dev_ps, ref_ps),
                         ref_dtype=torch.float64 if low_var else None)
                    log.settle(what)
                    for (n1, pd), (_, pr) in zip(bn_dev.named_parameters(), bn_ref.named_parameters()):
                        if not replay:
                            assert_close(pd.grad, pr.grad, what + " d" + n1, rel=2e-5, floor=max(1e-3, float(pr.grad.abs().max())))
                    if pr_ref is not None and not replay:
                        assert_close(pr_dev.weight.grad, pr_ref.weight.grad, what + " dalpha", rel=2e-5,
                                     floor=max(1e-3, float(pr_ref.weight.grad.abs().max())))
                    for k in ("running_mean", "running_var", "num_batches_tracked"):
                        assert_close(getattr(bn_dev, k).float(), getattr(bn_ref, k).float(), what + " " + k, rel=2e-5)


def check_norm_act_rows(device, shapes):
    """the row kernels with several samples of a channel per workgroup (cg_rows_per_block > 1), every combination of
    check_norm_act's first case, the reference on the PReLU branches of the HIP run (BranchLog).  shapes: (B, C, T, V)."""
    for (B, C, T, V) in shapes:
        _check_norm_act_shape(device, True, T, V, B=B, C=C, replay=True)


def check_norm_act(device, quick=False):
    _check_norm_act_shape(device, quick, 5, 7)      # odd rows: strided scalar path
    _check_norm_act_shape(device, True, 4, 6, trains=(True,) if quick else (True, False))   # rows of 24 contiguous floats: float4 path
    _check_norm_act_shape(device, True, 5, 6, trains=(True,) if quick else (True, False))   # rows of 30 floats, 8-byte aligned: float2 path
    # a larger float4 case (several rows per workgroup, addend before the PReLU, per-channel slopes)
    gb = _gen(21)
    bn_ref, pr_ref = nn.BatchNorm2d(3), nn.PReLU(3)
    bn_dev, pr_dev = nn.BatchNorm2d(3).to(device), nn.PReLU(3).to(device)
    nb = 5 if quick else 26
    xb, ab = _rand(gb, nb, 3, 8, 120, scale=2.0) + 0.5, _rand(gb, nb, 3, 8, 120)
    _run(lambda x_, a_: ops.norm_act(x_, bn=bn_dev, train=True, add=a_, prelu=pr_dev), lambda x_, a_: pr_ref(bn_ref(x_) + a_), [xb, ab],
         device, what="norm_act two-pass float4")
    assert_close(bn_dev.weight.grad, bn_ref.weight.grad, "two-pass dgamma", rel=2e-5, floor=float(bn_ref.weight.grad.abs().max()))
    assert_close(pr_dev.weight.grad, pr_ref.weight.grad, "two-pass dalpha", rel=2e-5, floor=float(pr_ref.weight.grad.abs().max()))
    g = _gen(2)
    B, C, T, V = 4, 6, 5, 7
    # BatchNorm1d on (B,C) and (B,C,L), no-BN PReLU-only, strided input and mm-scale statistics
    for shape in ((6, C), (4, C, 9)):
        bn_ref = nn.BatchNorm1d(C)
        bn_dev = nn.BatchNorm1d(C).to(device)
        xs = _rand(g, *shape, scale=350.0) + 50.0
        _run(lambda x_: ops.norm_act(x_, bn=bn_dev, train=True), lambda x_: bn_ref(x_), [xs], device, what="bn1d %s" % (shape,))
        assert_close(bn_dev.running_var, bn_ref.running_var, "bn1d running_var", rel=2e-5)
    pr = nn.PReLU()
    prd = nn.PReLU().to(device)
    xs = _rand(g, B, T, C, V)
    _run(lambda x_: ops.norm_act(x_.permute(0, 2, 1, 3), prelu=prd), lambda x_: pr(x_.permute(0, 2, 1, 3)), [xs], device,
         what="prelu on permuted view")
    # train-mode BN refuses a single value per channel exactly like nn.BatchNorm (SURVEY appendix "Minimum batch")
    try:
        ops.norm_act(torch.zeros(1, C, device=device), bn=nn.BatchNorm1d(C).to(device), train=True)
        raise AssertionError("expected ValueError for one value per channel")
    except ValueError:
        pass


def check_batched_ops(device):
    """Horizontal fusion: several contractions / row problems per launch give the same numbers as one by one,
    shared-input gradients are accumulated in the kernel, channel sums come out of the epilogues."""
    g = _gen(11)
    x = _rand(g, 3, 10, 5, 7)
    ws = [_rand(g, 8, 10), _rand(g, 4, 10, 5), _rand(g, 6, 10), _rand(g, 9, 12)]
    bias, z = _rand(g, 6), _rand(g, 3, 12)
    specs = ["oc,bchw->bohw", "och,bchw->bow", "oc,bchw->bohw", "oi,bi->bo"]

    def run(dev, batched):
        xs, zs, bs = _leaf(x, dev), _leaf(z, dev), _leaf(bias, dev)
        wl = [_leaf(w, dev) for w in ws]
        if batched:
            ops.begin_step(dev)
            outs = ops.contract_many([(specs[0], wl[0], xs, None, None, "o"), (specs[1], wl[1], xs, None, None, None),
                                      (specs[2], wl[2], xs, bs, "o", None), (specs[3], wl[3], zs, None, None, "o")])
            ys, sts = [o[0] for o in outs], [o[1] for o in outs]
        else:
            ys = [torch.einsum(specs[0], wl[0], xs), torch.einsum(specs[1], wl[1], xs),
                  torch.einsum(specs[2], wl[2], xs) + bs.view(1, -1, 1, 1), torch.einsum(specs[3], wl[3], zs)]
            sts = None
        gy = [_rand(_gen(50 + i), *y.shape).to(dev) for i, y in enumerate(ys)]
        torch.autograd.backward(ys, gy)
        return ys, sts, [xs.grad, zs.grad, bs.grad] + [w.grad for w in wl]

    ys, sts, gr = run(device, True)
    yr, _, grr = run("cpu", False)
    for i, (a, b) in enumerate(zip(ys, yr)):
        assert_close(a, b, "contract_many y%d" % i, rel=2e-5)
    for i, (a, b) in enumerate(zip(gr, grr)):
        assert_close(a, b, "contract_many grad%d" % i, rel=2e-5, floor=float(b.abs().max()))
    y0 = yr[0].detach().double()
    assert_close(_chan_sums(sts[0]), torch.stack((y0.sum((0, 2, 3)), (y0 * y0).sum((0, 2, 3))), 1).reshape(-1), "epilogue sums", rel=1e-6)
    assert sts[1] is None and sts[2] is None
    # the large-tensor plan for shared inputs (separate gradient outputs summed by one launch instead of atomics)
    ops._ACC_MAX_FLOATS, saved = 0, ops._ACC_MAX_FLOATS
    try:
        _, _, gr2 = run(device, True)
    finally:
        ops._ACC_MAX_FLOATS = saved
    for i, (a, b) in enumerate(zip(gr2, grr)):
        assert_close(a, b, "contract_many (summed outputs) grad%d" % i, rel=2e-5, floor=float(b.abs().max()))
    # row problems of different shapes in one launch, one of them emitting the sums of its output
    shapes = [(4, 6, 4, 7), (4, 3, 1, 9), (6, 5)]       # float4 rows, scalar rows, BatchNorm1d in one launch
    xs = [_rand(g, *sh, scale=2.0) + 0.5 for sh in shapes]
    bns_ref = [nn.BatchNorm2d(6), nn.BatchNorm2d(3), nn.BatchNorm1d(5)]
    bns_dev = [type(b)(b.num_features).to(device) for b in bns_ref]
    prs_ref = [nn.PReLU(), None, nn.PReLU(5)]
    prs_dev = [None if p is None else type(p)(p.num_parameters).to(device) for p in prs_ref]
    xd = [_leaf(t, device) for t in xs]
    xr = [_leaf(t, "cpu") for t in xs]
    ops.begin_step(device)
    outs = ops.norm_act_many([dict(x=xd[i], bn=bns_dev[i], train=True, prelu=prs_dev[i], emit_stats=(i == 0)) for i in range(3)])
    yd = [outs[0][0], outs[1], outs[2]]
    yr = [(prs_ref[i](bns_ref[i](xr[i])) if prs_ref[i] is not None else bns_ref[i](xr[i])) for i in range(3)]
    gy = [_rand(_gen(70 + i), *sh) for i, sh in enumerate(shapes)]
    torch.autograd.backward(yd, [t.to(device) for t in gy])
    torch.autograd.backward(yr, gy)
    for i in range(3):
        assert_close(yd[i], yr[i], "norm_act_many y%d" % i, rel=2e-5)
        assert_close(xd[i].grad, xr[i].grad, "norm_act_many dx%d" % i, rel=2e-5, floor=float(xr[i].grad.abs().max()))
        assert_close(bns_dev[i].weight.grad, bns_ref[i].weight.grad, "norm_act_many dgamma%d" % i, rel=2e-5, floor=1e-3)
        assert_close(bns_dev[i].running_var, bns_ref[i].running_var, "norm_act_many running_var%d" % i, rel=2e-5)
    y0 = yr[0].detach().double()
    assert_close(_chan_sums(outs[0][1]), torch.stack((y0.sum((0, 2, 3)), (y0 * y0).sum((0, 2, 3))), 1).reshape(-1), "emitted sums", rel=1e-6)


def check_dropout(device, mask=False):
    """Dropout cannot match the CPU RNG stream; check rate, scale and fwd/bwd mask agreement.  mask=True: also that the mask is the host
    restatement of the kernels' hash bit for bit, and its statistics (_check_dropout_mask)."""
    p = 0.3
    ops.manual_seed(123, device)
    x = torch.ones(8, 16, 10, 22, device=device, requires_grad=True)
    ops.begin_step(device, bump_seed=True)
    y = ops.norm_act(x, train=True, drop_p=p, salt=7)
    vals = y.detach().cpu()
    kept = vals != 0
    assert abs(kept.float().mean().item() - (1 - p)) < 0.02
    assert torch.allclose(vals[kept], torch.full_like(vals[kept], 1 / (1 - p)))
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad.cpu(), vals)                        # same mask and scale in backward
    y2 = ops.norm_act(x.detach(), train=True, drop_p=p, salt=8)   # another site -> another mask
    assert not torch.equal(y2.cpu(), vals)
    ops.begin_step(device, bump_seed=True)                        # next step -> another mask
    y3 = ops.norm_act(x.detach(), train=True, drop_p=p, salt=7)
    assert not torch.equal(y3.cpu(), vals)
    y4 = ops.norm_act(x.detach(), train=False, drop_p=p, salt=7)  # eval: identity
    assert torch.equal(y4.cpu(), torch.ones_like(vals))
    # the float4 path (contiguous rows) and the strided scalar path draw the same mask for the same logical element
    xs = torch.ones(8, 10, 22, 16, device=device).permute(0, 3, 1, 2)            # same logical shape, channel-last storage
    y5 = ops.norm_act(xs, train=True, drop_p=p, salt=7)
    assert torch.equal(y5.cpu(), y3.cpu())
    xo = torch.ones(3, 4, 5, 7, device=device, requires_grad=True)                 # odd row length: scalar path, fwd/bwd agreement
    yo = ops.norm_act(xo, train=True, drop_p=p, salt=9)
    yo.backward(torch.ones_like(yo))
    assert torch.equal(xo.grad.cpu(), yo.detach().cpu())
    # rows of 30 floats (8-byte aligned): the float2 path draws the mask of the strided scalar path, forward and backward
    x2 = torch.ones(3, 4, 5, 6, device=device, requires_grad=True)
    y6 = ops.norm_act(x2, train=True, drop_p=p, salt=11)
    y6.backward(torch.ones_like(y6))
    assert torch.equal(x2.grad.cpu(), y6.detach().cpu())
    y7 = ops.norm_act(torch.ones(3, 5, 6, 4, device=device).permute(0, 3, 1, 2), train=True, drop_p=p, salt=11)
    assert torch.equal(y7.cpu(), y6.detach().cpu())
    if mask:
        _check_dropout_mask(device, p)


DROP_MASK_SHAPES = ((8, 16, 32, 32), (8, 16, 33, 34), (8, 16, 33, 33))      # rows of 1024 / 1122 / 1089 floats: float4, float2, scalar path; >= 2^17 elements each
DROP_MASK_SEEDS, DROP_MASK_SALTS = (20240607, 77), (7, 1234567)


def dropout_mask_statistics(kept, shape, q):
    """[(what, observed rate, expected rate, 5 sigma)] of a keep mask (flat bool array of the logical (B, C, H, W) tensor) whose elements are
    kept with probability q: keep rate of every sample and every channel, and the rate at which elements i and i + lag agree, each against
    the binomial 5 sigma of its own count - sqrt(r (1 - r) / n) with r the expected rate."""
    B, C = shape[0], shape[1]
    m = kept.reshape(B, C, -1)
    out = []
    sig = lambda r, n: 5.0 * (r * (1.0 - r) / n) ** 0.5
    for b in range(B):
        out.append(("keep rate of sample %d" % b, float(m[b].mean()), q, sig(q, m[b].size)))
    for c in range(C):
        out.append(("keep rate of channel %d" % c, float(m[:, c].mean()), q, sig(q, m[:, c].size)))
    agree = q * q + (1.0 - q) * (1.0 - q)
    for lag in (1, 4, 16384):
        out.append(("agreement of elements i and i + %d" % lag, float((kept[:-lag] == kept[lag:]).mean()), agree, sig(agree, kept.size - lag)))
    return out


def _check_dropout_mask(device, p):
    """The mask the row kernels draw IS the host restatement (helpers.hip_keep_scale), bit for bit, on tensors of at least 2^17 elements (a
    mask that repeats after 16 384 elements or whose 16-bit draws overlap passes every assertion above): two seeds x two salts on the
    float4, float2 and scalar paths, forward and backward; and that mask has the statistics of independent draws
    (dropout_mask_statistics; the seeds are fixed, so is the result)."""
    from helpers import hip_keep_scale
    q = 1.0 - int(np.float32(p) * np.float32(65536.0)) / 65536.0
    for shape in DROP_MASK_SHAPES:
        n = int(np.prod(shape))
        assert n >= 1 << 17
        for seed in DROP_MASK_SEEDS:
            for salt in DROP_MASK_SALTS:
                ops.manual_seed(seed, device)
                ops.begin_step(device)
                word = int(ops.seed_state(device)[0].item())
                x = torch.ones(*shape, device=device, requires_grad=True)
                y = ops.norm_act(x, train=True, drop_p=p, salt=salt)
                y.backward(torch.ones_like(y))
                want = hip_keep_scale(word, salt, p, n)
                what = "dropout mask %s seed %d salt %d" % (shape, seed, salt)
                assert np.array_equal(y.detach().cpu().numpy().reshape(-1), want), what + ": not the host restatement"
                assert np.array_equal(x.grad.cpu().numpy().reshape(-1), want), what + ": backward mask is not the host restatement"
                for name, rate, expect, bound in dropout_mask_statistics(y.detach().cpu().numpy().reshape(-1) != 0, shape, q):
                    assert abs(rate - expect) <= bound, "%s: %s %.5f, expected %.5f +- %.5f" % (what, name, rate, expect, bound)


def check_reduce_and_gate(device):
    g = _gen(3)
    x = _rand(g, 3, 5, 4, 6)
    _run(ops.mean_bc, lambda t: t.mean((2, 3)), [x], device, what="mean_bc")
    _run(ops.max_bc, lambda t: t.flatten(2).max(-1)[0], [x], device, what="max_bc")
    _run(lambda t: ops.max_bc(t.permute(0, 2, 3, 1)), lambda t: t.permute(0, 2, 3, 1).flatten(2).max(-1)[0], [x], device,
         what="max_bc permuted")
    # (B, C, H): a batch larger than the grid of the sliced backward (several samples per workgroup, register dW sums), the 3 -> 1 gate of
    # the output block, a gate wider than one row of threads
    for B, C, H in ((4, 9, 2), (150, 64, 8), (70, 3, 1), (5, 300, 4)):
        _run(ops.se_gate, lambda p, w1, w2: torch.sigmoid(F.linear(F.relu(F.linear(p, w1)), w2)),
             [_rand(g, B, C), _rand(g, H, C), _rand(g, C, H)], device, what="se_gate B%d C%d H%d" % (B, C, H), rel=3e-5)


def check_contract_kred(device, quick=False):
    """weight-gradient shaped contractions (few outputs, long contiguous reduction) take the K-reduction kernel:
    one / four matrix-core tiles per wave, ragged edges, several output tiles, batch index, bias"""
    g = _gen(12)
    ops._KRED_MIN_K, saved = 0, ops._KRED_MIN_K          # the plan keeps short reductions on the tiled path; test sizes are short
    try:
        _check_contract_kred(device, g, quick)
    finally:
        ops._KRED_MIN_K = saved
    if quick:                                                          # the CPU shim is slow on long reductions
        return
    a, x = _rand(g, 2, 3, 8, 5000), _rand(g, 2, 5, 8, 5000)          # K = 80 000: selected by the default plan
    _run(lambda a_, x_: ops.contract("bohw,bchw->oc", a_, x_), lambda a_, x_: torch.einsum("bohw,bchw->oc", a_, x_), [a, x], device,
         what="kred long K", rel=3e-5)
    assert any(p.mode == 2 and p.K == 80000 for p in ops._plans.values())


def _check_contract_kred(device, g, quick=False):
    cases = [
        ("bohw,bchw->oc", (3, 7, 8, 12), (3, 5, 8, 12), None),          # 16x16 tile, K = 288
        ("bohw,bchw->oc", (2, 22, 20, 20), (2, 22, 20, 20), None),       # 32x32 tile, K = 800
        ("bohw,bchw->oc", (2, 40, 16, 32), (2, 60, 16, 32), None),       # 2 x 2 tiles of 32x32, K = 1024
        ("gok,gck->goc", (3, 9, 512), (3, 6, 512), None),                # batch index
        ("ok,ck->oc", (18, 1280 if quick else 5000), (33, 1280 if quick else 5000), 18),   # several splits per replica, bias
    ]
    for spec, sa, sx, nb in cases:
        a, x = _rand(g, *sa), _rand(g, *sx)
        bias = _rand(g, nb) if nb else None
        before = {k for k, p in ops._plans.items() if p.mode == 2}
        if bias is None:
            _run(lambda a_, x_: ops.contract(spec, a_, x_), lambda a_, x_: torch.einsum(spec, a_, x_), [a, x], device,
                 what="kred " + spec, rel=3e-5)
        else:
            _run(lambda a_, x_, b_: ops.contract(spec, a_, x_, b_, "o"), lambda a_, x_, b_: torch.einsum(spec, a_, x_) + b_[:, None],
                 [a, x, bias], device, what="kred+bias " + spec, rel=3e-5)
        assert {k for k, p in ops._plans.items() if p.mode == 2} - before or before, "K-reduction plan was not selected for " + spec
    assert any(p.mode == 2 for p in ops._plans.values())


def check_contract_stream(device):
    """pointwise maps over a long contiguous position axis take the streaming kernel: 1 / 2 / 4 matrix-core row tiles,
    ragged K and M, bias, channel sums in the epilogue, last workgroup partially filled, several row tiles"""
    g = _gen(13)
    ops._STREAM_MIN_N, saved = 256, ops._STREAM_MIN_N
    try:
        for (O, Cc, B, H, W) in ((5, 7, 2, 9, 20), (22, 22, 3, 10, 12), (50, 50, 2, 8, 28), (70, 33, 2, 6, 44), (8, 128, 1, 5, 52)):
            w, x, bias = _rand(g, O, Cc, scale=0.3), _rand(g, B, Cc, H, W), _rand(g, O)
            before = sum(1 for p in ops._plans.values() if p.mode == 1)
            _run(lambda w_, x_, b_: ops.contract("oc,bchw->bohw", w_, x_, b_, "o"),
                 lambda w_, x_, b_: torch.einsum("oc,bchw->bohw", w_, x_) + b_.view(1, -1, 1, 1), [w, x, bias], device,
                 what="stream %dx%d" % (O, Cc), rel=3e-5)
            assert sum(1 for p in ops._plans.values() if p.mode == 1) > before, "streaming plan was not selected"
            ops.begin_step(device)
            y, st = ops.contract_stats("oc,bchw->bohw", w.to(device), x.to(device), bias.to(device), "o")
            r = (torch.einsum("oc,bchw->bohw", w, x) + bias.view(1, -1, 1, 1)).double()
            assert st is not None
            assert_close(y, r, "stream+stats y", rel=3e-5)
            assert_close(_chan_sums(st), torch.stack((r.sum((0, 2, 3)), (r * r).sum((0, 2, 3))), 1).reshape(-1), "stream channel sums", rel=1e-5)
    finally:
        ops._STREAM_MIN_N = saved


def check_contract_chain(device):
    """input gradient of a tensor that feeds several pointwise maps + one collapsing map, large-tensor plan: the pointwise
    gradients run as ONE chained streaming problem (summed in registers), the rest is added by cg_sum_many"""
    g = _gen(16)
    x = _rand(g, 2, 6, 10, 16)                                    # N = 320 positions
    ws = [_rand(g, 5, 6), _rand(g, 9, 6), _rand(g, 5, 6), _rand(g, 4, 6, 10)]
    specs = ["oc,bchw->bohw", "oc,bchw->bohw", "oc,bchw->bohw", "och,bchw->bow"]
    saved = (ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N)
    ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N = 0, 64
    try:
        def run(dev, fused):
            xs = _leaf(x, dev)
            wl = [_leaf(w, dev) for w in ws]
            if fused:
                ops.begin_step(dev)
                ys = [o[0] for o in ops.contract_many([(sp, w, xs, None, None, None) for sp, w in zip(specs, wl)])]
            else:
                ys = [torch.einsum(sp, w, xs) for sp, w in zip(specs, wl)]
            torch.autograd.backward(ys, [_rand(_gen(60 + i), *y.shape).to(dev) for i, y in enumerate(ys)])
            return [xs.grad] + [w.grad for w in wl]
        chained = []
        orig = ops._lib.call
        def spy(name, *a):
            if name == "cg_contract_many":
                chained.append(sum(1 for i in range(a[1]) if a[0][i].chain))
            return orig(name, *a)
        ops._lib.call = spy
        try:
            got = run(device, True)
        finally:
            ops._lib.call = orig
        assert max(chained) == 2, "the three pointwise input gradients were not chained: %s" % chained
        for i, (a, b) in enumerate(zip(got, run("cpu", False))):
            assert_close(a, b, "chained grad%d" % i, rel=3e-5, floor=float(b.abs().max()))
    finally:
        ops._ACC_MAX_FLOATS, ops._STREAM_MIN_N = saved


def check_zero_pool(device):
    """Per-step zero pool (ops.step_scratch): split-K outputs, halos, SE / ST-GCN dW accumulators carved from one
    buffer that begin_step clears - same results as with per-launch memsets, also on the second step (dirty pool)."""
    ops.step_scratch(device, True, floats=1 << 20)
    try:
        for _ in range(2):
            ops.begin_step(device)
            pool = ops._zero_pools[ops._dev(device)]
            g = _gen(11)
            a, b = _rand(g, 3, 300, 7), _rand(g, 3, 300, 5)       # K = 900 -> split-K
            _run(lambda a_, b_: ops.contract("bko,bkc->oc", a_, b_), lambda a_, b_: torch.einsum("bko,bkc->oc", a_, b_), [a, b],
                 device, what="pooled split-K", rel=2e-5)
            assert pool.cur > 0, "split-K output did not come from the pool"
            check_reduce_and_gate(device)
            check_dilated_convs(device, shapes=((2, 5, 4, 10, 7), (3, 6, 5, 4, 6)))      # generic path with halos | whole-sample kernels
            check_stgcn_domain(device, shapes=((2, 3, 3, 6, 9),))
    finally:
        ops.step_scratch(device, False)


def check_copies(device):
    g = _gen(4)
    a, b, c = _rand(g, 2, 3, 4, 5), _rand(g, 2, 6, 4, 5), _rand(g, 2, 2)
    _run(lambda a_, b_, c_: ops.cat_channels([a_, b_, c_], bcast=(False, False, True)),
         lambda a_, b_, c_: torch.cat((a_, b_, c_[:, :, None, None].expand(-1, -1, 4, 5)), 1), [a, b, c], device, what="cat")
    _run(lambda a_, b_: ops.cat_channels([a_, b_]), lambda a_, b_: torch.cat((a_, b_), 1), [_rand(g, 3, 4), _rand(g, 3, 7)],
         device, what="cat 2-D")
    x, y, z = _rand(g, 2, 6, 5, 3), _rand(g, 2, 3, 5, 4), _rand(g, 2, 4, 5, 3)
    _run(lambda x_, y_, z_: ops.add3(x_[:, -1:], y_.permute(0, 3, 2, 1), z_),
         lambda x_, y_, z_: x_[:, -1:] + y_.permute(0, 3, 2, 1) + z_, [x, y, z], device, what="tail add3")
    _run(lambda t: ops.cumsum_time(t.permute(0, 2, 3, 1)), lambda t: t.permute(0, 2, 3, 1).cumsum(1), [_rand(g, 2, 3, 6, 4)],
         device, what="cumsum")
    # aliases for several consumers: their gradients are summed by one launch (3 consumers, strided + odd rows; 10 consumers,
    # float4 rows, two rounds of the 8-way sum; 2-D tensor)
    _run(lambda t: ops.add3(*[a * (i + 1.0) for i, a in enumerate(ops.fanout(t.permute(0, 2, 1, 3), 3))]),
         lambda t: 6.0 * t.permute(0, 2, 1, 3), [_rand(g, 2, 3, 5, 7)], device, what="fanout 3 strided")
    _run(lambda t: sum(a * (i + 1.0) for i, a in enumerate(ops.fanout(t, 10))), lambda t: 55.0 * t, [_rand(g, 2, 3, 4, 8)], device,
         what="fanout 10")
    _run(lambda t: sum(ops.fanout(t, 2)), lambda t: 2.0 * t, [_rand(g, 3, 6)], device, what="fanout 2-D")


def check_dilated_convs(device, shapes=((2, 5, 4, 10, 7), (3, 6, 5, 4, 6), (2, 25, 25, 10, 22), (2, 50, 25, 10, 22), (2, 25, 25, 10, 25), (2, 3, 4, 5, 5), (2, 50, 25, 5, 5))):
    """(B, Cin, Cout, H, W): odd H * W takes the generic contraction, the others the whole-sample kernels (csrc/fpn_conv.hip; float2 rows when
    H * W % 4 == 2: 10 x 7, 10 x 25).  (2, 50, 25, 5, 5): K = 450 with a bias, the split-K plan the model takes at T = 50
    (audit_checks.check_contract_edges asserts that plan)."""
    floor, ops._FPN_MIN_BATCH = ops._FPN_MIN_BATCH, 1          # the whole-sample kernels are switched on by batch size in production
    try:
        for shape in shapes:
            _check_dilated_convs(device, *shape)
    finally:
        ops._FPN_MIN_BATCH = floor


def _check_dilated_convs(device, B, Cin, Cout, H, W):
    g = _gen(5)
    convs_ref = [nn.Conv2d(Cin, Cout, 3, padding=d, dilation=d) for d in (1, 2, 3)]
    convs_dev = [nn.Conv2d(Cin, Cout, 3, padding=d, dilation=d) for d in (1, 2, 3)]
    for r, d in zip(convs_ref, convs_dev):
        d.load_state_dict(r.state_dict())
        d.to(device)
    base = _rand(g, B, H, Cin, W)          # consumed through a permuted (NTCV-style) view
    _run(lambda t: torch.cat(ops.dilated_convs(t.permute(0, 2, 1, 3), convs_dev), 1),
         lambda t: torch.cat([c(t.permute(0, 2, 1, 3)) for c in convs_ref], 1), [base], device, what="dilated convs %s" % ((B, Cin, Cout, H, W),))
    for r, d in zip(convs_ref, convs_dev):
        assert_close(d.weight.grad, r.weight.grad, "dilated dW", rel=2e-5, floor=float(r.weight.grad.abs().max()))
        assert_close(d.bias.grad, r.bias.grad, "dilated db", rel=2e-5, floor=float(r.bias.grad.abs().max()))


def check_rank1_adj(device):
    """rank-1 adjacency seeds (Map2Adj): both domains in one launch, float4 slabs (T*T % 4 == 0) and odd slabs"""
    g = _gen(14)
    for (B, T, V) in ((3, 6, 5), (2, 10, 22), (2, 25, 7), (1, 64, 3)):
        s0, q0, s1, q1 = _rand(g, B, V, T), _rand(g, B, T, V), _rand(g, B, V, T), _rand(g, B, T, V)
        _run(lambda a, b, c, d: torch.cat([t.reshape(-1) for t in ops.rank1_adj([(0, a, b), (1, c, d)])]),
             lambda a, b, c, d: torch.cat([torch.einsum("bvt,bxv->bvtx", a, b).reshape(-1), torch.einsum("bvt,btw->btvw", c, d).reshape(-1)]),
             [s0, q0, s1, q1], device, what="rank1_adj B%d T%d V%d" % (B, T, V))
    s, q = _rand(g, 2, 5, 6), _rand(g, 2, 6, 5)
    _run(lambda a, b: ops.rank1_adj([(1, a, b)])[0], lambda a, b: torch.einsum("bvt,btw->btvw", a, b), [s, q], device, what="rank1_adj single")


def check_eval_harness(device):
    """evaluation-harness kernels (input joint gather, prediction scatter + per-frame MPJPE) against the golden vectors of the
    reference's `_predict` / `losses.mpjpe` and against the oracle on ragged sizes"""
    from oracle import eval_ref as E
    from helpers import load_case
    rec = load_case("eval_h36m")
    t = lambda k: torch.from_numpy(rec[k])
    used, r22, r32 = rec["dim_used"].tolist(), rec["rep22"].tolist(), rec["rep32"].tolist()
    got = ops.gather_joints(t("inputs").to(device), used)
    assert torch.equal(got.cpu(), t("model_input")), "joint gather"
    full, frames = ops.eval_scatter_mpjpe(t("model_output").to(device), t("target").to(device), used, r32, r22)
    assert torch.equal(full.cpu(), t("predicted_full")), "scattered prediction"
    assert_close(frames, t("mpjpe_frames"), "per-frame MPJPE", rel=1e-5)
    g = _gen(15)
    pred, tgt = _rand(g, 3, 7, 4, 3), _rand(g, 3, 7, 9, 3)                 # no repeated joints, odd sizes, strided input
    used2 = [8, 0, 5, 2]
    full, frames = ops.eval_scatter_mpjpe(pred.to(device), tgt.to(device), used2)
    ref = E.scatter_prediction(pred, tgt, used2)
    assert torch.equal(full.cpu(), ref)
    assert_close(frames, E.mpjpe_frames(ref, tgt), "per-frame MPJPE (no repeats)", rel=1e-5)
    xs = _rand(g, 2, 9, 6, 3).to(device).permute(0, 2, 1, 3)               # non-contiguous
    assert torch.equal(ops.gather_joints(xs, [3, 3, 0]).cpu(), xs.cpu()[:, :, [3, 3, 0]])


def check_stage_kernels(device):
    g = _gen(6)
    x = 50 + 350 * _rand(g, 3, 6, 5, 3)
    x[1, 2, 3] = x[1, 3, 3]                 # one zero velocity: sub-gradient 0 of |vel|
    _run(ops.feature_lift, lambda t: O.CISTGCN.feature_lift(t).contiguous(), [x], device, rel=1e-5, what="feature_lift")
    xn = _rand(g, 3, 5, 6, 7)
    _run(ops.dstd_stats, O.CISTGCN.block_stats, [xn], device, what="dstd_stats")
    # rows of 40 joints (one wave per row), and a sample large enough for the 16-wave workgroup (8 x 50 x 22)
    _run(ops.dstd_stats, O.CISTGCN.block_stats, [_rand(g, 2, 3, 4, 40)], device, what="dstd_stats V=40")
    _run(ops.dstd_stats, O.CISTGCN.block_stats, [_rand(g, 2, 8, 50, 22) + 0.5], device, what="dstd_stats 8x50x22")
    _run(ops.dstd_stats, O.CISTGCN.block_stats, [_rand(g, 2, 3, 2, 70)], device, what="dstd_stats V=70")      # rows wider than a wave
    pred, tgt = 50 + 350 * _rand(g, 4, 25, 22, 3), 50 + 350 * _rand(g, 4, 25, 22, 3)
    pd = _leaf(pred, device)
    pr = _leaf(pred, "cpu")
    ld = ops.mpjpe(pd, tgt.to(device))
    lr = O.mpjpe(pr, tgt)
    assert_close(ld, lr, "mpjpe", rel=1e-6)
    ld.backward(); lr.backward()
    assert_close(pd.grad, pr.grad, "mpjpe grad", rel=1e-5, floor=float(pr.grad.abs().max()))


def check_stgcn_domain(device, shapes=((3, 10, 8, 5, 7), (2, 8, 8, 10, 22), (2, 3, 3, 22, 25), (2, 8, 10, 50, 22), (2, 64, 64, 10, 22), (2, 32, 10, 50, 25), (100, 3, 3, 45, 4), (128, 20, 24, 40, 6)),
                       planes=False):
    """planes=True pins the plane kernels (csrc/stgcn_domain_planes.hip) at any batch size; the default switch would send the
    small test batches to the tile kernels.  planes=None pins the tile / matrix-core kernels at any batch size."""
    from cistgcn_amd import _lib
    g = _gen(7)
    prev = _lib.lib().cg_stgcn_domain_planes_min_workgroups((1 << 40) if planes is None else 1 if planes else -1)
    if planes is None:
        assert _lib.lib().cg_stgcn_domain_planes_min_workgroups(-1) == 1 << 40, "the kernel-generation switch is locked: run the tests with CISTGCN_ABLATION=1 (tests/conftest.py sets it)"
    if planes:
        assert _lib.lib().cg_stgcn_domain_planes_min_workgroups(-1) == 1, "the kernel-generation switch is locked: run the tests with CISTGCN_ABLATION=1 (tests/conftest.py sets it)"
    try:
        for (B, Cin, Cout, T, V) in shapes:
            for domain in (0, 1):
                x = _rand(g, B, Cin, T, V)
                adj = _rand(g, B, V, T, T, scale=0.3) if domain == 0 else _rand(g, B, T, V, V, scale=0.3)
                w, bias = _rand(g, Cout, Cin, scale=0.3), _rand(g, Cout)
                spec = "bctv,bvtq->bcqv" if domain == 0 else "bctv,btvw->bctw"
                what = "stgcn_domain B%d Cin%d Cout%d T%d V%d dom%d%s" % (B, Cin, Cout, T, V, domain, " planes" if planes else "")
                _run(lambda x_, a_, w_, b_: ops.stgcn_domain(x_, a_, w_, b_, domain)[0],
                     lambda x_, a_, w_, b_: torch.einsum("oc,bchw->bohw", w_, torch.einsum(spec, x_, a_)) + b_.view(1, -1, 1, 1),
                     [x, adj, w, bias], device, rel=5e-5, what=what)
                ops.begin_step(device)
                y, st = ops.stgcn_domain(x.to(device), adj.to(device), w.to(device), bias.to(device), domain, want_stats=True)
                yc = y.detach().cpu().double()
                ref = torch.stack((yc.sum((0, 2, 3)), (yc * yc).sum((0, 2, 3))), 1).reshape(-1)
                assert_close(_chan_sums(st), ref, what + " channel sums", rel=1e-6)
    finally:
        _lib.lib().cg_stgcn_domain_planes_min_workgroups(prev)


# shapes that reach every instantiation of the plane kernels: (T, V) families 50x22 / 10x22 / 50x25 / 10x18, channel counts that
# are not multiples of 16, a batch that does not fill the last group of 8 samples
PLANE_SHAPES = ((2, 64, 64, 50, 22), (9, 64, 10, 50, 22), (2, 10, 64, 10, 22), (3, 32, 32, 50, 25), (2, 32, 16, 10, 18), (2, 16, 48, 10, 25))


# ---------------------------------------------------------------------------------------------
# whole model against the oracle and against the golden vectors of the real reference
# ---------------------------------------------------------------------------------------------
def _attr(net, dotted):
    obj = net
    for part in dotted.split("."):
        obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
    return obj


def build_pair(C, T, V, device, state=None, seed=0, fused=True, staged=True, stack_all=False, **cfg_kw):
    from cistgcn_amd.models import CISTGCN_0
    torch.manual_seed(seed)
    ora = O.CISTGCN(*make_cfg(C, T, V, **cfg_kw))
    torch.manual_seed(seed)
    net = CISTGCN_0(*make_cfg(C, T, V, **cfg_kw))
    if state is not None:
        ora.load_state_dict(state)
    net.load_state_dict(ora.state_dict(), strict=True)
    net.fused_domain = fused
    net.staged = staged
    if stack_all:                      # stacked first-level maps (tower_maps.hip, stacked gate convolutions) at any size
        net.stack_min_elements = 0
    return net.to(device), ora


def check_model_golden(device, name, modes=("eval", "train"), fused=True, staged=True, stack_all=False):
    """Product model vs the vectors the real reference produced (tests/golden, tools/gen_golden.py)."""
    from helpers import grad_summary
    rec = load_case(name)
    C, T, V, B = [int(v) for v in rec["meta"]]
    for mode in modes:
        net, _ = build_pair(C, T, V, device, state_of(rec), fused=fused, staged=staged, stack_all=stack_all)
        net.train(mode == "train")
        x = torch.from_numpy(rec["x"]).to(device).requires_grad_(True)
        tgt = torch.from_numpy(rec["target"]).to(device)
        if mode == "train":
            net.act_trace = {}
        try:
            pred, = net(x)
            loss = ops.mpjpe(pred, tgt)
            loss.backward()
            trace = net.act_trace
        finally:
            net.act_trace = None
        if mode == "train":
            # train mode: batch statistics over the fixture's four samples; the reference's own fp32 run is 1e-5 .. 4e-4 * max|ref| away from its
            # fp64 run of the same step (`train64/*`), so the comparison is with the fp64 truth and the reference's fp32 error is part of the bound
            def near_truth(got, key, what, floor):
                ref32, ref64 = np.asarray(rec["train/" + key], dtype=np.float64), np.asarray(rec["train64/" + key], dtype=np.float64)
                noise = float(np.abs(ref32 - ref64).max())
                err = float(np.abs(got.detach().cpu().double().numpy() - ref64).max())
                bound = 1e-4 * max(floor, float(np.abs(ref64).max())) + 3.0 * noise
                assert err <= bound, "%s train %s: err vs the reference's fp64 run %.3e > bound %.3e (reference fp32 error %.3e)" % (name, what, err, bound, noise)
            near_truth(pred, "pred", "pred", 1.0)
            near_truth(loss, "loss", "loss", 1.0)
            near_truth(x.grad, "dx", "dL/dx", 1e-1)
        else:
            assert_close(pred, rec[mode + "/pred"], "%s %s pred" % (name, mode))
            assert_close(loss, rec[mode + "/loss"], "%s %s loss" % (name, mode))
            assert_close(x.grad, rec[mode + "/dx"], "%s %s dL/dx" % (name, mode), floor=1e-1)
        for k, ref in rec.items():
            if k.startswith(mode + "/attr/"):
                got = _attr(net, k[len(mode + "/attr/"):]).detach()
                # train mode: BatchNorm over 4 samples amplifies rounding (reference fp32-vs-fp64: 1.6e-4..3.5e-4)
                # interpretation attributes are intermediates: 2e-4 in eval mode (context_layer.seq_joints_dims of the CMU fixture sits
                # behind an ill-conditioned BatchNorm and lands at 0.6 .. 1.03e-4 of its maximum from run to run - fp32 atomics order
                # of the split-K contractions in front of it); the prediction itself is held to 1e-4 above
                assert_close(got[: ref.shape[0]], ref, "%s %s" % (name, k), rel=2e-4 if mode == "eval" else 1e-3)
        if mode != "train":
            continue
        grads = dict(net.named_parameters())
        full = {k[len("train/grad/"):]: v for k, v in rec.items() if k.startswith("train/grad/")}
        assert len(full) == 698
        # the branches this run took against the ones the reference recorded in the fixture (`train/branch/*`)
        names = {m: n for n, m in net.named_modules()}
        flips, elements = 0, 0
        for mod, (y, add) in trace.items():
            if not bool((mod.weight > 0).all()):
                continue                                   # the branch cannot be read off the sign of the output
            y = y.detach().cpu()
            d = y if add is None else y - add.detach().cpu().expand_as(y)
            ref_pos = torch.from_numpy(np.unpackbits(rec["train/branch/" + names[mod]]).astype(bool))[:d.numel()].view_as(d)
            flips += int(((d > 0) != ref_pos)[d != 0].sum())
            elements += d.numel()
        assert flips <= 2e-5 * elements, "%s: %d of %d PReLU branches differ from the reference's" % (name, flips, elements)
        if flips == 0:
            # the same piecewise-linear function as the reference: every gradient against the reference's fp64 run of this step, bound
            # 1e-4 * max(0.25, max|ref64|) + 3 * max|ref32 - ref64| (the reference's own fp32 error on this fixture, test_oracle_golden.py)
            worst = (0.0, None)
            for k, ref32 in full.items():
                ref64 = rec["train64/grad/" + k]
                noise = float(np.abs(ref32.astype(np.float64) - ref64).max())
                bound = 1e-4 * max(0.25, float(np.abs(ref64).max())) + 3.0 * noise
                err = float(np.abs(grads[k].grad.detach().cpu().numpy().astype(np.float64) - ref64).max())
                assert err <= bound, "%s grad %s: err vs the reference's fp64 run %.3e > bound %.3e (reference fp32 error %.3e)" % (name, k, err, bound, noise)
                worst = max(worst, (err / bound, k))
            print("%s: same branches as the reference at all %d PReLU elements; worst gradient at %.2f of its bound (%s)" % (name, elements, worst[0], worst[1]))
        else:
            # a rounding-sized pre-activation landed on the other side of 0: the gradients are those of a neighbouring linear piece (kink
            # allowance of helpers.assert_grads_close); the strict link runs through the oracle: test_golden_case_on_the_branches_of_the_hip_run
            print("%s: %d of %d PReLU elements take the other branch than in the reference's run" % (name, flips, elements))
            assert_grads_close({k: grads[k].grad for k in full}, full, name)
        for k, ref in rec.items():
            if k.startswith("train/state_after/"):
                assert_close(net.state_dict()[k[len("train/state_after/"):]], ref, "%s %s" % (name, k))


def check_model_vs_oracle(device, C, T, V, B, mode, seed=0, scale=350.0, fused=True, smooth=False, edit=None, **cfg_kw):
    """smooth=True sets every PReLU slope to 1 (no kink): the network is then differentiable everywhere except the
    ContextLayer max, and gradients are held to the strict criterion 'as accurate as the reference fp32 CPU path
    against fp64'.  With the real slopes, kink flips are legitimate (helpers.assert_grads_close)."""
    """Product model vs the CPU oracle on fresh seeded inputs (any size the oracle finishes in seconds).  edit: a function of the input
    batch, applied before the target is derived from it (tests/degenerate_checks.py: a dead coordinate, a padded sample)."""
    g = _gen(1000 + seed)
    net, ora = build_pair(C, T, V, device, seed=seed, fused=fused, **cfg_kw)
    To = cfg_kw.get("To", 25)
    with torch.no_grad():                      # move off the init so Adj / gates are numerically alive
        for p in ora.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=g) / max(1.0, float(p[0].numel()) ** 0.5 if p.dim() > 1 else 3.0))
    if smooth:
        with torch.no_grad():
            for k, p in ora.named_parameters():
                if p.dim() == 1 and (p.numel() in (1, 3)) and not k.endswith("bias") and "excitation" not in k and \
                        isinstance(_attr(ora, k.rsplit(".", 1)[0]), nn.PReLU):
                    p.fill_(1.0)
    net.load_state_dict(ora.state_dict())
    x = 50 + scale * torch.randn(B, T, V, 3, generator=g)
    if edit is not None:
        x = edit(x)
    tgt = x[:, -1:] + 20 * torch.randn(B, To, V, 3, generator=g)
    ora.train(); net.train()
    with torch.no_grad():                      # settle running statistics on both sides identically
        ora(x)
    net.load_state_dict(ora.state_dict())
    ora.train(mode == "train"); net.train(mode == "train")
    import copy
    ora64 = copy.deepcopy(ora).double()        # ground truth: the same algorithm in fp64
    xo = x.clone().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    xd = x.clone().to(device).requires_grad_(True)
    po, = ora(xo)
    p64, = ora64(x64)
    pd, = net(xd)
    lo = O.mpjpe(po, tgt)
    l64 = O.mpjpe(p64, tgt.double())
    ld = ops.mpjpe(pd, tgt.to(device))
    lo.backward(); l64.backward(); ld.backward()
    assert_close(pd, po, "pred")
    assert_close(ld, lo, "loss")

    worst = [0.0, ""]

    def as_accurate_as_cpu(got, cpu32, ref64, what):
        """The HIP result must be as close to the fp64 truth as the reference's own fp32 CPU path is (x8 slack),
        or within 2e-4 relative (floor 1e-2) of it."""
        ref64 = ref64.detach()
        e_hip = float((got.detach().cpu().double() - ref64).abs().max())
        e_cpu = float((cpu32.detach().double() - ref64).abs().max())
        bound = max(8.0 * e_cpu, 2e-4 * max(1e-2, float(ref64.abs().max())))
        assert e_hip <= bound, "%s: HIP err vs fp64 %.3e > bound %.3e (CPU fp32 err vs fp64 %.3e)" % (what, e_hip, bound, e_cpu)
        if e_hip / max(bound, 1e-30) > worst[0]:
            worst[0], worst[1] = e_hip / max(bound, 1e-30), what

    gd, g64 = dict(net.named_parameters()), dict(ora64.named_parameters())
    if smooth:
        as_accurate_as_cpu(xd.grad, xo.grad, x64.grad, "dL/dx")
        for k, p in ora.named_parameters():
            as_accurate_as_cpu(gd[k].grad, p.grad, g64[k].grad, "grad " + k)
        print("accuracy vs fp64, worst error / bound: %.3f (%s)" % (worst[0], worst[1]))
    else:
        assert_close(xd.grad, xo.grad, "dL/dx", floor=1e-1)
        assert_grads_close({k: p.grad for k, p in gd.items()}, {k: p.grad for k, p in ora.named_parameters()}, "vs oracle")
    for k in ("st_gcnns.0.dsgn.Adj", "st_gcnns.2.tsgn.Adj", "st_gcnns_o.0.dsgn.Adj", "st_gcnns.1.w1", "st_gcnns_o.0.w2",
              "context_layer.joints", "context_layer.seq_joints_dims"):
        assert_close(_attr(net, k), _attr(ora, k), k, rel=1e-4 if mode == "eval" else 1e-3)   # train: BN over a few samples
    sd, so = net.state_dict(), ora.state_dict()
    for k in so:
        if "running" in k or "num_batches" in k:
            assert_close(sd[k].float(), so[k].float(), k)


def _interpretation_attrs(model):
    """the tensors the reference's evaluation reads after a forward (test.py:146-157): Adj of both domain layers and the gates w1 / w2 of
    every block, the ContextLayer maps"""
    out = {}
    for grp in ("st_gcnns", "st_gcnns_o"):
        for i, blk in enumerate(getattr(model, grp)):
            for k in ("dsgn.Adj", "tsgn.Adj", "w1", "w2"):
                out["%s.%d.%s" % (grp, i, k)] = _attr(blk, k)
    for k in ("joints", "displacements", "seq_joints", "seq_joints_n", "seq_joints_dims"):
        out["context_layer." + k] = getattr(model.context_layer, k)
    return out


def check_model_branch_replay(device, C, T, V, B, mode="train", seed=0, scale=350.0, grad_floor=1.0, max_flip_frac=2e-5,
                              x=None, tgt=None, net=None, ora=None, rel_bound=None, oracle_fp64=False, attr_rel=1e-3, rel_min_size=16, after_device_run=None,
                              **cfg_kw):
    """Flip-aware parity of EVERY parameter gradient (north_star tolerance 1e-4): the HIP model runs first and records
    the branch each PReLU element took (`net.act_trace`); the oracle then differentiates the same piecewise-linear
    function (helpers.BranchReplay), so no kink allowance is needed: pred, loss, dL/dx and all parameter gradients are
    held to max|a-b| <= 1e-4 * max(floor, max|ref|).  The branches the oracle would have taken on its own are compared
    too: they may differ from the HIP ones only on a vanishing fraction of elements whose pre-activation is rounding-sized.
    `after_device_run` (a callable) runs behind the forward + backward of the HIP model, before the oracle runs and before any number is
    compared (check_model_plan asserts the launch plan there)."""
    from helpers import BranchReplay, assert_grads_strict
    g = _gen(2000 + seed)
    To = cfg_kw.get("To", 25)
    if net is None:
        net, ora = build_pair(C, T, V, device, seed=seed, **cfg_kw)
        with torch.no_grad():                      # move off the init so Adj / gates are numerically alive
            for p in ora.parameters():
                p.add_(0.3 * torch.randn(p.shape, generator=g) / max(1.0, float(p[0].numel()) ** 0.5 if p.dim() > 1 else 3.0))
            for m in ora.modules():
                if isinstance(m, nn.PReLU):
                    m.weight.abs_().clamp_(min=0.05)   # branch replay reads the branch off the sign of the output
        net.load_state_dict(ora.state_dict())
    if x is None:
        x = 50 + scale * torch.randn(B, T, V, 3, generator=g)
        tgt = x[:, -1:] + 20 * torch.randn(B, To, V, 3, generator=g)
        ora.train(); net.train()
        with torch.no_grad():                      # settle running statistics on both sides identically
            ora(x)
        net.load_state_dict(ora.state_dict())
    ora.train(mode == "train"); net.train(mode == "train")
    xd = x.clone().to(device).requires_grad_(True)
    net.act_trace, net.drop_trace = {}, {}
    try:
        pd, = net(xd)
        ld = ops.mpjpe(pd, tgt.to(device))
        ld.backward()
        trace, drops = net.act_trace, net.drop_trace
        seed = int(ops.seed_state(device)[0].item())       # the word the kernels of this forward drew their masks from
    finally:
        net.act_trace, net.drop_trace = None, None
    if after_device_run is not None:
        after_device_run()
    dropping = mode == "train" and net.dropout > 0.0
    from helpers import DropReplay
    ora32 = ora
    if oracle_fp64:
        # the oracle in fp64: its result does not depend on the host's thread count or summation order (the fp32 CPU run moved single
        # ill-conditioned tensors by 1e-5 from box to box in round 3, which is why floors were raised there)
        import copy
        for blk in list(ora.st_gcnns) + list(ora.st_gcnns_o):          # attributes of an earlier forward are graph tensors: not copyable
            for holder in (blk, blk.dsgn, blk.tsgn):
                for k in ("Adj", "w1", "w2"):
                    holder.__dict__.pop(k, None)
        for k in ("joints", "displacements", "seq_joints", "seq_joints_n", "seq_joints_dims"):
            ora.context_layer.__dict__.pop(k, None)
        ora = copy.deepcopy(ora).double()
    odt = torch.float64 if oracle_fp64 else torch.float32
    xo = x.clone().to(odt).requires_grad_(True)
    with BranchReplay(net, ora, trace) as rep, DropReplay(net, ora, drops, seed, net.dropout) as drp:
        po, = ora(xo)
        lo = O.mpjpe(po, tgt.to(odt))
        lo.backward()
    # (a slope <= 0 - two PReLUs of the cmu fixture - hides the branch in the sign of the output: those layers take their own branches)
    assert rep.sites == sum(1 for m in ora.modules() if isinstance(m, nn.PReLU) and bool((m.weight > 0).all())), "a PReLU was not replayed (%d sites)" % rep.sites
    if dropping:
        # 14 sites per DSTD_GC block + 7 in the ContextLayer (91 in the shipped configuration); the drop rate must be p
        assert drp.sites == 14 * (len(ora.st_gcnns) + len(ora.st_gcnns_o)) + 7, "dropout sites replayed: %d" % drp.sites
        rate = drp.dropped / max(1, drp.elements)
        assert abs(rate - net.dropout) < 0.02 + 3.0 / max(1, drp.elements) ** 0.5, "drop rate %.4f for p = %.2f" % (rate, net.dropout)
    frac = rep.flips / max(1, rep.elements)
    assert frac <= max_flip_frac, "HIP and oracle disagree on %d of %d PReLU branches" % (rep.flips, rep.elements)
    assert rep.worst <= 1e-2, "a flipped pre-activation is not rounding-sized: |x| = %.2e of the mean magnitude" % rep.worst
    assert_close(pd, po, "pred")
    assert_close(ld, lo, "loss")
    assert_close(xd.grad, xo.grad, "dL/dx", floor=1e-1)
    gd = dict(net.named_parameters())
    rel_report = {}
    worst = assert_grads_strict({k: gd[k].grad for k, _ in ora.named_parameters()}, {k: p.grad for k, p in ora.named_parameters()},
                                "branch replay", floor=grad_floor, rel_bound=rel_bound, report=rel_report, rel_min_size=rel_min_size)
    sd, so = net.state_dict(), ora.state_dict()
    for k in so:
        if "running" in k or "num_batches" in k:
            assert_close(sd[k].float(), so[k].float(), k)
    # the interpretation attributes north_star names (Adj, w1, w2 of every block) and the ContextLayer maps, relative to each tensor's maximum
    worst_attr = (0.0, None)
    oattrs = _interpretation_attrs(ora)
    for k, got in _interpretation_attrs(net).items():
        ref = oattrs[k].detach().double()
        mx = float(ref.abs().max())
        err = float((got.detach().cpu().double() - ref).abs().max())
        assert err <= attr_rel * mx + 1e-30, "attribute %s: max err %.3e > %.1e * max|ref| (%.3e)" % (k, err, attr_rel, mx)
        worst_attr = max(worst_attr, (err / max(mx, 1e-30), k))
    if oracle_fp64:                      # the caller's fp32 oracle carries the updated running statistics on
        ora32.load_state_dict({k: (v.float() if v.dtype.is_floating_point else v) for k, v in so.items()})
    return {"flips": rep.flips, "elements": rep.elements, "worst_flip": rep.worst, "worst_grad": worst, "relative_error": rel_report,
            "worst_attr": worst_attr, "dropout_sites": drp.sites if dropping else 0, "dropped": drp.dropped if dropping else 0}


def check_model_plan(device, entry, mode, stack_all=False, **cfg_kw):
    """One entry of tests/plan_shapes.py: the model at a shape that puts a launch-plan predicate on the side the reference's YAML shapes
    never reach.  The plan first - how often each fused entry point ran in the forward, against the hand-written counts of the entry,
    asserted behind the HIP run and before the oracle runs -, then the numbers: check_model_branch_replay against the fp64 oracle on the
    PReLU branches (and dropout masks) of the HIP run, at the project's bound 1e-4 * max(floor, max|ref|) with floor 0.25 in eval mode and
    1 in train mode, attributes and running statistics at its defaults.  `cfg_kw` adds make_cfg keywords (dropout=0.1)."""
    import helpers
    import loop_shapes
    import plan_shapes
    C, T, V, B = entry["shape"]
    assert B >= 6, "batch statistics over fewer than six samples miss the bound on every plan"
    if entry["stage_geometry"]:
        for line in plan_shapes.stage_kernels(entry):
            print(line)
    saved = {k: getattr(ops, k) for k in entry["patch"]}
    helpers.reset_worst()
    try:
        for k, v in entry["patch"].items():
            setattr(ops, k, v)
        with loop_shapes.counted_calls() as launches:
            try:
                r = check_model_branch_replay(device, C, T, V, B, mode, grad_floor=0.25 if mode == "eval" else 1.0, oracle_fp64=True, stack_all=stack_all,
                                              after_device_run=lambda: plan_shapes.assert_plan(entry, stack_all, dict(launches)),
                                              **dict(entry["cfg"], **cfg_kw))
            except RuntimeError as e:
                if "cistgcn_hip:" not in str(e):
                    raise
                # a predicate lets through what the library refuses (a limit moved on one side only)
                raise AssertionError("launch plan of %s (stack_all=%s): the model called an entry point with a shape it refuses (%s); launches up to there %s"
                                     % (entry["name"], stack_all, e, {k: v for k, v in launches.items() if k in plan_shapes.ALWAYS + plan_shapes.STACKED})) from e
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
    print("plan %s %s stack_all=%s: %s; worst gradient at %.3f of its bound (%s); %s" % (entry["name"], mode, stack_all, helpers.worst_line(), r["worst_grad"][0], r["worst_grad"][1], r))
    return r


SITE_SHAPES = ((8, 10, 22, 8), (72, 10, 22, 8), (8, 70, 6, 8))          # (C, T, V, B): every fused route | past the tail and gate-head limits | past the adjacency limit
SITE_SWITCHES = ("fused_tail", "fused_adj", "fused_maps", "fused_defer")


def check_block_sites_are_route_independent(device):
    """The dropout-site ids of a DSTD_GC block are a property of its modules, not of the kernel route the staged block takes: one train-mode
    forward (dropout 0.1, blocks=1, txc=1) per route - everything on, each model switch off alone, `ops.block_mid_ok` saying no, all of
    them together - must leave the same `drop_trace` (module name -> site id) and the same final `_site`.  Later blocks and the context
    branch draw their masks from those ids, so a route that counted differently would silently change them.  The absolute numbers of the
    first shape (49 named sites, the counter at 95) are the ones every route of the one-method staged block produced."""
    routes = [("everything on", (), False)] + [(k + " off", (k,), False) for k in SITE_SWITCHES] + \
             [("block_mid_ok False", (), True), ("all off", SITE_SWITCHES, True)]
    for C, T, V, B in SITE_SHAPES:
        for stack_all in (False, True):
            net, _ = build_pair(C, T, V, device, stack_all=stack_all, dropout=0.1, blocks=1, txc=1)
            net.train()
            names = {m: n for n, m in net.named_modules()}
            x = (50 + 350.0 * torch.randn(B, T, V, 3, generator=_gen(7))).to(device)
            first = None
            for what, off, no_mid in routes:
                saved = ops.block_mid_ok
                for k in SITE_SWITCHES:
                    setattr(net, k, k not in off)
                if no_mid:
                    ops.block_mid_ok = lambda B_, items: False
                net.drop_trace = {}
                try:
                    with torch.no_grad():
                        net(x)
                    got = ({names[m]: s for m, s in net.drop_trace.items()}, net._site)
                finally:
                    ops.block_mid_ok = saved
                    net.drop_trace = None
                where = "(C, T, V, B) = %s stack_all=%s, route '%s'" % ((C, T, V, B), stack_all, what)
                print("%s: %d named sites, counter at %d" % (where, len(got[0]), got[1]))
                if first is None:
                    first = got
                    if (C, T, V, B) == SITE_SHAPES[0] and not stack_all:
                        assert (len(got[0]), got[1]) == (49, 95), "%s: %d sites, counter at %d" % (where, len(got[0]), got[1])
                assert got[1] == first[1], "%s: the site counter ends at %d, with everything on at %d" % (where, got[1], first[1])
                assert got[0] == first[0], "%s: sites differ from the first route: %s" % (
                    where, sorted((k, first[0].get(k), got[0].get(k)) for k in set(first[0]) | set(got[0]) if first[0].get(k) != got[0].get(k)))


# every shape predicate the launch plan asks, at its limit and one step past it: (family, operator check, its shape AT the limit)
LIMIT_SHAPES = (
    ("collapse_rows V = 32, O = 64", "check_collapse_rows", (2, 6, 4, 32, 64)),
    ("collapse_cols T = 64, O = 64", "check_collapse_cols", (2, 6, 64, 4, 64)),
    ("gate_head C = 64, S = 192", "check_gate_head", (5, 64, 192, 2)),
    ("context_heads hidden = 64", "check_context_heads", (3, 5, 12, 64)),
    ("context_heads H * W = 16384", "check_context_heads", (2, 128, 128, 4)),
    ("map2adj_tail T = 64", "check_map2adj_tail", (2, 64, 6)),          # these three with replay=True (limit_kwargs): at (2, 64, 6) one pre-activation of
    ("map2adj_tail V = 64", "check_map2adj_tail", (2, 6, 64)),          # the 49 152 lies within rounding of 0 and the fp64 reference, left to its own
    ("dstd_tail C = 64", "check_dstd_tail", (2, 64, 3, 5)),             # branches, takes the other one (a kink term of 0.7 in ds; see BranchLog)
    ("pointwise_maps C = 128, 32 tiles of 16 x 16", "check_pointwise_maps", (2, 128, (32, 32), 3, 4)),
    ("pointwise_maps 128 stacked rows", "check_pointwise_maps", (2, 10, (64, 64), 3, 4)),
    ("tower_maps C = 128", "check_tower_maps", (2, 128, (32, 32), 3, 4)),
    ("stgcn_domain Cin = Cout = 128", "check_stgcn_domain", (2, 128, 128, 3, 4)),
    ("dilated_convs H * W = 256", "check_dilated_convs", (2, 5, 4, 16, 16)),
)


def limit_kwargs(check):
    """keywords of the operator check `check` for a LIMIT_SHAPES entry"""
    return {"replay": True} if check in ("check_map2adj_tail", "check_dstd_tail", "check_tower_maps") else {}


def check_predicate_limits():
    """Host side only (no launch): every `*_ok` / `*_supported` predicate of the launch plan says yes AT its limit (the shapes of
    LIMIT_SHAPES, which the operator checks then run) and no one step past it.  Nothing here calls an entry point with a shape it refuses."""
    import ctypes
    from types import SimpleNamespace as NS
    from cistgcn_amd import _lib
    from cistgcn_amd.models.CISTGCN.CISTGCN import CISTGCN
    lib = _lib.lib()
    meta = lambda *shape: torch.empty(shape, device="meta")
    rows = lambda C, T, V, O: ops.collapse_rows_ok(meta(2, C, T, V), meta(O, C, T))
    cols = lambda C, T, V, O: ops.collapse_cols_ok(meta(2, C, T, V), meta(O, C, V))
    assert rows(6, 4, 32, 64) and not rows(6, 4, 33, 64) and not rows(6, 4, 32, 65) and not rows(5, 5, 32, 64), "collapse_rows_ok: V <= 32, O <= 64, C * T % 4 == 0"
    assert not ops.collapse_rows_ok(meta(2, 4, 6, 8).permute(0, 1, 3, 2), meta(5, 4, 8)), "collapse_rows_ok: contiguous input"
    assert cols(6, 64, 4, 64) and not cols(6, 65, 4, 64) and not cols(6, 64, 4, 65) and not cols(5, 64, 5, 64), "collapse_cols_ok: T <= 64, O <= 64, C * V % 4 == 0"
    for (C, T, V, O) in ((6, 64, 4, 64), (6, 65, 4, 64), (6, 64, 4, 65), (5, 64, 5, 64)):
        assert bool(lib.cg_collapse_cols_supported(C, T, V, O)) == cols(C, T, V, O), "collapse_cols_ok and cg_collapse_cols_supported disagree at %s" % ((C, T, V, O),)
    one, three = [nn.PReLU()] * 4, [nn.PReLU()] * 3 + [nn.PReLU(3)]
    assert ops.gate_head_ok(5, 64, 192, one) and not ops.gate_head_ok(5, 65, 192, one) and not ops.gate_head_ok(5, 64, 193, one) and not ops.gate_head_ok(5, 64, 192, three), \
        "gate_head_ok: C <= 64, S <= 192, shared slopes"
    assert ops.context_heads_ok(meta(2, 1, 128, 128), 64) and not ops.context_heads_ok(meta(2, 1, 128, 128), 65) and not ops.context_heads_ok(meta(2, 1, 1, 16385), 64) \
        and not ops.context_heads_ok(meta(2, 2, 4, 4), 8), "context_heads_ok: hidden <= 64, H * W <= 16384, one input channel"
    pw = lambda C, Ms, H, W: ops.pointwise_maps_ok(meta(2, C, H, W), [meta(M, C) for M in Ms])
    assert pw(128, (32, 32), 3, 4) and not pw(129, (32, 32), 3, 4) and not pw(128, (32, 32, 16), 3, 4), "pointwise_maps_ok: C <= 128, (rows / 16) * ceil(C / 16) <= 32"
    assert pw(10, (64, 64), 3, 4) and not pw(10, (64, 64, 1), 3, 4) and not pw(10, (65,), 3, 4) and not pw(10, (8,), 3, 3) and not pw(10, (8,) * 5, 3, 4), \
        "pointwise_maps_ok: 128 stacked rows, 64 rows per map, H * W even, four maps"
    tw = lambda prelus: ops.tower_maps_ok(meta(2, 10, 3, 4), [meta(8, 10)] * len(prelus), prelus)
    assert tw([nn.PReLU(), None]) and not tw([nn.PReLU(), nn.PReLU(8)]), "tower_maps_ok: shared slopes"
    stage = lambda cin, cout: CISTGCN._fused_stage_ok(NS(fused_domain=True), nn.Conv2d(cin, cout, 1))
    assert stage(128, 128) and not stage(129, 128) and not stage(128, 129), "_fused_stage_ok: Cin, Cout <= 128"
    geom = lambda cin, cout, T, V, dom: lib.cg_stgcn_domain_geometry(8, cin, cout, T, V, dom, 1, 0, (ctypes.c_int * 6)())
    assert geom(128, 128, 10, 22, 0) == 0 and geom(129, 128, 10, 22, 0) != 0 and geom(128, 129, 10, 22, 1) != 0, "cg_stgcn_domain_geometry: Cin, Cout <= 128"
    fpn = lambda H, W: bool(lib.cg_fpn_conv_supported(8, 5, 4, H, W))
    assert fpn(16, 16) and fpn(10, 25) and not fpn(10, 26) and not fpn(1, 257) and not fpn(9, 9) and not fpn(5, 5), "cg_fpn_conv_supported: H * W <= 256, H * W % 4 in (0, 2)"
    assert ops.block_input_ok(meta(2, 10, 10, 22)) and not ops.block_input_ok(meta(2, 10, 22, 10).permute(0, 1, 3, 2)), "block_input_ok: contiguous input"


def check_family_at_limit(device, case):
    """one entry of LIMIT_SHAPES: the operator-level check of the family AT the limit of its predicate, small batch"""
    import helpers
    what, check, shape = case
    helpers.reset_worst()
    globals()[check](device, shapes=(shape,), **limit_kwargs(check))
    print("%s: %s %s: %s" % (what, check, shape, helpers.worst_line()))


def check_dstd_tail_kink_branches(device):
    """The fused tail takes, in its backward, the PReLU branch its own forward took - also at pre-activations within an ulp of 0.
    Deterministic, eval mode: for eight channels with different BatchNorm constants, the 1024 positions of sample 0 carry z = the fp32
    neighbours (one ulp apart) of the zero z* = mean - beta / (gamma * rstd) of the prelu1 pre-activation gamma * (z - mean) * rstd + beta,
    so in every channel the pre-activation walks through 0 in steps of an ulp (y = 0, w = 1 and unit tcn constants make z = r, the
    residual input, bit for bit).  The reference (fp64 stock PyTorch) takes the branches read off the forward's PReLU outputs and nothing is
    explained away as a kink term: with two different roundings of the pre-activation in forward ((z - mean) * (gamma * rstd) + beta) and
    backward (gamma * zhat + beta) the elements between their two zero crossings got the slope forward and the factor 1 backward - dr off
    by (1 - alpha) * |dx| at those elements (0.23 against a bound of 6e-5 on the CPU shim).  At model level one such element among a million moved the most
    sensitive gradients of a train step (`map_t.0.weight` of the block and of the blocks in front of it) by ten times their bound in about
    one run of thirty, the elements changing with the order of the fp32 atomics."""
    from cistgcn_amd.models.layers.SE import SELayer2d
    B, C, T, V = 2, 8, 32, 32
    P = T * V
    g = _gen(77)
    bns = [nn.BatchNorm2d(C) for _ in range(5)]
    al = [nn.PReLU() for _ in range(5)]
    conv, se = nn.Conv2d(2 * C, C, 1, bias=False), SELayer2d(C, reduction=8)
    with torch.no_grad():
        for bn in bns[:2]:                       # tcn BatchNorms: y = 0 -> exactly 0 (mean 0, beta 0)
            bn.weight.fill_(1.0); bn.bias.zero_(); bn.running_mean.zero_(); bn.running_var.fill_(1.0)
        for bn in bns[2:]:
            bn.weight.copy_(1 + 0.3 * torch.rand(C, generator=g)); bn.running_mean.copy_(0.1 + 0.3 * torch.rand(C, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(C, generator=g)); bn.bias.copy_(-0.2 - 0.4 * torch.rand(C, generator=g))
        for i, a in enumerate(al):
            a.weight.fill_(0.1 + 0.07 * i)
        conv.weight.copy_(0.3 * torch.randn(conv.weight.shape, generator=g))
        se.w1.copy_(0.5 * torch.randn(se.w1.shape, generator=g)); se.w2.copy_(0.5 * torch.randn(se.w2.shape, generator=g))
    mods = nn.ModuleList(bns + al + [conv, se]).to(device).eval()
    bp = bns[2]
    rstd = 1.0 / torch.sqrt(bp.running_var.detach().cpu().double() + bp.eps)
    zstar = (bp.running_mean.detach().cpu().double() - bp.bias.detach().cpu().double() / (bp.weight.detach().cpu().double() * rstd)).float()
    assert bool((zstar > 0.1).all())
    r1 = 0.5 + torch.rand(B, C, T, V, generator=g)
    for c in range(C):
        z0 = np.float32(zstar[c].item())
        r1[0, c] = torch.from_numpy((z0 + np.spacing(z0) * np.arange(-P // 2, P // 2, dtype=np.float32)).astype(np.float32)).view(T, V)
    data = [torch.zeros(B, C, T, V), torch.zeros(B, C, T, V), r1, 0.5 + torch.rand(B, C, T, V, generator=g), torch.ones(B, C), torch.ones(B, C), _rand(g, B, C, T, V)]
    gout = _rand(g, B, C, T, V).to(device)
    rparams, rbufs = _ref_state(mods)
    leaves = [_leaf(t, device) for t in data]
    ops.begin_step(device)
    taps = []
    out, _ = ops.dstd_tail(leaves[:2], [None, None], leaves[2:4], (leaves[4], leaves[5]), list(mods[:5]), list(mods[5:10]), mods[10].weight, mods[11], leaves[6], False, taps=taps)
    out.backward(gout)
    a1 = taps[2].detach().cpu()[0]                        # prelu1 outputs of sample 0: both branches occur in every channel, one crossing each
    assert all(bool((a1[c] > 0).any()) and bool((a1[c] <= 0).any()) for c in range(C)), "the pre-activations do not cross 0"
    rleaves = [_leaf(t.double(), "cpu") for t in data]
    log = BranchLog()
    rout = _dstd_tail_ref(rleaves, rparams, rbufs, False, 0.0, (0, 0), 0, log, taps)
    rout.backward(gout.detach().cpu().double())
    log.settle("dstd_tail kink branches")
    assert_close(out, rout, "dstd_tail kink branches out", rel=2e-5)
    for k in (2, 0):
        ref = rleaves[k].grad
        assert_close(leaves[k].grad, ref, "dstd_tail kink branches: gradient of %s on the forward's branches" % ("r1" if k == 2 else "y1"), rel=5e-5, floor=float(ref.abs().max()))
    print("dstd_tail kink branches: %d of %d pre-activations of the reference within rounding of 0 on the other side than the kernel's forward; backward on the forward's branches everywhere"
          % (log.flips, B * C * P * 5))


# ---------------------------------------------------------------------------------------------
# fp64 stock-PyTorch references of the two fused tails: functional (F.batch_norm / F.prelu / F.conv2d / F.linear) on plain
# CPU tensors that carry the values of the device modules - no module, operator or kernel of cistgcn_amd is involved
# ---------------------------------------------------------------------------------------------
def _ref_state(mods, dtype=torch.float64):
    """CPU leaves and buffers (fp64) with the values of `mods`, keyed like named_parameters() / named_buffers()"""
    params = {k: p.detach().cpu().to(dtype).clone().requires_grad_(True) for k, p in mods.named_parameters()}
    bufs = {k: (b.detach().cpu().to(dtype).clone() if b.dtype.is_floating_point else b.detach().cpu().clone()) for k, b in mods.named_buffers()}
    return params, bufs


def _ref_bn(x, params, bufs, key, train):
    """nn.BatchNorm2d with default momentum / eps, functional"""
    if train:
        bufs[key + ".num_batches_tracked"] += 1
    return F.batch_norm(x, bufs[key + ".running_mean"], bufs[key + ".running_var"], params[key + ".weight"], params[key + ".bias"], train, 0.1, 1e-5)


def _ref_keep(seed, salt, p, shape):
    """the keep factors the kernels draw at dropout site `salt` for the flat element indices of a tensor of `shape`"""
    from helpers import hip_keep_scale
    n = 1
    for d in shape:
        n *= int(d)
    return torch.from_numpy(hip_keep_scale(seed, salt, p, n)).view(*shape)


def _dstd_tail_ref(data, params, bufs, train, p, salts, seed, log, taps):
    """DSTD_GC tail (CISTGCN.py:266-269, :388, :305-309, :390) in fp64.  Keys: 0-4 BatchNorm (tcn1, tcn2, prelu1, prelu2, compressor),
    5-9 the PReLU of the same five places, 10 the compressor convolution, 11 the SELayer2d.  taps: the five PReLU outputs of the HIP run
    (x_1, x_2, a_1, a_2, h) whose branches the reference takes (BranchLog), or None: its own."""
    y1, y2, r1, r2, w1, w2, bres = data
    taps = taps if taps is not None else [None] * 5
    acts = []
    for i, (y, r, w) in enumerate(((y1, r1, w1), (y2, r2, w2))):
        u = _ref_bn(y, params, bufs, str(i), train)
        if train and p > 0.0:
            u = u * _ref_keep(seed, salts[i], p, u.shape).to(u.dtype)
        x = log.prelu(u + r, params["%d.weight" % (5 + i)], taps[i])
        acts.append(log.prelu(_ref_bn(w[:, :, None, None] * x, params, bufs, str(2 + i), train), params["%d.weight" % (7 + i)], taps[2 + i]))
    h0 = F.conv2d(torch.cat(acts, 1), params["10.weight"])
    h = log.prelu(_ref_bn(h0, params, bufs, "4", train), params["9.weight"], taps[4])
    gate = torch.sigmoid(F.linear(F.relu(F.linear(h.mean((2, 3)), params["11.excitation.0.weight"])), params["11.excitation.2.weight"]))
    return h * gate[:, :, None, None] + bres


def _map2adj_tail_ref(data, params, bufs, train, p, salts, seed, log, dev_taps):
    """Map2Adj.forward CISTGCN.py:183-189 with the expansor of :165-170, both domains, in fp64.  Keys: <tower>.0 / .4 the convolutions,
    .1 the BatchNorm, .3 the PReLU.  dev_taps: the PReLU outputs of the HIP run whose branches the reference takes (BranchLog), or None: its
    own.  Returns (adjacencies, PReLU outputs)."""
    dev_taps = dev_taps if dev_taps is not None else [None] * 2
    s0, q0, s1, q1 = data
    seeds = (torch.einsum("bvt,bxv->bvtx", s0, q0), torch.einsum("bvt,btw->btvw", s1, q1))
    adj, taps = [], []
    for i, o in enumerate(seeds):
        u = _ref_bn(F.conv2d(o, params["%d.0.weight" % i]), params, bufs, "%d.1" % i, train)
        if train and p > 0.0:
            u = u * _ref_keep(seed, salts[i], p, u.shape).to(u.dtype)
        taps.append(log.prelu(u, params["%d.3.weight" % i], dev_taps[i]))
        adj.append(F.conv2d(taps[-1], params["%d.4.weight" % i]))
    return adj, taps


def _assert_tail_grads(got, ref_leaves, params, gamma_floor, what, log=None, fp32_run=None):
    """input gradients, then parameter gradients in named_parameters() order, against the fp64 reference: rel 5e-5 with the floor
    max(1e-3, max|ref|); `gamma_floor` maps a weight in front of a train-mode BatchNorm to that BatchNorm's weight (its gradient is the
    remainder of cancelling sums of the size of the BatchNorm weight's gradient, as in check_tower_maps).  log: kink terms accounted for
    (assert_grads_at_kinks).
    Every parameter gradient here is one sum over B*T*V terms and may exceed that bound at production size for no other reason than the
    order of an fp32 summation.  Only for a PARAMETER gradient that does: `fp32_run()` evaluates the same chain in fp32 stock PyTorch on
    the CPU (same masks, same branches; returns gradients in the same order), and the kernel is allowed 8 times that run's error against
    fp64 on this tensor - the factor of test_gradients_as_accurate_as_cpu_fp32.  Input gradients keep the bound.
    Measured on the MI355X, slopes of the default lists: one tensor needs it, the slope gradient of the second tcn PReLU of dstd_tail at
    (C, T, V) = (32, 50, 25), B = 129 - a sum over 5.2 million terms: kernel 9.4e-4 off fp64 (bound 4.9e-4, max|ref| 9.76), fp32 stock
    PyTorch on the CPU 4.2e-4, so the kernel is held to 3.3e-3 there."""
    names = ["input %d" % i for i in range(len(ref_leaves))] + list(params)
    leaves = list(ref_leaves) + [params[k] for k in params]
    refs = [t.grad for t in leaves]
    assert len(got) == len(refs), (len(got), len(refs))
    floors = []
    for k, b in zip(names, refs):
        floor = max(1e-3, float(b.abs().max()))
        if k in gamma_floor:
            floor = max(floor, float(params[gamma_floor[k]].grad.abs().max()))
        floors.append(floor)
    true_refs = refs
    refs = kink_adjusted(got, refs, floors, what, log, leaves)
    if fp32_run is not None:
        cpu32 = None
        for i, k in enumerate(names):
            err = float((got[i].detach().cpu().double() - refs[i]).abs().max())
            if i >= len(ref_leaves) and err > 5e-5 * floors[i] and refs[i].numel() <= 64 * 128:
                cpu32 = fp32_run() if cpu32 is None else cpu32
                err32 = float((cpu32[i].double() - true_refs[i]).abs().max())
                if 8.0 * err32 > 5e-5 * floors[i]:
                    print("%s fp64 grad %s: kernel error %.3e over the bound %.3e; fp32 stock PyTorch on the CPU is %.3e off fp64 (max|ref| %.3e): bound %.3e"
                          % (what, k, err, 5e-5 * floors[i], err32, float(refs[i].abs().max()), 8.0 * err32))
                    floors[i] = 8.0 * err32 / 5e-5
    for g, r, fl, k in zip(got, refs, floors, names):
        assert_close(g, r, "%s grad fp64 %s" % (what, k), rel=5e-5, floor=fl)


def check_dstd_tail(device, shapes=((3, 20, 7, 9), (2, 8, 10, 22), (5, 64, 6, 11), (3, 32, 5, 8), (4, 16, 6, 6), (2, 40, 4, 5)), replay=False, low_var=False):      # widths of every instantiation of the matrix phases: (1,1) (1,2) (2,4) (4,8) and the run-time form (20, 40)
    """ops.dstd_tail (phase kernels of csrc/dstd_tail.hip) against (a) the same chain built from the row kernels and the generic
    contraction: identical dropout draws (same seed word and site ids; exact to rounding, which pins the dropout site ids) and (b) the
    same chain in stock PyTorch in fp64 on the CPU (_dstd_tail_ref; its dropout sites multiply by helpers.hip_keep_scale): train and
    eval mode, output, emitted channel sums, every input / parameter gradient, running statistics.  shapes: (B, C, T, V).
    replay (tensors of millions of elements): the fp64 reference takes the PReLUs on the branches of the fused run and the elements whose
    backward took the other branch are accounted for (BranchLog, assert_grads_at_kinks).
    low_var: channels 0 and 1 of all five BatchNorms see a variance comparable to eps (LOW_VAR_BATCH; the two behind the gates w1 / w2 and
    the one behind the compressor through small gate columns / weight rows)."""
    from cistgcn_amd.models.layers.SE import SELayer2d
    g = _gen(31)
    for (B, C, T, V) in shapes:
        for train in (True, False):
            def make():
                gg = _gen(100 + B + C)
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
                    if low_var:
                        _low_var_rows(conv.weight)
                        for bn in bns:
                            _low_var_running(bn)
                    se.w1.copy_(0.5 * torch.randn(se.w1.shape, generator=gg)); se.w2.copy_(0.5 * torch.randn(se.w2.shape, generator=gg))
                mods = nn.ModuleList(bns + al + [conv, se]).to(device)
                return list(mods[:5]), list(mods[5:10]), mods[10], mods[11], mods
            data = [_rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C, T, V), _rand(g, B, C), _rand(g, B, C),
                    _rand(g, B, C, T, V)]
            if low_var:
                data[0], data[1] = _low_var_input(data[0]), _low_var_input(data[1])
                for w in (data[4], data[5]):
                    w[:, 0] *= LOW_VAR_ROWS[0]; w[:, 1] *= LOW_VAR_ROWS[1]
            gout = _rand(g, B, C, T, V).to(device)
            rparams, rbufs = _ref_state(make()[4])
            results = []
            for fused in (True, False):
                bns, al, conv, se, mods = make()
                mods.train(train)
                y1, y2, r1, r2, w1, w2, bres = [_leaf(t, device) for t in data]
                ops.manual_seed(1234, device)
                ops.begin_step(device)
                seed = int(ops.seed_state(device)[0].item())          # the word the kernels of this step draw their masks from
                def sums(y):
                    st = ops._arena(torch.device(device)).take(2 * C * 16)
                    yc = y.detach().double()
                    st.view(16, C, 2)[0].copy_(torch.stack((yc.sum((0, 2, 3)), (yc * yc).sum((0, 2, 3))), 1))
                    return st
                p = 0.25
                if fused:
                    acts = [] if replay else None
                    out, ost = ops.dstd_tail([y1, y2], [sums(y1), sums(y2)] if train else [None, None], [r1, r2], (w1, w2), bns, al, conv.weight, se,
                                             bres, train, drop_p=p, salts=(7, 9), emit_stats=train, taps=acts)
                else:
                    x12 = ops.norm_act_many([dict(x=y1, bn=bns[0], train=train, drop_p=p, salt=7, add=r1, prelu=al[0], stats=sums(y1) if train else None),
                                             dict(x=y2, bn=bns[1], train=train, drop_p=p, salt=9, add=r2, prelu=al[1], stats=sums(y2) if train else None)])
                    ab = ops.norm_act_many([dict(x=x12[0], pre=w1, bn=bns[2], train=train, prelu=al[2]),
                                            dict(x=x12[1], pre=w2, bn=bns[3], train=train, prelu=al[3])])
                    h0 = ops.contract("oc,bchw->bohw", conv.weight.view(C, 2 * C), ops.cat_channels(ab))
                    h = ops.norm_act(h0, bn=bns[4], train=train, prelu=al[4])
                    gate = ops.se_gate(ops.mean_bc(h), se.w1, se.w2)
                    out, ost = ops.norm_act(h, pre=gate, add=bres, add_post=True, emit_stats=True)
                    acts = [x12[0], x12[1], ab[0], ab[1], h]
                out.backward(gout)
                grads = [t.grad for t in (y1, y2, r1, r2, w1, w2, bres)] + [p_.grad for p_ in mods.parameters()]
                results.append((out.detach(), _chan_sums(ost) if (train or not fused) else None, grads, [b.clone() for b in mods.buffers()], acts))
            what = "dstd_tail%s B%d C%d T%d V%d %s" % (" low variance" if low_var else "", B, C, T, V, "train" if train else "eval")
            assert_close(results[0][0], results[1][0], what + " out", rel=2e-5)
            if train:
                assert_close(results[0][1], results[1][1], what + " sums", rel=1e-6)
            if replay:
                for a, b in zip(results[0][4], results[1][4]):
                    assert_close(a, b, what + " PReLU outputs", rel=2e-5)
            for k, (a, b) in enumerate(zip(results[0][3], results[1][3])):
                assert_close(a.float(), b.float(), "%s buffer[%d]" % (what, k), rel=1e-6)
            # (b) stock PyTorch in fp64
            gamma_floor = {"10.weight": "4.weight"} if train else {}
            rleaves = [_leaf(t.double(), "cpu") for t in data]
            log = BranchLog()
            rout = _dstd_tail_ref(rleaves, rparams, rbufs, train, 0.25, (7, 9), seed, log, results[0][4])
            rout.backward(gout.detach().cpu().double(), retain_graph=replay)
            log.settle(what)
            assert_close(results[0][0], rout, what + " fp64 out", rel=2e-5)
            if train:
                # emitted f64 sums of the fp32 output against the sums of the fp64 output: the bound check_tower_collapse holds its sums to
                ro = rout.detach()
                sums = results[0][1].double().view(-1, 2)
                assert_close(sums[:, 0], ro.sum((0, 2, 3)), what + " fp64 sums", rel=1e-4, floor=max(1.0, float(ro.abs().sum((0, 2, 3)).max())))
                assert_close(sums[:, 1], (ro * ro).sum((0, 2, 3)), what + " fp64 sums of squares", rel=1e-4, floor=max(1.0, float((ro * ro).sum((0, 2, 3)).max())))

            def fp32_run():
                p32, b32 = _ref_state(make()[4], torch.float32)
                leaves = [_leaf(t, "cpu") for t in data]
                _dstd_tail_ref(leaves, p32, b32, train, 0.25, (7, 9), seed, BranchLog(), results[0][4]).backward(gout.detach().cpu())
                return [t.grad for t in leaves] + [p32[k].grad for k in p32]
            _assert_tail_grads(results[0][2], rleaves, rparams, gamma_floor, what, log if replay else None, fp32_run if replay else None)
            for (k, bb), a in zip(rbufs.items(), results[0][3]):
                assert_close(a.float(), bb.float(), "%s fp64 buffer %s" % (what, k), rel=1e-5)
            # (a) again: the gradients of the fused run against the chain's (replay: either run may hold a kink term the other does not)
            leaves = rleaves + [rparams[k] for k in rparams]
            assert_grads_at_kinks(results[0][2], results[1][2], [max(1e-3, float(b.abs().max())) for b in results[1][2]], range(len(leaves)),
                                  what + " fused | chain", log if replay else None, leaves, both_ways=True)


def check_map2adj_tail(device, shapes=((3, 7, 9), (2, 10, 22), (4, 25, 6), (2, 40, 6), (2, 6, 36)), replay=False, low_var=False):
    """ops.map2adj_tail (phase kernels of csrc/map2adj_tail.hip) against (a) the same chain built from the rank-1 kernel, the
    generic contraction and the row kernels: identical dropout draws (exact to rounding, which pins the dropout site ids) and (b) the
    same chain in stock PyTorch in fp64 on the CPU (_map2adj_tail_ref; its dropout sites multiply by helpers.hip_keep_scale): train and
    eval mode, both adjacencies, the PReLU taps, every input / parameter gradient, running statistics.  shapes: (B, T, V).
    replay: as in check_dstd_tail (tensors of millions of elements, see BranchLog).  low_var: rows 0 and 1 of the first convolution of both
    expansors scaled so that their BatchNorm channels see the variances LOW_VAR_BATCH."""
    from cistgcn_amd.models.CISTGCN.CISTGCN import Stage, _conv
    g = _gen(47)
    for (B, T, V) in shapes:
        for train in (True, False):
            def make():
                gg = _gen(200 + B + T)
                exps = []
                for ch in (V, T):
                    e = Stage(s0=_conv(ch, ch), s1=nn.BatchNorm2d(ch), s3=nn.PReLU(), s4=_conv(ch, ch))
                    with torch.no_grad():
                        e[0].weight.copy_(0.4 * torch.randn(e[0].weight.shape, generator=gg)); e[4].weight.copy_(0.4 * torch.randn(e[4].weight.shape, generator=gg))
                        e[1].weight.copy_(1 + 0.3 * torch.randn(ch, generator=gg)); e[1].bias.copy_(0.3 * torch.randn(ch, generator=gg))
                        e[1].running_mean.copy_(0.2 * torch.randn(ch, generator=gg)); e[1].running_var.copy_(0.5 + torch.rand(ch, generator=gg))
                        e[3].weight.fill_(0.2 + 0.1 * len(exps))
                    if low_var:
                        seed_ = torch.einsum("bvt,bxv->bvtx", data[0], data[1]) if len(exps) == 0 else torch.einsum("bvt,btw->btvw", data[2], data[3])
                        _low_var_rows(e[0].weight, F.conv2d(seed_.double(), e[0].weight.detach().double()))
                        _low_var_running(e[1])
                    exps.append(e)
                mods = nn.ModuleList(exps).to(device)
                return list(mods), mods
            data = [_rand(g, B, V, T), _rand(g, B, T, V), _rand(g, B, V, T), _rand(g, B, T, V)]
            gouts = [_rand(g, B, V, T, T).to(device), _rand(g, B, T, V, V).to(device)]
            rparams, rbufs = _ref_state(make()[1])
            results = []
            for fused in (True, False):
                exps, mods = make()
                mods.train(train)
                s0, q0, s1, q1 = [_leaf(t, device) for t in data]
                seeds = [(0, s0, q0), (1, s1, q1)]
                ops.manual_seed(4321, device)
                ops.begin_step(device)
                seed = int(ops.seed_state(device)[0].item())          # the word the kernels of this step draw their masks from
                p = 0.25
                if fused:
                    taps = []
                    adj = ops.map2adj_tail(seeds, exps, train, drop_p=p, salts=(5, 6), taps=taps)
                else:
                    oo = ops.rank1_adj(seeds)
                    es = [ops.contract("oc,bchw->bohw", e[0].weight.view(e[0].out_channels, -1), o) for e, o in zip(exps, oo)]
                    taps = ops.norm_act_many([dict(x=es[i], bn=e[1], train=train, drop_p=p, salt=5 + i, prelu=e[3]) for i, e in enumerate(exps)])
                    adj = [ops.contract("oc,bchw->bohw", e[4].weight.view(e[4].out_channels, -1), h) for e, h in zip(exps, taps)]
                torch.autograd.backward(list(adj), gouts)
                grads = [t.grad for t in (s0, q0, s1, q1)] + [p_.grad for p_ in mods.parameters()]
                results.append(([a.detach() for a in adj], [t.detach() for t in taps], grads, [b.clone() for b in mods.buffers()]))
            what = "map2adj_tail%s B%d T%d V%d %s" % (" low variance" if low_var else "", B, T, V, "train" if train else "eval")
            for k in range(2):
                assert_close(results[0][0][k], results[1][0][k], "%s adj[%d]" % (what, k), rel=2e-5)
                assert_close(results[0][1][k], results[1][1][k], "%s tap[%d]" % (what, k), rel=2e-5)
            for k, (a, b) in enumerate(zip(results[0][3], results[1][3])):
                assert_close(a.float(), b.float(), "%s buffer[%d]" % (what, k), rel=1e-6)
            # (b) stock PyTorch in fp64
            rleaves = [_leaf(t.double(), "cpu") for t in data]
            log = BranchLog()
            radj, rtaps = _map2adj_tail_ref(rleaves, rparams, rbufs, train, 0.25, (5, 6), seed, log, results[0][1] if replay else None)
            torch.autograd.backward(radj, [t.detach().cpu().double() for t in gouts], retain_graph=replay)
            log.settle(what)
            for k in range(2):
                assert_close(results[0][0][k], radj[k], "%s fp64 adj[%d]" % (what, k), rel=2e-5)
                assert_close(results[0][1][k], rtaps[k], "%s fp64 tap[%d]" % (what, k), rel=2e-5)

            def fp32_run():
                p32, b32 = _ref_state(make()[1], torch.float32)
                leaves = [_leaf(t, "cpu") for t in data]
                a32, _ = _map2adj_tail_ref(leaves, p32, b32, train, 0.25, (5, 6), seed, BranchLog(), results[0][1])
                torch.autograd.backward(a32, [t.detach().cpu() for t in gouts])
                return [t.grad for t in leaves] + [p32[k].grad for k in p32]
            _assert_tail_grads(results[0][2], rleaves, rparams, {"0.0.weight": "0.1.weight", "1.0.weight": "1.1.weight"} if train else {}, what,
                               log if replay else None, fp32_run if replay else None)
            for (k, bb), a in zip(rbufs.items(), results[0][3]):
                assert_close(a.float(), bb.float(), "%s fp64 buffer %s" % (what, k), rel=1e-5)
            # (a) again: the gradients of the fused run against the chain's (replay: either run may hold a kink term the other does not)
            leaves = rleaves + [rparams[k] for k in rparams]
            assert_grads_at_kinks(results[0][2], results[1][2], [max(1e-3, float(b.abs().max())) for b in results[1][2]], range(len(leaves)),
                                  what + " fused | chain", log if replay else None, leaves, both_ways=True)


def check_gate_head(device, shapes=((5, 8, 10, 2), (37, 64, 102, 2), (4, 3, 46, 2), (20, 10, 22, 1)), low_var=False):
    """ops.gate_head (csrc/gate_head.hip) against stock PyTorch in fp64: BatchNorm2d -> Dropout(0) -> PReLU -> cat(statistics) -> Linear ->
    BatchNorm1d -> PReLU -> Linear per gate path (CISTGCN.py:337-352): gates, both PReLU taps, dz, the statistics' gradient, every
    parameter gradient, running statistics; train and eval mode; the statistics handed over as column slices of a wider tensor.
    Dropout: keep factors of helpers.hip_keep_scale applied in the reference.  shapes: (B, C, S, paths).  low_var: channels 0 and 1 of z
    have the variances LOW_VAR_BATCH (BatchNorm2d), rows 0 and 1 of the first Linear are small (BatchNorm1d)."""
    from cistgcn_amd.models.CISTGCN.CISTGCN import Stage
    from helpers import hip_keep_scale
    g = _gen(91)
    for (B, C, S, n) in shapes:
        for train, pdrop in ((True, 0.0), (True, 0.25), (False, 0.0)):
            def make(dt):
                gg = _gen(600 + C)
                convs, maps = [], []
                for k in range(n):
                    conv = Stage(s5=nn.BatchNorm2d(C), s7=nn.PReLU())
                    mp = Stage(s0=nn.Linear(C + S, C, bias=False), s1=nn.BatchNorm1d(C), s3=nn.PReLU(), s4=nn.Linear(C, C, bias=False))
                    with torch.no_grad():
                        for bn in (conv[5], mp[1]):
                            bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=gg)); bn.bias.copy_(0.3 * torch.randn(C, generator=gg))
                            bn.running_mean.copy_(0.2 * torch.randn(C, generator=gg)); bn.running_var.copy_(0.5 + torch.rand(C, generator=gg))
                        mp[0].weight.copy_(torch.randn(mp[0].weight.shape, generator=gg) * 0.3); mp[4].weight.copy_(torch.randn(C, C, generator=gg) * 0.3)
                        conv[7].weight.fill_(0.1 + 0.1 * k); mp[3].weight.fill_(0.3 - 0.1 * k)
                    if low_var:
                        _low_var_rows(mp[0].weight)
                        _low_var_running(conv[5]); _low_var_running(mp[1])
                    convs.append(conv); maps.append(mp)
                return nn.ModuleList(convs).to(dt), nn.ModuleList(maps).to(dt)
            z0 = [0.5 + 1.5 * _rand(g, B, C) for _ in range(n)]
            if low_var:
                z0 = [_low_var_input(t) for t in z0]
            wide = _rand(g, B, S + 5)
            gw = [_rand(g, B, C) for _ in range(n)]
            salts = [(3 + k, 11 + k) for k in range(n)]
            seed = 987654321
            what = "gate_head%s B%d C%d S%d x%d %s p=%.2f" % (" low variance" if low_var else "", B, C, S, n, "train" if train else "eval", pdrop)
            # fp64 reference (the keep factors of the kernels' hash)
            rc, rm = make(torch.float64)
            rc.train(train); rm.train(train)
            zr = [_leaf(t.double(), "cpu") for t in z0]
            sr = _leaf(wide.double(), "cpu")
            outs, taps_r = [], []
            for k in range(n):
                keep2 = torch.from_numpy(hip_keep_scale(seed, salts[k][0], pdrop, B * C)).view(B, C).double() if pdrop > 0 else 1.0
                keep3 = torch.from_numpy(hip_keep_scale(seed, salts[k][1], pdrop, B * C)).view(B, C).double() if pdrop > 0 else 1.0
                h2 = rc[k][7](rc[k][5](zr[k].view(B, C, 1, 1)).view(B, C) * keep2)
                y = rm[k][0](torch.cat((h2, sr[:, 2:2 + S]), 1))
                h3 = rm[k][3](rm[k][1](y) * keep3)
                outs.append(rm[k][4](h3)); taps_r += [h2, h3]
            torch.autograd.backward(outs, [t.double() for t in gw])
            # HIP
            dc, dm = make(torch.float32)
            dc, dm = dc.to(device).train(train), dm.to(device).train(train)
            zd = [_leaf(t, device) for t in z0]
            sd = _leaf(wide, device)
            ops.manual_seed(seed, device)
            ops.begin_step(device)
            taps = []
            ws = ops.gate_head(zd, [sd[:, 2:2 + S]] * n, list(dc), list(dm), train, drop_p=pdrop, salts=salts, taps=taps)
            torch.autograd.backward(ws, [t.to(device) for t in gw])
            for k in range(n):
                assert_close(ws[k], outs[k], "%s gate %d" % (what, k), rel=3e-5)
                assert_close(taps[2 * k], taps_r[2 * k], "%s tap2 %d" % (what, k), rel=3e-5)
                assert_close(taps[2 * k + 1], taps_r[2 * k + 1], "%s tap3 %d" % (what, k), rel=3e-5)
                assert_close(zd[k].grad, zr[k].grad, "%s dz %d" % (what, k), rel=5e-5, floor=max(1e-3, float(zr[k].grad.abs().max())))
            assert_close(sd.grad, sr.grad, what + " dstats", rel=5e-5, floor=max(1e-3, float(sr.grad.abs().max())))
            for mods_d, mods_r in ((dc, rc), (dm, rm)):
                for (kname, pa), (_, pb) in zip(mods_d.named_parameters(), mods_r.named_parameters()):
                    floor = max(1e-3, float(pb.grad.abs().max()))
                    if train and kname.endswith("0.weight"):      # Linear in front of a train-mode BatchNorm1d: remainder of cancelling sums
                        floor = max(floor, float(mods_r[int(kname.split(".")[0])][1].weight.grad.abs().max()))
                    if low_var and train and mods_d is dm and kname.endswith("3.weight"):
                        # the slope gradient behind the BatchNorm1d: one number, the sum of B * C cancelling terms (8.3e-3 here).  Measured on
                        # (5, 8, 10, 2), p = 0.25, path 1, against float64: stock float32 PyTorch on the CPU 3.922e-7, the kernel 2.047e-7 on the
                        # shim and 8.775e-7 on the MI355X, with the bound above at 4.167e-7; the bound is 4 x the stock error
                        floor = max(floor, 4.0 * 3.922e-7 / 5e-5)
                    assert_close(pa.grad, pb.grad, "%s grad %s" % (what, kname), rel=5e-5, floor=floor)
                for (kname, ba), (_, bb) in zip(mods_d.named_buffers(), mods_r.named_buffers()):
                    assert_close(ba.float(), bb.float(), "%s buffer %s" % (what, kname), rel=1e-5)


def check_tower_maps(device, shapes=((3, 10, (5, 5, 5, 5), 7, 8), (2, 20, (10, 16), 6, 6), (2, 12, (16, 5, 7), 3, 14), (3, 64, (32, 32, 32, 32), 5, 12), (2, 32, (16, 16, 16, 16), 5, 8)),
                     replay=False, low_var=False):
    """ops.tower_maps (pointwise maps + BatchNorm2d + PReLU as one operator; backward: cg_norm_act_bwd_reduce_many + cg_pointwise_maps_bwd
    undoing BatchNorm / PReLU on load) against stock PyTorch in fp64: outputs, dx, every dW / dgamma / dbeta / dalpha, running statistics,
    train and eval mode.  shapes: (B, Cin, (M_i), T, V).  replay: the reference takes the PReLU branches of the HIP run (BranchLog; for
    tensors of millions of elements).  low_var: rows 0 and 1 of every map scaled so that its BatchNorm channels see LOW_VAR_BATCH."""
    g = _gen(83)
    for (B, C, Ms, T, V) in shapes:
        for train in (True, False):
            def make(dt):
                gg = _gen(500 + C)
                mods = []
                for k, M in enumerate(Ms):
                    # residual-map form (conv bias, no PReLU: nn.Identity stands in) on the second map of the shapes with an even Cin
                    plain = k == 1 and C % 2 == 0
                    conv, bn, pr = nn.Conv2d(C, M, 1, bias=plain), nn.BatchNorm2d(M), (nn.Identity() if plain else nn.PReLU())
                    with torch.no_grad():
                        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gg) * 0.4)
                        if plain:
                            conv.bias.copy_(0.3 * torch.randn(M, generator=gg))
                        bn.weight.copy_(1 + 0.3 * torch.randn(M, generator=gg)); bn.bias.copy_(0.3 * torch.randn(M, generator=gg))
                        bn.running_mean.copy_(0.2 * torch.randn(M, generator=gg)); bn.running_var.copy_(0.5 + torch.rand(M, generator=gg))
                        if not plain:
                            pr.weight.fill_(0.1 + 0.1 * k)
                    if low_var:
                        _low_var_rows(conv.weight, F.conv2d(x0.double(), conv.weight.detach().double()), conv.bias if plain else None)
                        _low_var_running(bn)
                    mods.append(nn.Sequential(conv, bn, pr))
                return nn.ModuleList(mods).to(dt)
            x0 = 0.3 + _rand(g, B, C, T, V)
            gs = [_rand(g, B, M, T, V) for M in Ms]
            what = "tower_maps%s B%d C%d M%s T%d V%d %s" % (" low variance" if low_var else "", B, C, Ms, T, V, "train" if train else "eval")
            net = make(torch.float32).to(device).train(train)
            xd = _leaf(x0, device)
            ops.begin_step(device)
            hd = ops.tower_maps(xd, [m[0].weight.view(m[0].out_channels, C) for m in net], [m[1] for m in net],
                                [m[2] if isinstance(m[2], nn.PReLU) else None for m in net], train, biases=[m[0].bias for m in net])
            torch.autograd.backward(hd, [t.to(device) for t in gs])
            ref = make(torch.float64).train(train)
            xr = _leaf(x0.double(), "cpu")
            log = BranchLog()
            hr = [log.prelu(m[1](m[0](xr)), m[2].weight, h) if (replay and isinstance(m[2], nn.PReLU)) else m(xr) for m, h in zip(ref, hd)]
            torch.autograd.backward(hr, [t.double() for t in gs], retain_graph=replay)
            log.settle(what)
            for a, b in zip(hd, hr):
                assert_close(a, b, what + " output", rel=2e-5)
            names, got, leaves, floors = ["dx"], [xd.grad], [xr], [max(1e-3, float(xr.grad.abs().max()))]
            for (k, pa), (_, pb) in zip(net.named_parameters(), ref.named_parameters()):
                floor = max(1e-3, float(pb.grad.abs().max()))
                if train and (k.endswith("0.weight") or k.endswith("0.bias")):           # in front of a train-mode BatchNorm: the remainder of cancelling sums
                    floor = max(floor, float(ref[int(k.split(".")[0])][1].weight.grad.abs().max()))
                if low_var and train and k.endswith("0.bias"):
                    # analytically zero, and its cancelling sums carry the 1 / sqrt(var + eps) ~ 950 of a channel of variance 0.1 eps.  Measured
                    # on (3, 10, (5, 5, 5, 5), 7, 8) against float64: stock float32 PyTorch on the CPU 9.766e-4, the kernel 1.709e-3 (shim) with
                    # the bound above at 6.327e-4; the bound is 4 x the stock error, the factor of the kinematics checks
                    floor = max(floor, 4.0 * 9.766e-4 / 5e-5)
                names.append(k); got.append(pa.grad); leaves.append(pb); floors.append(floor)
            assert_grads_at_kinks(got, [t.grad for t in leaves], floors, names, what, log if replay else None, leaves)
            for (k, ba), (_, bb) in zip(net.named_buffers(), ref.named_buffers()):
                assert_close(ba.float(), bb.float(), "%s buffer %s" % (what, k), rel=1e-5)


def check_tower_collapse(device, shapes=((3, 10, (8, 8, 8, 8), 6, 8, 5), (2, 64, (32, 32, 32, 32), 50, 22, 32), (3, 16, (8, 8, 8, 8), 10, 18, 20), (2, 12, (16, 12), 5, 6, 7)),
                         replay=False, low_var=False):
    """The first tower level DEFERRED into its collapsing convolutions (`ops.tower_maps(defer=True)` + `ops.collapse_rows / collapse_cols`
    with `transform`: BatchNorm2d + PReLU applied on load, the activated maps never stored) against stock PyTorch in fp64: collapsed outputs,
    their channel sums, dx, every gradient (map weights, BatchNorm, PReLU slope, collapsing weights), running statistics; train and eval.
    Maps alternate between the frame-collapsing (T,1) and the joint-collapsing (1,V) convolution.  shapes: (B, Cin, (M_i), T, V, O).
    replay: the reference takes the PReLU branches of the HIP run (BranchLog; the activated maps are written out as branch records then).
    low_var: as in check_tower_maps - here the BatchNorm is the deferred transform of the collapsing kernels."""
    g = _gen(89)
    for (B, C, Ms, T, V, O) in shapes:
        for train in (True, False):
            def make(dt):
                gg = _gen(700 + C)
                mods = []
                for k, M in enumerate(Ms):
                    conv, bn, pr = nn.Conv2d(C, M, 1, bias=False), nn.BatchNorm2d(M), nn.PReLU()
                    col = nn.Conv2d(M, O, (T, 1) if k % 2 == 0 else (1, V), bias=False)
                    with torch.no_grad():
                        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gg) * 0.4)
                        col.weight.copy_(torch.randn(col.weight.shape, generator=gg) * 0.2)
                        bn.weight.copy_(1 + 0.3 * torch.randn(M, generator=gg)); bn.bias.copy_(0.3 * torch.randn(M, generator=gg))
                        bn.running_mean.copy_(0.2 * torch.randn(M, generator=gg)); bn.running_var.copy_(0.5 + torch.rand(M, generator=gg))
                        pr.weight.fill_(0.1 + 0.1 * k)
                    if low_var:
                        _low_var_rows(conv.weight, F.conv2d(x0.double(), conv.weight.detach().double()))
                        _low_var_running(bn)
                    mods.append(nn.Sequential(conv, bn, pr, col))
                return nn.ModuleList(mods).to(dt)
            x0 = 0.3 + _rand(g, B, C, T, V)
            gs = [_rand(g, B, O, 1, V) if k % 2 == 0 else _rand(g, B, O, T, 1) for k in range(len(Ms))]
            what = "tower_collapse%s B%d C%d M%s T%d V%d O%d %s" % (" low variance" if low_var else "", B, C, Ms, T, V, O, "train" if train else "eval")
            net = make(torch.float32).to(device).train(train)
            xd = _leaf(x0, device)
            ops.begin_step(device)
            ys, trs = ops.tower_maps(xd, [m[0].weight.view(m[0].out_channels, C) for m in net], [m[1] for m in net], [m[2] for m in net], train, defer=True)
            outs = []
            for k, m in enumerate(net):
                if replay:
                    trs[k]["want_tap"] = True
                w = m[3].weight.view(O, m[3].in_channels, -1)
                if k % 2 == 0:
                    assert ops.collapse_rows_ok(ys[k], w)
                    y, st = ops.collapse_rows(ys[k], w, want_stats=True, transform=trs[k])
                    outs.append((y.unsqueeze(2), st))
                else:
                    assert ops.collapse_cols_ok(ys[k], w)
                    y, st = ops.collapse_cols(ys[k], w, want_stats=True, transform=trs[k])
                    outs.append((y.unsqueeze(3), st))
            torch.autograd.backward([o for o, _ in outs], [t.to(device) for t in gs])
            ref = make(torch.float64).train(train)
            xr = _leaf(x0.double(), "cpu")
            log = BranchLog()
            yr = [m[3](log.prelu(m[1](m[0](xr)), m[2].weight, tr["tap"])) if replay else m(xr) for m, tr in zip(ref, trs)]
            torch.autograd.backward(yr, [t.double() for t in gs], retain_graph=replay)
            log.settle(what)
            for (a, st), b in zip(outs, yr):
                assert_close(a, b, what + " output", rel=3e-5)
                sums = _chan_sums(st).double().cpu().view(-1, 2)
                bb = b.detach()
                assert_close(sums[:, 0], bb.sum((0, 2, 3)), what + " sums", rel=1e-4, floor=max(1.0, float(bb.abs().sum((0, 2, 3)).max())))
            names, got, leaves, floors = ["dx"], [xd.grad], [xr], [max(1e-3, float(xr.grad.abs().max()))]
            for (k, pa), (_, pb) in zip(net.named_parameters(), ref.named_parameters()):
                floor = max(1e-3, float(pb.grad.abs().max()))
                if train and k.endswith("0.weight"):
                    floor = max(floor, float(ref[int(k.split(".")[0])][1].weight.grad.abs().max()))
                names.append(k); got.append(pa.grad); leaves.append(pb); floors.append(floor)
            assert_grads_at_kinks(got, [t.grad for t in leaves], floors, names, what, log if replay else None, leaves)
            for (k, ba), (_, bb) in zip(net.named_buffers(), ref.named_buffers()):
                assert_close(ba.float(), bb.float(), "%s buffer %s" % (what, k), rel=1e-5)


def check_block_input(device, shapes=((3, 5, 4, 6, 3), (2, 10, 10, 22, 7), (4, 64, 5, 22, 8), (2, 6, 5, 5, 2), (3, 3, 22, 25, 4)), low_var=False):
    """ops.block_input (csrc/block_input.hip) against stock PyTorch BatchNorm2d + the oracle's block statistics (CISTGCN.py:360-379):
    the aliases of xn, the statistics, running statistics; backward with a different gradient on every alias and on both statistics
    outputs: dx, dgamma, dbeta.  Train and eval mode, with and without channel sums handed over by the producer, plane sizes of
    16-, 8- and 4-byte alignment.  shapes: (B, C, T, V, n aliases).  low_var: channels 0 and 1 of x have the variances LOW_VAR_BATCH."""
    g = _gen(71)
    for (B, C, T, V, n) in shapes:
        for train in (True, False):
            for given_stats in ((False, True) if train else (False,)):
                def make(dt=torch.float32):
                    gg = _gen(400 + C)
                    bn = nn.BatchNorm2d(C)
                    with torch.no_grad():
                        bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=gg)); bn.bias.copy_(0.3 * torch.randn(C, generator=gg))
                        bn.running_mean.copy_(0.2 * torch.randn(C, generator=gg)); bn.running_var.copy_(0.5 + torch.rand(C, generator=gg))
                    if low_var:
                        _low_var_running(bn)
                    return bn.to(dt)
                x0 = 0.7 + 2.0 * _rand(g, B, C, T, V)
                if low_var:
                    x0 = _low_var_input(x0)
                gxs = [_rand(g, B, C, T, V) if i != 1 else None for i in range(n)]          # one consumer without a gradient
                gst = [_rand(g, B, 2 + 2 * T), _rand(g, B, 7 + 2 * T)[:, 3:5 + 2 * T]]         # the second one: a column slice (the gate inputs' gradient)
                what = "block_input%s B%d C%d T%d V%d %s%s" % (" low variance" if low_var else "", B, C, T, V, "train" if train else "eval", " (sums given)" if given_stats else "")
                # reference in fp64
                ref = make(torch.float64).train(train)
                xr = _leaf(x0.double(), "cpu")
                xnr = ref(xr)
                sr = O.CISTGCN.block_stats(xnr)
                torch.autograd.backward([xnr, sr], [sum(t.double() for t in gxs if t is not None), (gst[0] + gst[1]).double()])
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
                assert_close(xd.grad, xr.grad, what + " dx", rel=5e-5, floor=max(1e-3, float(xr.grad.abs().max())))
                assert_close(bn.weight.grad, ref.weight.grad, what + " dgamma", rel=5e-5)
                assert_close(bn.bias.grad, ref.bias.grad, what + " dbeta", rel=5e-5)
                for (k, ba), (_, bb) in zip(bn.named_buffers(), ref.named_buffers()):
                    assert_close(ba.float(), bb.float(), "%s buffer %s" % (what, k), rel=1e-5)
    # only the statistics reach the loss / only one alias does
    bn = nn.BatchNorm2d(6).to(device).train()
    x0, gx = _rand(g, 3, 6, 4, 6), _rand(g, 3, 6, 4, 6)
    for only in ("stats", "alias"):
        ref = nn.BatchNorm2d(6).double().train()
        xr = _leaf(x0.double(), "cpu")
        xnr = ref(xr)
        if only == "stats":
            O.CISTGCN.block_stats(xnr).sum().backward()
        else:
            xnr.backward(gx.double())
        xd = _leaf(x0, device)
        ops.begin_step(device)
        xs, (sa, sb) = ops.block_input(xd, bn, True, 3)
        if only == "stats":
            sa.backward(torch.ones_like(sa))
        else:
            xs[2].backward(gx.to(device))
        assert_close(xd.grad, xr.grad, "block_input dx (%s only)" % only, rel=5e-5, floor=max(1e-3, float(xr.grad.abs().max())))


def check_context_heads(device, shapes=((3, 5, 12, 7), (4, 25, 66, 64), (2, 3, 10, 33)), low_var=False):
    """ops.context_heads (csrc/context_heads.hip) against stock PyTorch modules Conv2d(1, C, 1) -> BatchNorm2d -> PReLU and the
    reference's reductions (CISTGCN.py:465, :467): outputs, the PReLU taps, input gradient, every parameter gradient, running
    statistics; train and eval mode.  shapes: (B, H, W, C).  low_var: w[0] and w[1] of both heads small enough for the variances
    LOW_VAR_BATCH of w[c] * x."""
    from cistgcn_amd.models.CISTGCN.CISTGCN import Stage, _conv
    g = _gen(61)
    for (B, H, W, C) in shapes:
        for train in (True, False):
            def make():
                gg = _gen(300 + B + C)
                heads = []
                for k in range(2):
                    hd = Stage(s0=_conv(1, C, 1), s1=nn.BatchNorm2d(C), s2=nn.PReLU())
                    with torch.no_grad():
                        hd[0].weight.copy_(torch.randn(hd[0].weight.shape, generator=gg) * 0.7)
                        hd[1].weight.copy_(1 + 0.3 * torch.randn(C, generator=gg)); hd[1].bias.copy_(0.3 * torch.randn(C, generator=gg))
                        hd[1].running_mean.copy_(0.2 * torch.randn(C, generator=gg)); hd[1].running_var.copy_(0.5 + torch.rand(C, generator=gg))
                        hd[2].weight.fill_(0.15 + 0.2 * k)
                    if low_var:
                        _low_var_rows(hd[0].weight, F.conv2d(x0.double(), hd[0].weight.detach().double()))
                        _low_var_running(hd[1])
                    heads.append(hd)
                return nn.ModuleList(heads)
            x0 = 1.5 + 3.0 * _rand(g, B, 1, H, W)
            g0, g1 = _rand(g, B, C), _rand(g, B, C)
            what = "context_heads%s B%d H%d W%d C%d %s" % (" low variance" if low_var else "", B, H, W, C, "train" if train else "eval")
            # stock PyTorch in fp64: the weight of a convolution in front of a train-mode BatchNorm has a gradient that is the small
            # remainder of cancelling sums; the stock fp32 path is 1e-4 .. 3e-4 off its own fp64 run there (B16 H25 W75), the kernel
            # (f64 channel sums, closed form) 2e-6 .. 3e-5
            ref = make().double().train(train)
            xr = _leaf(x0.double(), "cpu")
            z0 = ref[0][2](ref[0][1](ref[0][0](xr)))
            z1 = ref[1][2](ref[1][1](ref[1][0](xr)))
            r0, r1 = z0.max(-1)[0].max(-1)[0], z1.mean((2, 3))
            torch.autograd.backward([r0, r1], [g0.double(), g1.double()])
            # HIP
            net = make().to(device).train(train)
            xd = _leaf(x0, device)
            ops.begin_step(device)
            taps = []
            y0, y1 = ops.context_heads(xd, net[0], net[1], train, taps=taps)
            torch.autograd.backward([y0, y1], [g0.to(device), g1.to(device)])
            assert_close(y0, r0, what + " max", rel=2e-5)
            assert_close(y1, r1, what + " mean", rel=2e-5)
            assert_close(taps[0], z0, what + " tap 0", rel=2e-5)
            assert_close(taps[1], z1, what + " tap 1", rel=2e-5)
            assert_close(xd.grad, xr.grad, what + " dx", rel=5e-5, floor=max(1e-3, float(xr.grad.abs().max())))
            for (k, pa), (_, pb) in zip(net.named_parameters(), ref.named_parameters()):
                floor = max(1e-3, float(pb.grad.abs().max()))
                if train and k.endswith("0.weight"):
                    # a weight in front of a train-mode BatchNorm: its gradient is what is left (~eps / var) of cancelling terms of the size
                    # of the BatchNorm weight's gradient - stock fp32 PyTorch is itself 1e-6 .. 3e-6 off its fp64 run here
                    floor = max(floor, float(ref[int(k[0])][1].weight.grad.abs().max()))
                assert_close(pa.grad, pb.grad, "%s grad %s" % (what, k), rel=5e-5, floor=floor)
            for (k, ba), (_, bb) in zip(net.named_buffers(), ref.named_buffers()):
                assert_close(ba.float(), bb.float(), "%s buffer %s" % (what, k), rel=1e-5)
            # a head that does not reach the loss
            net.zero_grad()
            xd2 = _leaf(x0, device)
            ops.begin_step(device)
            y0, y1 = ops.context_heads(xd2, net[0], net[1], False)
            y1.backward(g1.to(device))
            ref.eval(); ref.zero_grad()
            xr2 = _leaf(x0.double(), "cpu")
            ref[1][2](ref[1][1](ref[1][0](xr2))).mean((2, 3)).backward(g1.double())
            assert_close(xd2.grad, xr2.grad, what + " dx (mean head only)", rel=5e-5, floor=max(1e-3, float(xr2.grad.abs().max())))


def check_pointwise_maps(device, shapes=((3, 10, (5, 5, 5, 5), 7, 8), (2, 64, (32, 32, 32, 32), 5, 12), (2, 20, (10, 33), 6, 6),
                                          (3, 10, (64, 64), 5, 8), (2, 64, (10, 10, 10), 6, 6), (2, 1, (64, 64), 25, 66), (3, 32, (16, 16, 16, 16), 5, 10), (3, 100, (25,), 10, 22), (2, 128, (3,), 6, 6), (2, 64, (16, 16, 16, 16), 4, 6))):      # P % 4 == 2: (25, 66) and (5, 10); the last two: more than 64 input channels (FPN compress)
    """ops.pointwise_maps (csrc/tower_maps.hip) against one generic contraction per map: outputs, f64 channel sums, the summed
    input gradient, every weight gradient; every other shape with biases on all maps but the last (the residual maps of a block,
    nn.Conv2d(cin, cout, 1) with its default bias) and their gradients.  shapes: (B, Cin, (M_i), T, V)."""
    g = _gen(53)
    for n_shape, (B, C, Ms, T, V) in enumerate(shapes):
        x0 = _rand(g, B, C, T, V)
        w0 = [0.3 * _rand(g, M, C) for M in Ms]
        b0 = [(_rand(g, M) if (n_shape % 2 == 1 and (k + 1 < len(Ms) or len(Ms) == 1)) else None) for k, M in enumerate(Ms)]
        gy = [_rand(g, B, M, T, V).to(device) for M in Ms]
        res = []
        for fused in (True, False):
            x = _leaf(x0, device)
            ws = [_leaf(w, device) for w in w0]
            bs = [None if b is None else _leaf(b, device) for b in b0]
            ops.begin_step(device)
            if fused:
                assert ops.pointwise_maps_ok(x, ws)
                outs = ops.pointwise_maps(x, ws, want_stats=True, biases=bs)
            else:
                outs = [ops.contract_stats("oc,bchw->bohw", w, x, b, "o" if b is not None else None) for w, b in zip(ws, bs)]
            ys = [o[0] for o in outs]
            sums = [_chan_sums(o[1]) for o in outs]
            torch.autograd.backward(ys, gy)
            res.append(([y.detach() for y in ys], sums, [x.grad] + [w.grad for w in ws] + [b.grad for b in bs if b is not None]))
        what = "pointwise_maps B%d C%d M%s T%d V%d%s" % (B, C, Ms, T, V, " +bias" if any(b is not None for b in b0) else "")
        for k in range(len(Ms)):
            assert_close(res[0][0][k], res[1][0][k], "%s y[%d]" % (what, k), rel=2e-5)
            assert_close(res[0][1][k], res[1][1][k], "%s sums[%d]" % (what, k), rel=1e-5)
        assert len(res[0][2]) == len(res[1][2])
        for k, (a, b) in enumerate(zip(res[0][2], res[1][2])):
            assert_close(a, b, "%s grad[%d]" % (what, k), rel=5e-5, floor=max(1e-3, float(b.abs().max())))


def check_collapse_rows(device, shapes=((3, 6, 4, 7, 5), (2, 32, 50, 22, 32), (5, 64, 10, 22, 64), (2, 10, 6, 25, 20), (3, 12, 5, 18, 40))):      # O = 5 .. 64: one to four 16-row output tiles; K = 24, 60: a last group of fewer than 16 rows
    """ops.collapse_rows (csrc/collapse_rows.hip) against the generic contraction: output, f64 channel sums, both gradients.
    shapes: (B, C, T, V, O)."""
    g = _gen(61)
    for (B, C, T, V, O) in shapes:
        x0, w0 = _rand(g, B, C, T, V), 0.2 * _rand(g, O, C, T)
        gy = _rand(g, B, O, V).to(device)
        res = []
        for fused in (True, False):
            x, w = _leaf(x0, device), _leaf(w0, device)
            ops.begin_step(device)
            if fused:
                assert ops.collapse_rows_ok(x, w)
                y, st = ops.collapse_rows(x, w, want_stats=True)
            else:
                y, st = ops.contract_stats("och,bchw->bow", w, x)
            y.backward(gy)
            res.append((y.detach(), _chan_sums(st) if st is not None else None, x.grad, w.grad))
        what = "collapse_rows B%d C%d T%d V%d O%d" % (B, C, T, V, O)
        assert_close(res[0][0], res[1][0], what + " y", rel=2e-5)
        if res[1][1] is not None:
            assert_close(res[0][1], res[1][1], what + " sums", rel=1e-5)
        assert_close(res[0][2], res[1][2], what + " dx", rel=5e-5, floor=max(1e-3, float(res[1][2].abs().max())))
        assert_close(res[0][3], res[1][3], what + " dW", rel=5e-5, floor=max(1e-3, float(res[1][3].abs().max())))



def check_collapse_cols(device, shapes=((3, 6, 4, 8, 5), (2, 32, 50, 22, 32), (4, 64, 10, 22, 64), (2, 10, 6, 22, 20), (3, 12, 25, 18, 40), (2, 32, 50, 25, 32), (3, 5, 3, 4, 3))):
    """ops.collapse_cols (joint-collapsing convolution, csrc/collapse_rows.hip) against the generic contraction: output, f64 channel sums,
    both gradients.  shapes: (B, C, T, V, O): one to four 16-row output tiles, 1 / 2 / 4 tiles of frames (T = 3 .. 50), K = C * V with and
    without a partial last group, steps that cross from one channel to the next (V = 22, 18, 25 are no multiples of 4)."""
    g = _gen(67)
    for (B, C, T, V, O) in shapes:
        x0, w0 = _rand(g, B, C, T, V), 0.2 * _rand(g, O, C, V)
        gy = _rand(g, B, O, T).to(device)
        res = []
        for fused in (True, False):
            x, w = _leaf(x0, device), _leaf(w0, device)
            ops.begin_step(device)
            if fused:
                assert ops.collapse_cols_ok(x, w)
                y, st = ops.collapse_cols(x, w, want_stats=True)
            else:
                y, st = ops.contract_stats("ocw,bchw->boh", w, x)
            y.backward(gy)
            res.append((y.detach(), _chan_sums(st) if st is not None else None, x.grad, w.grad))
        what = "collapse_cols B%d C%d T%d V%d O%d" % (B, C, T, V, O)
        assert_close(res[0][0], res[1][0], what + " y", rel=2e-5)
        if res[1][1] is not None:
            assert_close(res[0][1], res[1][1], what + " sums", rel=1e-5)
        assert_close(res[0][2], res[1][2], what + " dx", rel=5e-5, floor=max(1e-3, float(res[1][2].abs().max())))
        assert_close(res[0][3], res[1][3], what + " dW", rel=5e-5, floor=max(1e-3, float(res[1][3].abs().max())))

def check_flat_adam(device):
    """cg_adam_flat + FlatGrads against torch.optim.Adam with the reference's settings (weight decay, no amsgrad)."""
    from cistgcn_amd.runtime import FlatAdam
    torch.manual_seed(3)
    ref = nn.Sequential(nn.Linear(13, 7), nn.BatchNorm1d(7), nn.Linear(7, 300), nn.PReLU())
    dev = nn.Sequential(nn.Linear(13, 7), nn.BatchNorm1d(7), nn.Linear(7, 300), nn.PReLU())
    dev.load_state_dict(ref.state_dict())
    dev.to(device)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-4)
    opt_dev = FlatAdam(dev, lr=1e-2, weight_decay=1e-4)
    g = _gen(21)
    for step in range(4):
        for pr, pd in zip(ref.parameters(), dev.parameters()):
            gr = torch.randn(pr.shape, generator=g)
            pr.grad = gr.clone()
            pd.grad = gr.clone().to(device)
        opt_ref.step()
        opt_dev.step()
        for (k, pr), pd in zip(ref.named_parameters(), dev.parameters()):
            assert_close(pd, pr, "adam step %d %s" % (step, k), rel=1e-5)
    # the optimizer is driven by stock schedulers and by writes to param_groups (the reference's warm-up helper does that)
    sch_ref = torch.optim.lr_scheduler.StepLR(opt_ref, step_size=2, gamma=0.5)
    sch_dev = torch.optim.lr_scheduler.StepLR(opt_dev, step_size=2, gamma=0.5)
    for step in range(5):
        if step == 3:
            for o in (opt_ref, opt_dev):
                for grp in o.param_groups:
                    grp["lr"] = grp["lr"] * 3.0
        for pr, pd in zip(ref.parameters(), dev.parameters()):
            gr = torch.randn(pr.shape, generator=g)
            pr.grad = gr.clone()
            pd.grad = gr.clone().to(device)
        opt_ref.step(); opt_dev.step()
        sch_ref.step(); sch_dev.step()
        assert abs(opt_ref.param_groups[0]["lr"] - opt_dev.param_groups[0]["lr"]) < 1e-12
        for (k, pr), pd in zip(ref.named_parameters(), dev.parameters()):
            assert_close(pd, pr, "adam scheduled step %d %s" % (step, k), rel=2e-5)
    # checkpoint round trip of the optimizer state
    state = opt_dev.state_dict()
    dev_b = nn.Sequential(nn.Linear(13, 7), nn.BatchNorm1d(7), nn.Linear(7, 300), nn.PReLU())
    dev_b.load_state_dict(dev.state_dict()); dev_b.to(device)
    opt_b = FlatAdam(dev_b, lr=1.0)
    opt_b.load_state_dict(state)
    assert opt_b.step_count == opt_dev.step_count and abs(opt_b.lr - opt_dev.lr) < 1e-12
    for pd, pb in zip(dev.parameters(), dev_b.parameters()):
        gr = torch.randn(pd.shape, generator=g).to(device)
        pd.grad, pb.grad = gr.clone(), gr.clone()
    opt_dev.step(); opt_b.step()
    for pd, pb in zip(dev.parameters(), dev_b.parameters()):
        assert_close(pb, pd.detach().cpu(), "adam resumed", rel=1e-6)
    # clip_grad_value_ + gradient pre-scale (data-parallel mean)
    ref2, dev2 = nn.Linear(5, 4), nn.Linear(5, 4)
    dev2.load_state_dict(ref2.state_dict()); dev2.to(device)
    o_ref, o_dev = torch.optim.Adam(ref2.parameters(), lr=1e-2), FlatAdam(dev2, lr=1e-2, clip_value=0.5)
    for pr, pd in zip(ref2.parameters(), dev2.parameters()):
        gr = 3 * torch.randn(pr.shape, generator=g)
        pr.grad = gr.clone() / 2
        pd.grad = gr.clone().to(device)
    torch.nn.utils.clip_grad_value_(ref2.parameters(), 0.5)
    o_ref.step(); o_dev.step(grad_scale=0.5)
    for pr, pd in zip(ref2.parameters(), dev2.parameters()):
        assert_close(pd, pr, "adam clip/scale", rel=1e-5)
