"""Checks of the input attacks (cistgcn_amd/environment/attacks.py, ops.attack_step, ops.mpjpe_per_sample), shared by the CPU suite
(tests/test_attacks.py, kernels under the HIP shim) and the MI355X suite (tests/test_gpu_attacks.py).  Every check takes the device.

Two references:
* `ref_step` below: a stock-PyTorch restatement of one attack iteration, the operator-level reference on synthetic data;
* tests/golden/eval_attack_h36m_c8_t10_v22.npz: what the real reference's attack classes did on the `h36m_c8_t10_v22` model
  (tools/gen_golden_attacks.py), iteration by iteration, with fp64 gradients at the iterates the sign tests use.
"""
import os

import numpy as np
import torch

from cistgcn_amd import ops
from cistgcn_amd.environment import attacks
from helpers import GOLDEN_DIR, assert_close, load_case, state_of

CASE = "h36m_c8_t10_v22"
PATIENCE = 5
CONFIGS = {      # as tools/gen_golden_attacks.py ran them
    "F": (attacks.FGSM, dict(epsilon=0.01)),
    "I1": (attacks.IFGSM, dict(epsilon=0.01, iterations=10)),
    "I2": (attacks.IFGSM, dict(epsilon=0.2, iterations=12, frames=[0, 3, 9], joints=[1, 2, 5, 21])),
    "M": (attacks.MIFGSM, dict(epsilon=0.05, iterations=12, mu=0.5)),
    "I3": (attacks.IFGSM, dict(epsilon=1.0, iterations=14)),
}
_fixture = []


def fixture():
    if not _fixture:
        z = np.load(os.path.join(GOLDEN_DIR, "eval_attack_%s.npz" % CASE))
        _fixture.append({k: z[k] for k in z.files})
    return _fixture[0]


# ---------------------------------------------------------------------------------------------------------
# the restatement: one iteration in stock PyTorch, fp32, on the CPU
# ---------------------------------------------------------------------------------------------------------
class RefState:
    def __init__(self, B):
        self.B = B
        self.best = torch.zeros(B)
        self.stall = torch.zeros(B, dtype=torch.int32)
        self.active = torch.ones(B, dtype=torch.int32)
        self.w = torch.ones(B) / B
        self.queries = torch.zeros(B, dtype=torch.int32)
        self.n_active = torch.tensor([B], dtype=torch.int32)


def ref_step(mode, x_i, x0, grad, epsilon, iterations=1, mu=0.0, mask=None, g=None, loss=None, st=None):
    """Returns (x_adv, g); updates `st` in place.  Every tensor expression is evaluated in fp32 in the order the attack's definition
    gives: eps_b = epsilon * |max y - min y|, alpha = eps_b / iterations, x_adv = x_i + mask * (alpha * d)."""
    B = x_i.shape[0]
    fgsm = mode == "fgsm"
    act = torch.ones(B, dtype=torch.bool) if fgsm else st.active.bool()
    if not fgsm and not bool(act.any()):
        return x_i.clone(), (None if g is None else g.clone())          # every sample frozen: the loop has ended
    y = x_i[..., 1].reshape(B, -1)
    eps = (epsilon * (y.max(1)[0] - y.min(1)[0]).abs())[:, None, None, None]
    alpha = eps if fgsm else eps / iterations
    move = act.clone()
    if mode == "mifgsm":
        l1 = grad.abs().reshape(B, -1).sum(1)
        move &= l1 > 0
        g_new = mu * g + grad / l1[:, None, None, None]
        g = torch.where(move[:, None, None, None], g_new, g)
        d = torch.sign(g)
    else:
        d = torch.sign(grad)
    m = torch.ones(x_i.shape[1:3]) if mask is None else mask
    r = m[None, :, :, None] * (alpha * d)
    x_adv = torch.where(move[:, None, None, None], x_i + r, x_i)
    if fgsm:
        return x_adv, g
    far = (x_adv - x0).abs().reshape(B, -1).max(1)[0] > eps.flatten()
    out = (x_adv < x0 - eps) | (x_adv >= x0 + eps)
    x_adv = torch.where(far[:, None, None, None] & out, x0, x_adv)
    st.queries += act.int()
    improved = act & (loss > st.best)
    st.best = torch.where(improved, loss, st.best)
    st.stall += (act & ~improved).int()
    st.active = (act & (st.stall < PATIENCE)).int()
    st.w = st.active.float() * (torch.ones(B) / B)
    st.n_active = st.active.sum().reshape(1).int()
    return x_adv, g


def dev_state(st, device):
    s = ops.AttackState(st.B, device)
    copy_state(s, st)
    return s


def copy_state(dst, src):
    """reference state -> a fresh device state at step 0; a sample that is already frozen froze before step 0"""
    for k in ("best", "stall", "active", "w", "queries", "n_active"):
        getattr(dst, k).copy_(getattr(src, k))
    dst.steps.zero_()
    dst.frozen_at.copy_(torch.where(src.active.bool(), torch.tensor(2 ** 31 - 1, dtype=torch.int32), torch.tensor(-1, dtype=torch.int32)))


def assert_state_equal(s, st, what):
    for k in ("best", "stall", "active", "w", "queries", "n_active"):
        got, ref = getattr(s, k).cpu(), getattr(st, k)
        assert got.dtype == ref.dtype and torch.equal(got, ref), "%s: %s is %s, expected %s" % (what, k, got.tolist(), ref.tolist())


def run_step(device, mode, x_i, x0, grad, epsilon, iterations, mu, mask, g, loss, s):
    xd = x_i.clone().to(device)
    gd = None if g is None else g.clone().to(device)
    ops.attack_step(mode, xd, x0.to(device), grad.to(device), epsilon, iterations=iterations, mu=mu,
                    mask=None if mask is None else mask.to(device), g=gd, loss=None if loss is None else loss.to(device), state=s)
    return xd.cpu(), (None if gd is None else gd.cpu())


# ---------------------------------------------------------------------------------------------------------
# operator level
# ---------------------------------------------------------------------------------------------------------
MPJPE_SHAPES = [(1, 1, 2), (3, 25, 22), (5, 10, 25), (4, 25, 18)]


def check_mpjpe_per_sample(device, B, To, V):
    gen = torch.Generator().manual_seed(B * 1000 + To * 10 + V)
    pred = 50 + 350 * torch.randn(B, To, V, 3, generator=gen)
    tgt = pred + 20 * torch.randn(B, To, V, 3, generator=gen)
    tgt[0, 0, 0] = pred[0, 0, 0]                                     # a joint predicted exactly: norm 0, gradient 0
    w = torch.rand(B, generator=gen) + 0.1
    if B > 1:
        w[B // 2] = 0.0
    pd = pred.clone().to(device).requires_grad_(True)
    loss = ops.mpjpe_per_sample(pd, tgt.to(device))
    again = ops.mpjpe_per_sample(pd.detach(), tgt.to(device))
    assert torch.equal(loss.detach(), again), "per-sample MPJPE is not bit-reproducible"
    p64 = pred.double().requires_grad_(True)
    ref = torch.norm(p64 - tgt.double(), 2, dim=-1).mean((1, 2))
    assert loss.shape == (B,)
    err = float(((loss.detach().cpu().double() - ref.detach()).abs() / ref.detach().abs()).max())
    assert err <= 1e-6, "per-sample MPJPE: relative error %.3e" % err
    loss.backward(w.to(device))
    ref.backward(w.double())
    gref = p64.grad.clone()
    gref[0, 0, 0] = 0.0                                              # torch.norm's subgradient at 0 is 0 as well; stated, not assumed
    assert torch.equal(pd.grad[0, 0, 0].cpu(), torch.zeros(3)), "gradient at pred == target must be 0"
    assert_close(pd.grad, gref, "per-sample MPJPE gradient", rel=1e-5, floor=float(gref.abs().max()))
    if B > 1:
        assert float(pd.grad[B // 2].abs().max()) == 0.0, "a sample with weight 0 must get gradient 0"


STEP_SHAPES = [(1, 1, 2), (3, 10, 22), (2, 50, 25), (5, 7, 18)]
STEP_MODES = ["fgsm", "ifgsm", "mifgsm"]
STEP_MASKS = ["all", "joints", "frames", "both", "empty"]


def _mask(kind, T, V):
    if kind == "all":
        return None, None, None
    joints = list(range(0, V, 3)) if kind in ("joints", "both") else None
    frames = list(range(T - 1, -1, -2)) if kind in ("frames", "both") else None
    if kind == "empty":
        joints, frames = [], None
    return attacks.selection_mask(T, V, joints, frames), joints, frames


def synthetic(B, T, V, mode, mask, epsilon, seed):
    """x0, x_i, grad, g, state for one step: gradients with |g| >= 1e-3 except planted exact zeros; x_i displaced from x0 inside the
    box, plus - on the x / z coordinates, which leave the y extent and hence eps_b alone - one element above the box, one below it
    and, in a frozen sample or under a mask that holds it still, one exactly on the upper edge x0 + eps_b (reset by `>=`).
    Sample 1 is frozen and still gets the reset; the last sample of a batch of 3+ has y extent 0 (eps_b = 0); in MI-FGSM sample 0 of
    a batch of 3+ is active with an all-zero gradient."""
    gen = torch.Generator().manual_seed(seed)
    shape = (B, T, V, 3)
    x0 = 50 + 350 * torch.randn(shape, generator=gen)
    grad = (1e-3 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
    grad[torch.rand(shape, generator=gen) < 0.05] = 0.0              # sign(0) = 0
    st = RefState(B)
    if B > 1:
        st.active[1], st.w[1], st.stall[1], st.n_active[0] = 0, 0.0, PATIENCE, B - 1
        grad[1] = 0.0                                                # a frozen sample has no gradient
    if mode == "fgsm":
        return x0, x0.clone(), grad, None, st
    x_i = x0 + 0.3 * epsilon * 700 * (2 * torch.rand(shape, generator=gen) - 1)
    if B >= 3:
        x_i[B - 1, :, :, 1] = 123.25                                 # y extent 0
        if mode == "mifgsm":
            grad[0] = 0.0
    y = x_i[..., 1].reshape(B, -1)
    eps = epsilon * (y.max(1)[0] - y.min(1)[0]).abs()
    for b in range(B):
        x_i[b, 0, 0, 0] = x0[b, 0, 0, 0] + 1.7 * eps[b] + 1.0
        x_i[b, T - 1, V - 1, 2] = x0[b, T - 1, V - 1, 2] - 1.7 * eps[b] - 1.0
        still = (b == 1) or (mask is not None and float(mask[0, V - 1]) == 0.0)
        if still:
            x_i[b, 0, V - 1, 0] = x0[b, 0, V - 1, 0] + eps[b]       # exactly on the upper edge of the box
    g = None
    if mode == "mifgsm":
        n = T * V * 3
        g = (0.5 + torch.rand(shape, generator=gen)) / n * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
    return x0, x_i, grad, g, st


def check_attack_step_synthetic(device, shape, mode, mask_kind):
    B, T, V = shape
    epsilon, iterations, mu = 0.05, 7, 0.6
    mask, _, _ = _mask(mask_kind, T, V)
    x0, x_i, grad, g, st = synthetic(B, T, V, mode, mask, epsilon, seed=B * 100 + T + len(mode) + len(mask_kind))
    loss = torch.linspace(1.0, 2.0, B)
    s = dev_state(st, device)
    before = (x_i - x0).abs().reshape(B, -1).max(1)[0]
    xd, gd = run_step(device, mode, x_i, x0, grad, epsilon, iterations, mu, mask, g, None if mode == "fgsm" else loss, s)
    xr, gr = ref_step(mode, x_i, x0, grad, epsilon, iterations, mu, mask, g, loss, st)
    tol = 1e-6 * float(x0.abs().max())
    err = float((xd - xr).abs().max())
    assert err <= tol, "%s %s %s: x_adv differs from the restatement by %.3e (bound %.3e)" % (shape, mode, mask_kind, err, tol)
    if mode != "fgsm":
        assert_state_equal(s, st, "%s %s %s" % (shape, mode, mask_kind))
        # the planted elements were outside the box, so the reset has fired in every sample, the frozen one included
        assert bool(((xr - x0).abs().reshape(B, -1).max(1)[0] < before).all())
        assert float((xr[:, 0, 0, 0] - x0[:, 0, 0, 0]).abs().max()) == 0.0
    if mode == "mifgsm":
        gerr, gtol = float((gd - gr).abs().max()), 1e-6 * float(gr.abs().max())
        assert gerr <= gtol, "momentum differs by %.3e (bound %.3e)" % (gerr, gtol)
        if B >= 3:
            assert torch.equal(gd[0], g[0]) and torch.equal(gd[1], g[1]), "momentum of an all-zero-gradient / frozen sample must not change"
    if mask_kind == "empty" and mode == "fgsm":
        assert torch.equal(xd, x0)


def check_bookkeeping_script(device, mode="ifgsm"):
    """Scripted losses over 14 steps, patience 5, `best` starting at 0.  First script: sample 0 keeps improving (never frozen);
    sample 1 is flat (improves once, then stalls: frozen by step 5); sample 2 improves every other step and repeats in between
    ("equal is not improved": frozen by step 10); sample 3 starts at 0 and falls (never improves: frozen by step 4); sample 4 has a
    late improvement that clears nothing (the reference never resets the stall count: frozen by step 6).  Second script: every
    sample is frozen by step 5 and the eight steps after that must change nothing at all.  Every field is compared exactly after
    every step."""
    T, V, epsilon, iterations, mu = 2, 3, 0.01, 14, 0.5
    gen = torch.Generator().manual_seed(7)
    scripts = [
        ([[1.0 + k for k in range(14)], [1.0] * 14, [1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8], [0.0 - k for k in range(14)],
          [1, 1, 1, 5, 5, 5, 5, 9, 9, 9, 9, 9, 9, 9]], [None, 5, 10, 4, 6], [14, 6, 11, 5, 7]),
        ([[2.0] * 14, [0.0] * 14, [3.0 - k for k in range(14)]], [5, 4, 5], [6, 5, 6]),
    ]
    for script, frozen_by, queries in scripts:
        B = len(script)
        losses = torch.tensor(script, dtype=torch.float32).t().contiguous()      # (steps, B)
        x0 = 50 + 350 * torch.randn(B, T, V, 3, generator=gen)
        x, st = x0.clone(), RefState(B)
        g = torch.zeros_like(x0) if mode == "mifgsm" else None
        s = dev_state(st, device)
        seen = [None] * B
        for k in range(losses.shape[0]):
            grad = (1e-3 + torch.rand(x0.shape, generator=gen)) * (torch.randint(0, 2, x0.shape, generator=gen) * 2 - 1).float()
            over = not bool(st.active.any())
            xd, gd = run_step(device, mode, x, x0, grad, epsilon, iterations, mu, None, g, losses[k], s)
            xr, gr = ref_step(mode, x, x0, grad, epsilon, iterations, mu, None, g, losses[k], st)
            assert_state_equal(s, st, "script of %d samples, step %d" % (B, k))
            assert float((xd - xr).abs().max()) <= 1e-6 * float(x0.abs().max()), "step %d" % k
            if over:
                assert torch.equal(xd, x) and (g is None or torch.equal(gd, g)), "a step that starts with every sample frozen must change nothing"
            seen = [k if (f is None and not a) else f for f, a in zip(seen, st.active.tolist())]
            x, g = xr, gr
        assert seen == frozen_by and st.queries.tolist() == queries, (seen, st.queries.tolist())
        assert int(st.n_active) == sum(f is None for f in frozen_by)


# ---------------------------------------------------------------------------------------------------------
# against the real reference
# ---------------------------------------------------------------------------------------------------------
def teacher_forced_to(device, cid, upto=None):
    """Drive `ops.attack_step` through the recorded iterations [0, upto) of configuration `cid` with the recorded iterate, fp32 gradient
    and losses and the carried state; checks every step against the recording.  Returns (state, momentum) after the last step."""
    fx = fixture()
    cls, kw = CONFIGS[cid]
    att = cls(**kw)
    xs, grads, losses, actives = fx[cid + "/x"], fx[cid + "/grad"], fx[cid + "/loss"], fx[cid + "/active"]
    K = grads.shape[0] if upto is None else upto
    x0 = torch.from_numpy(xs[0]).to(device)
    s = ops.AttackState(x0.shape[0], device)
    mask, g = att.mask(x0), att.new_momentum(x0)
    tol = 1e-6 * float(np.abs(xs[0]).max())
    for k in range(K):
        x = torch.from_numpy(xs[k]).clone().to(device)          # stepped in place: never the fixture's own memory
        att.step(x, x0, torch.from_numpy(grads[k]).to(device), torch.from_numpy(losses[k]).to(device), s, mask, g)
        err = float(np.abs(x.cpu().numpy().astype(np.float64) - xs[k + 1]).max())
        assert err <= tol, "%s iteration %d: x_adv is %.3e from the reference's (bound %.3e)" % (cid, k, err, tol)
        assert s.active.cpu().tolist() == actives[k].astype(int).tolist(), "%s iteration %d: active %s, recorded %s" % (
            cid, k, s.active.cpu().tolist(), actives[k].astype(int).tolist())
        if g is not None:
            gr = fx[cid + "/g"][k]
            gerr, gtol = float(np.abs(g.cpu().numpy() - gr).max()), 1e-6 * float(np.abs(gr).max())
            assert gerr <= gtol, "%s iteration %d: momentum is %.3e from the reference's (bound %.3e)" % (cid, k, gerr, gtol)
    return att, s, g


def check_teacher_forced(device, cid):
    fx = fixture()
    _, s, _ = teacher_forced_to(device, cid)
    assert s.queries.cpu().tolist() == fx[cid + "/queries"].tolist(), (s.queries.cpu().tolist(), fx[cid + "/queries"].tolist())
    if cid == "I3":
        assert s.queries.cpu().tolist() == [7, 7, 8, 7] and int(s.n_active) == 0


_models = {}


def model_on(device):
    """The product model with the fixture's weights, eval mode (one per device for the whole session; the checks leave it unchanged)."""
    import checks
    key = str(device)
    if key not in _models:
        rec = load_case(CASE)
        C, T, V, _ = [int(v) for v in rec["meta"]]
        net, _ = checks.build_pair(C, T, V, device, state_of(rec))
        _models[key] = net.eval()
    rec = load_case(CASE)
    return _models[key], torch.from_numpy(rec["x"]).to(device), torch.from_numpy(rec["target"]).to(device)


def zone_of(cid, k):
    """(fp64 gradient, Z, share of elements within Z of zero) at recorded iterate k; the cap is asserted again from the fixture"""
    fx = fixture()
    ks = fx[cid + "/k64"].tolist()
    assert k in ks, "%s: iterate %d has no fp64 gradient in the fixture (has %s)" % (cid, k, ks)
    i = ks.index(k)
    g64, noise = fx[cid + "/grad64"][i], float(fx[cid + "/noise"][i])
    Z = float(fx["z_factor"]) * noise
    assert float(fx["z_factor"]) == 30.0 and float(fx["zone_cap"]) == 0.03
    started = fx[cid + "/started"][k]
    share = float((np.abs(g64[started]) <= Z).mean())
    assert share <= 0.03 and abs(share - float(fx[cid + "/zone_share"][i])) < 1e-12, "%s iterate %d: zone share %.4f" % (cid, k, share)
    return g64, Z, share


def sign_iterates():
    """k = 0 and the last usable recorded iterate of I1, M and I3 (the generator steps back from an iterate whose near-zero zone is over
    the cap or whose reference gradient is not finite: I3 at epsilon 1.0 overflows the reference's fp32 forward from iteration 2 on)"""
    fx = fixture()
    out = []
    for cid in ("I1", "M", "I3"):
        ks = fx[cid + "/k64"].tolist()
        for k in sorted({0, max(ks)}):
            out.append((cid, k))
    return out


def check_gradient_signs(device, cid, k):
    fx = fixture()
    net, _, target = model_on(device)
    g64, Z, share = zone_of(cid, k)
    started = fx[cid + "/started"][k]
    w = torch.from_numpy(started.astype(np.float32) / started.sum()).to(device)          # the mean over the active samples, as recorded
    x = torch.from_numpy(fx[cid + "/x"][k]).to(device).requires_grad_(True)
    _, dx = attacks.loss_and_input_grad(net, x, target, w)
    dx = dx.cpu().numpy().astype(np.float64)
    sel = (np.abs(g64) > Z) & started[:, None, None, None]
    err = float(np.abs(dx - g64)[started].max())
    wrong = int((np.sign(dx[sel]) != np.sign(g64[sel])).sum())
    print("%s k=%d on %s: max |dx_hip - g64| %.3e (reference fp32: %.3e), Z %.3e, zone share %.2f %%, wrong signs outside the zone %d of %d"
          % (cid, k, device, err, Z / 30.0, Z, 100 * share, wrong, int(sel.sum())))
    assert wrong == 0, "%s k=%d: %d elements with |g64| > %.3e have the wrong sign; max |dx - g64| %.3e" % (cid, k, wrong, Z, err)


def _assert_step_close(cid, k, got, what):
    fx = fixture()
    g64, Z, _ = zone_of(cid, k)
    ref = fx[cid + "/x"][k + 1] if cid != "F" else fx["F/adv_inputs"]
    diff = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref)
    tol = 1e-5 * float(np.abs(fx[cid + "/x"][0]).max())
    bad = (diff > tol) & (np.abs(g64) > Z)
    assert not bad.any(), "%s %s iterate %d: %d elements outside the near-zero zone differ by up to %.3e (bound %.3e)" % (
        what, cid, k, int(bad.sum()), float(diff[bad].max()), tol)
    return int((diff > tol).sum())


def check_fgsm_apply(device):
    net, x, target = model_on(device)
    res = attacks.FGSM(**CONFIGS["F"][1]).apply(net, x, target)
    n = _assert_step_close("F", 0, res["adv_inputs"], "FGSM.apply")
    assert res["queries"].cpu().tolist() == [0] * x.shape[0]
    print("FGSM.apply on %s: %d elements (all with |g64| <= Z) stepped the other way" % (device, n))


ONE_STEP = [("I1", 0), ("I1", 5), ("M", 0), ("M", 5)]


def check_one_step(device, cid, k, graphed=False):
    """One model-driven iteration from recorded iterate k: the state (and momentum) up to k come from the teacher-forced chain."""
    fx = fixture()
    net, x, target = model_on(device)
    att, s, g = teacher_forced_to(device, cid, upto=k)
    xk = torch.from_numpy(fx[cid + "/x"][k]).to(device)
    if graphed:
        from cistgcn_amd import runtime
        ga = runtime.GraphedAttack(net, x, target, att)
        with torch.no_grad():
            ga.x_i.detach().copy_(xk)
            for name in ("best", "stall", "active", "w", "queries", "n_active", "steps", "frozen_at"):
                getattr(ga.state, name).copy_(getattr(s, name))
            if g is not None:
                ga.g.copy_(g)
        ga.step()
        got, s = ga.x_i.detach(), ga.state
    else:
        xi = xk.clone().requires_grad_(True)
        loss, grad = attacks.loss_and_input_grad(net, xi, target, s.w)
        att.step(xi.detach(), x, grad, loss, s, att.mask(x), g)
        got = xi.detach()
    n = _assert_step_close(cid, k, got, "graph replay" if graphed else "eager step")
    assert s.active.cpu().tolist() == fx[cid + "/active"][k].astype(int).tolist()
    assert s.queries.cpu().tolist() == [k + 1] * x.shape[0]
    print("%s k=%d on %s (%s): %d elements in the near-zero zone stepped the other way" % (cid, k, device, "graph" if graphed else "eager", n))


def check_free_running(device):
    """Structure of free-running attacks on the GPU (no numeric comparison with the recording: one near-zero sign flip legitimately
    moves every later iterate)."""
    from cistgcn_amd import runtime
    net, x, target = model_on(device)
    kw = CONFIGS["I2"][1]
    att = attacks.IFGSM(**kw)
    res = att.apply(net, x, target)
    adv = res["adv_inputs"]
    mask = att.mask(x).bool()[None, :, :, None].expand_as(x)
    assert torch.equal(adv[~mask], x[~mask]), "elements outside the frame / joint selection must stay bit-identical"
    assert bool(torch.isfinite(adv).all()) and not torch.equal(adv, x)
    assert int(res["queries"].max()) <= kw["iterations"] and int(res["queries"].min()) >= PATIENCE
    att3 = attacks.IFGSM(**CONFIGS["I3"][1])
    ga = runtime.GraphedAttack(net, x, target, att3)
    first = ga.run()
    q1, adv1 = first["queries"].clone(), first["adv_inputs"].clone()
    assert bool(torch.isfinite(adv1).all()) and int(q1.max()) <= att3.iterations and int(q1.min()) >= PATIENCE
    second = ga.reset().run()
    assert torch.equal(second["queries"], q1), (second["queries"].tolist(), q1.tolist())
    third = ga.reset(x=x, target=target).run()
    assert torch.equal(third["queries"], q1)
    print("free-running on %s: IFGSM(I2) queries %s; GraphedAttack(I3) queries %s" % (device, res["queries"].tolist(), q1.tolist()))


def check_interface(device):
    import pytest
    for cls in (attacks.FGSM, attacks.IFGSM, attacks.MIFGSM, attacks.NoAttack):
        with pytest.raises(ValueError, match="max_val"):
            cls(typ_eval="max_val")
    att = attacks.from_config({"MIFGSM": dict(typ_eval="len_y", epsilon=0.02, iterations=2, mu=0.3, joints=[0, 4], frames=None, db="h36m")})
    assert isinstance(att, attacks.MIFGSM) and att.joints == [0, 4] and att.iterations == 2
    net, x, target = model_on(device)
    bufs = [b.clone() for b in net.buffers()]
    params = [p.detach().clone() for p in net.parameters()]
    seed = ops.seed_state(device).clone()
    net.train()
    try:
        res = att.apply(net, x, target)
        assert net.training, "apply must give the model its mode back"
    finally:
        net.eval()
    assert all(torch.equal(a, b) for a, b in zip(bufs, net.buffers())), "apply moved a buffer"
    assert all(torch.equal(a, b) for a, b in zip(params, net.parameters())) and all(p.grad is None for p in net.parameters())
    assert torch.equal(seed, ops.seed_state(device)), "apply moved the dropout seed"
    assert res["queries"].cpu().tolist() == [2] * x.shape[0] and res["adv_inputs"].shape == x.shape and res["loss"].shape == (x.shape[0],)
    keep = torch.zeros(x.shape[2], dtype=torch.bool)
    keep[[0, 4]] = True
    assert torch.equal(res["adv_inputs"][:, :, ~keep].cpu(), x[:, :, ~keep].cpu())


def check_noattack(device):
    rec = load_case(CASE)
    net, x, target = model_on(device)
    res = attacks.NoAttack(typ_eval="len_y", db="h36m").apply(net, x, target)
    assert torch.equal(res["adv_inputs"], x)
    assert_close(res["grad"], rec["eval/dx"], "NoAttack dL/dx", floor=1e-1)        # the bound of the eval/dx parity check
