"""Checks of the DeepFool input attack (environment.attacks.DEEPFOOL, ops.deepfool_step, cg_deepfool_step), shared by the CPU suite
(tests/test_deepfool.py, the kernel under the HIP shim) and the MI355X suite (tests/test_gpu_deepfool.py).  Every check takes the device.

Two references:
* `ref_deepfool_step` below: a stock-PyTorch fp64 restatement of one iteration, the operator-level reference on synthetic data;
* tests/golden/eval_deepfool_h36m_c8_t10_v22.npz: what the real reference's DEEPFOOL did on the `h36m_c8_t10_v22` model, in fp32 and
  in fp64 (tools/gen_golden_deepfool.py).

Bounds (u = 2^-24, the unit roundoff of fp32; A = |g| * mean_t |pred| / (||g||_1 + 1e-10), the scale of the products behind r):
* operator level: |x_dev - (x + mask * r64)| <= 4u (A + |x| + |r64|): the sums are fp64, r is rounded to fp32 once and so is x + r;
  the factor 4 leaves room for an fp32 product and division.  A kernel that sums the To products in fp32 does not meet it at To = 25.
* teacher-forced against the reference's fp32 step: (To + 4) u (A + |x_next|), the reference sums To fp32 products.
* model-driven: |r_dev - r64| <= z_factor * noise_b + 2u |x_out|, noise_b = max |r32_ref - r64| of the reference's own fp32 model and
  z_factor = 30 from the fixture: our fp32 forward and backward may deviate from fp64 by 30 times what the reference's do, the
  assumption the sign tests of the other attacks make; r_dev = x_out - x is known up to the rounding of x_out.
* free-running: queries exact, the highest loss within z_factor * loss_noise, adv_inputs within z_factor * drift_b + 2u |adv|, where
  loss_noise and drift_b are the distances between the reference's fp32 and fp64 runs.  The generator asserts that every decision of
  the bookkeeping has a gap of at least z_factor * loss_noise.
"""
import os

import numpy as np
import pytest
import torch

from attack_checks import RefState, assert_state_equal, dev_state, model_on
from cistgcn_amd import ops
from cistgcn_amd.environment import attacks
from helpers import GOLDEN_DIR

CASE = "h36m_c8_t10_v22"
PATIENCE = 5
U = 2.0 ** -24
CONFIGS = {      # as tools/gen_golden_deepfool.py ran them, with the reference's queries
    "D1": (dict(iterations=10), [10, 10, 10, 10]),
    "D2": (dict(iterations=16, frames=[9], joints=[0]), [6, 16, 16, 16]),
    "D3": (dict(iterations=14, frames=[0, 3, 9], joints=[1, 2, 5, 21]), [14, 14, 14, 14]),
}
RECORDED = [(cid, i) for cid in CONFIGS for i in range(3)]      # i indexes the fixture's iterates k64 = {0, K // 2, K - 1}
RATIOS = {}                                                     # (device, how) -> largest |r_dev - r64| / noise_b seen
_fixture = []


def fixture():
    if not _fixture:
        z = np.load(os.path.join(GOLDEN_DIR, "eval_deepfool_%s.npz" % CASE))
        _fixture.append({k: z[k] for k in z.files})
        assert float(_fixture[0]["z_factor"]) == 30.0
    return _fixture[0]


# ---------------------------------------------------------------------------------------------------------
# the restatement: one iteration in stock PyTorch, fp64, on the CPU
# ---------------------------------------------------------------------------------------------------------
def bookkeeping(st, loss):
    """adversarial_attacks.py:755-767 on a `RefState`: a sample still optimised counts the query, raises its best loss or counts a
    stall (a tie is a stall), and is frozen from the next iteration on once it has stalled PATIENCE times"""
    act = st.active.bool()
    st.queries += act.int()
    improved = act & (loss > st.best)
    st.best = torch.where(improved, loss, st.best)
    st.stall += (act & ~improved).int()
    st.active = (act & (st.stall < PATIENCE)).int()
    st.w = st.active.float() * (torch.ones(st.B) / st.B)
    st.n_active = st.active.sum().reshape(1).int()


def ref_deepfool_step(x, grad, pred, mask=None, loss=None, st=None):
    """Returns (x + mask * r, r, A) in fp64 with r = 0 for a sample that is frozen at the start; updates `st` in place."""
    B = x.shape[0]
    act = torch.ones(B, dtype=torch.bool) if st is None else st.active.bool()
    g, p = grad.double(), pred.double()
    n1 = g.abs().sum((1, 2, 3), keepdim=True) + 1e-10
    r = -(g[:, None] * p[:, :, None]).mean(1) / n1                   # (B,T,V,3): the prediction's joints broadcast onto the input's
    scale = g.abs() * p.abs().mean(1, keepdim=True) / n1
    m = torch.ones(x.shape[1:3]) if mask is None else mask
    r = m.double()[None, :, :, None] * r * act[:, None, None, None]
    if st is not None:
        bookkeeping(st, loss)
    return x.double() + r, r, scale


def assert_within(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), "%s: error up to %.3e, %.2f times its bound" % (what, float(err.max()), worst)
    return worst


# ---------------------------------------------------------------------------------------------------------
# operator level
# ---------------------------------------------------------------------------------------------------------
STEP_SHAPES = [          # (B, T, To, V)
    (1, 1, 1, 1),        # smallest
    (3, 10, 25, 22),     # h36m
    (5, 50, 25, 25),     # 3750 floats: many passes of the 256-thread group, not a multiple of 256
    (2, 7, 3, 90),       # 270 prediction columns: more than one pass of the group
    (4, 3, 1, 5),        # To = 1; 45 floats: fewer than one pass and not a multiple of 4
    (2, 1, 2, 1400),     # 4200 prediction columns: past the 4096 whose means the kernel keeps in LDS
]


def synthetic(B, T, To, V, seed):
    """Poses of a few hundred millimetres, gradients with |g| >= 1e-3 and planted exact zeros.  Sample 1 starts frozen - with a
    gradient, which the step has to ignore - and the last sample of a batch of 3+ has an all-zero gradient."""
    gen = torch.Generator().manual_seed(seed)
    shape = (B, T, V, 3)
    x = 50 + 350 * torch.randn(shape, generator=gen)
    pred = 50 + 350 * torch.randn(B, To, V, 3, generator=gen)
    grad = (1e-3 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
    grad[torch.rand(shape, generator=gen) < 0.05] = 0.0
    st = RefState(B)
    if B > 1:
        st.active[1], st.w[1], st.stall[1], st.n_active[0] = 0, 0.0, PATIENCE, B - 1
    if B >= 3:
        grad[B - 1] = 0.0
    return x, grad, pred, st


def check_step_synthetic(device, shape, masked):
    B, T, To, V = shape
    x, grad, pred, st = synthetic(B, T, To, V, seed=B * 1000 + T * 100 + To + V + masked)
    mask = attacks.selection_mask(T, V, list(range(0, V, 3)), list(range(T - 1, -1, -2))) if masked else None
    loss = torch.linspace(1.0, 2.0, B)
    outs = []
    for _ in range(2):
        s = dev_state(st, device)
        xd = x.clone().to(device)
        ops.deepfool_step(xd, grad.to(device), pred.to(device), mask=None if mask is None else mask.to(device), loss=loss.to(device), state=s)
        outs.append(xd.cpu())
    assert torch.equal(outs[0], outs[1]), "%s: two calls give different bits" % (shape,)
    frozen = ~st.active.bool()
    want, r, scale = ref_deepfool_step(x, grad, pred, mask, loss, st)
    worst = assert_within(outs[0], want, 4 * U * (scale + x.abs().double() + r.abs()), "%s masked=%d" % (shape, masked))
    assert_state_equal(s, st, "%s masked=%d" % (shape, masked))
    assert torch.equal(outs[0][frozen], x[frozen]), "a frozen sample moved"
    if B >= 3:
        assert torch.equal(outs[0][B - 1], x[B - 1]), "an all-zero gradient must give r = 0"
    if mask is not None:
        still = (mask == 0)[None, :, :, None].expand_as(x)
        assert torch.equal(outs[0][still], x[still]), "a masked element moved"
    assert not torch.equal(outs[0], x), "nothing moved"
    # without the bookkeeping every sample steps
    xp = x.clone().to(device)
    ops.deepfool_step(xp, grad.to(device), pred.to(device), mask=None if mask is None else mask.to(device))
    want, r, scale = ref_deepfool_step(x, grad, pred, mask)
    assert_within(xp.cpu(), want, 4 * U * (scale + x.abs().double() + r.abs()), "%s masked=%d, plain step" % (shape, masked))
    return worst


def check_bookkeeping_script(device):
    """Scripted losses over 14 steps, patience 5, `best` starting at 0.  First script: sample 0 rises (never frozen); sample 1 is flat
    (one rise, then ties: frozen by step 5); sample 2 rises every other step and ties in between (frozen by step 10); sample 3 falls
    from 0 (frozen by step 4); sample 4 has a late rise that clears nothing (frozen by step 6).  Second script: every sample is
    frozen by step 5 and the eight steps after that must change nothing at all, x included."""
    T, To, V = 2, 3, 3
    gen = torch.Generator().manual_seed(11)
    scripts = [
        ([[1.0 + k for k in range(14)], [1.0] * 14, [1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8], [0.0 - k for k in range(14)],
          [1, 1, 1, 5, 5, 5, 5, 9, 9, 9, 9, 9, 9, 9]], [None, 5, 10, 4, 6], [14, 6, 11, 5, 7]),
        ([[2.0] * 14, [0.0] * 14, [3.0 - k for k in range(14)]], [5, 4, 5], [6, 5, 6]),
    ]
    for script, frozen_by, queries in scripts:
        B = len(script)
        losses = torch.tensor(script, dtype=torch.float32).t().contiguous()      # (steps, B)
        x = 50 + 350 * torch.randn(B, T, V, 3, generator=gen)
        st = RefState(B)
        s = dev_state(st, device)
        seen = [None] * B
        for k in range(losses.shape[0]):
            grad = (1e-3 + torch.rand(x.shape, generator=gen)) * (torch.randint(0, 2, x.shape, generator=gen) * 2 - 1).float()
            pred = 50 + 350 * torch.randn(B, To, V, 3, generator=gen)
            over = not bool(st.active.any())
            xd = x.clone().to(device)
            ops.deepfool_step(xd, grad.to(device), pred.to(device), loss=losses[k].to(device), state=s)
            want, r, scale = ref_deepfool_step(x, grad, pred, None, losses[k], st)
            assert_state_equal(s, st, "script of %d samples, step %d" % (B, k))
            assert_within(xd.cpu(), want, 4 * U * (scale + x.abs().double() + r.abs()), "script of %d samples, step %d" % (B, k))
            if over:
                assert torch.equal(xd.cpu(), x), "a step that starts with every sample frozen must change nothing"
            seen = [k if (f is None and not a) else f for f, a in zip(seen, st.active.tolist())]
            x = xd.cpu()
        assert seen == frozen_by and st.queries.tolist() == queries, (seen, st.queries.tolist())
        assert int(st.n_active) == sum(f is None for f in frozen_by)


def check_operand_contract(device):
    B, T, To, V = 2, 3, 4, 5
    good = dict(x=torch.randn(B, T, V, 3), grad=torch.randn(B, T, V, 3), pred=torch.randn(B, To, V, 3), mask=torch.ones(T, V))
    bad = {
        "x": [torch.randn(B, T, V + 1, 3), torch.randn(B, T, V, 2)],
        "grad": [torch.randn(B, T + 1, V, 3), torch.randn(B, T * V * 3)],
        "pred": [torch.randn(B + 1, To, V, 3), torch.randn(B, To, V, 4), torch.randn(B, To, V + 1, 3), torch.randn(B, To * V * 3)],
        "mask": [torch.ones(V, T), torch.ones(T, V, 1)],
    }
    for name, ok in good.items():
        strided = torch.randn(*ok.shape[:-1], 2 * ok.shape[-1]).to(device)[..., ::2]      # sliced on the device: a copy there would be dense
        assert strided.shape == ok.shape and not strided.is_contiguous()
        for wrong in [ok.double(), strided] + bad[name]:
            ops_in = {k: (wrong if k == name else v).to(device) for k, v in good.items()}
            assert wrong is not strided or not ops_in[name].is_contiguous()
            keep = ops_in["x"].clone()
            with pytest.raises(ValueError, match="deepfool_step"):
                ops.deepfool_step(ops_in["x"], ops_in["grad"], ops_in["pred"], mask=ops_in["mask"])
            assert torch.equal(ops_in["x"], keep)
    dev = {k: v.to(device) for k, v in good.items()}
    with pytest.raises(ValueError, match="same V"):
        ops.deepfool_step(dev["x"], dev["grad"], torch.randn(B, To, V + 1, 3).to(device))
    with pytest.raises(ValueError, match="go together"):
        ops.deepfool_step(dev["x"], dev["grad"], dev["pred"], loss=torch.ones(B).to(device))
    with pytest.raises(ValueError, match="AttackState"):
        ops.deepfool_step(dev["x"], dev["grad"], dev["pred"], loss=torch.ones(B).to(device), state=ops.AttackState(B + 1, device))


def check_entry_point_statuses(device):
    """cg_deepfool_step itself: CG_EARG (-1) for a null operand or a partial state, CG_ESHAPE (-2) for a non-positive extent; nothing
    is launched in either case"""
    import ctypes
    from cistgcn_amd import _lib
    B, T, To, V = 2, 3, 4, 5
    x, grad, pred = (torch.ones(B, T, V, 3).to(device), torch.ones(B, T, V, 3).to(device), torch.ones(B, To, V, 3).to(device))
    loss, s = torch.ones(B).to(device), ops.AttackState(B, device)

    def status(**change):
        a = _lib.DeepfoolStep()
        a.B, a.T, a.To, a.V, a.patience = B, T, To, V, PATIENCE
        a.x, a.grad, a.pred = ops._ptr(x), ops._ptr(grad), ops._ptr(pred)
        for k, v in change.items():
            setattr(a, k, v)
        return _lib.lib().cg_deepfool_step(ctypes.byref(a), ops._stream(x))

    for name in ("x", "grad", "pred"):
        assert status(**{name: None}) == -1, name
    assert status(loss=ops._ptr(loss)) == -1, "loss without the state"
    full = dict(loss=ops._ptr(loss), **{k: ops._ptr(getattr(s, k)) for k in ("best", "stall", "active", "w", "queries", "n_active", "steps", "frozen_at")})
    for name in full:
        if name != "loss":
            assert status(**dict(full, **{name: None})) == -1, "state without " + name
    for name in ("B", "T", "To", "V"):
        assert status(**{name: 0}) == -2 and status(**{name: -1}) == -2, name
    assert status(patience=0, **full) == -2
    assert torch.equal(x.cpu(), torch.ones(B, T, V, 3)) and s.queries.cpu().tolist() == [0] * B
    assert status(**full) == 0 and s.queries.cpu().tolist() == [1] * B


# ---------------------------------------------------------------------------------------------------------
# against the real reference
# ---------------------------------------------------------------------------------------------------------
def state_before(cid, k):
    """the bookkeeping at the start of recorded iteration k, restated from the recorded losses"""
    fx = fixture()
    loss = torch.from_numpy(fx[cid + "/loss"])
    st = RefState(loss.shape[1])
    for j in range(k):
        bookkeeping(st, loss[j])
        assert st.active.bool().tolist() == fx[cid + "/active"][j].tolist()
    assert st.active.bool().tolist() == fx[cid + "/started"][k].tolist()
    return st


def check_teacher_forced(device, cid, i):
    """The reference's recorded fp32 gradient, prediction, iterate and active set through `ops.deepfool_step`."""
    fx = fixture()
    att = attacks.DEEPFOOL(**CONFIGS[cid][0])
    k = int(fx[cid + "/k64"][i])
    x, grad, pred = (torch.from_numpy(fx[cid + "/" + n][i]) for n in ("x", "grad", "pred"))
    x_next = torch.from_numpy(fx[cid + "/x_next"][i])
    st = state_before(cid, k)
    started = st.active.bool()
    s = dev_state(st, device)
    xd = x.clone().to(device)
    ops.deepfool_step(xd, grad.to(device), pred.to(device), mask=att.mask(xd), loss=torch.from_numpy(fx[cid + "/loss"][k]).to(device), state=s)
    _, _, scale = ref_deepfool_step(x, grad, pred)
    To = pred.shape[1]
    worst = assert_within(xd.cpu(), x_next.double(), (To + 4) * U * (scale + x_next.abs().double()), "%s iteration %d" % (cid, k))
    assert torch.equal(xd.cpu()[~started], x[~started]), "a sample that was not started moved"
    assert s.active.cpu().bool().tolist() == fx[cid + "/active"][k].tolist() and s.queries.cpu().tolist() == st.queries.add(started.int()).tolist()
    print("%s k=%d on %s: teacher-forced step at %.2f of its bound" % (cid, k, device, worst))


_graphs = {}


def graphed(device, cid):
    """one captured iteration per configuration and device for the whole session; every user re-arms it first"""
    from cistgcn_amd import runtime
    key = (str(device), cid)
    if key not in _graphs:
        net, x, target = model_on(device)
        _graphs[key] = runtime.GraphedAttack(net, x, target, attacks.DEEPFOOL(**CONFIGS[cid][0]))
    return _graphs[key]


def check_model_step(device, cid, i, graph=False):
    """Our model's own step from the recorded iterate against the step of the reference's fp64 model."""
    fx = fixture()
    net, x0, target = model_on(device)
    k = int(fx[cid + "/k64"][i])
    xk = torch.from_numpy(fx[cid + "/x"][i]).to(device)
    st = state_before(cid, k)
    if graph:
        ga = graphed(device, cid).reset(x0, target)
        with torch.no_grad():
            ga.x_i.detach().copy_(xk)
        s, at_k = ga.state, dev_state(st, device)
        for name in ("best", "stall", "active", "w", "queries", "n_active", "steps", "frozen_at"):
            getattr(s, name).copy_(getattr(at_k, name))
        ga.step()
        got = ga.x_i.detach().cpu()
    else:
        att = attacks.DEEPFOOL(**CONFIGS[cid][0])
        s = dev_state(st, device)
        xi = xk.clone().requires_grad_(True)
        att.iterate(net, xi, x0, target, s, att.mask(x0), None)
        got = xi.detach().cpu()
    r_dev = got.double() - xk.cpu().double()
    r64, noise = torch.from_numpy(fx[cid + "/r64"][i]), torch.from_numpy(fx[cid + "/noise"][i])
    err = (r_dev - r64).abs()
    z = float(fx["z_factor"])
    ratio = err.reshape(err.shape[0], -1).max(1)[0] / noise.clamp_min(1e-300)
    ratio = float(ratio[noise > 0].max())
    how = "graph" if graph else "eager"
    RATIOS[(str(device), how)] = max(RATIOS.get((str(device), how), 0.0), ratio)
    print("%s k=%d on %s (%s): max |r_dev - r64| / noise_b = %.2f (largest so far %.2f)" % (cid, k, device, how, ratio, RATIOS[(str(device), how)]))
    assert_within(got, xk.cpu().double() + r64, z * noise[:, None, None, None] + 2 * U * got.abs().double(), "%s iteration %d (%s)" % (cid, k, how))
    started = st.active.bool()
    assert torch.equal(got[~started], xk.cpu()[~started])
    assert s.active.cpu().bool().tolist() == fx[cid + "/active"][k].tolist()


def _assert_free_run(res, cid, what, order=None):
    fx = fixture()
    z = float(fx["z_factor"])
    order = list(range(len(CONFIGS[cid][1]))) if order is None else order
    queries, adv, drift = fx[cid + "/queries"][order], torch.from_numpy(fx[cid + "/adv_inputs"][order]), torch.from_numpy(fx[cid + "/drift"][order])
    best = torch.from_numpy(np.where(fx[cid + "/started"], fx[cid + "/loss"], 0.0).max(0)[order])
    assert queries.tolist() == list(np.asarray(CONFIGS[cid][1])[order])
    assert res["queries"].cpu().tolist() == queries.tolist(), "%s %s: queries %s, the reference's %s" % (what, cid, res["queries"].cpu().tolist(), queries.tolist())
    l = assert_within(res["loss"].cpu(), best.double(), torch.full_like(best, z * float(fx[cid + "/loss_noise"])).double(), "%s %s: highest loss" % (what, cid))
    got = res["adv_inputs"].cpu()
    a = assert_within(got, adv.double(), z * drift[:, None, None, None] + 2 * U * got.abs().double(), "%s %s: adv_inputs" % (what, cid))
    print("%s %s: queries %s; highest loss at %.2f, adv_inputs at %.2f of their bounds" % (what, cid, queries.tolist(), l, a))


def _snapshot(net, device):
    return ([b.clone() for b in net.buffers()], [p.detach().clone() for p in net.parameters()], ops.seed_state(device).clone())


def _assert_untouched(net, device, snap):
    bufs, params, seed = snap
    assert all(torch.equal(a, b) for a, b in zip(bufs, net.buffers())), "the attack moved a buffer"
    assert all(torch.equal(a, b) for a, b in zip(params, net.parameters())) and all(p.grad is None for p in net.parameters())
    assert torch.equal(seed, ops.seed_state(device)), "the attack moved the dropout seed"


def check_free_running(device, cid, graph=False):
    net, x, target = model_on(device)
    snap = _snapshot(net, device)
    if graph:
        res = graphed(device, cid).reset(x, target).run()
        assert not net.training
    else:
        net.train()
        try:
            res = attacks.DEEPFOOL(**CONFIGS[cid][0]).apply(net, x, target)
            assert net.training, "apply must give the model its mode back"
        finally:
            net.eval()
    _assert_free_run(res, cid, "%s on %s" % ("GraphedAttack.run" if graph else "DEEPFOOL.apply", device))
    _assert_untouched(net, device, snap)
    if cid != "D1":
        still = (attacks.DEEPFOOL(**CONFIGS[cid][0]).mask(x) == 0)[None, :, :, None].expand_as(x)
        assert torch.equal(res["adv_inputs"][still], x[still]), "elements outside the frame / joint selection must stay bit-identical"


def check_graph_reset(device, cid="D3"):
    """A second batch - the fixture's samples in reverse order; in eval mode the samples do not see one another - through
    `reset(x, target).run()` and through a fresh `apply`: both are the reference's result in that order."""
    net, x, target = model_on(device)
    order = list(range(x.shape[0]))[::-1]
    x2, t2 = x.flip(0).contiguous(), target.flip(0).contiguous()
    ga = graphed(device, cid)
    ga.reset(x, target).run()
    res = ga.reset(x2, t2).run()
    _assert_free_run(res, cid, "reset + run on %s" % device, order)
    fresh = attacks.DEEPFOOL(**CONFIGS[cid][0]).apply(net, x2, t2)
    _assert_free_run(fresh, cid, "fresh apply on %s" % device, order)
    assert torch.equal(res["queries"], fresh["queries"])
    print("reset + run against a fresh apply on %s: adv_inputs differ by up to %.3e" % (device, float((res["adv_inputs"] - fresh["adv_inputs"]).abs().max())))


def check_interface(device):
    kw = dict(typ_eval="len_y", iterations=2, overshoot=0.05, joints=[0, 4], frames=[1, 2], db="h36m")      # the reference's keywords (:671)
    for name in ("DEEPFOOL", "DeepFool"):
        att = attacks.from_config({name: dict(kw)})
        assert type(att) is attacks.DEEPFOOL and att.iterations == 2 and att.overshoot == 0.05 and att.joints == [0, 4] and att.frames == [1, 2]
    from cistgcn_amd import environment
    assert environment.DEEPFOOL is attacks.DEEPFOOL and environment.DeepFool is attacks.DEEPFOOL
    d = attacks.DEEPFOOL()
    assert (d.typ_eval, d.iterations, d.overshoot, d.joints, d.frames, d.db) == ("len_y", 10, 0.02, None, None, "h36m")
    with pytest.raises(TypeError):
        attacks.from_config({"DEEPFOOL": dict(epsilon=0.01)})
    with pytest.raises(TypeError):
        attacks.DEEPFOOL("len_y", 10)                    # keyword-only behind typ_eval, as the other attacks
    with pytest.raises(ValueError, match="max_val"):
        attacks.DEEPFOOL(typ_eval="max_val")
    with pytest.raises(ValueError, match="iterations"):
        attacks.DEEPFOOL(iterations=0)
    net, x, target = model_on(device)
    with pytest.raises(ValueError, match="V_in == V_out"):
        att.apply(net, x, torch.cat([target, target[:, :, :1]], 2))
    from cistgcn_amd import runtime
    for other in (attacks.FGSM(), attacks.NoAttack()):
        with pytest.raises(ValueError, match="iterative"):
            runtime.GraphedAttack(net, x, target, other)
    snap = _snapshot(net, device)
    res = att.apply(net, x, target)
    _assert_untouched(net, device, snap)
    assert res["queries"].cpu().tolist() == [2] * x.shape[0] and res["adv_inputs"].shape == x.shape and res["loss"].shape == (x.shape[0],)
    keep = torch.zeros(x.shape[1], x.shape[2], dtype=torch.bool)
    keep[1:3, [0, 4]] = True
    adv = res["adv_inputs"].cpu()
    assert torch.equal(adv[:, ~keep], x.cpu()[:, ~keep]) and not torch.equal(adv[:, keep], x.cpu()[:, keep])
    sheet = att.metrics(res["adv_inputs"], x, res["queries"])
    assert len(sheet) == 35 and sheet["metric_type"] == "len_y" and sheet["queries"] is res["queries"] and set(ops.ATTACK_METRICS) <= set(sheet)
