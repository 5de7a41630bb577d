"""Checks of the training losses (`ops.motion_loss` and its four named forms over cg_motion_loss_fwd / _bwd, `environment.TrainingLoss`,
the `loss=` / `target_gvel=` arguments of the step objects), device as an argument: tests/test_emu_losses.py runs them on the CPU-only box
through the HIP shim, tests/test_gpu_losses.py on the MI355X.

References: tests/golden/eval_losses.npz (the reference's own `train()` for one iteration per case, tools/gen_golden_losses.py) and the fp64
restatement tests/losses_ref.py, itself pinned in fp32 by that fixture.

The bound is the project's rule with no floor, `helpers.assert_close(rel=1e-4, floor=0)`: max|got - ref| <= 1e-4 * max|ref| per tensor
(a floor of 1 would be vacuous for gradients of order 1 / (B*T*V)).  What fp32 arithmetic costs on these inputs was measured before
relying on it: the stock-torch fp32 composition of the same formulas against the fp64 restatement, on the CPU, over every kind x
weight source at the shapes (3,5,4), (4,6,22) and (2,3,70) of `draw` gave at most 1.5e-7 relative on the loss and 1.9e-7 of max|ref| on
the gradient (relative L2 of the gradient: 8.6e-8 at most) - `fp32_torch_error` below computes it and test_emu_losses.py prints and bounds
it.  1e-4 leaves more than two orders of magnitude; a kernel that needs more has a defect."""
import ctypes
import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import losses_ref as R
from helpers import GOLDEN_DIR, assert_close, assert_grads_close, make_cfg

KINDS = R.KINDS
SOURCES = ("none", "table", "full", "speed", "table+speed")


def loop_shapes():
    """(B,T,V): the smallest shapes that reach each loop of the kernels; the last one has more frames than one pass of the capped grid"""
    from cistgcn_amd import _lib
    one_pass = _lib.LIMITS["CG_LOSS_MAX_BLOCKS"] * (_lib.LIMITS["CG_LOSS_THREADS"] // 64)
    return ((1, 1, 1), (1, 7, 22), (2, 3, 64), (2, 3, 70), (one_pass // 3 + 1, 3, 2))


def draw(shape, seed=0, equal=True):
    """(pred, target (B,T,V,3), target_gvel (B,T,V,1)), fp32 on the host: differences with per-coordinate standard deviations
    (0.3, 3, 30) around targets of scale 300, so that both branches of SmoothL1 are taken; with `equal` the joint `equal_joint(b)` of
    every sample is exactly its target (e = 0); speeds are cumulative and non-negative, the last frame of sample 0 has all-zero speeds"""
    B, T, V = shape
    g = torch.Generator().manual_seed(seed)
    target = 300 * torch.randn(B, T, V, 3, generator=g)
    pred = target + torch.randn(B, T, V, 3, generator=g) * torch.tensor([0.3, 3.0, 30.0])
    if equal:
        for b in range(B):
            t, v = equal_joint(b, shape)
            pred[b, t, v] = target[b, t, v]
    gvel = torch.cumsum(3 * torch.rand(B, T, V, 1, generator=g), 1)
    gvel[0, T - 1] = 0
    return pred, target, gvel


def equal_joint(b, shape):
    return b % shape[1], (2 * b + 1) % shape[2]


def weight_source(source, shape, gvel, seed=1):
    """keyword arguments of ops.motion_loss for a weight source, and the same weights for the restatement (fp32 host tensors)"""
    B, T, V = shape
    g = torch.Generator().manual_seed(seed)
    table = R.frame_table("sqrt", T)
    full = 0.5 + 2 * torch.rand(B, T, V, generator=g)
    if source == "none":
        return {}
    if source == "table":
        return dict(frame_weights=table)
    if source == "full":
        return dict(w=full)
    if source == "speed":
        return dict(speeds=gvel, speed_factor=1.0)
    return dict(frame_weights=table, speeds=gvel[..., 0], speed_factor=2.0)       # speeds in both accepted shapes


def reference_weights(kw, shape, dtype):
    base = kw.get("w", kw.get("frame_weights"))
    if base is not None:
        base = base.to(dtype)
        base = base[None, :, None].expand(*shape) if base.dim() == 1 else base
    sp = kw.get("speeds")
    return R.joint_weights(base, None if sp is None else sp.reshape(shape).to(dtype), kw.get("speed_factor", 1.0))


def on(device, kw):
    return {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}


def run_op(device, kind, pred, target, kw):
    """(loss, dpred) of ops.motion_loss on the device, as host tensors"""
    from cistgcn_amd import ops
    p = pred.clone().to(device).requires_grad_(True)       # a leaf of its own: on the shim `.to` would hand back `pred` itself
    val = ops.motion_loss(kind, p, target.to(device), **on(device, kw))
    val.backward()
    return val.detach().cpu().clone(), p.grad.cpu().clone()


def compare(got, ref, what):
    """loss and gradient within the bound; prints each figure before it asserts"""
    for name, g, r in (("loss", got[0], ref[0]), ("dpred", got[1], ref[1])):
        g, r = g.double().numpy(), r.double().numpy()
        err, mx = float(np.abs(g - r).max()), float(np.abs(r).max())
        print("%s %s: max err %.3e, max|ref| %.3e, ratio %.3e" % (what, name, err, mx, err / mx if mx else 0.0))
        assert np.isfinite(g).all(), (what, name)
        assert_close(g, r, "%s %s" % (what, name), rel=1e-4, floor=0)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "eval_losses.npz"))
    return {k: z[k] for k in z.files}


def cases():
    fx = fixture()
    return tuple("%s|%s" % (t, w) for t in fx["types"] for w in fx["weights"])


def fixture_inputs():
    fx = fixture()
    return tuple(torch.from_numpy(fx[k].copy()) for k in ("pred", "target", "target_gvel"))


def config(case):
    kind, weights = case.split("|")
    return NS(loss=NS(type=kind, weights=weights))


def check_fixture_covers_the_issue():
    fx = fixture()
    assert [str(t) for t in fx["types"]] == list(R.TYPES)
    assert [str(w) for w in fx["weights"]] == ["", "linear", "sqrt", "exp", "square", "speed", "speed2_sqrt", "speed_linear"]
    assert fx["pred"].shape == (3, 5, 4, 3) and fx["target_gvel"].shape == (3, 5, 4, 1)
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "eval_losses.npz")) < 256 * 1024
    e = np.linalg.norm(fx["pred"] - fx["target"], axis=-1)
    assert (e == 0).sum() == 3 and (fx["target_gvel"][0, -1] == 0).all()


def check_restatement(case):
    """the restatement in fp32 against the recording: loss, gradient, the weight tensor; the product's frame table bit for bit"""
    from cistgcn_amd.environment import frame_weights
    fx = fixture()
    pred, target, gvel = fixture_inputs()
    kind, weights = case.split("|")
    w = R.batch_weights(weights, pred.shape[:3], gvel)
    assert_close(w, fx[case + "/w"], case + " w", rel=1e-6, floor=0)          # elementwise fp32 arithmetic of a few operations
    got = R.loss_and_grad(R.TYPES[kind], pred, target, w, dtype=torch.float32)
    assert_close(got[0], fx[case + "/loss"], case + " loss", rel=1e-4, floor=0)
    assert_close(got[1], fx[case + "/grad"], case + " grad", rel=1e-4, floor=0)
    table = frame_weights(weights, pred.shape[1])
    assert table.dtype == torch.float32 and np.array_equal(table.numpy().view(np.uint32), fx[case + "/table"].view(np.uint32)), case
    assert np.array_equal(R.frame_table(weights, pred.shape[1]).numpy(), fx[case + "/table"])


def check_against_fixture(device, case):
    """`TrainingLoss` on the device against the recording and against the fp64 restatement; in the order of train.py:76,
    `(target, output)`, it gives the same bits"""
    from cistgcn_amd.environment import TrainingLoss, get_loss
    fx = fixture()
    pred, target, gvel = fixture_inputs()
    kind, weights = case.split("|")
    fn = TrainingLoss(config(case), pred.shape[1], device)
    assert type(get_loss(config(case), pred.shape[1], device)) is TrainingLoss
    p, t, gv = pred.clone().to(device).requires_grad_(True), target.to(device), gvel.clone().to(device)
    val = fn(p, t, gv)
    val.backward()
    got = (val.detach().cpu().clone(), p.grad.cpu().clone())
    compare(got, (torch.tensor(fx[case + "/loss"]), torch.from_numpy(fx[case + "/grad"])), case + " vs the recording")
    ref = R.loss_and_grad(R.TYPES[kind], pred, target, R.batch_weights(weights, pred.shape[:3], gvel, torch.float64))
    compare(got, ref, case + " vs fp64")
    q = pred.clone().to(device).requires_grad_(True)
    swapped = fn(t, q, gv)
    swapped.backward()
    assert torch.equal(swapped.detach().cpu(), got[0]) and torch.equal(q.grad.cpu(), got[1]), case
    assert torch.equal(gv.cpu(), gvel), "target_gvel was written"


# ---- the operator against the fp64 restatement -----------------------------------------------------------------------------------
def check_shape(device, shape, kind, source):
    pred, target, gvel = draw(shape, seed=5, equal=shape[1] * shape[2] > 1)
    kw = weight_source(source, shape, gvel)
    if kind in R.WEIGHTED and source == "none":
        from cistgcn_amd import ops
        with pytest.raises(ValueError):
            ops.motion_loss(kind, pred.to(device), target.to(device))
        return
    got = run_op(device, kind, pred, target, kw)
    ref = R.loss_and_grad(kind, pred, target, reference_weights(kw, shape, torch.float64) if kind in R.WEIGHTED else None)
    compare(got, ref, "%s %s %s" % ("x".join(str(v) for v in shape), kind, source))


def fp32_torch_error(shapes=((3, 5, 4), (4, 6, 22), (2, 3, 70))):
    """the stock-torch fp32 composition against the fp64 restatement on the inputs of `draw`: (worst relative error of the loss, worst
    max|gradient error| / max|ref|, worst relative L2 error of the gradient) - what the bound of `compare` has to leave room for"""
    worst = [0.0, 0.0, 0.0]
    for shape in shapes:
        pred, target, gvel = draw(shape, seed=5)
        for kind in KINDS:
            for source in SOURCES[1:] if kind in R.WEIGHTED else SOURCES[:1]:
                kw = weight_source(source, shape, gvel)
                w32, w64 = (reference_weights(kw, shape, d) if kind in R.WEIGHTED else None for d in (torch.float32, torch.float64))
                a, b = R.loss_and_grad(kind, pred, target, w32, torch.float32), R.loss_and_grad(kind, pred, target, w64)
                worst[0] = max(worst[0], abs(float(a[0]) - float(b[0])) / abs(float(b[0])))
                worst[1] = max(worst[1], float((a[1].double() - b[1]).abs().max() / b[1].abs().max()))
                worst[2] = max(worst[2], float((a[1].double() - b[1]).norm() / b[1].norm()))
    return tuple(worst)


def check_input_coverage(device, shape=(4, 6, 22)):
    """the inputs take both SmoothL1 branches; a joint equal to its target gets an exact, finite zero gradient in every kind; a frame
    of all-zero speeds weighs nothing"""
    pred, target, gvel = draw(shape, seed=9)
    share = float(((pred - target).abs() < 1).float().mean())
    print("share of |d| < 1: %.3f" % share)
    assert 0.2 <= share <= 0.8, share
    assert (gvel[0, -1] == 0).all() and (gvel[1:] > 0).all()
    for kind in KINDS:
        kw = weight_source("table+speed", shape, gvel) if kind in R.WEIGHTED else {}
        val, d = run_op(device, kind, pred, target, kw)
        assert torch.isfinite(d).all() and torch.isfinite(val), kind
        for b in range(shape[0]):
            t, v = equal_joint(b, shape)
            assert (d[b, t, v] == 0).all(), (kind, b, d[b, t, v])
        assert (d != 0).float().mean() > 0.9, kind
    # speed weights only: the all-zero frame gets weight 0, hence no gradient
    _, d = run_op(device, "weighted_mpjpe", pred, target, dict(speeds=gvel))
    assert (d[0, -1] == 0).all() and (d[0, 0] != 0).any()


def check_all_errors_zero(device):
    """pred == target everywhere: every loss is 0 and every gradient an exact zero - for rmpjpe torch gives NaN there (0 / 0), the
    kernel writes 0 (documented deviation)"""
    _, target, gvel = draw((2, 3, 5), seed=2)
    for kind in KINDS:
        val, d = run_op(device, kind, target.clone(), target, weight_source("table+speed", (2, 3, 5), gvel) if kind in R.WEIGHTED else {})
        assert float(val) == 0.0 and (d == 0).all(), kind


def check_untouched_and_reproducible(device, shape=(3, 7, 22)):
    from cistgcn_amd import ops
    from cistgcn_amd.environment import TrainingLoss
    pred, target, gvel = draw(shape, seed=3)
    w = weight_source("full", shape, gvel)["w"]
    dev = [t.clone().to(device) for t in (pred, target, w, gvel)]
    for kind in KINDS:
        outs = []
        for _ in range(2):
            p = dev[0].clone().requires_grad_(True)
            val = ops.motion_loss(kind, p, dev[1], w=dev[2], speeds=dev[3], speed_factor=2.0)
            val.backward()
            outs.append((val.detach().clone(), p.grad.clone()))
            assert torch.equal(p.detach(), dev[0])
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), kind
    fn = TrainingLoss(NS(loss=NS(type="w_mpjpe_soft", weights="speed2_sqrt")), shape[1], device)
    p = dev[0].clone().requires_grad_(True)
    fn(p, dev[1], dev[3]).backward()
    for t, host in zip(dev, (pred, target, w, gvel)):
        assert torch.equal(t.cpu(), host), "an input was written"


def check_named_forms(device, shape=(2, 3, 5)):
    """the four named operators are `motion_loss` of their kind"""
    from cistgcn_amd import ops
    pred, target, gvel = (t.to(device) for t in draw(shape, seed=4))
    w = weight_source("full", shape, gvel)["w"].to(device)
    assert torch.equal(ops.weighted_mpjpe(pred, target, w), ops.motion_loss("weighted_mpjpe", pred, target, w=w))
    assert torch.equal(ops.weighted_mpjpe_soft(pred, target, w), ops.motion_loss("weighted_mpjpe_soft", pred, target, w=w))
    assert torch.equal(ops.mpjpe_soft(pred, target), ops.motion_loss("mpjpe_soft", pred, target, w=w))         # w is ignored
    assert torch.equal(ops.rmpjpe(pred, target), ops.motion_loss("rmpjpe", pred, target))
    assert_close(ops.rmpjpe(pred, target) ** 2, ops.mpjpe(pred, target), "rmpjpe^2 = mpjpe", rel=1e-6, floor=0)
    for kind in KINDS:                                                                                          # symmetric in value
        kw = dict(w=w) if kind in R.WEIGHTED else {}
        assert torch.equal(ops.motion_loss(kind, pred, target, **kw), ops.motion_loss(kind, target, pred, **kw)), kind


def check_interface_errors(device):
    from cistgcn_amd import _lib, ops
    from cistgcn_amd.environment import TrainingLoss
    shape = (2, 3, 5)
    pred, target, gvel = (t.to(device) for t in draw(shape, seed=4))
    w = torch.ones(shape).to(device)
    with pytest.raises(TypeError):
        ops.mpjpe_soft(pred.double(), target.double())
    with pytest.raises(TypeError):
        ops.weighted_mpjpe(pred, target, w.double())
    with pytest.raises(TypeError):
        ops.motion_loss("weighted_mpjpe", pred, target, speeds=gvel.double())
    for bad in (target[:, :2], target[..., :2], target[0]):
        with pytest.raises(ValueError):
            ops.rmpjpe(pred, bad)
    with pytest.raises(ValueError):
        ops.rmpjpe(pred[..., :2], target[..., :2])
    for bad in (w[:1], w[:, :2], w[..., None], w[0]):
        with pytest.raises(ValueError):
            ops.weighted_mpjpe(pred, target, bad)
    with pytest.raises(ValueError):
        ops.weighted_mpjpe_soft(pred, target, None)
    with pytest.raises(ValueError):
        ops.motion_loss("weighted_mpjpe", pred, target, frame_weights=torch.ones(4).to(device))
    with pytest.raises(ValueError):
        ops.motion_loss("weighted_mpjpe", pred, target, speeds=gvel[:, :2])
    with pytest.raises(ValueError):
        ops.motion_loss("pa_mpjpe", pred, target)
    with pytest.raises(ValueError):
        ops.motion_loss("mpjpe", pred, target)                       # plain MPJPE is ops.mpjpe
    with pytest.raises(ValueError):
        ops.motion_loss("rmpjpe", pred.clone().requires_grad_(True), target.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        TrainingLoss(NS(loss=NS(type="l2", weights="")), 3, device)
    for kind in ("mpjpe", "w_mpjpe", "rmpjpe"):                         # train.py:63 reads target_gvel whatever the type
        with pytest.raises(ValueError):
            TrainingLoss(NS(loss=NS(type=kind, weights="speed2_sqrt")), 3, device)(pred, target)
    fn = TrainingLoss(NS(loss=NS(type="w_mpjpe", weights="speed13_exp")), 3, device)
    assert fn.speed_factor == 13.0 and fn.uses_speed and not fn.speed_only and fn.kind == "weighted_mpjpe"
    assert TrainingLoss(NS(loss=NS(type="w_mpjpe", weights="speed")), 3, device).speed_only
    assert TrainingLoss(NS(loss=NS(type="mpjpe", weights="sqrt2")), 3, device).speed_factor == 1.0
    # the C ABI itself: status codes, nothing launched (the pointers are never followed)
    p = ctypes.c_void_p(64)

    def status(name="cg_motion_loss_fwd", **kw):
        a = _lib.MotionLoss()
        a.kind, a.B, a.T, a.V, a.speed_factor = _lib.LIMITS["CG_LOSS_WEIGHTED_MPJPE"], 2, 3, 5, 1.0
        for k in ("pred", "target", "w_full", "part", "loss", "mean", "gloss", "dpred"):
            setattr(a, k, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(_lib.lib(), name)(ctypes.byref(a), None)

    assert _lib.lib().cg_motion_loss_fwd(None, None) == -1 and _lib.lib().cg_motion_loss_bwd(None, None) == -1
    for k in ("pred", "target", "part", "loss", "mean"):
        assert status(**{k: None}) == -1, k
    for k in ("pred", "target", "gloss", "dpred"):
        assert status("cg_motion_loss_bwd", **{k: None}) == -1, k
    assert status(w_full=None) == -1 and status("cg_motion_loss_bwd", w_full=None) == -1        # a weighted kind without any weight
    assert status("cg_motion_loss_bwd", kind=_lib.LIMITS["CG_LOSS_RMPJPE"], mean=None) == -1
    for kw in (dict(kind=4), dict(kind=-1), dict(B=0), dict(T=0), dict(V=0)):
        assert status(**kw) == -2 and status("cg_motion_loss_bwd", **kw) == -2, kw


def check_host_tensors_refused():
    """without the shim there is no CPU path: refused before anything is launched"""
    from cistgcn_amd import _lib, ops
    was = _lib._host_pointers_ok
    _lib._host_pointers_ok = False
    try:
        with pytest.raises(RuntimeError):
            ops.rmpjpe(torch.zeros(2, 3, 5, 3), torch.ones(2, 3, 5, 3))
        with pytest.raises(RuntimeError):
            ops.weighted_mpjpe(torch.zeros(2, 3, 5, 3), torch.ones(2, 3, 5, 3), torch.ones(2, 3, 5))
    finally:
        _lib._host_pointers_ok = was


# ---- the step objects --------------------------------------------------------------------------------------------------------------
STEP_LOSS = NS(loss=NS(type="w_mpjpe_soft", weights="speed2_sqrt"))


def step_setup(device, reduced, B=3, To=25):
    """the small model of the issue (C=8, T=10, V=22, dropout 0; fewer blocks on the shim), a batch and its loss object"""
    import checks
    from cistgcn_amd.environment import TrainingLoss
    kw = dict(blocks=1, txc=1, To=8, hidden=16) if reduced else dict(To=To)
    net, _ = checks.build_pair(8, 10, 22, device, seed=0, **kw)
    net.train()
    To = kw["To"]
    g = torch.Generator().manual_seed(5)
    x = (50 + 350 * torch.randn(B, 10, 22, 3, generator=g)).to(device)
    tgt = (x[:, -1:].cpu() + 20 * torch.randn(B, To, 22, 3, generator=g)).to(device)
    gvel = torch.cumsum(3 * torch.rand(B, To, 22, 1, generator=g), 1).to(device)
    return net, x, tgt, gvel, TrainingLoss(STEP_LOSS, To, device)


def by_hand(net, x, tgt, gvel, fn):
    """the same operator called by hand after model(x): (loss, {parameter name: gradient})"""
    from cistgcn_amd import ops
    for p in net.parameters():
        p.grad = None
    with ops.step_pool(ops.new_step_pool(x.device)):
        pred, = net(x)
        val = ops.motion_loss("weighted_mpjpe_soft", pred, tgt, frame_weights=fn.frame_weights, speeds=gvel, speed_factor=2.0)
        val.backward()
    return val.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()}


def check_eager_step(device, reduced):
    from cistgcn_amd.runtime import EagerStep
    net, x, tgt, gvel, fn = step_setup(device, reduced)
    ref_loss, ref_grads = by_hand(net, x, tgt, gvel, fn)
    keep = gvel.clone()
    step = EagerStep(net, x, tgt, loss=fn, target_gvel=gvel)
    val = step.replay()
    assert_close(val, ref_loss, "EagerStep loss", rel=1e-4, floor=0)
    assert_grads_close({k: p.grad for k, p in net.named_parameters()}, ref_grads, "EagerStep")
    assert torch.equal(gvel, keep)
    plain = float(EagerStep(net, x, tgt).replay().detach())    # the default is still MPJPE
    assert abs(plain - float(val.detach())) > 1e-3 * abs(plain)
    return net, x, tgt, gvel, fn, val.detach().clone()


def check_graphed_step(device="cuda"):
    """GraphedStep with the loss replays twice: the loss of the EagerStep, and target_gvel keeps its bits"""
    from cistgcn_amd.runtime import GraphedStep, _drop_graph_attributes
    net, x, tgt, gvel, fn, eager_loss = check_eager_step(device, reduced=False)
    # nothing of the eager passes' autograd graphs may be alive during the capture (their AccumulateGrad nodes belong to the
    # default stream; runtime.GraphedStep keeps only values for the same reason): the loss above is detached, and so are these
    _drop_graph_attributes(net)
    keep = gvel.clone()
    step = GraphedStep(net, x, tgt, warmup=2, loss=fn, target_gvel=gvel)
    assert step.target_gvel is not gvel and torch.equal(step.target_gvel, gvel)
    for _ in range(2):
        val = step.replay()
        torch.cuda.synchronize()
        assert_close(val, eager_loss, "GraphedStep loss", rel=1e-4, floor=0)
    assert torch.equal(gvel, keep) and torch.equal(step.target_gvel, keep)


def check_data_parallel_step(device, reduced):
    """DataParallelStep(graph=False) at world size 1: the loss of the operator by hand, the gradients in the flat buffer"""
    from cistgcn_amd.runtime import DataParallelStep
    net, x, tgt, gvel, fn = step_setup(device, reduced)
    ref_loss, ref_grads = by_hand(net, x, tgt, gvel, fn)
    step = DataParallelStep(net, x, tgt, graph=False, loss=fn, target_gvel=gvel)
    val = step.replay()
    assert_close(val, ref_loss, "DataParallelStep loss", rel=1e-4, floor=0)
    assert_grads_close({k: p.grad for k, p in net.named_parameters()}, ref_grads, "DataParallelStep")


def check_default_launches(device, reduced):
    """loss=None: one EagerStep.replay() launches cg_mpjpe_fwd / _bwd and no entry point of losses.hip; with a loss it launches those
    in their place"""
    from cistgcn_amd import _lib
    from cistgcn_amd.runtime import EagerStep
    net, x, tgt, gvel, fn = step_setup(device, reduced)

    def names(step):
        step.replay()                  # the first pass of a process sizes the step scratch: record a steady one
        seen, orig = [], _lib.call

        def spy(name, *a):
            seen.append(name)
            return orig(name, *a)
        _lib.call = spy
        try:
            step.replay()
        finally:
            _lib.call = orig
        return seen

    default = names(EagerStep(net, x, tgt))
    assert default.count("cg_mpjpe_fwd") == 1 and default.count("cg_mpjpe_bwd") == 1
    assert not [n for n in default if n.startswith("cg_motion_loss")]
    given = names(EagerStep(net, x, tgt, loss=fn, target_gvel=gvel))
    assert given.count("cg_motion_loss_fwd") == 1 and given.count("cg_motion_loss_bwd") == 1 and "cg_mpjpe_fwd" not in given
    swap = {"cg_motion_loss_fwd": "cg_mpjpe_fwd", "cg_motion_loss_bwd": "cg_mpjpe_bwd"}
    assert [swap.get(n, n) for n in given] == default, "the loss changed more than the two loss launches"
