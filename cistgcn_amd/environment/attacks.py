"""Input-space attacks on the eval-mode model, on the device: counterparts of the reference's robustness tooling
(`environment/adversarial_attacks.py`: FGSM :375-437, IFGSM :442-548, MIFGSM :553-665, DEEPFOOL :668-776, NOATTACK :781-805).

The classes take the reference's constructor keywords, so an `adversarial_attacks:` YAML section maps onto them directly, and
`attack.apply(model, x, target)` returns the adversarial poses.  `x` (B,T,V,3) is the model's own joint set (the `test_mode=False`
branch of `_predict`, test.py:102-103), `target` (B,To,V,3) the ground truth of the predicted frames.

One iteration is: eval-mode forward, `ops.mpjpe_per_sample` (one loss per sample), backward to the input with a DEVICE vector of
per-sample weights as root gradient, `ops.attack_step` (sign / momentum step with the per-sample epsilon, the reference's reset
"projection", the early-stop bookkeeping).  Nothing in it reads a value back to the host.

Fixed batch shape.  The reference re-slices the batch to the samples that are still optimised and takes the mean loss over them
(:518-521).  Here the batch keeps its shape and sample b enters the loss with weight w_b = 1/B while it is active and 0 once it is
frozen.  The update only uses the sign of the gradient (I-FGSM) or the gradient divided by its own L1 norm per sample (MI-FGSM); both
are unchanged by a positive rescaling, and in eval mode the samples are independent (every BatchNorm uses running statistics), so
this yields the same adversarial input - and an iteration whose shapes never change can be captured in a HIP graph
(`runtime.GraphedAttack`).  With every sample active the gradient is exactly that of the reference's full mean.

Deviation: an active sample whose gradient is all zero keeps its momentum and its poses in MI-FGSM; the reference divides by the
zero L1 norm and writes NaN.
"""
import torch

from .. import ops

PATIENCE = 5      # iterations without a higher loss before a sample is frozen (the literal of adversarial_attacks.py:538)


def _check_typ_eval(typ_eval):
    # `_get_bound_per_sample` (:344-365) asserts typ_eval in ["max_val", "len_y"], but "max_val" matches none of its branches:
    # "len_y" is the only bound the attacks can run with.
    if typ_eval != "len_y":
        raise ValueError("attacks: typ_eval=%r is not supported; the only bound is 'len_y' (epsilon times the y extent of the sample)" % (typ_eval,))


def selection_mask(T, V, joints=None, frames=None, device=None):
    """(T,V) float mask of the joints and frames an attack may move (:473-483); None when everything may move."""
    if joints is None and frames is None:
        return None
    m = torch.ones(T, V, dtype=torch.float32)
    if joints is not None:
        keep = torch.zeros(V, dtype=torch.float32)
        idx = torch.as_tensor(list(joints), dtype=torch.long)
        if idx.numel() and (int(idx.min()) < -V or int(idx.max()) >= V):
            raise IndexError("attacks: joint index out of range for %d joints" % V)
        keep[idx] = 1.0
        m = m * keep[None, :]
    if frames is not None:
        keep = torch.zeros(T, dtype=torch.float32)
        idx = torch.as_tensor(list(frames), dtype=torch.long)
        if idx.numel() and (int(idx.min()) < -T or int(idx.max()) >= T):
            raise IndexError("attacks: frame index out of range for %d frames" % T)
        keep[idx] = 1.0
        m = m * keep[:, None]
    return m.contiguous().to(device)


def loss_and_input_grad(model, x, target, w, with_pred=False):
    """Eval-mode forward, one loss per sample and d(sum_b w_b loss_b)/dx.  `x` is a leaf that requires grad; the parameters'
    `.grad` are not touched.  Returns (loss (B,), grad like x), both detached; with `with_pred` also the prediction of this pass
    (B,To,V,3), detached and contiguous."""
    from ..runtime import _drop_graph_attributes
    pred, = model(x)
    loss = ops.mpjpe_per_sample(pred, target)
    grad, = torch.autograd.grad(loss, x, grad_outputs=w)
    _drop_graph_attributes(model)      # the interpretation attributes would keep this pass's autograd graph alive
    grad = grad if grad.is_contiguous() else ops._copy(grad)
    if not with_pred:
        return loss.detach(), grad
    pred = pred.detach()
    return loss.detach(), grad, pred if pred.is_contiguous() else ops._copy(pred)


class _Attack:
    mode = None

    def __init__(self, typ_eval="len_y", *, epsilon=0.01, iterations=1, mu=0.01, joints=None, frames=None, db="h36m"):
        """The union of the reference's constructor keywords (:376, :443, :554, :786); a class ignores the ones its attack has no
        use for (`iterations` / `mu` in FGSM, everything but `typ_eval` in NoAttack), an unknown keyword is a TypeError.  Keyword-only
        behind `typ_eval`: the reference's classes order their positional parameters differently from one another."""
        _check_typ_eval(typ_eval)
        self.typ_eval = typ_eval
        self.epsilon = float(epsilon)
        self.iterations = int(iterations)
        self.mu = float(mu)
        self.joints = None if joints is None else [int(j) for j in joints]
        self.frames = None if frames is None else [int(f) for f in frames]
        self.db = db                      # accepted for YAML compatibility; the joint set is the model's own
        self.poll_every = 4               # iterations between two looks at the device's count of active samples
        if self.iterations < 1:
            raise ValueError("attacks: iterations must be >= 1, got %d" % self.iterations)

    # ---- pieces shared with runtime.GraphedAttack ---------------------------------------------------------------
    def mask(self, x):
        return selection_mask(x.shape[1], x.shape[2], self.joints, self.frames, x.device)

    def new_momentum(self, x):
        if self.mode != "mifgsm":
            return None
        g = torch.empty_like(x)
        ops._lib.call("cg_zero", ops._ptr(g), g.numel() * 4, ops._stream(g))
        return g

    def step(self, x_i, x0, grad, loss, state, mask, g):
        ops.attack_step(self.mode, x_i, x0, grad, self.epsilon, iterations=self.iterations, mu=self.mu, mask=mask, g=g, loss=loss,
                        state=state, patience=PATIENCE)

    def iterate(self, model, x_i, x0, target, state, mask, g):
        """One iteration on the leaf `x_i`: what `_apply` loops over and `runtime.GraphedAttack` captures."""
        loss, grad = loss_and_input_grad(model, x_i, target, state.w)
        self.step(x_i.detach(), x0, grad, loss, state, mask, g)

    @staticmethod
    def _prepare(x, target):
        if x.dim() != 4 or x.shape[-1] != 3 or target.dim() != 4 or target.shape[0] != x.shape[0]:
            raise ValueError("attacks: expected x (B,T,V,3) and target (B,To,V,3), got %s and %s" % (tuple(x.shape), tuple(target.shape)))
        x0 = x.detach()
        return x0.contiguous(), target.detach().contiguous()

    def apply(self, model, x, target):
        """{"adv_inputs": (B,T,V,3) on the device, "queries": (B,) model calls per sample, "loss": (B,) highest loss seen}.  The model
        runs in eval mode for the call and gets its mode back; parameters, their gradients, buffers and the dropout seed are untouched.
        At most one host synchronisation per `poll_every` iterations (the early exit once every sample is frozen), none otherwise."""
        was_training = model.training
        model.eval()
        try:
            return self._apply(model, *self._prepare(x, target))
        finally:
            model.train(was_training)
            from ..runtime import _drop_graph_attributes
            _drop_graph_attributes(model)

    def metrics(self, adv, orig, queries=None):
        """The reference's "adversarial_metrics" dictionary for this batch (`_get_metrics(adv_inputs, inputs)`, test.py:205;
        adversarial_attacks.py:187-342): how far `adv` (B,T,V,3) moved from the clean `orig`.  "metric_type" is `typ_eval`, "queries" the
        given per-sample vector (`apply(...)["queries"]`) or 0 as for the one-step attacks (:154), and the 33 numeric entries of
        `ops.ATTACK_METRICS` are numpy fp32, computed by `ops.attack_metrics` and fetched with one device-to-host copy.  The reference's
        velocity-input branch (:238-301) serves MlpMixer only and has no counterpart."""
        flat, layout, _, _ = ops._attack_metrics_flat(adv.detach(), orig.detach())
        host = flat.cpu().numpy()
        res = {"metric_type": self.typ_eval, "queries": 0 if queries is None else queries}
        for k, (at, shape) in layout.items():
            res[k] = host[at:at + (shape[0] if shape else 1)].reshape(shape)
        return res

    def _apply(self, model, x0, target):
        B = x0.shape[0]
        state = ops.AttackState(B, x0.device)
        x_i = x0.clone().requires_grad_(True)      # a leaf the step kernel rewrites in place between two passes
        mask, g = self.mask(x0), self.new_momentum(x0)
        for k in range(self.iterations):
            self.iterate(model, x_i, x0, target, state, mask, g)
            done = k + 1
            if done >= PATIENCE and done < self.iterations and done % self.poll_every == 0 and int(state.n_active.item()) == 0:
                break
        return {"adv_inputs": x_i.detach(), "queries": state.queries, "loss": state.best}


class FGSM(_Attack):
    """One signed step of epsilon times the sample's y extent (:375-437).  No reset, no bookkeeping; `queries` stays 0."""
    mode = "fgsm"

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.iterations = 1

    def _apply(self, model, x0, target):
        B = x0.shape[0]
        x_i = x0.clone().requires_grad_(True)
        w = (torch.ones(B, dtype=torch.float32) / B).to(x0.device)
        loss, grad = loss_and_input_grad(model, x_i, target, w)
        ops.attack_step("fgsm", x_i.detach(), x0, grad, self.epsilon, mask=self.mask(x0))
        return {"adv_inputs": x_i.detach(), "queries": torch.zeros(B, dtype=torch.int32, device=x0.device), "loss": loss}


class IFGSM(_Attack):
    """Iterated signed steps of epsilon / iterations times the y extent of the current iterate (:442-548)."""
    mode = "ifgsm"


class MIFGSM(_Attack):
    """The same with a momentum of L1-normalised gradients (:553-665)."""
    mode = "mifgsm"


class DEEPFOOL(_Attack):
    """The reference's DeepFool for multi-output regression (:668-776), the one attack of the family that steps in proportion to the
    gradient: per iteration and sample r = -grad * (mean of the prediction over its frames) / (||grad||_1 + 1e-10), x = x + mask * r
    (`ops.deepfool_step`).  No epsilon and no projection; queries, the highest loss and the freeze after 5 iterations without a higher
    loss are IFGSM's.  What is kept and what is dropped of the reference:

    * `overshoot` is accepted and stored; the reference never reads it either.
    * The `_init_func` call in front of the reference's loop (:739) is not made: in eval mode its prediction is overwritten in
      iteration 0 and its gradient only doubles that of iteration 0, which the L1 normalisation removes.  `queries` never counted it.
    * The prediction's joints are broadcast onto the input's (:699), so the model's output must have the input's V: ValueError else.
    * With `frames=None` the reference resets its mask to all ones and so ignores a joints-only selection (:709-710, as IFGSM does at
      :481-482).  Here `selection_mask` is used unchanged, as in the other attacks: joints-only restricts the joints.
    * Deviation: the reference differentiates the mean loss of the samples still optimised, here sample b enters with the fixed
      weight 1/B (the fixed batch shape above).  r is unchanged by that rescaling except through the 1e-10 beside the L1 norm:
      relative 1e-9 at the ||grad||_1 of about 0.1 of the recorded model.
    * A frozen sample does not move, and an all-zero gradient gives r = 0 / 1e-10 = 0, as in the reference."""
    mode = "deepfool"

    def __init__(self, typ_eval="len_y", *, iterations=10, overshoot=0.02, joints=None, frames=None, db="h36m"):
        super().__init__(typ_eval, iterations=iterations, joints=joints, frames=frames, db=db)
        self.overshoot = float(overshoot)

    @staticmethod
    def _prepare(x, target):
        x0, target = _Attack._prepare(x, target)
        if target.shape[2] != x0.shape[2]:
            raise ValueError("attacks: DEEPFOOL broadcasts the predicted joints onto the input's and needs V_in == V_out, got %d and %d"
                             % (x0.shape[2], target.shape[2]))
        return x0, target

    def iterate(self, model, x_i, x0, target, state, mask, g):
        loss, grad, pred = loss_and_input_grad(model, x_i, target, state.w, with_pred=True)
        ops.deepfool_step(x_i.detach(), grad, pred, mask=mask, loss=loss, state=state, patience=PATIENCE)


DeepFool = DEEPFOOL


class NoAttack(_Attack):
    """Returns the input unchanged together with dL/dx of the full-mean loss (:781-805, where the gradient is left on the input)."""
    mode = "none"

    def __init__(self, typ_eval="len_y", db="h36m", **kwargs):      # the reference's NOATTACK takes and drops any keyword (:786)
        super().__init__(typ_eval=typ_eval, db=db)

    def _apply(self, model, x0, target):
        B = x0.shape[0]
        x_i = x0.clone().requires_grad_(True)
        w = (torch.ones(B, dtype=torch.float32) / B).to(x0.device)
        loss, grad = loss_and_input_grad(model, x_i, target, w)
        return {"adv_inputs": x_i.detach(), "queries": torch.zeros(B, dtype=torch.int32, device=x0.device), "loss": loss, "grad": grad}


NOATTACK = NoAttack      # the reference's spelling, as an `adversarial_attacks:` YAML section names it

_BY_NAME = {"FGSM": FGSM, "IFGSM": IFGSM, "MIFGSM": MIFGSM, "DEEPFOOL": DEEPFOOL, "DeepFool": DEEPFOOL, "NOATTACK": NoAttack,
            "NoAttack": NoAttack}


def from_config(section):
    """`{"IFGSM": {"epsilon": 0.01, "iterations": 10, ...}}` (one `adversarial_attacks:` entry of an evaluation YAML) -> the attack."""
    if len(section) != 1:
        raise ValueError("attacks.from_config: expected one attack name with its keywords, got %s" % sorted(section))
    (name, kw), = section.items()
    if name not in _BY_NAME:
        raise ValueError("attacks.from_config: unknown attack %r (have %s)" % (name, sorted(_BY_NAME)))
    return _BY_NAME[name](**dict(kw or {}))
