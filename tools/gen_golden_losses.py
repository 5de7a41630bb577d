#!/usr/bin/env python
"""Golden vectors of the training losses from the REAL reference: its own `train()` (environment/train.py:46-120) driven for one
iteration per case, so that `get_loss` (:15-43) and the weight construction (:62-71) are the reference's own lines.  Build container
only, like tools/gen_golden_eval.py: the reference is imported at generation time, this script writes arrays only.

What stands in for the rest of a training run: the loader yields one dictionary (and its iterator has `_next_data`, which `get_loss`
reads the shapes from), the model returns `(leaf_pred,)` - a leaf tensor that requires a gradient - the optimizer and the scheduler do
nothing, and the writer keeps what `add_scalar` is given.  `leaf_pred.grad` after the call is the recorded gradient.  Two things are
added around the reference's lines without changing them: `Tensor.cuda()` returns the tensor itself (everything runs on the CPU, as in
tools/gen_golden_metrics.py), and the loss functions of `losses.losses` are wrapped by a recorder that keeps the `w` they are called
with and calls them unchanged.

tests/golden/eval_losses.npz: `pred`, `target` (B,T,V,3), `target_gvel` (B,T,V,1) fp32, shared by all cases (B,T,V = 3,5,4; the loader gets
a copy of `target_gvel`: the reference divides it in place); `types`, `weights`: the strings; per case `<type>|<weights>`:
`/loss` (what `add_scalar('losses/loss_pose', ...)` received), `/grad` (B,T,V,3), `/w` (B,T,V) and `/table` (T,) (the frame table of
`get_loss` after the `.float()` of train.py:62).  Note that train.py:76 calls `loss_func(target, output, w=w)`.

Inputs as the tests draw them (tests/losses_checks.py::draw): differences with per-coordinate standard deviations (0.3, 3, 30) around
targets of scale 300 (both SmoothL1 branches), one joint per sample equal to its target, one frame with all-zero speeds.
"""
import importlib
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
torch.Tensor.cuda = lambda self, *a, **k: self          # train() and get_loss() call .cuda(); everything here runs on the CPU
pkg = types.ModuleType("human_motion_prediction")
pkg.__path__ = ["/root/reference/human_motion_prediction"]
sys.modules["human_motion_prediction"] = pkg
ref_train = importlib.import_module("human_motion_prediction.environment.train")
ref_losses = ref_train.losses

import losses_checks as LC      # noqa: E402  (the draw of the inputs only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "eval_losses.npz")
TYPES = ("mpjpe", "weighted_mpjpe", "w_mpjpe", "rmpjpe", "mpjpe_soft", "weighted_mpjpe_soft", "w_mpjpe_soft")
WEIGHTS = ("", "linear", "sqrt", "exp", "square", "speed", "speed2_sqrt", "speed_linear")
SEEN = {}


def recorder(fn):
    def call(predicted, target, w=None, **kw):
        SEEN["w"] = w.detach().clone()
        return fn(predicted, target, w=w, **kw)
    return call


for name in ("mpjpe", "weighted_mpjpe", "rmpjpe", "mpjpe_soft", "weighted_mpjpe_soft"):
    setattr(ref_losses, name, recorder(getattr(ref_losses, name)))


class Loader:
    def __init__(self, item):
        self.item = item

    def __len__(self):
        return 1

    def __iter__(self):
        it = iter([self.item])
        return type("It", (), {"_next_data": lambda s: self.item, "__iter__": lambda s: s, "__next__": lambda s: next(it)})()


class Model:
    def __init__(self, pred):
        self.pred = pred

    def train(self):
        return self

    def __call__(self, inputs):
        return (self.pred,)


class Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, name, value, step):
        self.scalars[name] = value


NOOP = NS(zero_grad=lambda: None, step=lambda: None, param_groups=[{"lr": 0.0}])


def run(kind, weights, pred, target, gvel):
    leaf = pred.clone().requires_grad_(True)
    item = {"sample": torch.zeros(pred.shape[0], 2, pred.shape[2], 3), "target": target.clone(), "target_vel": torch.zeros_like(target),
            "target_gvel": gvel.clone()}
    cfg = NS(loss=NS(type=kind, weights=weights))
    writer = Writer()
    ref_train.train(Loader(item), Model(leaf), NOOP, NOOP, writer=writer, learning_config=cfg, epoch=0)
    _, table = ref_train.get_loss(Loader(item), cfg)
    return {"loss": np.float32(writer.scalars["losses/loss_pose"]), "grad": leaf.grad.numpy().copy(), "w": SEEN["w"].float().numpy().copy(),
            "table": table[0, :, 0].float().numpy().copy()}


def main():
    pred, target, gvel = LC.draw((3, 5, 4), seed=11)
    rec = {"pred": pred.numpy(), "target": target.numpy(), "target_gvel": gvel.numpy(), "types": np.array(TYPES), "weights": np.array(WEIGHTS)}
    for kind in TYPES:
        for weights in WEIGHTS:
            for k, v in run(kind, weights, pred, target, gvel).items():
                rec["%s|%s/%s" % (kind, weights, k)] = v
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes,", len(TYPES) * len(WEIGHTS), "cases")


if __name__ == "__main__":
    main()
