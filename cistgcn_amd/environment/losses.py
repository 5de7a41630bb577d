"""The loss selection of the reference's training iteration (`get_loss`, environment/train.py:15-43, and the per-batch weights of
train.py:62-71) over `ops.mpjpe` / `ops.motion_loss`.

`learning_config.loss.type` is `mpjpe`, `weighted_mpjpe` / `w_mpjpe`, `rmpjpe`, `mpjpe_soft` or `weighted_mpjpe_soft` / `w_mpjpe_soft`;
`learning_config.loss.weights` may name a frame ramp (`linear`, `sqrt`, `exp`, `square`) and / or `speed[N]`, which weights every joint
by its speed (`target_gvel[..., 0]`) over the largest speed of its frame, times N (the first run of digits of the string, 1 without).

Deviations from the reference, both on purpose:
* `target_gvel` is read-only here.  The reference normalises it in place (`speeds /= ...` on a view of the batch's tensor, train.py:66),
  so a caller that looks at `target_gvel` after the loss finds it divided there and untouched here.
* An unknown `loss.type` raises ValueError when the object is built.  The reference evaluates a bare `NotImplemented` (train.py:27-28)
  and fails a line later with an unbound local name.
"""
import re

import torch

from .. import ops

# `loss.type` -> kind of `ops.motion_loss` (None: plain `ops.mpjpe`), train.py:17-26
LOSS_TYPES = {"mpjpe": None, "weighted_mpjpe": "weighted_mpjpe", "w_mpjpe": "weighted_mpjpe", "rmpjpe": "rmpjpe", "mpjpe_soft": "mpjpe_soft",
              "weighted_mpjpe_soft": "weighted_mpjpe_soft", "w_mpjpe_soft": "weighted_mpjpe_soft"}


def frame_weights(weights_string, T):
    """The per-frame table of `get_loss` (train.py:29-40) as a float32 host tensor (T,): `arange(1, T + 1)`, which `linear` leaves as it
    is, then the first of `sqrt`, `exp`, `square` the string contains, by the reference's own expressions on the host - the bits the
    reference uploads (its `.float()` of train.py:62 included)."""
    weights = torch.arange(1, int(T) + 1)
    w_vals = str(weights_string)
    if "sqrt" in w_vals:
        weights = torch.sqrt(weights)
    elif "exp" in w_vals:
        weights = torch.exp(weights / (weights.max() / 5))
    elif "square" in w_vals:
        weights = torch.pow(weights / (weights.max() / 5), 2)
    return weights.float()


class TrainingLoss:
    """`loss(pred, target, target_gvel=None)` -> the scalar training loss of `learning_config.loss` for predictions of `output_n` frames.
    The frame table is built and uploaded once; a call is the two launches of the forward (`ops.motion_loss`; `type: mpjpe` is the
    existing `ops.mpjpe`), its backward one.  With `speed` in the weights string `target_gvel` ((B,T,V,1) or (B,T,V)) is required
    (ValueError without) and is not written - see the module docstring for this and the other deviation."""

    def __init__(self, learning_config, output_n, device):
        cfg = learning_config.loss
        self.type, self.weights = str(cfg.type), str(getattr(cfg, "weights", "") or "")
        if self.type not in LOSS_TYPES:
            raise ValueError("loss.type %r: expected one of %s" % (self.type, ", ".join(sorted(LOSS_TYPES))))
        self.kind = LOSS_TYPES[self.type]
        self.uses_speed = "speed" in self.weights                      # train.py:50, :63
        digits = re.findall(r"\d+", self.weights)                      # train.py:52-53
        self.speed_factor = float(digits[0]) if self.uses_speed and digits else 1.0
        self.speed_only = self.weights == "speed"                      # train.py:67-68: the speeds replace the table
        self.output_n = int(output_n)
        self.frame_weights = frame_weights(self.weights, self.output_n).to(device)
        self.weighted = self.kind in ops._WEIGHTED_LOSSES

    def __call__(self, pred, target, target_gvel=None):
        if self.uses_speed and target_gvel is None:
            raise ValueError("loss.weights %r weights the joints by their speed: target_gvel is required" % self.weights)
        if self.kind is None:               # `ops.mpjpe` differentiates its first argument; train.py:76 passes (target, output)
            return ops.mpjpe(target, pred) if target.requires_grad and not pred.requires_grad else ops.mpjpe(pred, target)
        if not self.weighted:
            return ops.motion_loss(self.kind, pred, target)
        speeds = None
        if self.uses_speed:
            speeds = target_gvel[:, :, :, 0] if target_gvel.dim() == 4 else target_gvel                 # train.py:64
        return ops.motion_loss(self.kind, pred, target, frame_weights=None if self.speed_only else self.frame_weights,
                               speeds=speeds, speed_factor=self.speed_factor)


def get_loss(learning_config, output_n, device):
    """The reference's name (train.py:15) for `TrainingLoss(learning_config, output_n, device)`."""
    return TrainingLoss(learning_config, output_n, device)
