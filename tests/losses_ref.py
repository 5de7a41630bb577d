"""Restatement in stock torch of the training losses and their weights (reference: losses/losses.py rmpjpe :36-47, weighted_mpjpe
:64-76, mpjpe_soft :241-252, weighted_mpjpe_soft :255-267; environment/train.py get_loss :15-43, the batch weights :62-71), in the dtype
of its arguments: fp64 it is the reference the kernels of csrc/losses.hip are held to, fp32 it is pinned itself by the recording of
the real reference (tests/golden/eval_losses.npz, tools/gen_golden_losses.py).  Nothing here is written in place."""
import re

import torch

KINDS = ("weighted_mpjpe", "mpjpe_soft", "weighted_mpjpe_soft", "rmpjpe")
WEIGHTED = ("weighted_mpjpe", "weighted_mpjpe_soft")
SOFT = ("mpjpe_soft", "weighted_mpjpe_soft")
# loss.type of the YAML -> kind ("mpjpe": the plain mean)
TYPES = {"mpjpe": "mpjpe", "weighted_mpjpe": "weighted_mpjpe", "w_mpjpe": "weighted_mpjpe", "rmpjpe": "rmpjpe", "mpjpe_soft": "mpjpe_soft",
         "weighted_mpjpe_soft": "weighted_mpjpe_soft", "w_mpjpe_soft": "weighted_mpjpe_soft"}


def frame_table(weights_string, T, dtype=torch.float32):
    """the per-frame table: 1..T, then the first of sqrt / exp / square the string names ("linear" changes nothing)"""
    t = torch.arange(1, T + 1).to(dtype)
    if "sqrt" in weights_string:
        t = t.sqrt()
    elif "exp" in weights_string:
        t = (t / (t.max() / 5)).exp()
    elif "square" in weights_string:
        t = (t / (t.max() / 5)) ** 2
    return t


def speed_factor(weights_string):
    digits = re.findall(r"\d+", weights_string)
    return float(digits[0]) if digits else 1.0


def joint_weights(base, speeds, factor):
    """base (broadcastable to (B,T,V)) or None, plus factor * speeds / (max over the joints of the frame + 1e-6); speeds (B,T,V) or None"""
    if speeds is None:
        return base
    sn = speeds / (speeds.max(2, keepdim=True)[0] + 1e-6)
    return sn * factor if base is None else base + sn * factor


def batch_weights(weights_string, shape, target_gvel, dtype=torch.float32):
    """w (B,T,V) of train.py:62-71 for a weights string; target_gvel (B,T,V,1)"""
    B, T, V = shape
    base = frame_table(weights_string, T, dtype)[None, :, None].expand(B, T, V)
    if "speed" not in weights_string:
        return base.clone()
    return joint_weights(None if weights_string == "speed" else base, target_gvel[:, :, :, 0].to(dtype), speed_factor(weights_string))


def joint_error(kind, pred, target):
    d = pred - target
    if kind in SOFT:
        a = d.abs()
        d = torch.where(a < 1, 0.5 * d * d, a - 0.5)
    return torch.linalg.vector_norm(d, 2, dim=-1)      # its gradient at 0 is 0


def loss(kind, pred, target, w=None):
    e = joint_error(kind, pred, target)
    if kind in WEIGHTED:
        return (w * e).mean()
    return e.mean().sqrt() if kind == "rmpjpe" else e.mean()


def loss_and_grad(kind, pred, target, w=None, dtype=torch.float64):
    """(loss, d loss / d pred) evaluated in `dtype` on the given (fp32) inputs"""
    p = pred.detach().cpu().to(dtype).requires_grad_(True)
    val = loss(kind, p, target.detach().cpu().to(dtype), None if w is None else w.detach().cpu().to(dtype))
    val.backward()
    return val.detach(), p.grad
