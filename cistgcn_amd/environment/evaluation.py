"""Evaluation-harness counterparts around the model; the joint gather / scatter and the per-frame
MPJPE kernel live in `ops.gather_joints` / `ops.eval_scatter_mpjpe`.

* `capture_interpretation`: `environment/test.py:146-157` - after a forward, every dotted key of
  `evaluation_config.interpretation.layers` (predict.yaml:162-197) is resolved attribute by attribute on the model and
  appended as `squeeze().cpu().numpy()`; a key the model does not have prints "<key> is not available on model" and is
  skipped (model sizes differ in the number of blocks).
* `save_interpretation`: the `.npy` dictionary the reference's figure scripts read back with `np.load(..., allow_pickle=True).all()`
  (figures_temp.py:54-69): {action: {"interpretation": {key: [arrays]}}}.
* `mpjpe_ms_table`: the per-horizon line of `train.py:40-43`: frames are 40 ms apart, indices [1, 4, 9, 13, 17, 24] of a
  25-frame prediction (80 ... 1000 ms), [1, 4, 9] of a 10-frame one.
* `EvalMetrics`: `Metrics` + `LossOperator` + the result dictionary of `test()` (`environment/test.py:11-63`, `:315-334`;
  `losses/losses.py:13-33`) over `ops.eval_metrics`: one operator call per batch, the results stay on the device until `result()`.
"""
import numpy as np
import torch

from .. import ops


def capture_interpretation(model, interpretation_keywords, store=None):
    store = {} if store is None else store
    for key in interpretation_keywords or ():
        try:
            obj = model
            for part in key.split("."):
                obj = getattr(obj, part)
            value = obj.detach().squeeze().cpu().numpy()
        except Exception:
            print("%s is not available on model" % key)
            continue
        store.setdefault(key, []).append(value)
    return store


def save_interpretation(path, store, action="all"):
    np.save(path, {action: {"interpretation": store}}, allow_pickle=True)
    return path


def mpjpe_ms_table(mpjpe_seq):
    """(values at the reported horizons as {ms: error}, the reference's printed line)"""
    v = np.asarray(mpjpe_seq, dtype=np.float64).reshape(-1)
    idx = [1, 4, 9, 13, 17, 24] if len(v) > 10 else [1, 4, 9]
    idx = [i for i in idx if i < len(v)]
    cells = ["%d:%.2f," % (40 * (i + 1), v[i]) for i in idx]
    return {40 * (i + 1): float(v[i]) for i in idx}, "mpjpe: " + " ".join(cells)


class EvalMetrics:
    """Accumulates the metrics of an evaluation pass.  `bones`: the (i,j) joint pairs of the skeleton the loader uses (the
    reference looks them up by data-set name, `utils/body_utils.py::get_reduced_skeleton`; here the caller passes them).
    `compute_joint_error` as in `test()` (:303-304): False keeps one value per frame and batch, True one per joint and sample.
    `mae` / `mae_seq` of the reference are not computed."""

    def __init__(self, bones, compute_joint_error=False):
        self.bones = [(int(i), int(j)) for i, j in bones]
        self.compute_joint_error = bool(compute_joint_error)
        self.batches = {k: [] for k in ops.EVAL_METRICS}
        self.frame_shape = None

    def update(self, pred, target, speeds):
        """One batch: pred / target (B,To,J,3), speeds (B,To,J).  B may differ between batches, To and J may not.  No host
        synchronisation."""
        if self.frame_shape is None:
            self.frame_shape = tuple(pred.shape[1:3])
        if tuple(pred.shape[1:3]) != self.frame_shape:
            raise ValueError("EvalMetrics.update: this batch has (To,J) = %s, earlier ones had %s" % (tuple(pred.shape[1:3]), self.frame_shape))
        res = ops.eval_metrics(pred, target, speeds, self.bones, reduce=None if self.compute_joint_error else "frames")
        for k, v in res.items():
            self.batches[k].append(v)

    def result(self):
        """{name: scalar, name_seq: array} with the reference's keys (test.py:315-334).  `*_seq`: the mean over the batches of the
        per-frame values (`LossOperator.mean(0)`, not weighted by batch size) or, with `compute_joint_error`, the per-joint values of
        all samples (`get_all`); the scalar is the mean of all entries.  One device-to-host copy."""
        if not self.batches["mpjpe"]:
            raise ValueError("EvalMetrics.result: no batch has been added")
        stacked = {k: (torch.cat(v, 0) if self.compute_joint_error else torch.stack(v, 0)) for k, v in self.batches.items()}
        sizes = [t.numel() for t in stacked.values()]
        host = torch.cat([t.reshape(-1) for t in stacked.values()]).cpu().numpy()
        out, at = {}, 0
        for (k, t), n in zip(stacked.items(), sizes):
            arr = host[at:at + n].reshape(tuple(t.shape))
            at += n
            out[k] = arr.mean(dtype=np.float64)
            out[k + "_seq"] = arr if self.compute_joint_error else arr.mean(0, dtype=np.float64)
        return out
