"""On-device input pipeline: the reference augments every sequence on the DataLoader's CPU
workers (scipy `Rotation`, one Python call chain per sample; `num_workers = 0` in the shipped YAMLs,
train_h36m.yaml:86) and copies the finished batch with `.cuda()` (`environment/train.py:57-58`).  Here the raw windows go
to the GPU once, one kernel augments the whole batch and emits the per-item tensors of `H36m_Motion3D.__getitem__`
(`loaders/h36m_motion_3d.py:94-108`), and the next batch's host->device copy runs on a side stream under the current step.

`DeviceAugmentation(opt_trs)` takes the same `learning_config.augmentations` section as `loaders/loader.py::
get_transformations` (:42-130) and keeps its order: flip, rotation, scale, noise, translation, pose inversion.  The random
numbers are drawn on the host with `np.random.uniform` in exactly the order the reference's transform objects would draw them for
the samples of the batch one after the other, so a seeded run reproduces the reference's augmentations; the data-dependent parts
(centroids, extents, the rotation itself) run on the device.  `RandomNoise` (custom_transforms.py:350-400) and `RandomPoseInvers`
(:301-347) are taken in their whole-sequence form; the `seq_idx` / `continuous` variants (unused by the shipped YAML) raise.

`RobustnessTest(opt_trs)` is the other user of these transforms: the `robustness_test:` section of an evaluation YAML
(`loaders/loader.py:75-127`), where every transform also has a frame window (`seq_idx`), may ramp in linearly (`continuous`) and
persists behind its window or stops there (`keep`), and where the order of the kinds is no longer fixed.  It drives a second kernel
that executes a step list (cg_perturb_sequences); the draws, the outputs and the two methods are those of `DeviceAugmentation`.
"""
import ctypes

import numpy as np
import torch

from .. import _lib, ops

NPAR = 24

# RandomPoseInvers: body_utils.get_reduced_skeleton("h36m", inverse=True) (utils/body_utils.py:167-170) - pairs of the 32-joint
# H3.6M skeleton.  (The reference applies them to whatever tensor it is given: a 22-joint sequence raises IndexError there, and here.)
H36M_INVERSE_PAIRS = ((6, 1), (7, 2), (8, 3), (9, 4), (10, 5), (16, 24), (17, 25), (18, 26), (19, 27), (20, 28), (22, 30), (21, 29), (23, 31))


def _range(v, what):
    """the reference's constructors: a scalar means the degenerate interval [v, v], '' / None / 0 means [0, 0]"""
    if v is None or v == "" or v is False:
        return None
    if isinstance(v, (int, float)):
        return (float(v), float(v))
    v = list(v)
    if len(v) != 2:
        raise ValueError("augmentation %s: expected [low, high], got %r" % (what, v))
    return (float(v[0]), float(v[1]))


def _rotvec_matrix(deg):
    """Rotation matrix of a rotation vector given in degrees (what scipy's `Rotation.from_rotvec(., degrees=True).as_matrix()`
    returns; Rodrigues' formula in f64)."""
    v = np.deg2rad(np.asarray(deg, dtype=np.float64))
    th = float(np.linalg.norm(v))
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _item_tensors(raw, input_n, keep_processed, out):
    """the five output tensors of a batch (new ones, or the dictionary `out` of an earlier call after a shape check) and `processed`"""
    B, L, J, _ = raw.shape
    dev, f32, To = raw.device, torch.float32, L - input_n
    shapes = {"sample": (B, input_n, J, 3), "target": (B, To, J, 3), "target_vel": (B, To, J, 3), "target_gvel": (B, To, J, 1),
              "sample_vel": (B, input_n, J, 3)}
    if out is None:
        out = {k: torch.empty(shp, dtype=f32, device=dev) for k, shp in shapes.items()}
    else:
        for k, shp in shapes.items():
            t = out.get(k)
            if t is None or tuple(t.shape) != shp or t.dtype != f32 or t.device != dev or not t.is_contiguous():
                raise ValueError("out[%r] must be a contiguous float32 %s tensor on %s" % (k, shp, dev))
        out = {k: out[k] for k in shapes}
    proc = torch.empty(B, L, J, 3, dtype=f32, device=dev) if keep_processed else None
    return out, proc


def _draw_device(steps, layout, batch, joints, device, stream, out):
    """the step list as descriptors of `ops.draw_augmentation`, one launch, the result in the form of the host `draw`"""
    desc = []
    for st in steps:
        if st.kind == "flip":
            lo, hi = [1.0 if a else 0.0 for a in st.ranges], (0.0, 0.0, 0.0)
        elif st.kind == "noise":
            lo, hi = (float(st.ranges), 0.0, 0.0), (0.0, 0.0, 0.0)
        elif st.kind == "invert":
            lo = hi = (0.0, 0.0, 0.0)
        else:
            lo, hi = [r[0] for r in st.ranges], [r[1] for r in st.ranges]
        desc.append((st.kind, st.prob_threshold, lo, hi))
    n_noise = sum(st.kind == "noise" for st in steps)
    if n_noise and joints is None:
        raise ValueError("draw_device: RandomNoise draws one number per joint and axis: pass joints=")
    tab = noise = None
    if out is not None:
        tab, noise = (out["params"], out["noise"]) if isinstance(out, dict) else (out, None)
        if noise is not None and layout == "table24":
            noise = noise.view(int(batch), 1, int(joints), 3)
    if tab is None and noise is None:
        tab, noise = ops.draw_augmentation(desc, batch, joints, layout, stream=stream, device=device)
    else:
        tab, noise = ops.draw_augmentation(desc, batch, joints, layout, stream=stream, out=tab, noise_out=noise)
    if not n_noise:
        return tab
    return {"params": tab, "noise": noise.view(int(batch), int(joints), 3) if layout == "table24" else noise}


class _Step:
    def __init__(self, kind, ranges, prob_threshold):
        self.kind, self.ranges, self.prob_threshold = kind, ranges, float(prob_threshold)


class DeviceAugmentation:
    def __init__(self, opt_trs=None):
        self.steps = []
        if opt_trs is None:
            return

        def section(name):
            s = getattr(opt_trs, name, None)
            return None if (s is None or s == "") else s

        def variant(s, name):
            for k in ("seq_idx", "continuous"):
                if getattr(s, k, None):
                    raise ValueError("augmentation %s.%s is not supported by the on-device pipeline" % (name, k))
            return float(getattr(s, "prob_threshold", 0.5))

        # loaders/loader.py:46-73 then :74-128 - the order of these blocks is the order of the transforms
        for name in ("random_flip", "random_rotation", "random_scale", "random_noise", "random_translation", "rotation", "scale", "noise",
                     "translation", "flip", "pose_invers"):
            s = section(name)
            if s is None:
                continue
            kind = name.replace("random_", "")
            if name == "random_noise":                     # loader.py:62-64: RandomNoise(opt_trs.random_noise), a bare amplitude
                self.steps.append(_Step("noise", float(s), 0.5))
                continue
            if name == "noise":                            # loader.py:97-103
                self.steps.append(_Step("noise", float(s.noise), variant(s, name)))
                continue
            if name == "pose_invers":                      # loader.py:121-125: always the "h36m" skeleton
                self.steps.append(_Step("invert", H36M_INVERSE_PAIRS, variant(s, name)))
                continue
            if kind == "flip":
                axes = tuple(bool(getattr(s, a, "")) for a in "xyz")
                self.steps.append(_Step("flip", axes, variant(s, name)))
                continue
            r = [_range(getattr(s, a, ""), "%s.%s" % (name, a)) for a in "xyz"]
            if all(v is None for v in r):
                continue                                   # the reference skips a transform whose three entries are ''
            self.steps.append(_Step(kind, tuple(v if v is not None else (0.0, 0.0) for v in r), variant(s, name)))

    @property
    def needs_joints(self):
        return any(st.kind in ("noise", "invert") for st in self.steps)

    def draw(self, batch, rng=None, joints=None):
        """(batch, 24) float32 parameter rows (plus the per-joint noise draws when RandomNoise is configured: then the result is a
        dict {"params", "noise"} and `joints` is required); consumes `rng.uniform` (default: the global `np.random`, which is what
        the reference's transforms use) sample by sample, transform by transform, in the reference's order and only where the
        reference draws (the amounts are drawn only when the coin of that transform says 'apply')."""
        rng = np.random if rng is None else rng
        out = np.zeros((batch, NPAR), dtype=np.float32)
        out[:, 13:16] = 1.0
        has_noise = any(st.kind == "noise" for st in self.steps)
        if has_noise and joints is None:
            raise ValueError("DeviceAugmentation.draw: RandomNoise draws one number per joint and axis: pass joints=")
        noise = np.zeros((batch, int(joints), 3), dtype=np.float32) if has_noise else None
        for b in range(batch):
            # composed parameters of this sample, applied by the kernel in the canonical order flip -> rotate -> scale ->
            # translate; the config order is that order (asserted below), repeated kinds compose only if adjacent steps allow
            seen = []
            for st in self.steps:
                if st.kind in seen:
                    raise ValueError("augmentation '%s' configured twice (random_* and explicit): not supported on device" % st.kind)
                seen.append(st.kind)
                if st.kind == "flip":
                    for a in range(3):
                        if st.ranges[a] and rng.uniform() > st.prob_threshold:
                            out[b, a] = 1.0
                    continue
                if not (rng.uniform() > st.prob_threshold):
                    continue
                if st.kind == "noise":                     # custom_transforms.py:368-370: one array draw of (joints, 3) numbers
                    out[b, 19] = st.ranges
                    noise[b] = np.asarray(rng.uniform(-1, 1, (int(joints), 3)), dtype=np.float64).astype(np.float32)
                    continue
                if st.kind == "invert":
                    out[b, 20] = 1.0
                    continue
                vals = [np.float32(rng.uniform(lo, hi)) for lo, hi in st.ranges]
                if st.kind == "rotation":
                    out[b, 3] = 1.0
                    out[b, 4:13] = _rotvec_matrix(vals).astype(np.float32).reshape(-1)
                elif st.kind == "scale":
                    out[b, 13:16] = vals
                else:
                    out[b, 16:19] = vals
            order = [k for k in ("flip", "rotation", "scale", "noise", "translation", "invert") if k in seen]
            if seen != order:
                raise ValueError("augmentation order %s is not the reference's flip/rotation/scale/noise/translation/inversion order" % seen)
        return {"params": out, "noise": noise} if has_noise else out

    def _check_order(self):
        """what `draw` checks per sample, once per call for the device draws"""
        seen = [st.kind for st in self.steps]
        for k in seen:
            if seen.count(k) > 1:
                raise ValueError("augmentation '%s' configured twice (random_* and explicit): not supported on device" % k)
        order = [k for k in ("flip", "rotation", "scale", "noise", "translation", "invert") if k in seen]
        if seen != order:
            raise ValueError("augmentation order %s is not the reference's flip/rotation/scale/noise/translation/inversion order" % seen)

    def draw_device(self, batch, joints=None, device="cuda", stream=0, out=None):
        """What `draw` returns, as device tensors drawn on the device from the seed word of `ops.seed_state` (one launch,
        capturable; `ops.draw_augmentation`): a DIFFERENT random stream than `draw`, which reproduces the reference's `np.random`
        order.  The seed is read, not advanced; `stream` (0 .. 65535) separates independent draws under one seed.  `out`: what an
        earlier call returned, to be filled again (the static buffers of a captured step)."""
        self._check_order()
        return _draw_device(self.steps, "table24", batch, joints, device, stream, out)

    def _perm(self, J, device):
        """joint permutation the reference's sequential pair swaps compose to: output joint j shows joint perm[j]"""
        for st in self.steps:
            if st.kind == "invert":
                idx = list(range(J))
                for x, y in st.ranges:
                    if x >= J or y >= J:
                        raise IndexError("RandomPoseInvers: joint pair (%d, %d) out of range for %d joints (the reference indexes the "
                                         "same way and fails the same way)" % (x, y, J))
                    idx[x], idx[y] = idx[y], idx[x]
                return ops._index_tensor(idx, device)          # uploaded once per permutation and device: the call stays capturable
        return None

    def __call__(self, raw, input_n, params=None, keep_processed=False, out=None, stream=0):
        """raw: (B, L, J, 3) float32 on the HIP device (un-augmented windows of input_n + output_n frames).  Returns the dict
        of `H36m_Motion3D.__getitem__` / `Amass_Motion3D.__getitem__` (the two are the same code) for the batch: sample, sample_vel,
        target, target_vel, target_gvel (and processed on request; "original" is the caller's `raw`, "item" its indices).
        params: what `draw` or `draw_device` returned; None: `draw` (host, the reference's stream); "device": `draw_device` with
        `stream`.  out: a dictionary an earlier call returned, written again instead of new tensors."""
        ops._chk(raw, "raw")
        if raw.dim() != 4 or raw.shape[3] != 3:
            raise ValueError("expected windows of shape (B, L, J, 3), got %s" % (tuple(raw.shape),))
        raw = raw if raw.is_contiguous() else ops._copy(raw)
        B, L, J, _ = raw.shape
        if params is None:
            params = self.draw(B, joints=J)
        elif isinstance(params, str):
            if params != "device":
                raise ValueError("params: a table, None (host draws) or \"device\", got %r" % params)
            params = self.draw_device(B, joints=J, device=raw.device, stream=stream)
        noise = None
        if isinstance(params, dict):
            params, noise = params["params"], params["noise"]
            if isinstance(noise, np.ndarray):
                noise = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(raw.device, non_blocking=True)
            if tuple(noise.shape) != (B, J, 3):
                raise ValueError("expected (%d, %d, 3) noise draws" % (B, J))
        perm = self._perm(J, raw.device)
        if isinstance(params, np.ndarray):
            params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(raw.device, non_blocking=True)
        if tuple(params.shape) != (B, NPAR):
            raise ValueError("expected a (%d, %d) parameter table" % (B, NPAR))
        out, proc = _item_tensors(raw, int(input_n), keep_processed, out)
        _lib.call("cg_augment_sequences", ops._ptr(raw), ops._ptr(params), ops._ptr(out["sample"]), ops._ptr(out["target"]),
                  ops._ptr(out["target_vel"]), ops._ptr(out["target_gvel"]), ops._ptr(proc), ops._ptr(out["sample_vel"]), ops._ptr(noise), ops._ptr(perm),
                  B, L, J, int(input_n), ops._stream(raw))
        if keep_processed:
            out["processed"] = proc
        return out


MAX_STEPS = _lib.LIMITS["CG_PERTURB_MAX_STEPS"]
_KIND = {k: _lib.LIMITS["CG_PERTURB_" + k.upper()] for k in ("rotation", "scale", "noise", "translation", "flip", "invert")}


class _WindowStep(_Step):
    """a step of a `robustness_test:` section: `_Step` plus the frame window (None: the whole sequence) and its two switches"""

    def __init__(self, kind, ranges, prob_threshold, seq_idx=None, continuous=False, keep=True):
        _Step.__init__(self, kind, ranges, prob_threshold)
        self.seq_idx = None if not seq_idx else tuple(int(v) for v in seq_idx)       # '' / [] / None: the whole sequence
        if self.seq_idx is not None and len(self.seq_idx) != 2:
            raise ValueError("robustness test %s: seq_idx must be [first, last + 1], got %r" % (kind, seq_idx))
        self.continuous, self.keep = bool(continuous), bool(keep)


class RobustnessTest:
    """The transforms of a `robustness_test:` section (`evaluate_robustness.py` writes one per point of its sweep over
    config/robustness-test-CISTGCN.yaml) on the device.  Takes the section object `loaders/loader.py::get_transformations` takes
    and builds the same list in the same order (:46-127): random_flip, random_rotation, random_scale, random_noise,
    random_translation (threshold 0.5, whole sequence), then rotation, scale, noise, translation, flip, pose_invers with their
    `prob_threshold`, `seq_idx`, `continuous` and `keep`.  A kind may occur twice; an explicit flip after a translation is fine.
    `draw` / `__call__` are those of `DeviceAugmentation`, so `DevicePrefetcher` takes either.

    Where this differs from the reference, on purpose:
      * scalars of either number type become degenerate intervals (`_range`); the reference's RandomScale / RandomTranslation
        raise IndexError on an int scalar.  Falsy entries mean [0, 0] as there: `scale: {x: 1.2, y: 0, z: 0}` collapses y and z,
        which is what the sweep produces.
      * a window outside [0, L] or with first >= last + 1 is refused (ValueError) for every kind, when L is known; the
        reference fails with a shape error for rotation / scale / noise / translation and silently clamps for flip / inversion.
      * RandomPoseInvers swaps the joints inside the dataset's own array when it is the first transform; `raw` is never
        written here.
    """

    def __init__(self, opt_trs=None):
        self.steps = []
        if opt_trs is None or opt_trs == "":
            return

        def section(name):
            s = getattr(opt_trs, name, None)
            return None if (s is None or s == "") else s

        for name in ("random_flip", "random_rotation", "random_scale", "random_noise", "random_translation", "rotation", "scale", "noise",
                     "translation", "flip", "pose_invers"):
            s = section(name)
            if s is None:
                continue
            rand = name.startswith("random_")
            kind = name.replace("random_", "")
            if name == "random_noise":                     # loader.py:65-67: a bare amplitude
                self.steps.append(_WindowStep("noise", float(s), 0.5))
                continue
            # loader.py:46-74 leaves the four keywords at the constructors' defaults, :75-127 passes them
            kw = {} if rand else {"seq_idx": getattr(s, "seq_idx", None), "keep": getattr(s, "keep", True)}
            thr = 0.5 if rand else float(getattr(s, "prob_threshold", 0.5))
            if kind == "pose_invers":
                self.steps.append(_WindowStep("invert", H36M_INVERSE_PAIRS, thr, **kw))
                continue
            if kind == "flip":
                self.steps.append(_WindowStep("flip", tuple(bool(getattr(s, a, "")) for a in "xyz"), thr, **kw))
                continue
            if not rand:
                kw["continuous"] = getattr(s, "continuous", False)
            if kind == "noise":
                self.steps.append(_WindowStep("noise", float(s.noise), thr, **kw))
                continue
            if all(getattr(s, a, "") == "" for a in "xyz"):
                continue                                   # the reference skips a transform whose three entries are ''
            r = [_range(getattr(s, a, ""), "%s.%s" % (name, a)) for a in "xyz"]
            self.steps.append(_WindowStep(kind, tuple(v if v is not None else (0.0, 0.0) for v in r), thr, **kw))
        self._check_count()

    def _check_count(self):
        if len(self.steps) > MAX_STEPS:
            raise ValueError("robustness test: %d steps, the kernel takes %d" % (len(self.steps), MAX_STEPS))

    @property
    def needs_joints(self):
        return any(st.kind in ("noise", "invert") for st in self.steps)

    @property
    def n_noise(self):
        return sum(st.kind == "noise" for st in self.steps)

    def draw(self, batch, rng=None, joints=None):
        """(batch, n_steps, 4) float32 rows [apply?, v0, v1, v2] (with a RandomNoise step: a dict {"params", "noise"}, noise
        (batch, n_noise, joints, 3), and `joints` is required).  Consumes `rng.uniform` (default: the global `np.random`, which the
        reference's transforms use) exactly where the reference does, sample by sample and step by step: one coin per step - for a
        flip one coin per enabled axis - and, where the coin says 'apply' (coin > prob_threshold), the three amounts or the
        (joints, 3) array."""
        self._check_count()
        rng = np.random if rng is None else rng
        out = np.zeros((batch, len(self.steps), 4), dtype=np.float32)
        n_noise = self.n_noise
        if n_noise and joints is None:
            raise ValueError("RobustnessTest.draw: RandomNoise draws one number per joint and axis: pass joints=")
        noise = np.zeros((batch, n_noise, int(joints), 3), dtype=np.float32) if n_noise else None
        for b in range(batch):
            slot = 0
            for i, st in enumerate(self.steps):
                if st.kind == "flip":                      # custom_transforms.py:265, :275, :285
                    for a in range(3):
                        if st.ranges[a] and rng.uniform() > st.prob_threshold:
                            out[b, i, 1 + a] = 1.0
                    out[b, i, 0] = float(out[b, i, 1:].any())
                    continue
                if st.kind == "noise":
                    slot += 1
                if not (rng.uniform() > st.prob_threshold):
                    continue
                out[b, i, 0] = 1.0
                if st.kind == "noise":                     # :372: one array draw of (joints, 3) numbers
                    out[b, i, 1] = st.ranges
                    noise[b, slot - 1] = np.asarray(rng.uniform(-1, 1, (int(joints), 3)), dtype=np.float64).astype(np.float32)
                elif st.kind != "invert":
                    out[b, i, 1:] = [np.float32(rng.uniform(lo, hi)) for lo, hi in st.ranges]
        return {"params": out, "noise": noise} if n_noise else out

    _perm = DeviceAugmentation._perm

    def draw_device(self, batch, joints=None, device="cuda", stream=0, out=None):
        """What `draw` returns, as device tensors drawn on the device (`DeviceAugmentation.draw_device`: another random stream than
        `draw`; the seed is read, not advanced)."""
        self._check_count()
        return _draw_device(self.steps, "steps4", batch, joints, device, stream, out)

    def step_table(self, L):
        """(n_steps, 6) int32 [kind, s0, s1, continuous, keep, noise slot] for sequences of L frames; ValueError for a window that
        does not satisfy 0 <= s0 < s1 <= L"""
        self._check_count()
        tab = np.zeros((len(self.steps), 6), dtype=np.int32)
        slot = 0
        for i, st in enumerate(self.steps):
            s0, s1 = (0, L) if st.seq_idx is None else st.seq_idx
            if not (0 <= s0 < s1 <= L):
                raise ValueError("robustness test %s: seq_idx [%d, %d] is not a window of a %d-frame sequence" % (st.kind, s0, s1, L))
            tab[i] = (_KIND[st.kind], s0, s1, st.continuous, st.keep, slot if st.kind == "noise" else 0)
            slot += st.kind == "noise"
        return tab

    def __call__(self, raw, input_n, params=None, keep_processed=False, out=None, stream=0):
        """raw: (B, L, J, 3) float32 on the HIP device.  Returns the dictionary `DeviceAugmentation.__call__` returns; `params`, `out`
        and `stream` as there."""
        ops._chk(raw, "raw")
        if not raw.is_cuda and not _lib._host_pointers_ok:
            raise ValueError("RobustnessTest runs on MI355X only: got a %s tensor (no CPU path exists)" % raw.device)
        if raw.dim() != 4 or raw.shape[3] != 3:
            raise ValueError("expected windows of shape (B, L, J, 3), got %s" % (tuple(raw.shape),))
        raw = raw if raw.is_contiguous() else ops._copy(raw)
        B, L, J, _ = raw.shape
        tab = self.step_table(L)
        n_steps, n_noise = len(self.steps), self.n_noise
        if params is None:
            params = self.draw(B, joints=J)
        elif isinstance(params, str):
            if params != "device":
                raise ValueError("params: a table, None (host draws) or \"device\", got %r" % params)
            params = self.draw_device(B, joints=J, device=raw.device, stream=stream)
        noise = None
        if isinstance(params, dict):
            params, noise = params["params"], params["noise"]
        if n_noise:
            if noise is None:
                raise ValueError("the section has a RandomNoise step: pass the dictionary `draw` returns")
            if isinstance(noise, np.ndarray):
                noise = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(raw.device, non_blocking=True)
            if tuple(noise.shape) != (B, n_noise, J, 3):
                raise ValueError("expected (%d, %d, %d, 3) noise draws" % (B, n_noise, J))
        perm = self._perm(J, raw.device)
        if isinstance(params, np.ndarray):
            params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(raw.device, non_blocking=True)
        if tuple(params.shape) != (B, n_steps, 4):
            raise ValueError("expected a (%d, %d, 4) parameter table" % (B, n_steps))
        out, proc = _item_tensors(raw, int(input_n), keep_processed, out)
        steps = (ctypes.c_int * max(1, tab.size))(*[int(v) for v in tab.reshape(-1)])
        _lib.call("cg_perturb_sequences", ops._ptr(raw), steps, ops._ptr(params) if n_steps else None, ops._ptr(noise) if n_noise else None,
                  ops._ptr(perm), ops._ptr(out["sample"]), ops._ptr(out["target"]), ops._ptr(out["target_vel"]), ops._ptr(out["target_gvel"]),
                  ops._ptr(proc), ops._ptr(out["sample_vel"]), B, L, J, int(input_n), n_steps, n_noise, ops._stream(raw))
        if keep_processed:
            out["processed"] = proc
        return out


class DevicePrefetcher:
    """Iterates (B, L, J, 3) host batches (numpy or CPU tensors) and yields augmented device batches; the host->device copy
    and the augmentation kernel of batch k+1 are issued on a side stream while batch k is being consumed, through two pinned
    staging buffers (`environment/train.py:57-58` copies synchronously inside the hot loop instead)."""

    def __init__(self, batches, augmentation, input_n, device="cuda"):
        self.it, self.aug, self.input_n = iter(batches), augmentation, int(input_n)
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.stream = torch.cuda.Stream(device=self.device) if self.cuda else None
        self._pinned = [None, None]
        self._copied = [None, None]          # event behind the last host->device copy out of each staging buffer
        self._k = 0
        self._next = None
        self._preload()

    def _preload(self):
        try:
            host = next(self.it)
        except StopIteration:
            self._next = None
            return
        host = torch.as_tensor(host, dtype=torch.float32)
        params = self.aug.draw(host.shape[0], joints=host.shape[2])  # host RNG, reference order
        if not self.cuda:
            self._next = self.aug(host.to(self.device), self.input_n, params)
            return
        slot = self._k % 2
        self._k += 1
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()                         # the DMA out of this staging buffer has finished
        if self._pinned[slot] is None or self._pinned[slot].shape != host.shape:
            self._pinned[slot] = torch.empty(host.shape, dtype=torch.float32).pin_memory()
        self._pinned[slot].copy_(host)
        with torch.cuda.stream(self.stream):
            raw = self._pinned[slot].to(self.device, non_blocking=True)
            self._copied[slot] = torch.cuda.Event()
            self._copied[slot].record(self.stream)
            self._next = self.aug(raw, self.input_n, params)
            self._ready = torch.cuda.Event()
            self._ready.record(self.stream)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next is None:
            raise StopIteration
        batch = self._next
        if self.cuda:
            torch.cuda.current_stream(self.device).wait_event(self._ready)
            for t in batch.values():
                t.record_stream(torch.cuda.current_stream(self.device))
        self._preload()
        return batch
