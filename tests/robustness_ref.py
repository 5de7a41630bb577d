"""TEST INFRASTRUCTURE ONLY (fp64 numpy restatement, never imported by the product package).

The robustness-test transforms of the reference restated for one sequence: `RandomRotation`, `RandomScale`, `RandomTranslation`,
`RandomFlip`, `RandomPoseInvers`, `RandomNoise` (environment/custom_transforms.py:10-84, 87-161, 164-240, 243-298, 301-347, 350-400)
WITH `seq_idx`, `continuous` and `keep`, composed in the order `loaders/loader.py::get_transformations` (:42-130) builds them from a
`robustness_test:` section, and the per-item tensors of `H36m_Motion3D.__getitem__` (loaders/h36m_motion_3d.py:94-108).
Pinned by tests/golden/aug_robustness.npz (tools/gen_golden_robustness.py runs the reference's own classes with recorded draws).
It shares no code with cistgcn_amd/environment/input_pipeline.py: the section is parsed here a second time."""
import json
from types import SimpleNamespace as NS

import numpy as np

INVERSE_PAIRS = ((6, 1), (7, 2), (8, 3), (9, 4), (10, 5), (16, 24), (17, 25), (18, 26), (19, 27), (20, 28), (22, 30), (21, 29), (23, 31))
ORDER = ("random_flip", "random_rotation", "random_scale", "random_noise", "random_translation", "rotation", "scale", "noise", "translation",
         "flip", "pose_invers")


class Replay:
    """rng stand-in that replays recorded `uniform` draws (the value is returned whatever the bounds)"""

    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def uniform(self, *a):
        if len(a) == 3 and a[2] is not None:
            n = int(np.prod(a[2]))
            v = np.asarray(self.draws[self.i:self.i + n], dtype=np.float64).reshape(a[2])
            self.i += n
            return v
        v = self.draws[self.i]
        self.i += 1
        return v


def section(cfg):
    """dict (or the JSON string of the fixture) -> the attribute object `yaml_utils.Struct` would present"""
    if isinstance(cfg, (str, bytes, np.ndarray)):
        cfg = json.loads(str(cfg))
    return NS(**{k: (NS(**v) if isinstance(v, dict) else v) for k, v in cfg.items()})


def _interval(v):
    if not v:
        return (0.0, 0.0)
    if isinstance(v, (int, float)):
        return (float(v), float(v))
    return (float(v[0]), float(v[1]))


def steps_of(cfg):
    """[(kind, amounts, prob_threshold, seq_idx or None, continuous, keep)] in loader order"""
    if cfg is None or (isinstance(cfg, str) and cfg == ""):
        return []
    cfg = cfg if isinstance(cfg, dict) else vars(cfg) if isinstance(cfg, NS) else vars(section(cfg))
    out = []
    for name in ORDER:
        s = cfg.get(name, "")
        if s is None or s == "":
            continue
        s = vars(s) if isinstance(s, NS) else s
        rand = name.startswith("random_")
        kind = name.replace("random_", "")
        if name == "random_noise":
            out.append(("noise", float(s), 0.5, None, False, True))
            continue
        thr = 0.5 if rand else float(s["prob_threshold"])
        seq_idx = None if rand or not s.get("seq_idx") else (int(s["seq_idx"][0]), int(s["seq_idx"][1]))
        cont = False if rand else bool(s.get("continuous", False))
        keep = True if rand else bool(s["keep"])
        if kind == "noise":
            out.append(("noise", float(s["noise"]), thr, seq_idx, cont, keep))
        elif kind == "pose_invers":
            out.append(("invert", None, thr, seq_idx, False, keep))
        elif kind == "flip":
            out.append(("flip", tuple(bool(s[a]) for a in "xyz"), thr, seq_idx, False, keep))
        elif any(s[a] != "" for a in "xyz"):
            out.append((kind, tuple(_interval(s[a]) for a in "xyz"), thr, seq_idx, cont, keep))
    return out


def weights(L, seq_idx, cont, keep):
    """f(t): 0 before the window, the ramp (or 1) inside, the last value (keep) or 0 after it"""
    s0, s1 = (0, L) if seq_idx is None else seq_idx
    n = s1 - s0
    assert 0 <= s0 < s1 <= L
    inside = np.linspace(0.0, 1.0, n) if (cont and n > 1) else (np.zeros(n) if cont else np.ones(n))
    f = np.zeros(L)
    f[s0:s1] = inside
    if keep:
        f[s1:] = inside[-1]
    return f


def rotvec_matrices(deg):
    """(n, 3) rotation vectors in degrees -> (n, 3, 3) matrices (Rodrigues; what scipy's from_rotvec(..).as_matrix() returns)"""
    v = np.deg2rad(np.asarray(deg, dtype=np.float64))
    th = np.linalg.norm(v, axis=1)
    out = np.tile(np.eye(3), (len(v), 1, 1))
    for i in np.nonzero(th > 0)[0]:
        k = v[i] / th[i]
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        out[i] = np.eye(3) + np.sin(th[i]) * K + (1.0 - np.cos(th[i])) * (K @ K)
    return out


def perturb_one(data, steps, rng):
    """one (L, J, 3) sequence through the step list; fp64 throughout"""
    data = np.array(data, dtype=np.float64)
    L, J, _ = data.shape
    for kind, amt, thr, seq_idx, cont, keep in steps:
        s0, s1 = (0, L) if seq_idx is None else seq_idx
        frames = np.arange(L)
        touched = (frames >= s0) & ((frames < s1) | keep)           # flip and inversion: no ramp
        if kind == "flip":
            c = data.mean((0, 1))
            src = data.copy()
            for a in range(3):
                if amt[a] and rng.uniform() > thr:
                    data[touched, :, a] = c[a] - (src[touched, :, a] - c[a])
            continue
        if not (rng.uniform() > thr):
            continue
        if kind == "invert":
            for x, y in INVERSE_PAIRS:
                tx, ty = data[touched, x].copy(), data[touched, y].copy()
                data[touched, x], data[touched, y] = ty, tx
            continue
        f = weights(L, seq_idx, cont, keep)
        if kind == "noise":
            u = np.asarray(rng.uniform(-1, 1, (J, 3)), dtype=np.float64)
            ext = data.max((0, 1)) - data.min((0, 1))
            data = data + f[:, None, None] * amt * u[None] * ext
            continue
        v = np.array([np.float32(rng.uniform(lo, hi)) for lo, hi in amt], dtype=np.float64)
        if kind == "rotation":
            c = data.mean((0, 1))
            R = rotvec_matrices(f[:, None] * v[None])
            data = np.einsum("tja,tab->tjb", data - c, R) + c
        elif kind == "scale":
            data = data * (1.0 + f[:, None, None] * (v - 1.0))
        else:
            ext = data.max((0, 1)) - data.min((0, 1))
            data = data + f[:, None, None] * v * ext
    return data


def item_tensors(proc, input_n):
    proc = np.asarray(proc, dtype=np.float64)
    vel = np.diff(proc, axis=0)
    gvel = np.linalg.norm(vel, axis=-1, keepdims=True)
    return {"sample": proc[:input_n], "sample_vel": vel[:input_n], "target": proc[input_n:], "target_vel": vel[input_n - 1:].cumsum(0),
            "target_gvel": gvel[input_n - 1:].cumsum(0), "processed": proc}


def perturb_batch(raw, cfg, draws, input_n):
    """(B, L, J, 3) batch with recorded draws -> (dict of stacked item tensors, number of draws consumed)"""
    steps, rng = steps_of(cfg), Replay(draws)
    items = [item_tensors(perturb_one(r, steps, rng), input_n) for r in raw]
    return {k: np.stack([it[k] for it in items]) for k in items[0]}, rng.i
