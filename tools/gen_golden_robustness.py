#!/usr/bin/env python3
"""Golden vectors for the robustness-test transforms (`robustness_test:` section of an evaluation YAML, the sweep of
`evaluate_robustness.py` over `config/robustness-test-CISTGCN.yaml`), from the REAL reference: the chain
`loaders/loader.py::get_transformations` (:42-130) builds from such a section - `RandomRotation`, `RandomScale`, `RandomNoise`,
`RandomTranslation`, `RandomFlip`, `RandomPoseInvers` with `prob_threshold`, `seq_idx`, `continuous` and `keep` - applied by
`H36m_Motion3D.__getitem__` (`loaders/h36m_motion_3d.py:94-108`), with every `np.random.uniform` draw recorded so that the device
path can be driven by the same numbers.  Build container only; writes data only (tests/golden/aug_robustness.npz): per case the
windows, the reference's processed sequence and cumulative velocities, the draws, and the section as a JSON string."""
import importlib, json, os, sys, types
import numpy as np
import torch

sys.dont_write_bytecode = True
pkg = types.ModuleType("human_motion_prediction")
pkg.__path__ = ["/root/reference/human_motion_prediction"]
sys.modules["human_motion_prediction"] = pkg
for sub in ("utils", "environment", "loaders"):          # package __init__ files pull in plotting / fvcore: stub them
    m = types.ModuleType("human_motion_prediction." + sub)
    m.__path__ = ["/root/reference/human_motion_prediction/" + sub]
    sys.modules["human_motion_prediction." + sub] = m
trs = importlib.import_module("human_motion_prediction.environment.custom_transforms")
ds_mod = importlib.import_module("human_motion_prediction.loaders.h36m_motion_3d")

L, INPUT_N = 12, 8


def build_chain(cfg, applied):
    """loaders/loader.py:42-130: importing loader.py itself needs torchvision + every dataset module, so the same constructor
    calls are issued here in the order of its source lines; `applied[i]` collects, per call, whether transform i changed its input"""
    chain = [trs.ToTensor()]
    g = cfg.get
    if g("random_flip", "") != "":
        chain.append(trs.RandomFlip(g("random_flip")["x"], g("random_flip")["y"], g("random_flip")["z"]))
    if "random_rotation" in cfg and any(cfg["random_rotation"][a] != "" for a in "xyz"):
        s = cfg["random_rotation"]
        chain.append(trs.RandomRotation(s["x"], s["y"], s["z"]))
    if "random_scale" in cfg and any(cfg["random_scale"][a] != "" for a in "xyz"):
        s = cfg["random_scale"]
        chain.append(trs.RandomScale(s["x"], s["y"], s["z"]))
    if g("random_noise", "") != "":
        chain.append(trs.RandomNoise(cfg["random_noise"]))
    if "random_translation" in cfg and any(cfg["random_translation"][a] != "" for a in "xyz"):
        s = cfg["random_translation"]
        chain.append(trs.RandomTranslation(s["x"], s["y"], s["z"]))
    if "rotation" in cfg and any(cfg["rotation"][a] != "" for a in "xyz"):
        s = cfg["rotation"]
        chain.append(trs.RandomRotation(s["x"], s["y"], s["z"], s["prob_threshold"], s["seq_idx"], s["continuous"], s["keep"]))
    if "scale" in cfg and any(cfg["scale"][a] != "" for a in "xyz"):
        s = cfg["scale"]
        chain.append(trs.RandomScale(s["x"], s["y"], s["z"], s["prob_threshold"], s["seq_idx"], s["continuous"], s["keep"]))
    if g("noise", "") != "":
        s = cfg["noise"]
        chain.append(trs.RandomNoise(s["noise"], s["prob_threshold"], s["seq_idx"], s["continuous"], s["keep"]))
    if "translation" in cfg and any(cfg["translation"][a] != "" for a in "xyz"):
        s = cfg["translation"]
        chain.append(trs.RandomTranslation(s["x"], s["y"], s["z"], s["prob_threshold"], s["seq_idx"], s["continuous"], s["keep"]))
    if g("flip", "") != "":
        s = cfg["flip"]
        chain.append(trs.RandomFlip(s["x"], s["y"], s["z"], s["prob_threshold"], s["seq_idx"], s["keep"]))
    if "pose_invers" in cfg:
        s = cfg["pose_invers"]
        chain.append(trs.RandomPoseInvers("h36m", s["prob_threshold"], s["seq_idx"], s["keep"]))

    def compose(data):
        for i, t in enumerate(chain):
            before = None if i == 0 else data.clone()
            data = t(data)
            if before is not None:
                applied[i - 1].append(not torch.equal(before.double(), data.double()))
        return data

    for _ in chain[1:]:
        applied.append([])
    return compose


draws = []
orig_uniform = np.random.uniform


def logged(*a, **k):
    v = orig_uniform(*a, **k)
    if isinstance(v, np.ndarray):                 # RandomNoise draws a (joints, 3) array in one call
        draws.extend(float(t) for t in v.reshape(-1))
    else:
        draws.append(float(v))
    return v


def run_case(cfg, B, J, data_seed, rng_seed):
    ds = object.__new__(ds_mod.H36m_Motion3D)               # __getitem__ only needs these three attributes
    g = np.random.RandomState(data_seed)
    raw = (50 + 350 * g.randn(B, L, J, 3)).astype(np.float32)
    ds.target = raw.copy()                                  # RandomPoseInvers as the first transform writes into this storage
    applied = []
    ds.transform = build_chain(cfg, applied)
    ds.input_n = INPUT_N
    draws.clear()
    np.random.seed(rng_seed)
    np.random.uniform = logged
    out = {"processed": [], "target_vel": [], "target_gvel": [], "ndraws": []}
    try:
        for i in range(B):
            n0 = len(draws)
            item = ds[i]
            out["ndraws"].append(len(draws) - n0)
            for k in ("processed", "target_vel", "target_gvel"):
                out[k].append(np.asarray(item[k], dtype=np.float32))
    finally:
        np.random.uniform = orig_uniform
    rec = {"raw": raw, "draws": np.array(draws, dtype=np.float64), "ndraws": np.array(out["ndraws"]),
           "processed": np.stack(out["processed"]), "target_vel": np.stack(out["target_vel"]), "target_gvel": np.stack(out["target_gvel"])}
    return rec, applied


def win(seq_idx, continuous, keep, thr=0.0):
    return {"prob_threshold": thr, "seq_idx": seq_idx, "continuous": continuous, "keep": keep}


# window settings every ramp kind is recorded with: (name, seq_idx, continuous, keep)
WINDOWS = [("whole_const", "", False, True), ("whole_cont", "", True, True), ("w37_cont_keep", [3, 7], True, True),
           ("w37_const_nokeep", [3, 7], False, False), ("w37_cont_nokeep", [3, 7], True, False), ("w37_const_keep", [3, 7], False, True),
           ("w34_cont", [3, 4], True, True), ("w0L", [0, L], True, False), ("wLast", [L - 1, L], False, True), ("w3L_cont", [3, L], True, True)]
# amounts per window setting, cycled: rotation includes 0, 90 and 360 degrees and two-axis vectors (int and float scalars, ranges);
# scale includes a 0 axis (falsy entry -> [0, 0], what the sweep of evaluate_robustness.py produces); scale / translation scalars
# are floats (the reference's constructors raise IndexError on an int scalar)
ROT = [{"x": 90, "y": "", "z": ""}, {"x": "", "y": 360, "z": ""}, {"x": 30.0, "y": "", "z": -45.0}, {"x": [-40, 40], "y": [-180, 180], "z": [-40, 40]},
       {"x": "", "y": 90.0, "z": 360}, {"x": 0, "y": 0, "z": 0}, {"x": 120, "y": 17.5, "z": ""}, {"x": [-5, 5], "y": [100, 180], "z": ""},
       {"x": "", "y": "", "z": 90}, {"x": 360, "y": "", "z": ""}]
SCALE = [{"x": 1.2, "y": 0.8, "z": 1.1}, {"x": 1.2, "y": 0, "z": 0}, {"x": [0.5, 1.5], "y": [0.5, 1.5], "z": [0.5, 1.5]}, {"x": 0.7, "y": "", "z": 1.3},
         {"x": 1.5, "y": 1.5, "z": 1.5}, {"x": [1.0, 2.0], "y": 1.0, "z": 0.25}, {"x": 1.2, "y": 0.8, "z": 1.1}, {"x": 0, "y": 2.0, "z": 1.0},
         {"x": 0.9, "y": 1.1, "z": 1.0}, {"x": [0.5, 1.5], "y": 0.5, "z": 1.5}]
TRANS = [{"x": 0.1, "y": -0.2, "z": 0.3}, {"x": 0.5, "y": "", "z": ""}, {"x": [-0.3, 0.3], "y": [-0.3, 0.3], "z": [-0.3, 0.3]}, {"x": "", "y": 0.25, "z": -0.25},
         {"x": 1.0, "y": 1.0, "z": 1.0}, {"x": [0.0, 0.5], "y": 0, "z": -0.4}, {"x": 0.1, "y": -0.2, "z": 0.3}, {"x": -0.05, "y": "", "z": 0.05},
         {"x": 0.2, "y": 0.2, "z": ""}, {"x": [-0.3, 0.3], "y": 0.3, "z": ""}]
NOISE = [0.05, 0.1, 0.02, 0.2, 0.05, 0.5, 0.01, 0.1, 0.3, 0.05]

CASES = []          # (name, section, B, J)
for i, (wname, seq_idx, cont, keep) in enumerate(WINDOWS):
    CASES.append(("rotation_" + wname, {"rotation": dict(ROT[i], **win(seq_idx, cont, keep))}, 3, 5))
    CASES.append(("scale_" + wname, {"scale": dict(SCALE[i], **win(seq_idx, cont, keep))}, 3, 5))
    CASES.append(("translation_" + wname, {"translation": dict(TRANS[i], **win(seq_idx, cont, keep))}, 3, 5))
    CASES.append(("noise_" + wname, {"noise": dict({"noise": NOISE[i]}, **win(seq_idx, cont, keep))}, 3, 5))
for wname, seq_idx, keep in (("whole", "", True), ("w37_keep", [3, 7], True), ("w37_nokeep", [3, 7], False), ("w3L_nokeep", [3, L], False)):
    w = win(seq_idx, False, keep)
    del w["continuous"]
    CASES.append(("flip_xz_" + wname, {"flip": dict({"x": True, "y": "", "z": True}, **w)}, 3, 5))
    CASES.append(("invert_" + wname, {"pose_invers": dict(w)}, 2, 32))
flipw = lambda seq_idx, keep, thr=0.0: {"prob_threshold": thr, "seq_idx": seq_idx, "keep": keep}
# all six explicit steps, each with its own window, behind random_flip and random_rotation (threshold 0.5, whole sequence): two
# rotations, two flips, an explicit flip after a translation; centroids and extents are recomputed from what the step before left
CHAIN = {"random_flip": {"x": True, "y": True, "z": ""}, "random_rotation": {"x": [-20, 20], "y": [-180, 180], "z": [-20, 20]},
         "rotation": dict({"x": [-30, 30], "y": 45.0, "z": ""}, **win([2, 9], True, True)),
         "scale": dict({"x": 1.3, "y": [0.7, 0.9], "z": 1.1}, **win([4, 6], False, True)),
         "noise": dict({"noise": 0.05}, **win([1, 11], True, False)),
         "translation": dict({"x": 0.2, "y": [-0.3, 0.3], "z": -0.1}, **win([5, 12], True, True)),
         "flip": dict({"x": "", "y": True, "z": True}, **flipw([6, 10], False)),
         "pose_invers": flipw([3, 8], True)}
CASES.append(("chain_all", CHAIN, 4, 32))
# prob_threshold 0.5: the seed is searched so that every step is applied for at least one sample and skipped for at least one
THR_A = {"rotation": dict({"x": [-40, 40], "y": [-180, 180], "z": ""}, **win([3, 7], True, True, 0.5)),
         "scale": dict({"x": [0.5, 1.5], "y": 1.2, "z": 0.8}, **win("", True, True, 0.5)),
         "noise": dict({"noise": 0.1}, **win([2, 10], False, False, 0.5)),
         "translation": dict({"x": [-0.3, 0.3], "y": 0.2, "z": ""}, **win([3, L], True, True, 0.5))}
THR_B = {"scale": dict({"x": 1.25, "y": [0.6, 0.9], "z": ""}, **win([3, 7], False, False, 0.5)),
         "flip": dict({"x": True, "y": "", "z": True}, **flipw([3, 7], True, 0.5)),
         "pose_invers": flipw([5, 9], False, 0.5)}
CASES.append(("thr_half_ramps", THR_A, 6, 5))
CASES.append(("thr_half_flip_invert", THR_B, 6, 32))

store, names = {}, []
for idx, (name, cfg, B, J) in enumerate(CASES):
    half = name.startswith("thr_half")
    for seed in range(1000, 1400):
        rec, applied = run_case(cfg, B, J, data_seed=100 + idx, rng_seed=seed)
        if not half or all(any(a) and not all(a) for a in applied):
            break
    else:
        raise SystemExit("no seed applies and skips every step of %s" % name)
    if half:
        assert all(any(a) and not all(a) for a in applied), (name, applied)
        print(name, "seed", seed, "applied per step:", [[int(v) for v in a] for a in applied])
    names.append(name)
    store[name + "/config"] = np.array(json.dumps(cfg))
    for k, v in rec.items():
        store[name + "/" + k] = v
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "aug_robustness.npz")
np.savez_compressed(path, cases=np.array(names), input_n=np.array(INPUT_N), **store)
print("wrote", os.path.normpath(path), len(names), "cases,", os.path.getsize(path), "bytes")
