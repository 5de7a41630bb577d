#!/usr/bin/env python
"""Golden vectors of forward kinematics and of the dataset loaders from the REAL reference.  Build container only, like the other
tools/gen_golden_*.py: the reference is imported at generation time with `Tensor.cuda()` returning the tensor itself (everything
runs on the CPU), this script writes arrays only.

tests/golden/aug_kinematics.npz (the `aug_` prefix: tests/helpers.py takes any other *.npz for a model fixture):

  trees, recorded as data
    tree/h36m/{parent,rest}      `forward_kinematics._some_variables()` (32 joints), parent zero-based with root -1
    tree/cmu/{parent,rest}       `forward_kinematics._some_variables_cmu()` (38 joints)
    tree/smpl24/{parent,rest}    the default `parent` of `ang2joint` (24 joints) with a seeded rest pose
    tree/smplh52/{parent,rest}   a seeded 52-joint SMPL-H-like tree (body of 22, two hands of 15)
  forward-kinematics cases `fk/<name>/...`: `tree` (its name), `convention`, `angles` (chain: (N, 3 + 3J); smpl: (N, J_pose, 3)),
    `out` the reference's fp32 result (`fkl_torch` / `ang2joint(...) * scale`), `scale`, and `ref_err` = max |out - restatement| with the
    fp64 restatement of tests/kinematics_ref.py: the reference's own fp32 error, the yardstick of the kernel's tolerance.
    Rows: seeded rotation vectors with |r| in [0.1, 2]; rows scaled by 1e-3 (tiny angles); rows where some joints are exactly zero; the
    chain cases have a non-zero joint 0 throughout (the reference ignores it for every other joint: `if parent[i] > 0`).  SMPL cases
    hold no 0 < |r| < 1e-4, so the reference's N(0, 1e-8) noise stays below fp32 resolution of the result.
  a miniature H3.6M directory `h36m/...`: `files` (names `S<subj>/<action>_<subact>.txt`), `file/<name>` (F, 99) fp32 (written by the
    tests with %.9g), `input_n`, `output_n`, `action`; `target` = `H36m_Motion3D(split="train").target`, `class_seq`, `up_joints` (the head
    and hip joints its inversion check uses), `dim_used`, `inverted` (the windows its fix mirrored)
  a miniature AMASS directory `amass/...`: `p3d0`, `parents`, `files` (paths below the root), `poses/<i>`, `rate/<i>`; `target` =
    `Amass_Motion3D(split="train").target`, `class_seq`; one more file without `poses`
  `find256/<F1>_<F2>/{s1,s2}`: first rows of `find_indices_256(F1, F2, seq_len, input_n)` for two pairs, with `find256/input_n`,
    `find256/seq_len`
"""
import importlib
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
torch.Tensor.cuda = lambda self, *a, **k: self
pkg = types.ModuleType("human_motion_prediction")
pkg.__path__ = ["/root/reference/human_motion_prediction"]
sys.modules["human_motion_prediction"] = pkg
for sub in ("utils", "loaders"):         # the packages' own __init__ import plotting code; the modules below do not need it
    m = types.ModuleType("human_motion_prediction." + sub)
    m.__path__ = ["/root/reference/human_motion_prediction/" + sub]
    sys.modules["human_motion_prediction." + sub] = m
FK = importlib.import_module("human_motion_prediction.utils.forward_kinematics")
DU = importlib.import_module("human_motion_prediction.utils.data_utils")
A2J = importlib.import_module("human_motion_prediction.utils.ang2joint")
BU = importlib.import_module("human_motion_prediction.utils.body_utils")
H36 = importlib.import_module("human_motion_prediction.loaders.h36m_motion_3d")
AMS = importlib.import_module("human_motion_prediction.loaders.amass_motion_3d")

import kinematics_ref as KR      # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "aug_kinematics.npz")
N_ROWS = 12


def rotvecs(g, n, J):
    """(n, J, 3): rows 0..5 |r| in [0.1, 2]; rows 6..8 the same x 1e-3; rows 9..11 with a third of the joints exactly zero"""
    d = g.randn(n, J, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    r = d * g.uniform(0.1, 2.0, size=(n, J, 1))
    r[6:9] *= 1e-3
    r[9:] *= (g.uniform(size=(n - 9, J, 1)) > 1.0 / 3.0)
    return r.astype(np.float32)


def smplh_tree(g):
    """22 body joints of the SMPL tree, then 15 joints per hand hanging off the wrists (20, 21) in chains of three"""
    body = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19]
    parent = list(body)
    for wrist in (20, 21):
        for _ in range(5):
            first = len(parent)
            parent += [wrist, first, first + 1]
    rest = np.cumsum(g.uniform(-0.25, 0.25, size=(len(parent), 3)), 0).astype(np.float32)
    return np.asarray(parent, dtype=np.int32), rest


def main():
    g = np.random.RandomState(20260)
    torch.manual_seed(20260)
    rec = {}
    trees = {}
    for name, fn in (("h36m", FK._some_variables), ("cmu", FK._some_variables_cmu)):
        parent, offset, _, _ = fn()
        trees[name] = (np.asarray(parent, dtype=np.int32), np.asarray(offset, dtype=np.float32).reshape(-1, 3))
    default_parent = A2J.ang2joint.__defaults__[0]
    trees["smpl24"] = (np.asarray([default_parent[i] for i in range(len(default_parent))], dtype=np.int32),
                       np.cumsum(g.uniform(-0.3, 0.3, size=(24, 3)), 0).astype(np.float32))
    trees["smplh52"] = smplh_tree(g)
    for name, (parent, rest) in trees.items():
        assert parent[0] == -1 and all(-1 <= parent[i] < i for i in range(1, len(parent))), name
        rec["tree/%s/parent" % name], rec["tree/%s/rest" % name] = parent, rest

    cases = []
    for name in ("h36m", "cmu"):
        parent, rest = trees[name]
        J = len(parent)
        ang = np.concatenate([g.randn(N_ROWS, 3).astype(np.float32), rotvecs(g, N_ROWS, J).reshape(N_ROWS, -1)], 1)
        ang[:, 3:6] = rotvecs(g, N_ROWS, 1)[:, 0] + 0.05          # joint 0 rotates in every row
        out = FK.fkl_torch(torch.from_numpy(ang), parent, rest.astype(np.float64), None, None).numpy()
        assert out.dtype == np.float32
        cases.append(("chain_" + name, name, "expmap_chain", ang, out, 1.0, KR.fk_chain(ang, parent, rest)))
    for name, J_pose, scale in (("smpl24", 24, 1.0), ("smpl24", 30, 1000.0), ("smplh52", 52, 1000.0)):
        parent, rest = trees[name]
        J = len(parent)
        pose = rotvecs(g, N_ROWS, J_pose)
        nrm = np.linalg.norm(pose, axis=-1)
        assert not ((nrm > 0) & (nrm < 1e-4)).any()
        pdict = {i: int(parent[i]) for i in range(J)}
        p3d0 = torch.from_numpy(rest)[None].repeat(N_ROWS, 1, 1)
        out = (A2J.ang2joint(p3d0, torch.from_numpy(pose[:, :J].copy()), pdict) * scale).numpy()
        assert out.dtype == np.float32
        cases.append(("smpl_%s_p%d" % (name, J_pose), name, "smpl", pose, out, scale, KR.fk_smpl(pose, parent, rest, scale=scale)))
    rec["fk/cases"] = np.array([c[0] for c in cases])
    for cname, tree, conv, ang, out, scale, ref64 in cases:
        err = float(np.abs(out.astype(np.float64) - ref64).max())
        assert 0 < err < 2e-6 * max(1.0, np.abs(ref64).max()) * 64, (cname, err)
        rec.update({"fk/%s/tree" % cname: np.array(tree), "fk/%s/convention" % cname: np.array(conv), "fk/%s/angles" % cname: ang,
                    "fk/%s/out" % cname: out, "fk/%s/scale" % cname: np.float32(scale), "fk/%s/ref_err" % cname: np.float64(err)})
        print("%-22s ref fp32 error %.3e at max |coord| %.1f" % (cname, err, np.abs(ref64).max()))

    # ---- miniature H3.6M directory ----
    input_n, output_n, action = 3, 2, "walking"
    with tempfile.TemporaryDirectory() as tmp:
        names = []
        for subj in (1, 6, 7, 8, 9):
            os.makedirs(os.path.join(tmp, "dataset", "S%d" % subj))
            for subact in (1, 2):
                F = int(g.randint(12, 17))
                a = np.concatenate([g.randn(F, 3) * 100, rotvecs(g, F, 32).reshape(F, -1) * (0.4, 1.6)[subact - 1]], 1).astype(np.float32)
                name = "S%d/%s_%d.txt" % (subj, action, subact)
                np.savetxt(os.path.join(tmp, "dataset", name), a, fmt="%.9g", delimiter=",")
                rec["h36m/file/" + name] = a
                names.append(name)
        ds = H36.H36m_Motion3D(tmp, [action], input_n=input_n, output_n=output_n, split="train", transform=lambda x: x, return_class=True)
        _, joint_names = BU.get_reduced_skeleton(skeleton_type="h36m")
        head = int(np.where(["Head" in j for j in joint_names])[0][0])
        hips = int(np.where(["Site" in j for j in joint_names])[0][0])
        # which windows the fix mirrored: the loader's array before the fix
        all_seqs = DU.load_data_h36m(Path(tmp, "dataset"), [action], input_n, output_n, is_test="train")[0]
        before = np.float32(all_seqs.reshape(all_seqs.shape[0], input_n + output_n, -1, 3))[:, :, ds.dim_used]
        inverted = np.sign(before[:, 0, head, 1] - before[:, 0, hips, 1]) == -1
        assert inverted.any() and (~inverted).any(), "the recording needs inverted and upright windows"
        assert np.array_equal(before[~inverted], ds.target[~inverted])
        rec.update({"h36m/files": np.array(names), "h36m/input_n": np.int32(input_n), "h36m/output_n": np.int32(output_n),
                    "h36m/action": np.array(action), "h36m/target": ds.target, "h36m/class_seq": np.array(ds.class_seq),
                    "h36m/up_joints": np.array([head, hips], dtype=np.int32), "h36m/dim_used": np.asarray(ds.dim_used, dtype=np.int32),
                    "h36m/inverted": inverted})
        print("h36m: %d windows, %d inverted, target %s" % (len(ds.target), int(inverted.sum()), ds.target.shape))

    # ---- miniature AMASS directory ----
    parent, rest = trees["smplh52"]
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "smpl_skeleton.npz"), p3d0=rest[None], parents=parent)
        files = []
        for i, (rate, frames) in enumerate(((50, 30), (100, 64), (120, 52))):
            rel = "train/ACCAD/subject%d/take%d_poses.npz" % (i % 2, i)
            os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
            poses = (g.randn(frames, 156) * 0.4).astype(np.float64)
            np.savez(os.path.join(tmp, rel), poses=poses, mocap_framerate=np.float64(rate))
            rec["amass/poses/%d" % i], rec["amass/rate/%d" % i] = poses.astype(np.float32), np.float64(rate)
            files.append(rel)
        np.savez(os.path.join(tmp, "train/ACCAD/subject0/shape.npz"), betas=np.zeros(16))
        ds = AMS.Amass_Motion3D(tmp, ["ACCAD"], input_n=input_n, output_n=output_n, split="train", transform=lambda x: x, return_class=True)
        rec.update({"amass/p3d0": rest[None], "amass/parents": parent, "amass/files": np.array(files), "amass/target": ds.target,
                    "amass/class_seq": np.array(ds.class_seq), "amass/input_n": np.int32(input_n), "amass/output_n": np.int32(output_n)})
        print("amass: %d windows, target %s" % (len(ds.target), ds.target.shape))

    rec["find256/input_n"], rec["find256/seq_len"] = np.int32(10), np.int32(35)
    for F1, F2 in ((400, 523), (1210, 987)):
        i1, i2 = DU.find_indices_256(F1, F2, 35, input_n=10)
        rec["find256/%d_%d/s1" % (F1, F2)], rec["find256/%d_%d/s2" % (F1, F2)] = i1[:, 0].astype(np.int64), i2[:, 0].astype(np.int64)
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
