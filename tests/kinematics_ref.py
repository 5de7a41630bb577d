"""fp64 numpy restatement of the two forward-kinematics conventions and of the window gather (include/cistgcn_hip.h:
CgForwardKinematics, CgGatherWindows), written after the reference's lines and independent of the kernels:
  fk_chain   utils/forward_kinematics.py::fkl_torch (:219-241) with utils/data_utils.py::expmap2rotmat_torch (:1175-1194)
  fk_smpl    utils/ang2joint.py::ang2joint (:11-58) with rodrigues (:64-91), without its N(0, 1e-8) noise
  gather     the_sequence[fs_sel] (data_utils.py:891-896), target[:, :, dim_used], (x - mean) / std and the inversion fix of
             H36m_Motion3D.__init__ (loaders/h36m_motion_3d.py:62-74)
tools/gen_golden_kinematics.py records the reference's own fp32 error against these per fixture case."""
import numpy as np


def _skew(k):
    """(N,3) -> (N,3,3) with K[0,1] = -kz, K[0,2] = ky, K[1,2] = -kx, antisymmetric"""
    K = np.zeros(k.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -k[..., 2], k[..., 1], -k[..., 0]
    return K - np.swapaxes(K, -1, -2)


def fk_chain(angles, parent, rest, select=None, scale=1.0):
    """angles (N, 3 + 3J) -> (N, J_out, 3) in fp64.  Only joints with parent[i] > 0 compose (the reference's quirk)."""
    angles, rest = np.asarray(angles, dtype=np.float64), np.asarray(rest, dtype=np.float64)
    J, N = len(parent), angles.shape[0]
    r = angles[:, 3:].reshape(N, J, 3)
    th = np.linalg.norm(r, axis=-1)
    K = _skew(r / (th[..., None] + 1e-7))
    R = np.eye(3) + np.sin(th)[..., None, None] * K + (1.0 - np.cos(th))[..., None, None] * (K @ K)
    p = np.broadcast_to(rest, (N, J, 3)).copy()
    for i in range(1, J):
        if parent[i] > 0:
            R[:, i] = R[:, i] @ R[:, parent[i]]
            p[:, i] = np.einsum("k,nkc->nc", rest[i], R[:, parent[i]]) + p[:, parent[i]]
    out = p if select is None else p[:, list(select)]
    return out * float(np.float32(scale))


def fk_smpl(pose, parent, rest, select=None, scale=1.0):
    """pose (N, J_pose, 3), the first J = len(parent) joints are read -> (N, J_out, 3) in fp64; theta == 0 gives R = I exactly."""
    pose, rest = np.asarray(pose, dtype=np.float64), np.asarray(rest, dtype=np.float64)
    J, N = len(parent), pose.shape[0]
    r = pose[:, :J]
    th = np.linalg.norm(r, axis=-1)
    zero = th == 0.0
    k = r / np.where(zero, 1.0, th)[..., None]
    R = (np.cos(th)[..., None, None] * np.eye(3) + (1.0 - np.cos(th))[..., None, None] * (k[..., :, None] * k[..., None, :])
         + np.sin(th)[..., None, None] * _skew(k))
    R[zero] = np.eye(3)
    Rg, t = R.copy(), np.broadcast_to(rest, (N, J, 3)).copy()
    for i in range(1, J):
        q = parent[i]
        if q < 0:
            continue
        t[:, i] = np.einsum("nck,k->nc", Rg[:, q], rest[i] - rest[q]) + t[:, q]
        Rg[:, i] = Rg[:, q] @ R[:, i]
    out = t if select is None else t[:, list(select)]
    return out * float(np.float32(scale))


def gather(frames, starts, items, L, select=None, mean=0.0, std=1.0, up_joints=None):
    """Returns (raw fp64 (B,L,J,3), flipped (B,) bool).  frames: fp32, or - without normalisation - the fp64 output of fk_* above (a
    pipeline restated in fp64 end to end).  The normalisation is the kernel's fp32 `(v - mean) / std` (exact where it is off); the
    flip decision is taken on the fp32 values, strictly `< 0`; the centroid and the mirrored y are fp64."""
    frames = np.asarray(frames)
    idx = np.asarray(starts, dtype=np.int64)[np.asarray(items, dtype=np.int64)][:, None] + np.arange(L)[None, :]
    raw = frames[idx]
    if select is not None:
        raw = raw[:, :, list(select)]
    if not (float(mean) == 0.0 and float(std) == 1.0):
        assert raw.dtype == np.float32
        raw = (raw - np.float32(mean)) / np.float32(std)
        assert raw.dtype == np.float32
    raw32 = raw.astype(np.float32)
    flipped = np.zeros(raw.shape[0], dtype=bool)
    out = raw.astype(np.float64)
    if up_joints is not None:
        hi, lo = up_joints
        flipped = (raw32[:, 0, hi, 1] - raw32[:, 0, lo, 1]) < 0
        c = out[:, :, :, 1].mean((1, 2))
        out[flipped, :, :, 1] = c[flipped, None, None] - out[flipped, :, :, 1]
    return out, flipped
