"""The generator of cg_draw_augmentation restated from its specification in include/cistgcn_hip.h, with Python integers mod 2^64 and
numpy scalars - not an import of the kernel, the operator or the host draws of the product.

  bits(seed, salt, counter)   the splitmix64 finaliser of the dropout hash
  u = (bits >> 40) * 2^-24    in [0, 1), exact in fp32
  parameters                  salt = DRAW_SALT + stream, counter = (b * n_steps + step) * 4 + slot (slot 0 the coin, 1 - 3 the amounts; a
                              flip: the coins of x, y, z in slots 0 - 2)
  noise                       salt = DRAW_SALT + 0x10000 + stream, counter = ((b * n_noise + noise_slot) * J + j) * 3 + axis, 2 u - 1
  applies iff u > threshold (fp32); amount = lo + (hi - lo) * u in f64 on the fp32 bounds, rounded once

A step is (kind, threshold, lo[3], hi[3]) with kind one of KINDS; flip: lo[a] != 0 enables axis a; noise: the amplitude is lo[0]."""
import numpy as np

M64 = (1 << 64) - 1
DRAW_SALT = 0x800000
KINDS = ("rotation", "scale", "noise", "translation", "flip", "invert")


def bits(seed, salt, counter):
    z = (counter + seed * 0x9E3779B97F4A7C15 + (salt << 40) + 0x632BE59BD9B4E019) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform(seed, salt, counter):
    """u as a Python float: k / 2^24 with k < 2^24 is exact in fp32 (and in f64)"""
    return (bits(seed & M64, salt, counter) >> 40) * 2.0 ** -24


def bump(seed):
    """what cg_seed_bump does to the seed word"""
    return (seed * 6364136223846793005 + 1442695040888963407) & M64


def param_counter(b, n_steps, step, slot):
    return (b * n_steps + step) * 4 + slot


def noise_counter(b, n_noise, noise_slot, J, j, axis):
    return ((b * n_noise + noise_slot) * J + j) * 3 + axis


def uniforms(seed, stream, B, n_steps):
    """(B, n_steps, 4) f64: u of every parameter slot"""
    out = np.zeros((B, n_steps, 4))
    for b in range(B):
        for i in range(n_steps):
            for s in range(4):
                out[b, i, s] = uniform(seed, DRAW_SALT + stream, param_counter(b, n_steps, i, s))
    return out


def amount(lo, hi, u):
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    return np.float32(lo + (hi - lo) * np.float64(u))


def rotvec_matrix(deg):
    """Rodrigues' formula in f64 on fp32 degrees, rounded to fp32 once; row-major, p' = p R"""
    v = np.asarray(deg, dtype=np.float32).astype(np.float64) * (np.pi / 180.0)
    th = float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    if not th > 0.0:
        return np.eye(3, dtype=np.float32)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return (np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)).astype(np.float32)


def step_rows(steps, seed, stream, B):
    """(B, n_steps, 4) fp32 [apply?, v0, v1, v2]: the CG_DRAW_STEPS4 table"""
    n = len(steps)
    u = uniforms(seed, stream, B, n)
    out = np.zeros((B, n, 4), dtype=np.float32)
    for b in range(B):
        for i, (kind, thr, lo, hi) in enumerate(steps):
            thr = np.float32(thr)
            if kind == "flip":
                for a in range(3):
                    out[b, i, 1 + a] = float(np.float32(lo[a]) != 0 and np.float32(u[b, i, a]) > thr)
                out[b, i, 0] = float(out[b, i, 1:].any())
                continue
            if not np.float32(u[b, i, 0]) > thr:
                continue
            out[b, i, 0] = 1.0
            if kind == "noise":
                out[b, i, 1] = np.float32(lo[0])
            elif kind != "invert":
                out[b, i, 1:] = [amount(lo[a], hi[a], u[b, i, 1 + a]) for a in range(3)]
    return out


def table24(steps, seed, stream, B):
    """(B, 24) fp32: the CG_DRAW_TABLE24 table.  The steps are walked in order, each writing the columns of its kind - the identity when
    it does not apply -, so of a kind that occurs twice the last step stands."""
    rows = step_rows(steps, seed, stream, B)
    out = np.zeros((B, 24), dtype=np.float32)
    out[:, 13:16] = 1.0
    for b in range(B):
        for i, (kind, _, _, _) in enumerate(steps):
            on, v = rows[b, i, 0] != 0, rows[b, i, 1:]
            if kind == "flip":
                out[b, 0:3] = v
            elif kind == "rotation":
                out[b, 3] = float(on)
                out[b, 4:13] = rotvec_matrix(v).reshape(-1) if on else 0.0
            elif kind == "scale":
                out[b, 13:16] = v if on else 1.0
            elif kind == "translation":
                out[b, 16:19] = v if on else 0.0
            elif kind == "noise":
                out[b, 19] = v[0] if on else 0.0
            else:
                out[b, 20] = float(on)
    return out


def noise_table(steps, seed, stream, B, J):
    """(B, n_noise, J, 3) fp32 of U(-1, 1), or None without a noise step"""
    n_noise = sum(kind == "noise" for kind, _, _, _ in steps)
    if not n_noise:
        return None
    out = np.zeros((B, n_noise, J, 3), dtype=np.float32)
    salt = DRAW_SALT + 0x10000 + stream
    for b in range(B):
        for s in range(n_noise):
            for j in range(J):
                for a in range(3):
                    out[b, s, j, a] = np.float32(2.0 * uniform(seed, salt, noise_counter(b, n_noise, s, J, j, a)) - 1.0)
    return out
