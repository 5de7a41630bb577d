"""Shared test helpers: golden-fixture loading, config objects, the tolerance rule."""
import glob
import os
from types import SimpleNamespace as NS

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# model fixtures (tools/gen_golden.py); eval_*.npz belong to the evaluation-harness counterpart (tools/gen_golden_eval.py)
# (a model fixture is stored as <case>.part0.npz, <case>.part1.npz, ...: tools/gen_golden.save_case keeps each file under 1 MiB)
CASES = sorted({n for n in (os.path.basename(p).split(".")[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz"))) if not n.startswith(("eval_", "aug_"))})


def make_cfg(C, T, V, dropout=0.0, To=25, hidden=64, interp=None, interp_o=(True,), blocks=4, txc=4, widths=None):
    """Attribute-style config with the schema of the reference YAML (train_h36m.yaml:1-28); `blocks` / `txc` shrink the
    depth (model_complexity entries, n_txcnn_layers) for the emulated CPU runs; `widths` gives model_complexity entry by entry
    (non-uniform layers) in place of `[C] * blocks`."""
    widths = [C] * blocks if widths is None else list(widths)
    interp = (True,) * (len(widths) + 1) if interp is None else interp
    arch = NS(model_params=NS(
        input_n=T, output_n=To, joints=V, n_txcnn_layers=txc, txc_kernel_size=3, reduction=8,
        hidden_dim=hidden, clipping=15,
        input_gcn=NS(model_complexity=widths, interpretable=list(interp)),
        output_gcn=NS(model_complexity=[3], interpretable=list(interp_o))))
    return arch, NS(dropout=dropout)


_cache = {}


def case_files(name):
    """<name>.npz, or the parts <name>.part0.npz, <name>.part1.npz, ... in order"""
    whole = os.path.join(GOLDEN_DIR, name + ".npz")
    if os.path.exists(whole):
        return [whole]
    parts = glob.glob(os.path.join(GOLDEN_DIR, glob.escape(name) + ".part*.npz"))
    if not parts:
        raise FileNotFoundError("no golden fixture %s(.part*).npz under %s" % (name, GOLDEN_DIR))
    return sorted(parts, key=lambda p: int(p[:-len(".npz")].rsplit(".part", 1)[1]))


def load_case(name):
    if name not in _cache:
        rec = {}
        for path in case_files(name):
            z = np.load(path)
            rec.update({k: z[k] for k in z.files})
        _cache[name] = rec
    return _cache[name]


def state_of(rec):
    return {k[len("state/"):]: torch.from_numpy(v.copy()) for k, v in rec.items() if k.startswith("state/")}


def tol_ok(a, ref, rel=1e-4, floor=1.0):
    """SURVEY §7 rule: max|a-b| <= 1e-4 * max(floor, max|ref|) per tensor (fp32 north_star tolerance)."""
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    err = float(np.abs(a - ref).max()) if a.size else 0.0
    bound = rel * max(floor, float(np.abs(ref).max()) if ref.size else 0.0)
    return err <= bound, err, bound


# the comparison of this process that came closest to its bound since `reset_worst()`: [error / bound, what, error, bound]
WORST = [0.0, "", 0.0, 0.0]


def reset_worst():
    WORST[:] = [0.0, "", 0.0, 0.0]


def worst_line():
    return "worst error / bound %.3f (%s: %.3e against %.3e)" % tuple(WORST)


def assert_close(a, ref, what, rel=1e-4, floor=1.0):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    if isinstance(ref, torch.Tensor):
        ref = ref.detach().cpu().numpy()
    ok, err, bound = tol_ok(a, ref, rel, floor)
    assert ok, "%s: max err %.3e > bound %.3e" % (what, err, bound)
    if bound > 0.0 and err / bound > WORST[0]:
        WORST[:] = [err / bound, what, err, bound]


def grad_summary(g):
    f = g.detach().cpu().flatten().double()
    return np.concatenate([[f.sum().item(), f.abs().sum().item(), f.norm().item()], f[:61].numpy()])


def assert_grads_close(named_got, named_ref, what=""):
    """Parameter-gradient comparison that tolerates PReLU-kink sign flips.

    A pre-activation within fp32 rounding of 0 may take the other PReLU branch in another fp32 implementation
    (the reference's CPU path does it too against its own fp64 run: the branch-replay tests print the flip counts).
    One flipped element changes dy there by (1-alpha)*dy, i.e. a few percent of every weight-gradient entry of that
    output channel (sum of ~N random terms, one of them changed) and of scalar gradients such as a PReLU slope.
    So with the real slopes tensors are compared in relative L2 norm with a 5 % bound (plus a floor for
    analytically-zero gradients); a real defect gives O(100 %) and still fails.  The tight bound (1e-4) is enforced on
    the kink-free network in checks.check_model_vs_oracle(smooth=True)."""
    def arr(v):
        return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    norms = {k: float(np.linalg.norm(arr(v))) / max(1, arr(v).size) ** 0.5 for k, v in named_ref.items()}   # rms
    med = float(np.median([s for s in norms.values() if s > 0.0] or [0.0]))
    for k, ref in named_ref.items():
        ref, got = arr(ref), arr(named_got[k])
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        err = float(np.linalg.norm(got - ref)) / max(1, ref.size) ** 0.5
        # scalar-like tensors (PReLU slopes, 3-channel BN) are single cancelling sums: one flip moves them by O(10 %)
        rel, floor = (5e-2, 2e-3) if ref.size >= 16 else (0.25, 0.2)
        bound = max(rel * norms[k], floor * med)
        assert err <= bound, "%s grad %s: rms err %.3e > bound %.3e (rms|ref| %.3e, median rms %.3e)" % (what, k, err, bound, norms[k], med)


# ---------------------------------------------------------------------------------------------------------
# flip-aware gradient comparison: the oracle replays the PReLU branches the HIP run took
# ---------------------------------------------------------------------------------------------------------
class BranchReplay:
    """Context manager around an oracle forward/backward.  `trace` is `net.act_trace` of the HIP run ({PReLU module ->
    (output, post-activation addend)}); inside the context every PReLU of the oracle takes, element by element, the
    branch the HIP run took, so that both implementations differentiate the SAME piecewise-linear function and the
    strict fp32 bound applies to every parameter gradient.  A pre-activation within fp32 rounding of 0 may legitimately
    land on the other side in another fp32 implementation; those elements are counted (`flips`) and their
    pre-activations checked to be rounding-sized (`worst`), so a systematic disagreement still fails."""

    def __init__(self, net, ora, trace):
        from oracle import cistgcn_ref as O
        self.O = O
        self.masks = {}
        self.flips, self.elements, self.worst, self.sites = 0, 0, 0.0, 0
        if net is None:
            return
        names = {m: n for n, m in net.named_modules()}
        omods = dict(ora.named_modules())
        for mod, (y, add) in trace.items():
            y = y.detach().cpu()
            if add is None:
                pos, known = y > 0, torch.ones_like(y, dtype=torch.bool)
            else:                       # y = PReLU(.) + add: the sign of y - add is the branch, or 0 = not recoverable
                d = y - add.detach().cpu().expand_as(y)
                pos, known = d > 0, d != 0
            self.masks[omods[names[mod]]] = (pos, known)

    @classmethod
    def from_golden(cls, rec, ora, prefix="train/branch/"):
        """the branches the REAL reference took on this fixture (tools/gen_golden.py: forward hooks on its nn.PReLU modules, `input > 0`
        bit-packed under `<prefix><module name>`)"""
        self = cls(None, ora, None)
        omods = dict(ora.named_modules())
        for k, bits in rec.items():
            if k.startswith(prefix):
                pos = torch.from_numpy(np.unpackbits(bits).astype(bool))
                self.masks[omods[k[len(prefix):]]] = (pos, None)
        assert self.masks, "the fixture holds no branch record"
        return self

    def __enter__(self):
        self._orig = self.O._act

        def act(x, m):
            alpha = m.weight.reshape((1, -1) + (1,) * (x.dim() - 2)) if m.weight.numel() > 1 else m.weight
            own = x > 0
            rec = self.masks.get(m)
            # a record read off the sign of an OUTPUT needs a positive slope; a recorded input sign (fixture bits) does not
            if rec is None or (rec[1] is not None and not bool((m.weight > 0).all())):
                return self._orig(x, m)
            pos, known = rec
            if known is None:           # bit-packed record: padded to a multiple of eight
                pos = pos[:own.numel()].view_as(own)
            else:
                pos = torch.where(known.view_as(own), pos.view_as(own), own)
            diff = pos != own
            n = int(diff.sum())
            self.sites += 1
            self.elements += own.numel()
            if n:
                self.flips += n
                scale = float(x.detach().abs().mean()) + 1e-30
                self.worst = max(self.worst, float(x.detach().abs()[diff].max()) / scale)
            return torch.where(pos, x, alpha * x)

        self.O._act = act
        return self

    def __exit__(self, *exc):
        self.O._act = self._orig
        return False


# ---------------------------------------------------------------------------------------------------------
# dropout: the oracle applies the very masks the HIP run drew
# ---------------------------------------------------------------------------------------------------------
def hip_keep_scale(seed, salt, p, n):
    """numpy restatement of cg_drop_scale (cistgcn_amd/csrc/cg_common.h: cg_drop_bits / cg_drop_pick) for the flat element indices
    0 .. n-1 of a tensor: splitmix64 of (seed word, site id, index / 4), 16 bits per element, keep when bits >= p * 65536;
    returns the float32 factors 0 or 1 / (1 - p)."""
    mask64 = (1 << 64) - 1
    base = ((int(seed) & mask64) * 0x9E3779B97F4A7C15 + ((int(salt) & 0xFFFFFFFF) << 40) + 0x632BE59BD9B4E019) & mask64
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (idx >> np.uint64(2)) + np.uint64(base)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    bits = (z >> (np.uint64(16) * (idx & np.uint64(3)))) & np.uint64(0xFFFF)
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(bits >= thr, scale, np.float32(0.0)).astype(np.float32)


class DropReplay:
    """Context manager around an oracle forward/backward in train mode with dropout: every dropout site of the oracle multiplies by the
    keep factors the HIP kernels generated for that site (`net.drop_trace`: site module -> site id; `seed`: the device seed word the HIP
    forward ran with; element index = flat index of the site's logical (B, C, ...) tensor), so both implementations evaluate the same
    function and the fp32 bound applies to the configuration the benchmark times (dropout 0.1)."""

    def __init__(self, net, ora, drop_trace, seed, p):
        names = {m: n for n, m in net.named_modules()}
        omods = dict(ora.named_modules())
        self.salts = {omods[names[mod]]: salt for mod, salt in drop_trace.items()}
        self.ora, self.seed, self.p = ora, seed, float(p)
        self.sites, self.elements, self.dropped = 0, 0, 0

    def __enter__(self):
        def hook(x, site):
            salt = self.salts.get(site)
            assert salt is not None, "dropout site %r of the oracle has no counterpart in the HIP run" % (site,)
            keep = torch.from_numpy(hip_keep_scale(self.seed, salt, self.p, x.numel())).view(x.shape).to(x.dtype)
            self.sites += 1
            self.elements += x.numel()
            self.dropped += int((keep == 0).sum())
            return x * keep

        self.ora.drop_hook = hook
        return self

    def __exit__(self, *exc):
        self.ora.drop_hook = None
        return False


def assert_grads_strict(named_got, named_ref, what="", rel=1e-4, floor=1.0, rel_bound=None, rel_min_ref=1e-4, report=None, rel_abs=3e-7, rel_min_size=16):
    """north_star tolerance on every parameter gradient: max|a-b| <= rel * max(floor, max|ref|) per tensor.
    Most gradient tensors of this network are far smaller than the floor (median max|g| ~ 1e-2), so the rule above alone is an
    ABSOLUTE bound for them.  `rel_bound` adds a relative one: max|a-b| <= rel_bound * max|ref| + rel_abs for every tensor of at least 16
    entries with max|ref| >= rel_min_ref (analytically-zero gradients - biases in front of a train-mode BatchNorm - stay under the absolute
    rule only).  `rel_abs` (3e-7) is the fp32 summation noise of a gradient whose terms cancel: an entry of 1e-4 that is the sum
    of B*T*V terms of 1e-2 cannot be reproduced to 2e-3 of ITSELF by any other summation order (seen: 2.7e-7 on a tensor with
    max|g| = 1.3e-4, the only one of 650 above 1.1e-4 relative).  `report` (a dict) receives the distribution of the raw
    relative errors."""
    worst = (0.0, None)
    rels = []
    ranked = []
    for k, ref in named_ref.items():
        got = named_got[k]
        got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
        ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
        ok, err, bound = tol_ok(got, ref, rel, floor)
        ranked.append((err / bound, k, err, float(np.abs(ref).max()) if ref.size else 0.0))
    ranked.sort(reverse=True)
    listing = "; ".join("%s %.2f of the bound (err %.2e, max|ref| %.2e)" % (k, r, e, m) for r, k, e, m in ranked[:6])
    for k, ref in named_ref.items():
        got = named_got[k]
        got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
        ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
        ok, err, bound = tol_ok(got, ref, rel, floor)
        assert ok, "%s grad %s: max err %.3e > bound %.3e; the six tensors closest to the bound: %s" % (what, k, err, bound, listing)
        if err / bound > worst[0]:
            worst = (err / bound, k)
        mx = float(np.abs(ref).max()) if ref.size else 0.0
        if mx >= rel_min_ref and ref.size >= rel_min_size:     # single numbers (the gradient of a shared PReLU slope: one fp32 sum over the negative side
            rels.append((err / mx, k, mx))           # of a whole tensor on the reference side) stay under the absolute rule: seen at 0.5 % of
            if rel_bound is not None:                # 5.5e-4 in one run and at 0.01 % in the others, same code, same seeds, same box type
                assert err <= rel_bound * mx + rel_abs, "%s grad %s: error %.3e > %.1e * max|ref| (%.3e) + %.1e" % (what, k, err, rel_bound, mx, rel_abs)
    if rels:
        rels.sort()
        vals = np.array([r[0] for r in rels])
        dist = {"tensors": len(rels), "median": float(np.median(vals)), "p90": float(np.percentile(vals, 90)), "p99": float(np.percentile(vals, 99)),
                "max": float(vals[-1]), "max_tensor": rels[-1][1], "max_tensor_ref": rels[-1][2]}
        if report is not None:
            report.update(dist)
    return worst
