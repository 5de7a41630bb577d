#!/usr/bin/env python3
"""Fingerprint of the host operators: every C-ABI call of one training and one evaluation step (forward + backward) of five launch
plans on the CPU shim (tests/hipemu), no GPU.  The full log has one line per call with the entry point and every argument - structs
expanded field by field (null / zero fields left out), scalars as `repr`, pointers as set / null only.  Two trees whose full logs are
byte-identical marshal the same arguments into the same launches:
    python tools/call_log.py DIGEST.txt [FULL.txt]
The digest is what a person can read: per step the number of calls and the SHA-256 of its part of the full log, per entry point
the number of calls and a hash of their lines, and the first call of every entry point in full."""
import ctypes, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import checks, emu
from cistgcn_amd import ops, _lib

CONFIGS = (("fused", (8, 10, 22), {}, False), ("one-launch-per-op", (8, 10, 22), {"staged": False}, False),
           ("generic-domain", (8, 10, 22), {"fused": False}, False), ("branch-records", (8, 10, 22), {}, True),
           ("width-changing", (64, 10, 22), {}, False))
B = 6
BLANK = ("null", "0", "0.0", "{}", "[]")      # a struct field that is null / zero throughout is left out, such an array is written []


def show(v, tp=None):
    """one value as text; `tp` is the declared type of a struct field or array element (their reads lose it)"""
    tp = tp or type(v)
    if tp is ctypes.c_void_p or v is None:
        return "set" if (v.value if isinstance(v, ctypes.c_void_p) else v) else "null"
    if issubclass(tp, ctypes.Structure):
        fields = [(f[0], show(getattr(v, f[0]), f[1])) for f in tp._fields_]
        return "{" + " ".join("%s=%s" % f for f in fields if f[1] not in BLANK) + "}"
    if issubclass(tp, ctypes.Array):
        elems = [show(e, tp._type_) for e in v]
        return "[" + " ".join(elems) + "]" if any(e not in BLANK for e in elems) else "[]"
    return repr(getattr(v, "value", v))


def line(name, args):
    out = []
    for i, a in enumerate(args):
        if hasattr(a, "_obj"):                         # byref(struct)
            a = a._obj
        elif hasattr(a, "contents"):                   # pointer into an array: as many elements as the count behind it says
            n = next(b for b in args[i + 1:] if isinstance(b, int))
            a = [a[k] for k in range(n)]
        out.append("[" + " ".join(show(e) for e in a) + "]" if isinstance(a, list) else show(a))
    return name + " " + " ".join(out)


def digest(log):
    """the lines of the digest from the full log (`# ...` lines open a step)"""
    sha = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()
    out, sample, steps = [], {}, []
    for l in log:
        if l.startswith("#"):
            steps.append((l[2:], []))
        else:
            steps[-1][1].append(l)
            sample.setdefault(l.split(" ", 1)[0], l)
    for head, ls in steps:
        out.append("## %s: %d calls, sha256 %s" % (head, len(ls), sha(ls)))
        by = {}
        for l in ls:
            by.setdefault(l.split(" ", 1)[0], []).append(l)
        out += ["%s %d %s" % (name, len(v), sha(v)[:16]) for name, v in by.items()]      # in the order of their first call
    return out + ["## the first call of every entry point"] + list(sample.values())


def main(path, full=None):
    emu.install()
    orig, log = _lib.call, []

    def call(name, *args):
        log.append(line(name, args))
        orig(name, *args)

    _lib.call = call
    for tag, (C, T, V), kw, trace in CONFIGS:
        net, _ = checks.build_pair(C, T, V, "cpu", dropout=0.1, stack_all=True, **kw)
        g = torch.Generator().manual_seed(7)
        x = 50 + 350 * torch.randn(B, T, V, 3, generator=g)
        tgt = x[:, -1:] + 20 * torch.randn(B, 25, V, 3, generator=g)
        for train in (True, False):
            log.append("# %s C=%d T=%d V=%d B=%d %s" % (tag, C, T, V, B, "train" if train else "eval"))
            net.train(train)
            net.act_trace = {} if trace else None
            ops.manual_seed(1234, "cpu")
            ops.begin_step("cpu")
            xd = x.clone().requires_grad_(True)
            ops.mpjpe(net(xd)[0], tgt).backward()
    _lib.call = orig
    if full:
        with open(full, "w") as f:
            f.write("\n".join(log) + "\n")
    with open(path, "w") as f:
        f.write("\n".join(digest(log)) + "\n")
    print("%d calls -> %s" % (sum(not l.startswith("#") for l in log), path))


if __name__ == "__main__":
    main(*sys.argv[1:3])
