#!/usr/bin/env python
"""Seeded value errors against the operator checks, CPU only (tests/MUTANTS.md holds the results in prose).

For every row of tools/mutants_table.py: copy cistgcn_amd/csrc and include/ to a temporary directory, apply the row's ONE edit (the old text
must occur exactly as often as the row says), build the CPU shim library from the copy (tests/hipemu/build_emu.py with CSRC, INCLUDE and
OUT pointed at the copy), run the checks the row names in a child process with device "cpu", and report whether a check failed (the
mutant is killed) and by what margin (error / bound of the comparison that failed; the closest comparison when none failed).

    python tools/mutants.py                 every row, then the unedited sources against every check a row names
    python tools/mutants.py -k eps -k tie   rows whose id contains one of the words
    python tools/mutants.py -j 4            rows in flight at a time

Exit status 0 only if the unedited sources pass every named check and every row is killed by a check it names or is listed, by its id, under
"Survivors that stay" in tests/MUTANTS.md.  The real library is never loaded and nothing here belongs on a GPU machine: the edits change
values only (a constant, an operator, an addend, a salt, a branch), never an index, a bound, a pointer, a launch geometry or a barrier.
Not a test and not collected by pytest."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TESTS = os.path.join(ROOT, "tests")
MARK = "MUTANT_RESULT "


def _spec(check):
    """a check of a row: "module.function" or ("module.function", args after the device, kwargs)"""
    if isinstance(check, str):
        return check, (), {}
    name, args = check[0], tuple(check[1]) if len(check) > 1 else ()
    return name, args, dict(check[2]) if len(check) > 2 else {}


def _label(check):
    name, args, kw = _spec(check)
    inner = ", ".join([repr(a) for a in args] + ["%s=%r" % kv for kv in sorted(kw.items())])
    return "%s(%s)" % (name, inner) if inner else name


# ---- child: build the shim from the tree under `work`, load it, run the checks ---------------------------------------------------------
def child(work, checks):
    os.environ.setdefault("CISTGCN_ABLATION", "1")
    for p in (HERE, ROOT, TESTS, os.path.join(TESTS, "hipemu")):
        sys.path.insert(0, p)
    import ctypes
    import build_emu
    build_emu.CSRC = os.path.join(work, "cistgcn_amd", "csrc")
    build_emu.INCLUDE = os.path.join(work, "include")
    build_emu.OUT = os.path.join(work, "_build", "libcistgcn_emu.so")
    path = build_emu.build()
    assert path.startswith(work)
    from cistgcn_amd import _lib
    _lib._handle = _lib.declare(ctypes.CDLL(path))          # what tests/emu.install() does, for the library of the copy
    _lib._host_pointers_ok = True
    import importlib
    import helpers
    out = []
    for check in checks:
        name, args, kw = _spec(check)
        mod, fn = name.rsplit(".", 1)
        helpers.reset_worst()
        rec = {"check": _label(check), "failed": False, "ratio": None, "message": ""}
        t0 = time.time()
        try:
            getattr(importlib.import_module(mod), fn)("cpu", *args, **kw)
            rec["ratio"], rec["message"] = helpers.WORST[0], helpers.worst_line()
        except AssertionError as e:
            msg = str(e).strip().splitlines()[0] if str(e).strip() else "assert"
            m = re.search(r"max err ([0-9.eE+-]+|nan|inf) > bound ([0-9.eE+-]+)", str(e))
            rec.update(failed=True, message=msg[:300], ratio=(float(m.group(1)) / float(m.group(2))) if m and float(m.group(2)) > 0 else None)
        rec["seconds"] = round(time.time() - t0, 1)
        out.append(rec)
    print(MARK + json.dumps(out))


# ---- parent ----------------------------------------------------------------------------------------------------------------------
def _tree(tmp, name, base_objs):
    """a copy of the sources (the relative places of csrc and include kept: cg_common.h includes the header by its place in the tree) with
    the objects of the unedited build, so that only what an edit touches compiles again"""
    work = os.path.join(tmp, name)
    shutil.copytree(os.path.join(ROOT, "cistgcn_amd", "csrc"), os.path.join(work, "cistgcn_amd", "csrc"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(work, "include"))
    os.makedirs(os.path.join(work, "_build"))
    if base_objs:
        for f in os.listdir(base_objs):
            if f.endswith(".o"):
                shutil.copy2(os.path.join(base_objs, f), os.path.join(work, "_build", f))
    return work


def _run_child(work, checks, timeout=3600):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", work, json.dumps(checks)], capture_output=True, text=True,
                         timeout=timeout, cwd=ROOT)
    for line in reversed(res.stdout.splitlines()):
        if line.startswith(MARK):
            return json.loads(line[len(MARK):]), None
    return None, "child ended with status %d:\n%s" % (res.returncode, (res.stdout[-1500:] + res.stderr[-3000:]))


def _apply(work, row):
    rel = row["file"]
    path = os.path.join(work, rel) if rel.startswith("include") else os.path.join(work, "cistgcn_amd", "csrc", rel)
    text = open(path).read()
    n = text.count(row["old"])
    if n != row.get("count", 1):
        raise SystemExit("%s: the old text occurs %d times in %s, the row says %d:\n%s" % (row["id"], n, rel, row.get("count", 1), row["old"]))
    with open(path, "w") as f:
        f.write(text.replace(row["old"], row["new"]))


def _equivalents():
    """ids listed under "Survivors that stay" in tests/MUTANTS.md"""
    text = open(os.path.join(TESTS, "MUTANTS.md")).read()
    part = text.split("## Survivors that stay", 1)
    return set(re.findall(r"^- `([^`]+)`", part[1].split("\n## ", 1)[0], flags=re.M)) if len(part) == 2 else set()


def _fmt(r):
    return "-" if r is None else ("%.3g" % r)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-k", action="append", default=[], help="only rows whose id contains this word (may be repeated)")
    ap.add_argument("-j", type=int, default=max(1, min(4, (os.cpu_count() or 2) // 2)), help="rows in flight")
    ap.add_argument("--keep", action="store_true", help="keep the temporary trees")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], json.loads(a.child[1]))
    sys.path.insert(0, HERE)
    from mutants_table import ROWS
    ids = [r["id"] for r in ROWS]
    assert len(set(ids)) == len(ids), "row ids repeat"
    rows = [r for r in ROWS if not a.k or any(w in r["id"] for w in a.k)]
    equivalents = _equivalents()
    tmp = tempfile.mkdtemp(prefix="cistgcn_mutants_")
    bad = []
    try:
        # the unedited sources: the objects every row starts from, and every named check must pass on them
        base = _tree(tmp, "unedited", None)
        named = []
        for r in rows:
            for c in r["checks"]:
                if _label(c) not in [_label(x) for x in named]:
                    named.append(c)
        t0 = time.time()
        parts = [named[i::a.j] for i in range(a.j) if named[i::a.j]]
        first, err = _run_child(base, parts[0])
        if err:
            raise SystemExit("unedited sources: " + err)
        with ThreadPoolExecutor(max_workers=a.j) as pool:
            rest = list(pool.map(lambda p: _run_child(base, p), parts[1:]))
        for res, err in [(first, None)] + rest:
            if err:
                raise SystemExit("unedited sources: " + err)
            for rec in res:
                print("unedited  %-62s %s  worst error / bound %s  (%.0f s)" % (rec["check"], "FAILS" if rec["failed"] else "passes", _fmt(rec["ratio"]), rec["seconds"]))
                if rec["failed"]:
                    bad.append("unedited sources fail %s: %s" % (rec["check"], rec["message"]))
        print("unedited sources: %d checks in %.0f s\n" % (len(named), time.time() - t0))

        def one(row):
            work = _tree(tmp, row["id"], os.path.join(base, "_build"))
            _apply(work, row)
            res, err = _run_child(work, row["checks"])
            if not a.keep:
                shutil.rmtree(work, ignore_errors=True)
            return row, res, err

        with ThreadPoolExecutor(max_workers=a.j) as pool:
            results = list(pool.map(one, rows))
        print("%-34s %-10s %-10s %s" % ("row", "outcome", "margin", "check (error / bound; '-': an assertion without a bound)"))
        for row, res, err in results:
            if err:
                print("%-34s ERROR\n%s" % (row["id"], err))
                bad.append("%s: %s" % (row["id"], err.splitlines()[0]))
                continue
            killers = [rec for rec in res if rec["failed"]]
            ratios = [rec["ratio"] for rec in killers if rec["ratio"] is not None]
            if killers:
                best = max(killers, key=lambda rec: float("inf") if rec["ratio"] is None else rec["ratio"])
                print("%-34s %-10s %-10s %s" % (row["id"], "killed", _fmt(max(ratios)) if len(ratios) == len(killers) else "-", best["check"]))
            else:
                stays = row["id"] in equivalents
                closest = max(res, key=lambda rec: rec["ratio"] or 0.0)
                print("%-34s %-10s %-10s %s" % (row["id"], "equivalent" if stays else "SURVIVED", _fmt(closest["ratio"]), closest["check"]))
                if not stays:
                    bad.append("%s survived %s" % (row["id"], ", ".join(rec["check"] for rec in res)))
            for rec in res:
                print("    %-60s %-7s %-10s %s" % (rec["check"], "fails" if rec["failed"] else "passes", _fmt(rec["ratio"]), rec["message"][:160]))
        for i in equivalents - set(ids):
            bad.append("tests/MUTANTS.md lists %s as a survivor that stays, the table has no such row" % i)
    finally:
        if not a.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    print()
    for b in bad:
        print("NOT OK: " + b)
    print("%d rows, %d not ok" % (len(rows), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
