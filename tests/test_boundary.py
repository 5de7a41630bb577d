"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol of
include/cistgcn_hip.h, the ctypes mirror in cistgcn_amd/_lib.py agrees with that header field by field and argument by argument,
the nn.Module surface mirrors the reference, and nothing runs on the CPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from helpers import CASES, load_case, make_cfg, state_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from cistgcn_amd import _lib, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "cistgcn_hip.h")).read()
    declared = set(re.findall(r"^(?:int|long long) (cg_\w+)\(", header, flags=re.M))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    handle = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(handle, name), name
    _lib.declare(handle)


HEADER = os.path.join(ROOT, "include", "cistgcn_hip.h")


def _binding_structs():
    from cistgcn_amd import _lib
    classes = [c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    return [(_lib.C_STRUCT_NAMES.get(c.__name__, "Cg" + c.__name__), c) for c in classes]


def test_binding_layout_matches_header(tmp_path):
    """The hand-written ctypes classes and the limits table of cistgcn_amd/_lib.py against the header the kernels are compiled with:
    a C++ program that includes only cistgcn_hip.h prints sizeof of every struct, offsetof and sizeof of every field the Python class
    names (array lengths included), and every macro of `_lib.LIMITS`; each number must be the one ctypes computes.  A field the C struct
    does not have fails the compilation; a field the Python class lacks moves sizeof or a later offset."""
    from cistgcn_amd import _lib
    structs = _binding_structs()
    assert len(structs) >= 23 and len({name for name, _ in structs}) == len(structs)
    lines, expected = [], []      # one printed number per entry of `expected`: (struct or "limit", field or macro, ctypes value)
    for cname, cls in structs:
        lines.append("sizeof(%s)" % cname)
        expected.append((cname, "sizeof", ctypes.sizeof(cls)))
        for field in cls._fields_:
            desc = getattr(cls, field[0])
            lines += ["offsetof(%s, %s)" % (cname, field[0]), "sizeof(%s::%s)" % (cname, field[0])]
            expected += [(cname, field[0] + " offset", desc.offset), (cname, field[0] + " size", desc.size)]
    for macro, value in _lib.LIMITS.items():
        lines.append(macro)
        expected.append(("limit", macro, value))
    src = tmp_path / "abi_layout.cpp"
    src.write_text("#include \"cistgcn_hip.h\"\n#include <cstddef>\n#include <cstdio>\nint main() {\n"
                   + "".join("  std::printf(\"%%lld\\n\", (long long)(%s));\n" % e for e in lines) + "  return 0;\n}\n")
    exe = tmp_path / "abi_layout"
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                         capture_output=True, text=True)
    assert res.returncode == 0, "the binding names something the header does not have:\n" + res.stderr[-4000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == len(expected)
    wrong = [(s, f, c, py) for (s, f, py), c in zip(expected, got) if c != py]
    assert not wrong, "%s %s: header %d, ctypes %d (%d numbers differ)" % (wrong[0] + (len(wrong),))


def test_binding_signatures_match_header():
    """Every prototype of the header against its `_lib._SIGNATURES` entry: the number of arguments, then each argument's class.
    `CgX*` needs POINTER of the class that mirrors CgX; `int*` - in the header's prototypes always a HOST array (`out`, `M`,
    `need_reduce`; device integers are `int32_t*`) - needs POINTER(c_int); any other pointer c_void_p; `long long` c_longlong;
    `int` / `unsigned` c_int or c_uint; `float` c_float.  `long long` is returned by exactly the names declare() gives c_longlong."""
    from ctypes import POINTER, c_float, c_int, c_longlong, c_uint, c_void_p
    from cistgcn_amd import _lib
    by_cname = dict(_binding_structs())
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"^(int|long long) (cg_\w+)\(([^)]*)\);", text, flags=re.M)
    assert sorted(name for _, name, _ in protos) == sorted(_lib._SIGNATURES)

    def wanted(param):
        ctype = re.sub(r"\s*\w+$", "", re.sub(r"\bconst\b", "", param).strip())      # without `const` and the parameter's name
        ctype = re.sub(r"\s+", " ", ctype).replace(" *", "*")
        if ctype.endswith("*"):
            base = ctype[:-1]
            return (POINTER(by_cname[base]),) if base.startswith("Cg") else (POINTER(c_int),) if base == "int" else (c_void_p,)
        return {"long long": (c_longlong,), "int": (c_int, c_uint), "unsigned": (c_int, c_uint), "unsigned int": (c_int, c_uint),
                "float": (c_float,)}[ctype]

    for _, name, params in protos:
        params = [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
        argtypes = _lib._SIGNATURES[name]
        assert len(argtypes) == len(params), "%s: header has %d arguments, _SIGNATURES %d" % (name, len(params), len(argtypes))
        for i, (param, got) in enumerate(zip(params, argtypes)):
            assert got in wanted(param), "%s argument %d (%s): _SIGNATURES has %s" % (name, i, param, got.__name__)

    class _Fn:
        pass
    handle = type("Handle", (), {name: _Fn() for name in _lib.EXPORTS})
    _lib.declare(handle)
    returns_ll = {name for name in _lib.EXPORTS if getattr(handle, name).restype is c_longlong}
    assert all(getattr(handle, name).restype in (c_int, c_longlong) for name in _lib.EXPORTS)
    assert returns_ll == {name for ret, name, _ in protos if ret == "long long"}, returns_ll ^ {n for r, n, _ in protos if r == "long long"}


def test_registry_and_choose_net_errors():
    from cistgcn_amd import models
    assert models.CISTGCN_0 is models.CISTGCN_eval
    assert models.CISTGCN_0.__name__ == "CISTGCN"          # callers branch on the class name (test.py:99)
    assert models.CISTGCN_0.__module__.endswith("models.CISTGCN.CISTGCN")
    with pytest.raises(ValueError):
        models.choose_net("NoSuchNet", None)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_reference_manifest(name):
    from cistgcn_amd.models import CISTGCN_0
    rec = load_case(name)
    C, T, V, _ = [int(v) for v in rec["meta"]]
    net = CISTGCN_0(*make_cfg(C, T, V))
    ref = state_of(rec)
    sd = net.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(tuple(sd[k].shape) == tuple(ref[k].shape) for k in sd)
    net.load_state_dict(ref, strict=True)


def test_same_seed_same_init_as_oracle():
    from cistgcn_amd.models import CISTGCN_0
    from oracle import cistgcn_ref as O
    torch.manual_seed(0)
    a = CISTGCN_0(*make_cfg(16, 10, 22)).state_dict()
    torch.manual_seed(0)
    b = O.CISTGCN(*make_cfg(16, 10, 22)).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in b)


def test_ctor_keeps_config_lists_intact():
    from cistgcn_amd.models import CISTGCN_0
    arch, learn = make_cfg(8, 10, 22)
    CISTGCN_0(arch, learn)
    CISTGCN_0(arch, learn)
    assert arch.model_params.input_gcn.model_complexity == [8] * 4
    assert arch.model_params.output_gcn.model_complexity == [3]


def test_no_cpu_path():
    from cistgcn_amd import _lib, ops
    from cistgcn_amd.models import CISTGCN_0
    _lib._host_pointers_ok = False
    net = CISTGCN_0(*make_cfg(8, 10, 22))
    with pytest.raises(RuntimeError):
        net(torch.zeros(2, 10, 22, 3))
    with pytest.raises(RuntimeError):
        ops.mpjpe(torch.zeros(2, 3), torch.zeros(2, 3))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "cistgcn_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f


def test_reference_checkpoint_layout_loads(tmp_path):
    """Checkpoint I/O compatibility: a `*.pth.tar` written the way the reference does
    (train.py:184-194 via environment/utils.py:60-66: {epoch, lr, err, metric_used_to_save, state_dict, optimizer})
    loads by key into the MI355X model exactly as model_loader.py:24-26 does it."""
    from cistgcn_amd.models import CISTGCN_0
    from oracle import cistgcn_ref as O
    torch.manual_seed(1)
    src = O.CISTGCN(*make_cfg(8, 10, 22))
    opt = torch.optim.Adam(src.parameters(), lr=1e-2, weight_decay=1e-4)
    path = os.path.join(tmp_path, "CISTGCN_0_best.pth.tar")
    torch.save({"epoch": 3, "lr": 1e-2, "err": 42.0, "metric_used_to_save": "mpjpe", "state_dict": src.state_dict(),
                "optimizer": opt.state_dict()}, path)
    ckpt = torch.load(path, map_location="cpu")
    net = CISTGCN_0(*make_cfg(8, 10, 22))
    missing = net.load_state_dict(ckpt["state_dict"])
    assert not missing.missing_keys and not missing.unexpected_keys
    assert ckpt["epoch"] == 3 and ckpt["err"] == 42.0
    sd = net.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in src.state_dict().items())


def test_no_memset_nodes_in_the_library():
    """hipMemsetAsync as a node of a captured HIP graph was not reliably ordered against the kernels around it on ROCm 7.2
    (tests/test_gpu_parity.py::test_graph_replay_survives_allocator_churn): the library zero-fills with a kernel only."""
    import glob
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cistgcn_amd", "csrc")
    for path in glob.glob(os.path.join(root, "*.hip")):
        code = "\n".join(line.split("//")[0] for line in open(path).read().splitlines())
        assert "hipMemsetAsync" not in code and "hipMemset(" not in code, path
