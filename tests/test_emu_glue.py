"""The glue operators on the CPU-only box (the kernel sources through the test-only HIP shim, tests/hipemu): the operand contract of
the wrappers in cistgcn_amd/ops.py, the kernels past their first pass against float64 (tests/glue_shapes.py, tests/glue_checks.py),
and the proof that the shapes take those paths.  tests/test_gpu_glue.py runs the same lists on the MI355X."""
import pytest

import emu
import glue_checks
import glue_shapes as G
import helpers


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


def test_shapes_take_their_paths():
    """the limits come from the library (cg_glue_geometry); a halved shape fails here, before any number is compared"""
    g = G.assert_properties()
    print("glue geometry: %s" % g)
    halved = {"mpjpe_shape": (50,) + G.MPJPE_SHAPE[1:], "adam_linear": (512, 512), "scale_n": G.SCALE_N // 2, "se_gate": ((3, 128, 8), (3, 257, 8), (5, 520, 4), (67, 2, 1)),
              "dstd_lds": (2, 45, 50, 4), "zero_big": (G.ZERO_BIG[0] // 2, G.ZERO_BIG[1]), "reduce_shape": (2, 3, 10, 35), "eval_scatter": (3, 5, 35, 33),
              "dstd_stats": tuple((B, C, T, V) if V != 16 else (B, 8, 32, V) for (B, C, T, V) in G.DSTD_STATS)}      # 256 rows fill the iteration
    for key, value in halved.items():
        with pytest.raises(AssertionError):
            G.assert_properties(**{key: value})


@pytest.mark.parametrize("case", glue_checks.contract_cases(), ids=lambda c: c.name.replace(" ", "_"))
def test_operand_contract(case):
    """float64, strided, transposed and expanded operands one at a time: TypeError / ValueError before any launch, or the bits of the
    contiguous float32 call"""
    print("%s: %s" % (case.name, glue_checks.check_operand_contract("cpu", case)))


def test_unsupported_operands_no_longer_give_wrong_numbers():
    glue_checks.check_issue_table("cpu")


@pytest.mark.parametrize("check", glue_checks.KERNEL_CHECKS, ids=lambda f: f.__name__[len("check_"):])
def test_glue_kernel(check):
    G.assert_properties()
    helpers.reset_worst()
    check("cpu")
    print("%s: %s" % (check.__name__[len("check_"):], helpers.worst_line()))
