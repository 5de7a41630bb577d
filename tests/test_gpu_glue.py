"""The glue operators on the MI355X: the lists of tests/glue_shapes.py through tests/glue_checks.py on "cuda", one case per operator so
that a failure names it.  What only the hardware can show: the DPP row sums and the raised LDS limit of cg_dstd_stats_*, float atomics
of the loss and the SE-gate kernels, the tie rule of the arg-max across waves.  Run with `-m gpu`."""
import pytest
import torch

import glue_checks
import glue_shapes as G
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    from cistgcn_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib._handle = None
    _lib._host_pointers_ok = False
    _lib.lib()          # raises if libcistgcn_hip.so has not been built
    yield


def test_shapes_take_their_paths():
    print("glue geometry: %s" % G.assert_properties())


@pytest.mark.parametrize("case", glue_checks.contract_cases(), ids=lambda c: c.name.replace(" ", "_"))
def test_operand_contract(case):
    print("%s: %s" % (case.name, glue_checks.check_operand_contract("cuda", case)))


def test_unsupported_operands_no_longer_give_wrong_numbers():
    glue_checks.check_issue_table("cuda")


@pytest.mark.parametrize("check", glue_checks.KERNEL_CHECKS, ids=lambda f: f.__name__[len("check_"):])
def test_glue_kernel(check):
    G.assert_properties()
    helpers.reset_worst()
    check("cuda")
    torch.cuda.synchronize()
    print("%s: %s" % (check.__name__[len("check_"):], helpers.worst_line()))
