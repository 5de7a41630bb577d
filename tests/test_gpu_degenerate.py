"""Constant rows, channels and samples in the block statistics on the MI355X: the lists of tests/degenerate_checks.py on "cuda", one case
per check so that a failure names it.  What only the hardware can show: the DPP row sums and the equal-values count of
cg_dstd_stats_*, the contraction of `a * b + c` the compiler chooses in the sums of squares.  Run with `-m gpu`."""
import pytest
import torch

import degenerate_checks as D
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


@pytest.mark.parametrize("check", D.KERNEL_CHECKS, ids=lambda f: f.__name__[len("check_"):])
def test_degenerate_kernel(check):
    helpers.reset_worst()
    check("cuda")
    torch.cuda.synchronize()
    print("%s: %s" % (check.__name__[len("check_"):], helpers.worst_line()))


@pytest.mark.parametrize("edit,fused,mode", D.MODEL_CASES, ids=lambda v: {True: "fused", False: "unfused"}.get(v, v))
def test_degenerate_model(edit, fused, mode):
    helpers.reset_worst()
    D.check_model_degenerate("cuda", edit, fused, mode)
    torch.cuda.synchronize()
    print("model %s %s %s: %s" % (edit, "fused" if fused else "unfused", mode, helpers.worst_line()))
