"""Constant rows, channels and samples in the block statistics on the CPU-only box (the kernel sources through the test-only HIP shim,
tests/hipemu): ops.dstd_stats and ops.block_input against float64 autograd, and the whole model on a planar batch and on a padded one
(tests/degenerate_checks.py).  tests/test_gpu_degenerate.py runs the same lists on the MI355X."""
import pytest

import degenerate_checks as D
import emu
import helpers


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("check", D.KERNEL_CHECKS, ids=lambda f: f.__name__[len("check_"):])
def test_degenerate_kernel(check):
    helpers.reset_worst()
    check("cpu")
    print("%s: %s" % (check.__name__[len("check_"):], helpers.worst_line()))


@pytest.mark.parametrize("edit,fused,mode", D.MODEL_CASES, ids=lambda v: {True: "fused", False: "unfused"}.get(v, v))
def test_degenerate_model(edit, fused, mode):
    helpers.reset_worst()
    D.check_model_degenerate("cpu", edit, fused, mode)
    print("model %s %s %s: %s" % (edit, "fused" if fused else "unfused", mode, helpers.worst_line()))
