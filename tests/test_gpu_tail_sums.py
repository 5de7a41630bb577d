"""The backward of ops.dstd_tail with its BatchNorm sums formed a phase early (csrc/dstd_tail.hip) on the MI355X (the tests of tests/test_emu_tail_sums.py): every gradient against
fp64, the derived tcn sums and the compressor sums from the row sums at 16 * 2^-24 * sum |term|, the same bits twice, the route with a
pass per sum, the shared residual gradient.  Checks, shapes and bounds: tests/tail_sums_checks.py."""
import pytest

import tail_sums_checks as C

pytestmark = pytest.mark.gpu


def test_geometry_has_the_properties_the_shapes_are_chosen_for():
    C.assert_properties()


@pytest.mark.parametrize("shared", (False, True), ids=("separate", "shared"))
@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.ident)
def test_tail_sums(shape, train, shared):
    C.check("cuda", shape, train, shared)


def test_shared_residual_bookkeeping():
    C.check_shared_bookkeeping("cuda")
