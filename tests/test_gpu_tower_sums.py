"""The tests of tests/test_emu_tower_sums.py on the MI355X: the channel sums of the collapsing backward kernels against fp64 at
16 * 2^-24 * sum |term|, next to cg_norm_act_bwd_reduce_many on the same inputs, bit-equal from run to run; the mixed case through `ops`
and the agreement with the route through the reduction pass.  Checks, shapes and bounds: tests/tower_sums_checks.py."""
import pytest

import collapse_pieces_shapes as S
import tower_sums_checks as C

pytestmark = pytest.mark.gpu


def test_geometry_has_the_properties_the_shapes_are_chosen_for():
    C.assert_properties()


@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("shape", C.FRAME, ids=C.ident)
def test_frame_axis_sums(shape, train):
    C.check_sums("cuda", shape, cols=False, train=train)


@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("shape", C.JOINT, ids=C.ident)
def test_joint_axis_sums(shape, train):
    C.check_sums("cuda", shape, cols=True, train=train)


def test_mixed_case_two_maps_fused_one_without_sums():
    C.check_routes_agree("cuda", (5, 10, (6, 12, 8), 14, 6, 5), fuse=(True, True, False))


@pytest.mark.parametrize("shape", S.TOWER, ids=S.ident)
def test_fused_route_agrees_with_the_reduction_pass(shape):
    C.check_routes_agree("cuda", shape, fuse=[True] * len(shape[2]))
