"""The tests of tests/test_emu_block_mid.py on the MI355X: `ops.block_mid` against the norm_act_many + contract_many chain it replaces and
against fp64, at the loop edges of the kernels, between NaN guards, bit-equal from run to run, with the row kernels' masks, and inside a
small model.  Checks, shapes and the condition: tests/block_mid_checks.py."""
import pytest

import block_mid_checks as C

pytestmark = pytest.mark.gpu


def test_geometry_has_the_properties_the_shapes_are_chosen_for():
    C.assert_properties()


@pytest.mark.parametrize("mode", list(C.MODES))
@pytest.mark.parametrize("name", list(C.CASES))
def test_operator_against_the_chain_and_fp64(name, mode):
    C.check_operator("cuda", name, mode)


@pytest.mark.parametrize("mode", ("train-drop", "eval-drop"))
@pytest.mark.parametrize("name", list(C.CASES))
def test_guard_bands_and_same_bits_twice(name, mode):
    C.check_guards_and_determinism("cuda", name, mode)


def test_small_model_with_the_route_on_and_off():
    C.check_model("cuda")
