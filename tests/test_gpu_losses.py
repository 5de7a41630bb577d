"""The training losses on the MI355X through libcistgcn_hip.so: the checks of tests/losses_checks.py on the real device (the restatement
and the fixture's own properties are checked on the CPU box, tests/test_emu_losses.py)."""
import pytest

import losses_checks as LC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE_IDS = ["x".join(str(v) for v in s) for s in LC.loop_shapes()]


@pytest.mark.parametrize("case", LC.cases())
def test_case_matches_the_reference(case):
    LC.check_against_fixture(DEV, case)


@pytest.mark.parametrize("source", LC.SOURCES)
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("shape", LC.loop_shapes(), ids=SHAPE_IDS)
def test_loop_shapes_against_the_restatement(shape, kind, source):
    LC.check_shape(DEV, shape, kind, source)


def test_inputs_take_both_branches_and_zero_errors_get_zero_gradients():
    LC.check_input_coverage(DEV)


def test_all_errors_zero_gives_zero_gradients():
    LC.check_all_errors_zero(DEV)


def test_inputs_are_not_written_and_two_calls_give_the_same_bits():
    LC.check_untouched_and_reproducible(DEV)


def test_named_operators_are_motion_loss_of_their_kind():
    LC.check_named_forms(DEV)


def test_interface_errors():
    LC.check_interface_errors(DEV)


def test_host_tensors_are_refused():
    LC.check_host_tensors_refused()


def test_graphed_step_with_a_loss_replays_the_eager_loss():
    LC.check_graphed_step(DEV)


def test_data_parallel_step_with_a_loss_at_world_size_one():
    LC.check_data_parallel_step(DEV, reduced=False)


def test_default_step_launches_what_it_launched():
    LC.check_default_launches(DEV, reduced=False)
