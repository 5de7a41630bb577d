"""The robustness-test transforms on the MI355X through libcistgcn_hip.so: the checks of tests/robustness_checks.py on the real
device (the restatement and the fixture's own properties are checked on the CPU box, tests/test_emu_robustness.py)."""
import pytest

import robustness_checks as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", RC.CASES)
def test_case_matches_the_reference(case):
    RC.check_against_fixture(DEV, case)


@pytest.mark.parametrize("case", RC.CASES)
def test_draws_are_consumed_as_the_reference_consumes_them(case):
    RC.check_draws(DEV, case)


@pytest.mark.parametrize("shape", RC.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_loop_shapes_against_the_restatement(shape):
    RC.check_shape(DEV, shape)


def test_random_sections_give_the_bits_of_the_augmentation_kernel():
    RC.check_equivalence_with_old_kernel(DEV)


def test_no_steps_is_the_raw_window_and_its_velocities():
    RC.check_no_steps(DEV)


def test_inputs_are_not_written_and_two_calls_give_the_same_bits():
    RC.check_inputs_untouched_and_reproducible(DEV)


def test_prefetcher_yields_the_batches_of_direct_calls():
    RC.check_prefetcher(DEV)


def test_interface_errors():
    RC.check_interface_errors(DEV)


def test_host_tensors_are_refused():
    RC.check_host_tensors_refused()
