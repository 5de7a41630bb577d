"""The attack distortion metrics on the MI355X through libcistgcn_hip.so: the checks of tests/attack_metrics_checks.py on the real
device, and the dictionary of an attack that ran as a HIP graph."""
import pytest

import attack_metrics_checks as AM

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("key", AM.KEYS)
@pytest.mark.parametrize("case", AM.CASES)
def test_entry_matches_the_reference(case, key):
    AM.check_against_fixture(DEV, case, key)


@pytest.mark.parametrize("case", AM.CASES)
def test_counts_and_ranges_match_the_reference(case):
    AM.check_counts_against_fixture(DEV, case)


@pytest.mark.parametrize("case", AM.CASES)
def test_restatement_matches_the_reference(case):
    AM.check_restatement(case)


def test_unmoved_sample_has_zero_distortion():
    AM.check_identical_sample(DEV)


def test_swapped_arguments_would_be_noticed():
    AM.check_roles(DEV)


@pytest.mark.parametrize("shape", AM.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_loop_shapes_against_the_restatement(shape):
    AM.check_shape(DEV, shape)


def test_inputs_are_not_written_and_two_calls_give_the_same_bits():
    AM.check_inputs_untouched_and_reproducible(DEV)


def test_strided_inputs_are_copied():
    AM.check_strided_inputs(DEV)


def test_interface_errors():
    AM.check_interface_errors(DEV)


def test_host_tensors_are_refused():
    AM.check_host_tensors_refused()


def test_attack_classes_return_the_reference_dictionary():
    AM.check_attack_dictionary(DEV)


def test_ifgsm_then_metrics_end_to_end():
    AM.check_end_to_end(DEV)


def test_graphed_attack_then_metrics_end_to_end():
    AM.check_end_to_end(DEV, graphed=True)
