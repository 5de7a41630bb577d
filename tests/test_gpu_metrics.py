"""The evaluation metrics on the MI355X through libcistgcn_hip.so: the checks of tests/metrics_checks.py on the real device, plus one
shape that takes many workgroups and a partly filled last one."""
import pytest

import metrics_checks as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("case", M.CASES)
def test_metric_matches_the_reference(case, mode, metric):
    M.check_against_fixture(DEV, case, mode, metric)


def test_nan_rule_and_reflected_sample():
    M.check_nan_rule_and_reflection(DEV)


@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("case", M.CASES)
def test_restatement_matches_the_reference(case, mode):
    M.check_restatement(case, mode)


def test_a_missing_replacement_would_be_noticed():
    M.check_quirk_is_detected()


@pytest.mark.parametrize("case", M.CASES)
def test_frames_mpjpe_agrees_with_eval_scatter_mpjpe(case):
    M.check_mpjpe_matches_eval_scatter(DEV, case)


@pytest.mark.parametrize("joint", [False, True], ids=["frames", "joint"])
def test_accumulator_over_two_batches(joint):
    M.check_accumulator(DEV, joint)


def test_inputs_are_not_written():
    M.check_inputs_untouched(DEV)


def test_two_calls_give_the_same_bits():
    M.check_bit_reproducible(DEV)


def test_strided_inputs_are_copied():
    M.check_strided_inputs(DEV)


def test_interface_errors():
    M.check_interface_errors(DEV)


def test_sixty_four_joints_and_more_bones_than_lanes():
    M.check_full_wave(DEV)


def test_large_random_shape_against_the_restatement():
    M.check_large_random(DEV)
