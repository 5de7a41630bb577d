"""The evaluation metrics on the CPU-only box: the shipped kernels of csrc/eval_metrics.hip under the test-only HIP shim (tests/hipemu)
against the recording of the real reference's `Metrics` and the stock-PyTorch restatement (tests/metrics_checks.py).  The same checks,
plus a shape of many workgroups, run on the MI355X in tests/test_gpu_metrics.py."""
import pytest

import emu
import metrics_checks as M


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("case", M.CASES)
def test_metric_matches_the_reference(case, mode, metric):
    M.check_against_fixture("cpu", case, mode, metric)


def test_nan_rule_and_reflected_sample():
    M.check_nan_rule_and_reflection("cpu")


@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("case", M.CASES)
def test_restatement_matches_the_reference(case, mode):
    M.check_restatement(case, mode)


def test_a_missing_replacement_would_be_noticed():
    M.check_quirk_is_detected()


@pytest.mark.parametrize("case", M.CASES)
def test_frames_mpjpe_agrees_with_eval_scatter_mpjpe(case):
    M.check_mpjpe_matches_eval_scatter("cpu", case)


@pytest.mark.parametrize("joint", [False, True], ids=["frames", "joint"])
def test_accumulator_over_two_batches(joint):
    M.check_accumulator("cpu", joint)


def test_inputs_are_not_written():
    M.check_inputs_untouched("cpu")


def test_two_calls_give_the_same_bits():
    M.check_bit_reproducible("cpu")


def test_strided_inputs_are_copied():
    M.check_strided_inputs("cpu")


def test_interface_errors():
    M.check_interface_errors("cpu")


def test_sixty_four_joints_and_more_bones_than_lanes():
    M.check_full_wave("cpu")
