"""The attack distortion metrics on the CPU-only box: the shipped kernels of csrc/attack_metrics.hip under the test-only HIP shim
(tests/hipemu) against the recording of the real reference's `ComputeAttackMetrics._get_metrics` and the stock-PyTorch restatement
(tests/attack_metrics_checks.py).  The same checks run on the MI355X in tests/test_gpu_attack_metrics.py."""
import pytest

import attack_metrics_checks as AM
import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("key", AM.KEYS)
@pytest.mark.parametrize("case", AM.CASES)
def test_entry_matches_the_reference(case, key):
    AM.check_against_fixture("cpu", case, key)


@pytest.mark.parametrize("case", AM.CASES)
def test_counts_and_ranges_match_the_reference(case):
    AM.check_counts_against_fixture("cpu", case)


@pytest.mark.parametrize("case", AM.CASES)
def test_restatement_matches_the_reference(case):
    AM.check_restatement(case)


def test_unmoved_sample_has_zero_distortion():
    AM.check_identical_sample("cpu")


def test_swapped_arguments_would_be_noticed():
    AM.check_roles("cpu")


@pytest.mark.parametrize("shape", AM.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_loop_shapes_against_the_restatement(shape):
    AM.check_shape("cpu", shape)


def test_inputs_are_not_written_and_two_calls_give_the_same_bits():
    AM.check_inputs_untouched_and_reproducible("cpu")


def test_strided_inputs_are_copied():
    AM.check_strided_inputs("cpu")


def test_interface_errors():
    AM.check_interface_errors("cpu")


def test_host_tensors_are_refused_without_the_shim():
    AM.check_host_tensors_refused()


def test_attack_classes_return_the_reference_dictionary():
    AM.check_attack_dictionary("cpu")


def test_ifgsm_then_metrics_end_to_end():
    AM.check_end_to_end("cpu")
