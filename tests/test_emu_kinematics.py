"""Forward kinematics, the window gather and the motion bank on the CPU-only box: the shipped kernels of csrc/kinematics.hip under the
test-only HIP shim (tests/hipemu) against the recording of the real reference and the fp64 restatement (tests/kinematics_checks.py),
plus what needs no kernel: the restatement against the recording and the fixture's own coverage.  The same kernel checks run on the
MI355X in tests/test_gpu_kinematics.py."""
import pytest

import emu
import kinematics_checks as KC

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("case", KC.CASES)
def test_fk_case_within_four_times_the_reference_error(case):
    KC.check_fk_fixture(DEV, case)


@pytest.mark.parametrize("case", KC.CASES)
def test_restatement_matches_the_reference(case):
    KC.check_restatement(case)


def test_fixture_covers_tiny_zero_and_inverted_cases():
    KC.fixture_covers_the_issue()


@pytest.mark.parametrize("shape", KC.fk_shapes(), ids=KC.shape_id)
def test_fk_loop_shapes_against_the_restatement(shape):
    KC.check_fk_shape(DEV, shape)


def test_fk_zero_rotation_is_the_identity_exactly():
    KC.check_fk_zero_rotations(DEV)


def test_fk_inputs_are_not_written_and_two_calls_give_the_same_bits():
    KC.check_fk_inputs_untouched_and_reproducible(DEV)


def test_fk_interface_errors():
    KC.check_fk_interface_errors(DEV)


def test_host_tensors_are_refused_without_the_shim():
    KC.check_host_tensors_refused()


@pytest.mark.parametrize("shape", KC.GATHER_SHAPES, ids=KC.shape_id)
def test_gather_against_the_restatement(shape):
    KC.check_gather_shape(DEV, shape)


def test_gather_inputs_are_not_written_and_two_calls_give_the_same_bits():
    KC.check_gather_inputs_untouched_and_reproducible(DEV)


def test_gather_clamps_ids_given_on_the_device():
    KC.check_gather_clamps_device_ids(DEV)


def test_gather_and_bank_range_errors():
    KC.check_gather_errors(DEV)


def test_h36m_bank_reproduces_the_reference_loader(tmp_path):
    KC.check_h36m_bank(DEV, tmp_path)


def test_amass_bank_reproduces_the_reference_loader(tmp_path):
    KC.check_amass_bank(DEV, tmp_path)


def test_find_indices_256_matches_the_recording():
    KC.check_find_indices_256()


def test_original_test_split_uses_the_recorded_starts(tmp_path):
    KC.check_original_test_starts(DEV, tmp_path)


def test_batches_visit_every_window_once_and_feed_the_augmentation():
    KC.check_batches(DEV)
