"""The device draws, the gather at a device cursor, `BankFeed` and the eager `BankStep` on the CPU-only box: the shipped kernels of
csrc/augment_draw.hip and csrc/kinematics.hip under the test-only HIP shim (tests/hipemu) against the restatement of the generator
(tests/draws_ref.py; checks in tests/draws_checks.py).  The same checks, and the captured step, run on the MI355X in
tests/test_gpu_draws.py."""
import pytest

import draws_checks as DC
import emu

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("case", DC.table_cases(), ids=DC.case_id)
def test_table_against_the_restatement(case):
    DC.check_table(DEV, case)


def test_degenerate_thresholds():
    DC.check_degenerate_thresholds(DEV)


def test_draw_interface_errors():
    DC.check_interface_errors(DEV)


def test_same_seed_same_bits_other_seed_or_stream_other_bits():
    DC.check_same_seed_same_bits_other_seed_other_bits(DEV)


def test_counters_of_two_samples_never_coincide():
    DC.check_counters_of_two_samples_never_coincide(DEV)


def test_dropout_is_untouched_by_a_draw():
    DC.check_dropout_is_untouched_by_a_draw(DEV, reduced=True)


def test_distribution_within_five_sigma():
    DC.check_distribution(DEV)


@pytest.mark.parametrize("which", ("augmentation", "robustness"))
@pytest.mark.parametrize("shape", DC.PIPE_SHAPES, ids=DC.case_id)
def test_device_params_equal_the_same_table_from_the_host(shape, which):
    DC.check_device_params_pipeline(DEV, shape, which)


def test_host_draws_are_unchanged():
    DC.check_host_draws_are_unchanged(DEV)


def test_order_is_checked_once_per_call():
    DC.check_order_is_checked_once_per_call(DEV)


def test_gather_at_the_cursor():
    DC.check_cursor_gather(DEV)


def test_feed_epochs_keep_their_buffers():
    DC.check_feed_epochs(DEV)


def test_bank_step_eager():
    DC.check_bank_step_eager(DEV, reduced=True)
