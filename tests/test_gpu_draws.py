"""The device draws, the gather at a device cursor, `BankFeed` and `BankStep` - eager and captured in a HIP graph - on the MI355X
through libcistgcn_hip.so: the checks of tests/draws_checks.py on the real device (the shim run: tests/test_emu_draws.py)."""
import pytest

import draws_checks as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"


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
    DC.check_dropout_is_untouched_by_a_draw(DEV, reduced=False)


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
    DC.check_bank_step_eager(DEV, reduced=False)


def test_bank_step_graphed_matches_eager():
    DC.check_bank_step_graphed(DEV)


def test_every_kernel_of_a_bank_step_is_ours():
    DC.check_every_kernel_of_a_bank_step_is_ours(DEV)
