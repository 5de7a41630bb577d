"""The training losses on the CPU-only box: the shipped kernels of csrc/losses.hip (cg_motion_loss_fwd / _bwd) under the test-only HIP
shim (tests/hipemu) against the recording of the real reference's `train()` and the fp64 restatement (tests/losses_checks.py).  The
same checks run on the MI355X in tests/test_gpu_losses.py; the restatement and the fixture's own properties are checked here only."""
import pytest

import emu
import losses_checks as LC

DEV = "cpu"
SHAPE_IDS = ["x".join(str(v) for v in s) for s in LC.loop_shapes()]


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


def test_fixture_has_the_cases_of_the_issue():
    LC.check_fixture_covers_the_issue()


@pytest.mark.parametrize("case", LC.cases())
def test_restatement_matches_the_reference(case):
    LC.check_restatement(case)


def test_fp32_torch_composition_is_far_inside_the_bound():
    """the figures the docstring of losses_checks.py quotes; an order of magnitude under the 1e-4 the kernels are held to"""
    loss, grad_max, grad_l2 = LC.fp32_torch_error()
    print("fp32 torch vs fp64: loss %.3e relative, gradient %.3e of max|ref|, %.3e relative L2" % (loss, grad_max, grad_l2))
    assert loss <= 1e-5 and grad_max <= 1e-5 and grad_l2 <= 1e-5


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


def test_host_tensors_are_refused_without_the_shim():
    LC.check_host_tensors_refused()


def test_eager_step_with_a_loss_matches_the_operator_by_hand():
    LC.check_eager_step(DEV, reduced=True)


def test_data_parallel_step_with_a_loss_at_world_size_one():
    LC.check_data_parallel_step(DEV, reduced=True)


def test_default_step_launches_what_it_launched():
    LC.check_default_launches(DEV, reduced=True)
