"""The input attacks on the CPU-only box: the shipped kernels of csrc/attack.hip under the test-only HIP shim (tests/hipemu) against the
stock-PyTorch restatement and the recording of the real reference's attack classes (tests/attack_checks.py).  The same checks, plus
the HIP-graph objects, run on the MI355X in tests/test_gpu_attacks.py."""
import pytest

import attack_checks as A
import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("shape", A.MPJPE_SHAPES, ids=str)
def test_mpjpe_per_sample(shape):
    A.check_mpjpe_per_sample("cpu", *shape)


@pytest.mark.parametrize("mask", A.STEP_MASKS)
@pytest.mark.parametrize("mode", A.STEP_MODES)
@pytest.mark.parametrize("shape", A.STEP_SHAPES, ids=str)
def test_attack_step_matches_the_restatement(shape, mode, mask):
    A.check_attack_step_synthetic("cpu", shape, mode, mask)


@pytest.mark.parametrize("mode", ["ifgsm", "mifgsm"])
def test_bookkeeping_follows_scripted_losses(mode):
    A.check_bookkeeping_script("cpu", mode)


@pytest.mark.parametrize("cid", ["I1", "I2", "M", "I3"])
def test_teacher_forced_chain_reproduces_the_reference(cid):
    A.check_teacher_forced("cpu", cid)


@pytest.mark.parametrize("cid,k", A.sign_iterates(), ids=lambda v: str(v))
def test_input_gradient_signs_at_recorded_iterates(cid, k):
    A.check_gradient_signs("cpu", cid, k)


def test_fgsm_apply_against_the_reference():
    A.check_fgsm_apply("cpu")


@pytest.mark.parametrize("cid,k", A.ONE_STEP, ids=lambda v: str(v))
def test_one_model_driven_step(cid, k):
    A.check_one_step("cpu", cid, k)


def test_interface():
    A.check_interface("cpu")


def test_noattack_returns_the_eval_input_gradient():
    A.check_noattack("cpu")
