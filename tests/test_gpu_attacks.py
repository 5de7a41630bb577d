"""The input attacks on the MI355X through libcistgcn_hip.so: the checks of tests/attack_checks.py on the real device, eagerly and
through `runtime.GraphedAttack` (both are held to the recording of the reference, not to each other)."""
import pytest
import torch

import attack_checks as A

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("shape", A.MPJPE_SHAPES, ids=str)
def test_mpjpe_per_sample(shape):
    A.check_mpjpe_per_sample(DEV, *shape)


@pytest.mark.parametrize("mask", A.STEP_MASKS)
@pytest.mark.parametrize("mode", A.STEP_MODES)
@pytest.mark.parametrize("shape", A.STEP_SHAPES, ids=str)
def test_attack_step_matches_the_restatement(shape, mode, mask):
    A.check_attack_step_synthetic(DEV, shape, mode, mask)


@pytest.mark.parametrize("mode", ["ifgsm", "mifgsm"])
def test_bookkeeping_follows_scripted_losses(mode):
    A.check_bookkeeping_script(DEV, mode)


@pytest.mark.parametrize("cid", ["I1", "I2", "M", "I3"])
def test_teacher_forced_chain_reproduces_the_reference(cid):
    A.check_teacher_forced(DEV, cid)


@pytest.mark.parametrize("cid,k", A.sign_iterates(), ids=lambda v: str(v))
def test_input_gradient_signs_at_recorded_iterates(cid, k):
    A.check_gradient_signs(DEV, cid, k)


def test_fgsm_apply_against_the_reference():
    A.check_fgsm_apply(DEV)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("cid,k", A.ONE_STEP, ids=lambda v: str(v))
def test_one_model_driven_step(cid, k, graphed):
    A.check_one_step(DEV, cid, k, graphed=graphed)


def test_free_running_structure():
    A.check_free_running(DEV)


def test_interface():
    A.check_interface(DEV)


def test_noattack_returns_the_eval_input_gradient():
    A.check_noattack(DEV)
