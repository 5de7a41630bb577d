"""The DeepFool input attack on the MI355X through libcistgcn_hip.so: the checks of tests/deepfool_checks.py on the real device, eagerly
and through `runtime.GraphedAttack` (both are held to the recording of the reference, not to each other)."""
import pytest

import deepfool_checks as D

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("masked", [0, 1], ids=["all", "masked"])
@pytest.mark.parametrize("shape", D.STEP_SHAPES, ids=str)
def test_step_matches_the_fp64_restatement(shape, masked):
    D.check_step_synthetic(DEV, shape, masked)


def test_bookkeeping_follows_scripted_losses():
    D.check_bookkeeping_script(DEV)


def test_operand_contract():
    D.check_operand_contract(DEV)


def test_entry_point_statuses():
    D.check_entry_point_statuses(DEV)


@pytest.mark.parametrize("cid,i", D.RECORDED, ids=lambda v: str(v))
def test_teacher_forced_step_reproduces_the_reference(cid, i):
    D.check_teacher_forced(DEV, cid, i)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("cid,i", D.RECORDED, ids=lambda v: str(v))
def test_model_driven_step_at_recorded_iterates(cid, i, graph):
    D.check_model_step(DEV, cid, i, graph=graph)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("cid", list(D.CONFIGS))
def test_free_running_against_the_reference(cid, graph):
    D.check_free_running(DEV, cid, graph=graph)


def test_graph_reset_runs_a_second_batch():
    D.check_graph_reset(DEV)


def test_interface():
    D.check_interface(DEV)
