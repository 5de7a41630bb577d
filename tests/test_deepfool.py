"""The DeepFool input attack on the CPU-only box: the shipped kernel of csrc/attack.hip under the test-only HIP shim (tests/hipemu)
against the fp64 restatement and the recording of the real reference's DEEPFOOL (tests/deepfool_checks.py).  The same checks, plus
the HIP-graph object and the free-running attacks (10 to 16 passes through the emulated model take half a minute and more per
configuration here), run on the MI355X in tests/test_gpu_deepfool.py."""
import pytest

import deepfool_checks as D
import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("masked", [0, 1], ids=["all", "masked"])
@pytest.mark.parametrize("shape", D.STEP_SHAPES, ids=str)
def test_step_matches_the_fp64_restatement(shape, masked):
    D.check_step_synthetic("cpu", shape, masked)


def test_bookkeeping_follows_scripted_losses():
    D.check_bookkeeping_script("cpu")


def test_operand_contract():
    D.check_operand_contract("cpu")


def test_entry_point_statuses():
    D.check_entry_point_statuses("cpu")


@pytest.mark.parametrize("cid,i", D.RECORDED, ids=lambda v: str(v))
def test_teacher_forced_step_reproduces_the_reference(cid, i):
    D.check_teacher_forced("cpu", cid, i)


@pytest.mark.parametrize("cid,i", D.RECORDED, ids=lambda v: str(v))
def test_model_driven_step_at_recorded_iterates(cid, i):
    D.check_model_step("cpu", cid, i)


def test_interface():
    D.check_interface("cpu")
