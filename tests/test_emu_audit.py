"""The checks that came out of the seeded-error audit of the kernels (tools/mutants.py, tests/MUTANTS.md) on the CPU-only box, the kernel
sources through the test-only HIP shim (tests/hipemu): plan branches of the generic contraction, equal maxima in the fused context heads,
BatchNorm channels whose variance is comparable to eps in every family that applies one, channels far off centre in every operator that
sums BatchNorm statistics (tests/off_centre_checks.py), and the dropout mask against its host restatement.  tests/test_gpu_audit.py runs
the same checks on the MI355X."""
import pytest

import audit_checks
import checks
import emu
import helpers
import off_centre_checks


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


def _report(name, check, *args, **kw):
    helpers.reset_worst()
    check("cpu", *args, **kw)
    print("%s: %s" % (name, helpers.worst_line()))


def test_contract_edges():
    _report("contract_edges", audit_checks.check_contract_edges)


def test_context_heads_equal_maxima():
    _report("context_ties", audit_checks.check_context_ties)


@pytest.mark.parametrize("family", [name for name, _ in audit_checks.LOW_VARIANCE])
def test_low_variance_channels(family):
    _report("low_variance " + family, audit_checks.check_low_variance, family)


@pytest.mark.parametrize("name", [name for name, _ in off_centre_checks.OFF_CENTRE_CASES])
def test_off_centre_channels(name):
    """channels at |mean| / std = 30 and 300 in every operator that sums BatchNorm statistics: within 4 x stock float32 of float64"""
    _report("off_centre " + name, off_centre_checks.check_off_centre, name)


def test_stgcn_rows_wider_than_a_wave():
    _report("stgcn_wide_rows", audit_checks.check_stgcn_wide_rows)


def test_dropout_mask_is_its_host_restatement():
    _report("dropout_mask", checks.check_dropout, mask=True)
