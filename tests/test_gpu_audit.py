"""The checks of tests/test_emu_audit.py on the MI355X (real libcistgcn_hip.so): plan branches of the generic contraction, equal maxima in
the fused context heads, BatchNorm channels whose variance is comparable to eps or which lie far off centre, the dropout mask against its
host restatement.  Run with
`-m gpu`; every test prints the comparison that came closest to its bound."""
import pytest
import torch

import audit_checks
import checks
import helpers
import off_centre_checks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    from cistgcn_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib._handle = None
    _lib._host_pointers_ok = False
    _lib.lib()          # raises if libcistgcn_hip.so has not been built
    yield


def _report(name, check, *args, **kw):
    helpers.reset_worst()
    check("cuda", *args, **kw)
    torch.cuda.synchronize()
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
