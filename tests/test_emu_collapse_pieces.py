"""Backward of the collapsing convolutions (csrc/collapse_rows.hip) on the CPU shim, on the shapes that decide how a workgroup's piece of
x / dx travels and how the weight gradient leaves: several K ranges with a short last one, three samples per slice with a short last
slice, pieces of 16-, 8- and 4-byte alignment, every tile count and the limits of the predicates.  The checks and their bounds are those
of tests/checks.py."""
import pytest

import checks
import emu
import collapse_pieces_shapes as S


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


def test_geometry_has_the_properties_the_shapes_are_chosen_for():
    S.assert_properties()


@pytest.mark.parametrize("shape", S.ROWS, ids=S.ident)
def test_collapse_rows_pieces(shape):
    checks.check_collapse_rows("cpu", shapes=(shape,))


@pytest.mark.parametrize("shape", S.COLS, ids=S.ident)
def test_collapse_cols_pieces(shape):
    checks.check_collapse_cols("cpu", shapes=(shape,))


@pytest.mark.parametrize("shape", S.TOWER, ids=S.ident)
def test_tower_collapse_pieces(shape):
    checks.check_tower_collapse("cpu", shapes=(shape,), replay=True)
