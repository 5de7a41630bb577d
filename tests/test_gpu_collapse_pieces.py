"""The shapes of tests/test_emu_collapse_pieces.py on the MI355X: backward of the collapsing convolutions with several K ranges, three
samples per slice, short last range and slice, pieces of every alignment, the limits of the predicates; the weight gradient is the same
from run to run (per-slice partials summed in a fixed order)."""
import pytest
import torch

import checks
import collapse_pieces_shapes as S

pytestmark = pytest.mark.gpu


def test_geometry_has_the_properties_the_shapes_are_chosen_for():
    S.assert_properties()


@pytest.mark.parametrize("shape", S.ROWS, ids=S.ident)
def test_collapse_rows_pieces(shape):
    checks.check_collapse_rows("cuda", shapes=(shape,))


@pytest.mark.parametrize("shape", S.COLS, ids=S.ident)
def test_collapse_cols_pieces(shape):
    checks.check_collapse_cols("cuda", shapes=(shape,))


@pytest.mark.parametrize("shape", S.TOWER, ids=S.ident)
def test_tower_collapse_pieces(shape):
    checks.check_tower_collapse("cuda", shapes=(shape,), replay=True)


@pytest.mark.parametrize("cols", (False, True), ids=("rows", "cols"))
def test_weight_gradient_is_deterministic(cols):
    """two backward runs on the same operands give bitwise the same dW and dx (several K ranges, three samples per slice)"""
    from cistgcn_amd import ops
    B, C, T, V, O = S.COLS[0] if cols else S.ROWS[0]
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(B, C, T, V, generator=g).cuda()
    w0 = (0.2 * torch.randn(O, C, V if cols else T, generator=g)).cuda()
    gy = torch.randn(B, O, T if cols else V, generator=g).cuda()
    res = []
    for _ in range(2):
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        ops.begin_step(torch.device("cuda"))
        y, _st = (ops.collapse_cols if cols else ops.collapse_rows)(x, w)
        y.backward(gy)
        res.append((x.grad.clone(), w.grad.clone()))
    assert torch.equal(res[0][1], res[1][1]), "dW differs between two runs"
    assert torch.equal(res[0][0], res[1][0]), "dx differs between two runs"
