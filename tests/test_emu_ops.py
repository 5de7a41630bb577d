"""Operator parity on the CPU-only box: the shipped .hip kernels, compiled by g++ against the
test-only HIP shim (tests/hipemu), are checked against stock-PyTorch references - on the shape lists the
MI355X run uses (tests/test_gpu_parity.py), minus the few chip-filling ones."""
import os
import subprocess
import sys

import pytest

import checks
import emu
import helpers
import loop_shapes as L


@pytest.fixture(scope="module", autouse=True)
def _emulated_kernels():
    emu.install()
    yield
    emu.uninstall()


@pytest.mark.parametrize("check", [checks.check_contract, checks.check_norm_act, checks.check_batched_ops, checks.check_dropout,
                                   checks.check_reduce_and_gate, checks.check_copies, checks.check_dilated_convs,
                                   checks.check_stage_kernels, checks.check_flat_adam, checks.check_zero_pool, checks.check_contract_kred, checks.check_contract_stream, checks.check_rank1_adj, checks.check_eval_harness, checks.check_contract_chain, checks.check_dstd_tail, checks.check_map2adj_tail, checks.check_pointwise_maps, checks.check_collapse_rows, checks.check_collapse_cols, checks.check_tower_collapse, checks.check_context_heads, checks.check_block_input, checks.check_tower_maps, checks.check_gate_head], ids=lambda f: f.__name__)
def test_operator(check):
    if check is checks.check_context_heads:
        check("cpu", shapes=((3, 5, 12, 7), (4, 25, 66, 64), (2, 3, 10, 33), (16, 25, 75, 64)))
    elif check is checks.check_gate_head:
        check("cpu", shapes=((5, 8, 10, 2), (37, 64, 102, 2), (4, 3, 46, 2), (20, 10, 22, 1), (40, 32, 102, 2)))
    elif check is checks.check_block_input:
        check("cpu", shapes=((3, 5, 4, 6, 3), (2, 10, 10, 22, 7), (4, 64, 5, 22, 8), (2, 6, 5, 5, 2), (3, 3, 22, 25, 4), (9, 32, 50, 25, 6)))
    else:
        check("cpu")


def _loops_map2adj_tail():
    L.assert_map2adj_tail_loops()
    checks.check_map2adj_tail("cpu", shapes=L.MAP2ADJ_TAIL, replay=True)


def _loops_dstd_tail():
    L.assert_dstd_tail_loops()
    checks.check_dstd_tail("cpu", shapes=L.DSTD_TAIL, replay=True)


def _loops_tower_maps():
    L.assert_pointwise_maps_loops(L.TOWER_MAPS, name="tower_maps")
    checks.check_tower_maps("cpu", shapes=L.TOWER_MAPS, replay=True)


def _loops_pointwise_maps():
    L.assert_pointwise_maps_loops(L.POINTWISE_MAPS)
    checks.check_pointwise_maps("cpu", shapes=L.POINTWISE_MAPS)


def _loops_tower_collapse():
    L.assert_pointwise_maps_loops(L.TOWER_COLLAPSE, deep=False, name="tower_collapse")
    for (B, C, Ms, T, V, O) in L.TOWER_COLLAPSE:          # the collapsing convolutions of the deferred maps: M_i input channels each
        L.assert_collapse_loops(((B, Ms[0], T, V, O),), cols=False, name="tower_collapse rows")
        L.assert_collapse_loops(((B, Ms[1], T, V, O),), cols=True, name="tower_collapse cols")
    checks.check_tower_collapse("cpu", shapes=L.TOWER_COLLAPSE, replay=True)


def _loops_collapse_rows():
    assert L.assert_collapse_loops(L.COLLAPSE_ROWS, cols=False), "collapse_rows: geometry gives no slice three samples"
    checks.check_collapse_rows("cpu", shapes=L.COLLAPSE_ROWS)


def _loops_collapse_cols():
    assert L.assert_collapse_loops(L.COLLAPSE_COLS, cols=True), "collapse_cols: geometry gives no slice three samples"
    checks.check_collapse_cols("cpu", shapes=L.COLLAPSE_COLS)


def _loops_dilated_convs():
    L.assert_dilated_convs_loops()
    checks.check_dilated_convs("cpu", shapes=L.DILATED_CONVS)


def _loops_block_input():
    L.assert_block_input_loops()
    checks.check_block_input("cpu", shapes=L.BLOCK_INPUT)


def _loops_norm_act():
    L.assert_norm_act_rows_loop()
    checks.check_norm_act_rows("cpu", L.NORM_ACT_ROWS)


@pytest.mark.parametrize("family", [_loops_map2adj_tail, _loops_dstd_tail, _loops_tower_maps, _loops_pointwise_maps, _loops_tower_collapse,
                                    _loops_collapse_rows, _loops_collapse_cols, _loops_dilated_convs, _loops_block_input, _loops_norm_act], ids=lambda f: f.__name__[len("_loops_"):])
def test_operator_loop_shapes(family):
    """the operator checks on shapes whose launch geometry - asked from the library (tests/loop_shapes.py) - gives a workgroup several tiles or
    samples, a short last range and ranges that cross samples; the default lists above stay at one tile per workgroup everywhere"""
    helpers.reset_worst()
    family()
    print("%s: %s" % (family.__name__[len("_loops_"):], helpers.worst_line()))


def test_tail_backward_takes_the_branches_of_its_forward():
    """fused DSTD tail, pre-activations of prelu1 walking through 0 in steps of one ulp: the backward takes the forward's branch at every
    element (forward and backward once rounded the pre-activation differently)"""
    checks.check_dstd_tail_kink_branches("cpu")


def test_plan_predicates_at_their_limits():
    """host side only: every `*_ok` / `*_supported` predicate of the model's launch plan says yes at its limit and no one step past it"""
    checks.check_predicate_limits()


@pytest.mark.parametrize("case", checks.LIMIT_SHAPES, ids=lambda c: c[0].replace(" ", "").replace(",", "-"))
def test_family_at_the_limit_of_its_predicate(case):
    """the operator check of a family on the last shape its predicate takes (V = 32, T = 64, O = 64, C = 64 / 128, S = 192, H * W = 256 /
    16384 ...); one step past it the model takes the fallback, which tests/plan_shapes.py holds at model level"""
    checks.check_family_at_limit("cpu", case)


def test_stgcn_domain_loop_shapes():
    """tile and matrix-core kernels of the fused ST-GCN stage with several tiles per workgroup (the plane generation pinned off: it would take
    these batch sizes where it has the (T, V) family), and the plane kernels with a batch that does not fill its last group of eight samples"""
    helpers.reset_worst()
    L.assert_stgcn_domain_loops(L.STGCN_TILE, kind=0)
    checks.check_stgcn_domain("cpu", shapes=L.STGCN_TILE, planes=None)
    L.assert_stgcn_domain_loops(L.STGCN_MFMA, kind=1)
    checks.check_stgcn_domain("cpu", shapes=L.STGCN_MFMA, planes=None)
    assert all(s[0] % 8 != 0 and s[0] > 64 and s[4] % 4 != 0 and s[3] % 8 != 0 for s in L.STGCN_PLANES)
    checks.check_stgcn_domain("cpu", shapes=L.STGCN_PLANES, planes=True)
    print("stgcn_domain: %s" % helpers.worst_line())


def test_stgcn_domain_small():
    checks.check_stgcn_domain("cpu", shapes=((3, 10, 8, 5, 7), (2, 3, 3, 6, 9), (2, 18, 16, 5, 7)))


def test_stgcn_domain_planes():
    """plane kernels of the fused ST-GCN stage (forward both domains, both backward kernels) on every instantiated (T, V) family"""
    checks.check_stgcn_domain("cpu", shapes=checks.PLANE_SHAPES, planes=True)


@pytest.mark.timeout(1200)
@pytest.mark.skipif(os.environ.get("HIPEMU_SANITIZE", "0") == "1", reason="this IS the sanitizer run")
def test_kernels_under_address_sanitizer():
    """The same kernel sources built with -fsanitize=address (the GPU pool offers no device sanitizer): the operator tests above and
    a part of the model tests of test_emu_model.py (the golden case at T = 10, the tiny models, the dropout step) in a child
    interpreter under libasan; an out-of-bounds LDS / global access or a stack overflow of a kernel aborts the child.  The whole of
    test_emu_model.py passes under the sanitizer too (four minutes; its torch.jit test excepted, which ends the sanitized interpreter
    inside torch's tracer)."""
    asan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no libasan next to g++")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIPEMU_SANITIZE="1", LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0", CISTGCN_ABLATION="1")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_emu_ops.py"), os.path.join(here, "test_emu_model.py"), "-x", "-q",
                          "-m", "not gpu", "-p", "no:cacheprovider", "-n", str(min(6, os.cpu_count() or 1)), "-k", "test_operator or test_stgcn or h36m_c8_t10_v22 or tiny or dropout_step"], env=env, capture_output=True, text=True, cwd=os.path.dirname(here), timeout=1100)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr
