"""Shapes that take the glue operators (csrc/stages.hip, the reductions, copies and sums of csrc/rowops.hip, csrc/optim.hip) past their
first pass, and the assertions that they do.

The default lists of tests/checks.py keep every one of these kernels inside one workgroup pass on freshly allocated float32 tensors.
The lists here are the smallest shapes at which a grid-stride loop takes a second iteration, a fallback kernel is chosen, a lane
group or a thread block changes its width, or a launch is split.  The limits are asked from the library (the host-only
cg_glue_geometry of include/cistgcn_hip.h, answered from the constants the launchers use), so a moved limit fails in
`assert_properties` with a message about geometry instead of passing without testing anything.

Both tests/test_emu_glue.py (CPU shim) and tests/test_gpu_glue.py (MI355X) run these lists through tests/glue_checks.py.
"""
import ctypes

from cistgcn_amd import _lib

# ---- mpjpe: points.  One grid of cg_mpjpe_fwd covers 1024 x 256 = 262 144 points, the rest is a thread's second iteration; the points
# past one grid carry MPJPE_TAIL_SHARE of the summed error (their targets are moved away), so a dropped second pass is far out of bound.
MPJPE_GRID = 262144
MPJPE_SHAPE = (100, 25, 105, 3)                       # 262 144 + 356 points; the permuted case stores it as (100, 105, 25, 3)
MPJPE_TAIL_SHARE = 0.10
MPJPE_BLOCKS = 1024                                    # float32 partial sums the loss is made of (one atomic per workgroup)

# ---- cg_adam_flat / cg_scale: one grid covers 2048 x 256 = 524 288 elements.  nn.Linear(1025, 512): 525 312 parameters; its weight is
# 257 chunks of the gradient gather (runtime.FlatGrads), the last one short.
ADAM_LINEAR = (1025, 512)
SCALE_N = 524288 + 37

# ---- se_gate (B, C, H): C * H = 2048 is the last shape of the sliced backward, 2056 / 2080 take the kernel with one workgroup per sample;
# 67 samples on the 64 workgroups of the sliced kernel: three of them walk two samples
SE_GATE = ((3, 256, 8), (3, 257, 8), (5, 520, 4), (67, 2, 1))

# ---- reduce_bc: P = 700 positions: 256 threads, the third iteration partial.  Rows with the maximum planted at several positions
REDUCE_SHAPE = (2, 3, 20, 35)
REDUCE_TIES = {(0, 0): (300, 520), (0, 1): (64, 320, 699), (1, 2): (699, 255, 256)}      # (b, c) -> positions of the maximum
REDUCE_CONSTANT_ROW = (0, 2)

# ---- cumsum: (shape of the stored tensor, permutation or None); 297 and 270 scans: two workgroups, the second one partial
CUMSUM = (((3, 3, 25, 33), (0, 2, 3, 1)), ((2, 64, 5, 27), None))

# ---- feature_lift (B, T, V): several workgroups with a tail, T = 1 and T = 2
FEATURE_LIFT = ((3, 10, 22), (300, 1, 1), (5, 2, 30), (2, 1, 7))

# ---- dstd_stats (B, C, T, V): the lane groups of a row at V = 16 | 17, 32 | 33, 64 | 65, rows walked in two and three steps of 64 (129, 193),
# a partial last iteration of the four-rows-in-flight loop everywhere, the smallest legal shape, and more dynamic LDS than a kernel gets
# without a raised limit
DSTD_STATS = ((2, 7, 50, 16), (2, 4, 45, 17), (2, 5, 30, 32), (2, 5, 30, 33), (2, 4, 9, 64), (2, 4, 9, 65), (3, 4, 5, 129), (3, 4, 5, 193),
              (2, 2, 1, 2), (2, 90, 50, 4))
DSTD_STATS_LDS = (2, 90, 50, 4)

# ---- cg_sum_many through fanout (consumers, shape): float2 rows with exactly eight inputs | float2, three iterations of the vector loop,
# two rounds (the partial sum is the ninth input's partner) | float4, three rounds | scalar rows longer than a workgroup
FANOUT = ((8, (2, 3, 5, 6)), (9, (2, 3, 50, 25)), (17, (2, 3, 4, 8)), (3, (2, 3, 17, 61)))

# ---- cg_copy_many: more than four items = a second launch
CAT_CHANNELS = (3, 1, 6, 2, -4, 5)                     # channels per input, negative: a (B, C) map broadcast over the positions
CAT_POSITIONS = (20, 35)
SPLIT_SHAPE = (3, 11, 4, 9)
SPLIT_SIZES = (2, 1, 3, 4, 1)

# ---- cg_zero: head offsets from a 16-byte boundary x lengths, and one fill longer than a grid of 4096 x 256 threads x 16 bytes
ZERO_OFFSETS = tuple(range(17))
ZERO_LENGTHS = (0, 1, 3, 15, 16, 17, 31, 32, 33, 100, 1000)
ZERO_BIG = ((4096 * 256 + 700) * 16 + 21, 3)          # (bytes, offset)

# ---- norm_act: float offsets of the input's base address from a 16-byte boundary -> rows read as float4, scalar, float2
NORM_ACT_ALIGN_SHAPE = (3, 4, 4, 6)
NORM_ACT_ALIGN_OFFSETS = (0, 1, 2)

# ---- eval_scatter_mpjpe: more joints than the 64 threads of its workgroup
EVAL_SCATTER = (3, 5, 70, 66)                          # B, To, J32, J22

GEOMETRY = ("mpjpe_grid", "flat_grid", "zero_grid_bytes", "se_sliced_max", "se_sliced_workgroups", "lds_default", "dstd_lds", "dstd_lanes",
            "dstd_rows_per_iteration", "dstd_iterations", "dstd_last_rows")


def glue_geometry(C=2, T=1, V=2):
    """cg_glue_geometry as a dict: the limits of the glue launchers and the plan of cg_dstd_stats_* for a (C, T, V) sample"""
    out = (ctypes.c_int * len(GEOMETRY))()
    _lib.check(_lib.lib().cg_glue_geometry(C, T, V, out), "cg_glue_geometry")
    return dict(zip(GEOMETRY, out))


def _prod(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def assert_properties(mpjpe_shape=MPJPE_SHAPE, adam_linear=ADAM_LINEAR, scale_n=SCALE_N, se_gate=SE_GATE, dstd_stats=DSTD_STATS,
                      dstd_lds=DSTD_STATS_LDS, zero_big=ZERO_BIG, reduce_shape=REDUCE_SHAPE, eval_scatter=EVAL_SCATTER):
    """every list above takes the path it is meant to take, by the library's own limits"""
    g = glue_geometry()
    n = _prod(mpjpe_shape) // 3
    assert g["mpjpe_grid"] == MPJPE_GRID and g["mpjpe_grid"] // 256 == MPJPE_BLOCKS, "mpjpe: the grid limit moved to %d points: adjust MPJPE_*" % g["mpjpe_grid"]
    assert g["mpjpe_grid"] < n < 2 * g["mpjpe_grid"], "mpjpe: %d points do not start a second pass of a grid of %d" % (n, g["mpjpe_grid"])
    params = adam_linear[0] * adam_linear[1] + adam_linear[1]
    assert params > g["flat_grid"], "adam: %d parameters fit one grid of %d" % (params, g["flat_grid"])
    assert adam_linear[0] * adam_linear[1] % 2048 != 0 and adam_linear[0] * adam_linear[1] > 2048, "adam: the weight has no short last chunk"
    assert scale_n > g["flat_grid"] and scale_n % 256 != 0, "scale: %d elements fit one grid of %d" % (scale_n, g["flat_grid"])
    prods = [C * H for _, C, H in se_gate]
    assert g["se_sliced_max"] in prods, "se_gate: no shape at the limit C * H = %d of the sliced backward" % g["se_sliced_max"]
    assert sum(p > g["se_sliced_max"] for p in prods) >= 2, "se_gate: fewer than two shapes take the kernel past C * H = %d" % g["se_sliced_max"]
    assert any(p <= g["se_sliced_max"] and B > g["se_sliced_workgroups"] and B % g["se_sliced_workgroups"] % 2 == 1 for (B, _, _), p in zip(se_gate, prods)), \
        "se_gate: no shape gives the %d workgroups of the sliced backward an odd number of second samples" % g["se_sliced_workgroups"]
    lanes = set()
    for (B, C, T, V) in dstd_stats:
        d = glue_geometry(C, T, V)
        assert d["dstd_lds"] > 0, "dstd_stats %s: unsupported" % ((B, C, T, V),)
        assert d["dstd_last_rows"] < d["dstd_rows_per_iteration"], "dstd_stats %s: %d rows fill the last of %d iterations of %d rows" % (
            (B, C, T, V), C * T, d["dstd_iterations"], d["dstd_rows_per_iteration"])
        lanes.add((d["dstd_lanes"], V <= d["dstd_lanes"], d["dstd_iterations"] > 1))
    for lpr in (16, 32, 64):
        assert (lpr, True, True) in lanes, "dstd_stats: no shape walks several iterations with %d lanes per row" % lpr
    assert (64, False, False) in lanes or (64, False, True) in lanes, "dstd_stats: no row wider than 64 lanes"
    assert {V for (_, _, _, V) in dstd_stats} >= {16, 17, 32, 33, 64, 65}, "dstd_stats: a lane-group boundary is missing"
    assert max(V for (_, _, _, V) in dstd_stats) > 128, "dstd_stats: no row takes a third step of 64 lanes"
    d = glue_geometry(*dstd_lds[1:])
    assert d["dstd_lds"] > g["lds_default"], "dstd_stats %s: %d bytes of LDS stay under the default limit of %d" % (dstd_lds, d["dstd_lds"], g["lds_default"])
    assert dstd_lds in dstd_stats
    assert zero_big[0] > g["zero_grid_bytes"] + 16 and zero_big[1] % 16 != 0 and (zero_big[0] - (16 - zero_big[1] % 16)) % 16 != 0, \
        "cg_zero: %d bytes at offset %d do not give a head, more than one grid of %d bytes and a tail" % (zero_big + (g["zero_grid_bytes"],))
    P = reduce_shape[2] * reduce_shape[3]
    assert 512 < P < 768, "reduce_bc: %d positions do not give 256 threads a partial third iteration" % P
    assert eval_scatter[2] > 64, "eval_scatter_mpjpe: %d joints fit one pass of 64 threads" % eval_scatter[2]
    return g
