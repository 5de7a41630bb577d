"""Shapes that enter the multi-tile loops of the phase kernels, and the assertions that they do.

Most kernels of the hot path hand a workgroup a contiguous range of tiles (or samples) once the batch is large: the next tile
is prefetched while the current one is computed, the last workgroup gets a short range, statistics are folded over hundreds of
workgroups.  The default shape lists of tests/checks.py (B <= 5) stay at one tile per workgroup in every family.  The lists here
are chosen from the host geometry; what the launchers choose is asked from the library itself (the host-only cg_*_geometry
queries of include/cistgcn_hip.h, answered by the functions the launchers call), so a shape that silently stops looping - a
moved threshold - fails with a message about geometry instead of passing without testing anything.

Every list serves (a) the CPU shim (tests/test_emu_ops.py, also under AddressSanitizer) and (b) the MI355X (tests/test_gpu_parity.py).
The shim's cost is per element, not per workgroup: the loops are reached with many tiny samples.

Wanted of a list, where the family has the feature: (a) a workgroup walks >= 2 tiles, >= 3 where the next tile is prefetched,
(b) the last workgroup's range is shorter than the others, (c) a prefetched tile lies in the next sample, (d) the last tile of a
sample is partial, (e) B is odd, (f) the grid is rounded up past the work.
"""
import contextlib
import ctypes

from cistgcn_amd import _lib


def _geom(name, *args, n):
    """the `n` ints a host-only cg_*_geometry query (include/cistgcn_hip.h) writes for the shape `args`"""
    out = (ctypes.c_int * n)()
    _lib.check(getattr(_lib.lib(), name)(*args, out), name)
    return list(out)


def _ranges(what, total, per, nwg):
    """a launch of `nwg` workgroups with `per` consecutive tiles each: the size of the last range"""
    assert nwg >= 1 and (nwg - 1) * per < total <= nwg * per, "%s: inconsistent geometry total %d per %d workgroups %d" % (what, total, per, nwg)
    return total - (nwg - 1) * per


@contextlib.contextmanager
def counted_calls():
    """names of the C entry points launched inside the block -> count"""
    launches = {}
    orig = _lib.call

    def counting(name, *args):
        launches[name] = launches.get(name, 0) + 1
        return orig(name, *args)

    _lib.call = counting
    try:
        yield launches
    finally:
        _lib.call = orig


# ---- Map2Adj tail: (B, T, V).  tiles per workgroup 2 / 4 / 8 at B >= 32 / 64 / 128; a tower has ceil(J * J / PT) tiles per sample with
# PT = 256 / 128 / 64 positions for Kc <= 16 / <= 32 / > 32 (space tower: Kc = V, J = T; time tower: Kc = T, J = V).
#   (33, 34, 12)  tpw 2: space 1156 / 256 -> 5 tiles in 3 ranges (2, 2, 1), time 144 / 64 -> 3 tiles in 2 ranges (2, 1): the time tower's third
#                 workgroup of every sample is surplus
#   (67, 34, 6)   tpw 4: space 5 tiles in 2 ranges (4, 1): three prefetches in a row; time 1 tile
#   (129, 10, 22) tpw 8: time 484 / 256 -> 2 tiles in one range
#   (131, 50, 3)  tpw 8: space 2500 / 256 -> 10 tiles in 2 ranges (8, 2)
MAP2ADJ_TAIL = ((33, 34, 12), (67, 34, 6), (129, 10, 22), (131, 50, 3))


def assert_map2adj_tail_loops(shapes=MAP2ADJ_TAIL, whole_list=True):
    seen_tpw, deep, ragged, surplus = set(), False, False, False
    for (B, T, V) in shapes:
        towers = []
        for dom, (Kc, J) in enumerate(((V, T), (T, V))):
            PT, ntiles, tpw, nch = _geom("cg_map2adj_tail_geometry", B, Kc, J, n=4)
            last = _ranges("map2adj_tail %s tower %d" % ((B, T, V), dom), ntiles, tpw, nch)
            towers.append(dict(PT=PT, tiles=ntiles, tpw=tpw, ranges=nch, loops=min(tpw, ntiles), last=last, partial=(J * J) % PT != 0))
        print("map2adj_tail geometry B%d T%d V%d: space %s | time %s" % (B, T, V, towers[0], towers[1]))
        best = max(towers, key=lambda t: t["loops"])
        assert best["loops"] >= 2, "map2adj_tail %s: geometry keeps one tile per workgroup (%s): the shape does not test the tile loop" % ((B, T, V), towers)
        assert best["partial"], "map2adj_tail %s: geometry has no partial last tile (%s)" % ((B, T, V), towers)
        assert B % 2 == 1
        seen_tpw.add(best["tpw"])
        deep = deep or best["loops"] >= 3
        ragged = ragged or any(t["ranges"] >= 2 and t["last"] < t["tpw"] and t["loops"] >= 2 for t in towers)
        surplus = surplus or towers[0]["ranges"] != towers[1]["ranges"]
    if whole_list:
        assert seen_tpw >= {2, 4, 8}, "map2adj_tail: geometry reaches only %s tiles per workgroup, wanted 2, 4 and 8" % sorted(seen_tpw)
        assert deep, "map2adj_tail: geometry gives no workgroup three tiles (two prefetches in a row)"
        assert ragged, "map2adj_tail: geometry gives no sample a short last range"
        assert surplus, "map2adj_tail: geometry launches no surplus workgroups (towers with different range counts)"


# ---- DSTD tail: (B, C, T, V).  Matrix phases: B * ceil(T*V / 64) tiles (F2) / B * ceil(T*V / 32) tiles (K3) in sample-major order,
# ceil(total / 512) consecutive ones per workgroup.  Row phases: cg_tail_rows samples of a channel per workgroup.
#   (701, 8, 4, 8)    P = 32: one tile per sample, 2 per workgroup (last range 1): every prefetched tile lies in the next sample
#   (523, 16, 6, 13)  P = 78: F2 2 tiles per sample (the second partial), 1046 tiles, 3 per workgroup, last range 2; K3 3 tiles per sample,
#                     1569 tiles, 4 per workgroup, last range 1; rows: 13 samples per workgroup, the last one 3
#   (1031, 20, 3, 5)  P = 15: 1031 tiles, 3 per workgroup, last range 2; the run-time form of the matrix phases (C = 20)
#   (131, 64, 6, 11)  rows: 16 samples per workgroup, the last one 3; widest instantiation of the matrix phases, one tile per workgroup
DSTD_TAIL = ((701, 8, 4, 8), (523, 16, 6, 13), (1031, 20, 3, 5), (131, 64, 6, 11))


def dstd_tail_geometry(B, C, T, V):
    o = _geom("cg_dstd_tail_geometry", B, C, T, V, n=12)
    what = "dstd_tail %s" % ((B, C, T, V),)
    g = {"rows": o[0], "row_groups": o[1], "row_last": _ranges(what + " rows", B, o[0], o[1])}
    for k, base in (("F2", 2), ("K3", 7)):
        PT, tps, total, per, nwg = o[base:base + 5]
        g[k] = dict(PT=PT, tps=tps, total=total, per=per, nwg=nwg, last=_ranges(what + " " + k, total, per, nwg), partial=(T * V) % PT != 0)
    return g


def assert_dstd_tail_loops(shapes=DSTD_TAIL, whole_list=True):
    got = {"F2": [False] * 4, "K3": [False] * 4}
    rows_ragged = False
    for shape in shapes:
        g = dstd_tail_geometry(*shape)
        print("dstd_tail geometry B%d C%d T%d V%d: %s" % (shape + (g,)))
        assert g["F2"]["per"] >= 2 or g["K3"]["per"] >= 2 or g["rows"] >= 2, "dstd_tail %s: geometry keeps one tile and one sample per workgroup (%s)" % (shape, g)
        assert shape[0] % 2 == 1
        for k in ("F2", "K3"):
            m = g[k]
            got[k][0] |= m["per"] >= 3                                # two prefetches in a row
            got[k][1] |= m["per"] >= 2 and m["last"] < m["per"]       # short last range
            got[k][2] |= m["per"] >= 2 and m["tps"] < m["per"]        # every range crosses into the next sample
            got[k][3] |= m["per"] >= 2 and m["tps"] >= 2 and m["partial"]     # partial last tile of a sample inside a range
        rows_ragged |= g["rows"] >= 2 and g["row_last"] < g["rows"]
    if whole_list:
        for k in ("F2", "K3"):
            names = ("three tiles per workgroup", "a short last range", "ranges that cross samples", "a partial last tile inside a range")
            for ok, name in zip(got[k], names):
                assert ok, "dstd_tail: geometry of phase %s gives no shape with %s" % (k, name)
        assert rows_ragged, "dstd_tail: geometry of the row phases gives no shape with several samples per workgroup and a short last group"


# ---- stacked pointwise maps (tower_maps / pointwise_maps / the deferred tower level): (B, Cin, (M_i), T, V[, O]).  B * ceil(T*V / PT) tiles
# in sample-major order over at most 512 workgroups (PT = 256 positions forward; backward 128 when 64 stacked rows are staged).
#   (1031, 10, (5, 5, 5, 5), 4, 5)   P = 20: 1031 tiles, 3 per workgroup, last range 2
#   (701, 20, (10, 33), 3, 6)        P = 18: 701 tiles, 2 per workgroup, last range 1 (biases in check_pointwise_maps: second shape of a list)
#   (523, 10, (5, 5, 5, 5), 10, 30)  P = 300: 2 tiles per sample forward (the second partial), 3 backward; 3 / 4 per workgroup
TOWER_MAPS = ((1031, 10, (5, 5, 5, 5), 4, 5),)
TOWER_MAPS_WIDE = ((523, 10, (5, 5, 5, 5), 10, 30),)
POINTWISE_MAPS = ((1031, 10, (5, 5, 5, 5), 4, 5), (701, 20, (10, 33), 3, 6))
# the deferred level also loops in the backward of its collapsing convolutions (B > 768 samples per K range, see below)
TOWER_COLLAPSE = ((803, 10, (8, 8, 8, 8), 6, 8, 5),)


def assert_pointwise_maps_loops(shapes, deep=True, name="pointwise_maps"):
    seen_deep, seen_ragged = False, False
    for shape in shapes:
        B, Cin, Ms, T, V = shape[:5]
        arr = (ctypes.c_int * len(Ms))(*Ms)
        for bwd in (0, 1):
            PT, tps, total, per, nwg = _geom("cg_pointwise_maps_geometry", B, Cin, T * V, len(Ms), arr, bwd, n=5)
            last = _ranges("%s %s" % (name, shape), total, per, nwg)
            print("%s geometry %s %s: %d positions per tile, %d tiles per sample, %d tiles, %d per workgroup, %d workgroups, last range %d"
                  % (name, shape, "backward" if bwd else "forward", PT, tps, total, per, nwg, last))
            assert per >= 2, "%s %s: geometry keeps one tile per workgroup (%d tiles): the shape does not test the tile loop" % (name, shape, total)
            assert tps < per or tps == 1
            seen_deep |= per >= 3
            seen_ragged |= last < per
        assert B % 2 == 1 and (T * V) % 2 == 0
    assert seen_ragged, "%s: geometry gives no shape a short last range" % name
    assert seen_deep or not deep, "%s: geometry gives no workgroup three tiles (two prefetches in a row)" % name


# ---- collapsing convolutions, backward: (B, C, T, V, O).  grid = K ranges x sample slices, ceil(B / (768 / K ranges)) samples per slice.
#   (803, ...)   one K range: 2 samples per slice, 402 slices, the last one sample
#   (1543, ...)  3 samples per slice, 515 slices, the last one sample
COLLAPSE_ROWS = ((803, 6, 4, 7, 5), (1543, 6, 4, 7, 5))
COLLAPSE_COLS = ((803, 6, 4, 8, 5), (1543, 6, 3, 4, 3))


def assert_collapse_loops(shapes, cols, name=None):
    name = name or ("collapse_cols" if cols else "collapse_rows")
    seen_deep = False
    for (B, C, T, V, O) in shapes:
        kranges, slices, per = _geom("cg_collapse_geometry", B, C, T, V, O, 1 if cols else 0, n=3)
        last = _ranges("%s %s" % (name, (B, C, T, V, O)), B, per, slices)
        print("%s geometry B%d C%d T%d V%d O%d backward: %d K ranges x %d slices of %d samples, last slice %d" % (name, B, C, T, V, O, kranges, slices, per, last))
        assert per >= 2, "%s %s: geometry keeps one sample per slice: the shape does not test the sample loop" % (name, (B, C, T, V, O))
        assert last < per and B % 2 == 1
        seen_deep |= per >= 3
    return seen_deep


# ---- dilated convolutions of the FPN, weight gradient: (B, Cin, Cout, H, W).  at most 170 workgroups per dilation, ceil(B / 170) samples each.
#   (173, ...)  2 samples per workgroup, 87 workgroups, the last one sample;  (343, ...)  3 per workgroup, 115 workgroups, the last one sample
DILATED_CONVS = ((173, 5, 4, 10, 7), (343, 6, 5, 4, 6))


def assert_dilated_convs_loops(shapes=DILATED_CONVS, whole_list=True):
    seen_deep = False
    for (B, Cin, Cout, H, W) in shapes:
        assert _lib.lib().cg_fpn_conv_supported(B, Cin, Cout, H, W) == 1, "dilated_convs %s: not a shape of the whole-sample kernels" % ((B, Cin, Cout, H, W),)
        per, nwg = _geom("cg_fpn_conv_geometry", B, Cin, Cout, H, W, n=2)
        last = _ranges("dilated_convs %s" % ((B, Cin, Cout, H, W),), B, per, nwg)
        print("dilated_convs geometry B%d Cin%d Cout%d H%d W%d dW: %d samples per workgroup, %d workgroups, last %d" % (B, Cin, Cout, H, W, per, nwg, last))
        assert per >= 2, "dilated_convs %s: geometry keeps one sample per workgroup: the shape does not test the sample loop" % ((B, Cin, Cout, H, W),)
        assert last < per and B % 2 == 1
        seen_deep |= per >= 3
    assert seen_deep or not whole_list, "dilated_convs: geometry gives no workgroup three samples"


# ---- fused ST-GCN stage: (B, Cin, Cout, T, V).  Tile kernels (both sides narrower than 16 channels; space-domain forward of wide layers):
# total / 2048 tiles per workgroup (1 in the space-domain forward).  Matrix-core kernels (wide layers: time-domain forward, both backwards):
# ceil(total / 512).  Both grids are rounded up to a multiple of eight workgroups.
#   (4211, 3, 3, 6, 9)     tile kernels: 2 tiles per workgroup, last range 1
#   (1543, 18, 16, 5, 7)   matrix-core kernels (pinned: the plane generation would take this batch size where it has the (T, V) family)
STGCN_TILE = ((4211, 3, 3, 6, 9),)
STGCN_MFMA = ((1543, 18, 16, 5, 7),)
# plane kernels (no query: the launchers of stgcn_domain_planes.hip hold this arithmetic inline; derived from its constants):
#   forward: one workgroup per (sample, chunk of 16 output channels), grid = 8 * ceil(B / 8) * ceil(Cout / 16); a workgroup walks ALL groups
#   of its sample (NG = V joints in the space domain, T frames in the time domain), one group per wave at a time over 4 waves;
#   backward: one workgroup per (sample, chunk of frames), <= 16 frames (space) / 8 frames (time) per chunk, the same grid rounding.
#   (131, 32, 16, 10, 18): 18 | 10 groups per forward workgroup (5 | 3 rounds of 4 waves, the last round short); T = 10 is one chunk in the
#   space backward and two chunks (8 + 2 frames, the second short) in the time backward; 131 samples: the workgroups of 5 surplus samples
#   return at once.  What can be observed from outside is asserted by the tests: B % 8 != 0, B > 64, V % 4 != 0 and T % 8 != 0.
STGCN_PLANES = ((131, 32, 16, 10, 18),)


def assert_stgcn_domain_loops(shapes, kind):
    """geometry with the plane generation pinned off, as checks.check_stgcn_domain(planes=None) runs these shapes"""
    prev = _lib.lib().cg_stgcn_domain_planes_min_workgroups(1 << 40)
    try:
        _assert_stgcn_domain_loops(shapes, kind)
    finally:
        _lib.lib().cg_stgcn_domain_planes_min_workgroups(prev)


def _assert_stgcn_domain_loops(shapes, kind):
    name = "stgcn_domain (%s kernels)" % ("matrix-core" if kind else "tile")
    for (B, Cin, Cout, T, V) in shapes:
        wide = Cin >= 16 or Cout >= 16
        assert wide == bool(kind), "%s %s: the dispatch sends this width to the other generation" % (name, (B, Cin, Cout, T, V))
        launches = [(1, 1), (0, 1), (1, 0)] if kind else [(0, 1), (1, 1), (1, 0)]        # (domain, backward): space forward is one tile per workgroup / tile kernel
        rounded = False
        for dom, bwd in launches:
            ntiles, total, per, nwg, grid, planes = _geom("cg_stgcn_domain_geometry", B, Cin, Cout, T, V, dom, bwd, kind, n=6)
            assert planes == 0, "%s %s: the plane generation is not pinned off" % (name, (B, Cin, Cout, T, V))
            last = _ranges("%s %s" % (name, (B, Cin, Cout, T, V)), total, per, nwg)
            print("%s geometry B%d Cin%d Cout%d T%d V%d domain %d %s: %d tiles per sample, %d tiles, %d per workgroup, %d workgroups (last range %d) in a grid of %d"
                  % (name, B, Cin, Cout, T, V, dom, "backward" if bwd else "forward", ntiles, total, per, nwg, last, grid))
            assert per >= 2, "%s %s: geometry keeps one tile per workgroup (%d tiles): the shape does not test the tile loop" % (name, (B, Cin, Cout, T, V), total)
            assert grid >= nwg and grid % 8 == 0
            rounded |= grid > nwg
        assert B % 2 == 1
        assert rounded, "%s %s: no grid of this shape is rounded up past the work" % (name, (B, Cin, Cout, T, V))


# ---- block input: (B, C, T, V, aliases).  A workgroup owns one span of floor(4608 / (T * V)) planes (channels) of one sample and walks them;
# grid = B * spans per sample.  No workgroup takes tiles of another sample, so what can loop is the plane walk and the short last span.
#   (523, 48, 5, 22, 3)  110 positions per plane: 41 planes per span, 2 spans per sample (41 + 7 planes), 1046 workgroups
BLOCK_INPUT = ((523, 48, 5, 22, 3),)


def assert_block_input_loops(shapes=BLOCK_INPUT):
    for (B, C, T, V, n) in shapes:
        npl, cps, grid = _geom("cg_block_input_geometry", B, C, T, V, n=3)
        print("block_input geometry B%d C%d T%d V%d: %d planes per span, %d spans per sample (last %d planes), %d workgroups" % (B, C, T, V, npl, cps, C - (cps - 1) * npl, grid))
        assert cps >= 2 and npl >= 2, "block_input %s: geometry gives a sample one span (%d planes): the shape does not test the span split" % ((B, C, T, V), npl)
        assert (cps - 1) * npl < C < cps * npl, "block_input %s: geometry gives no short last span" % ((B, C, T, V),)
        assert grid == B * cps and grid >= 1000 and B % 2 == 1


# ---- families without a list of their own:
#   cg_chan_stats(_many) walks cg_rows_per_block samples like the row kernels and runs in every train-mode case of check_norm_act_rows
#   (no channel sums are handed over there); the batched row ops (norm_act_many) are the same kernels and run in the chain of check_dstd_tail
#   at the DSTD_TAIL shapes.
#   contract.hip: the streaming and K-reduction variants size their per-workgroup ranges from N and K (cg_contract_blocks); their own checks
#   (check_contract_stream: last workgroup partially filled, several row tiles; check_contract_kred: several splits per replica, K = 80 000)
#   choose sizes for that already and assert through ops._plans that the variant ran; they have no batch-driven loop of the kind listed here.
#
# ---- row kernels (cg_norm_act_*, cg_chan_stats): (B, C, T, V).  cg_rows_per_block samples of one channel per workgroup.
#   (701, 3, 5, 7)  4 samples per workgroup, 176 groups per channel, the last one sample
NORM_ACT_ROWS = ((701, 3, 5, 7),)


def assert_norm_act_rows_loop(shapes=NORM_ACT_ROWS):
    for (B, C, T, V) in shapes:
        v = _lib.View4()
        for i, (n, s) in enumerate(zip((B, C, T, V), (C * T * V, T * V, V, 1))):
            v.n[i], v.s[i] = n, s
        rb = _lib.lib().cg_norm_act_rows_per_block(ctypes.byref(v))
        print("norm_act geometry B%d C%d T%d V%d: %d samples of a channel per workgroup, last group %d" % (B, C, T, V, rb, B - (B - 1) // max(rb, 1) * rb))
        assert rb >= 2, "norm_act %s: geometry keeps one sample per workgroup (%d): the shape does not test the row loop" % ((B, C, T, V), rb)
        assert B % rb != 0 and B % 2 == 1
