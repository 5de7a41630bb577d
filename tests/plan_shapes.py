"""Model configurations that put a launch-plan predicate of models/CISTGCN/CISTGCN.py on the side the reference's YAML shapes never
reach, and the plan each of them must produce.

The staged block chooses per call between a fused kernel and a generic fallback (contract_many, the row-kernel chain).  The shapes of
the golden fixtures and of helpers.make_cfg's defaults keep every choice on one side; the entries below move one (sometimes two) of
them across.  checks.check_model_plan runs an entry through check_model_branch_replay (fp64 oracle on the kernels' PReLU branches)
and asserts, BEFORE any number is compared, how often each C entry point below ran in the one forward: a moved limit then fails
with a message about the plan, and a fallback that is no longer reached cannot leave the test green.

The counts are written by hand as (launches per block) * (blocks inside the limit); they are not derived by calling the predicates.
Blocks of a model with model_complexity [w1 .. wn]: input blocks 10 -> w1 -> .. -> wn -> 10 on (T, V) = (input_n, joints), then the
output block 3 -> 3 on (T, V) = (joints, output_n), whose input is a permuted view (never contiguous).  Per block (cin -> cout, T, V):

  cg_map2adj_tail_fwd   2 (two phases)        T <= 64 and V <= 64
  cg_dstd_tail_fwd      4 (four phases)       cout <= 64
  cg_stgcn_domain_fwd   2 (two domains)       cin <= 128 and cout <= 128
  cg_gate_head_fwd      1                     cout <= 64 and 2 + 2 * T <= 192
  cg_block_input_fwd    1                     contiguous input: every input block, never the output block
  cg_context_heads_fwd  1 per model           hidden_dim <= 64 and output_n * 3 * joints <= 16384
  cg_fpn_conv_fwd       1 per FPN (txc)       B >= ops._FPN_MIN_BATCH, 10 * joints <= 256, 10 * joints % 4 in (0, 2)
  cg_rank1_adj_fwd      never                 only with CISTGCN.fused_adj switched off

and, only once the block input is `big` (numel >= stack_min_elements: `stack_all=True` sets that to 0; 0 launches otherwise):

  cg_collapse_rows_fwd  1 (stacked gates)     contiguous input, cin * T % 4 == 0, V <= 32, 2 * (cout // 2) <= 64
                      + 2 (towers)            (cin // 2) * T % 4 == 0, V <= 32, cin // 2 <= 64
  cg_collapse_cols_fwd  2 (towers)            (cin // 2) * V % 4 == 0, T <= 64, cin // 2 <= 64
  cg_pointwise_maps_fwd 1 (stacked towers)    contiguous input, T * V even, cin <= 128, 4 * ceil16(cin // 2) <= 128
                      + 1 per residual group  cin != cout: three maps of cout rows, groups of <= 128 stacked rows (ceil16 each);
                                              T * V even, cin <= 128, cout <= 64
"""
from cistgcn_amd import _lib

A, D, S, G, I = "cg_map2adj_tail_fwd", "cg_dstd_tail_fwd", "cg_stgcn_domain_fwd", "cg_gate_head_fwd", "cg_block_input_fwd"
X, F, R1 = "cg_context_heads_fwd", "cg_fpn_conv_fwd", "cg_rank1_adj_fwd"
ROWS, COLS, PWM = "cg_collapse_rows_fwd", "cg_collapse_cols_fwd", "cg_pointwise_maps_fwd"
ALWAYS = (A, D, S, G, I, X, F, R1)          # asserted whatever `stack_all` is
STACKED = (ROWS, COLS, PWM)                 # 0 without `stack_all`, the `stacked` counts with it

SMALL = dict(blocks=1, txc=1)               # three DSTD blocks: 10 -> C, C -> 10 and the output block


def _entry(name, shape, cfg, flips, plan, stacked, patch=None, stage_geometry=False):
    return dict(name=name, shape=shape, cfg=cfg, flips=flips, plan=plan, stacked=stacked, patch=patch or {}, stage_geometry=stage_geometry)


# `plan` lists the entry points whose count differs from "every block inside every limit" next to the ones that do not, so that each
# line can be read without the baseline.  (C, T, V, B); B = 8 everywhere: BatchNorm over two or three samples is ill-conditioned and
# misses the 1e-4 rule on fused and generic paths alike.
PLANS = (
    _entry("baseline", (8, 10, 22, 8), SMALL, "nothing: the plan every other entry is read against",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           # rows: 10 -> 8: gates (100); towers 5 * 10 = 50 no.  8 -> 10: gates + towers (80, 40).  output block: 1 * 22 no
           # cols: 5 * 22 = 110 no; 4 * 22 = 88; output block 1 * 25 no.  maps: towers + one residual group in both input blocks
           {ROWS: 1 + 3, COLS: 2 * 1, PWM: 2 + 2}),
    _entry("T70", (8, 70, 6, 8), SMALL, "map2adj tail T <= 64, collapse_cols T <= 64",
           {A: 2 * 1, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},            # adjacency tail: the output block (6, 25) only
           # rows: gates 700 | gates 560 + towers 280 (5 * 70 = 350 no); cols: T = 70 in both input blocks, 1 * 25 in the output block
           {ROWS: 1 + 3, COLS: 0, PWM: 2 + 2}),
    _entry("T70-wide", (16, 70, 22, 8), dict(blocks=2, txc=2), "map2adj tail T <= 64, collapse_cols T <= 64, two-block depth",
           {A: 2 * 1, D: 4 * 4, S: 2 * 4, G: 1 * 4, I: 1 * 3, X: 1, F: 0, R1: 0},
           # rows: 10 -> 16 gates | 16 -> 16 gates + towers (8 * 70) | 16 -> 10 the same; maps: 2 | 1 (no residual maps) | 2
           {ROWS: 1 + 3 + 3, COLS: 0, PWM: 2 + 1 + 2}),
    _entry("V40", (8, 10, 40, 8), SMALL, "collapse_rows V <= 32 (still inside map2adj tail V <= 64)",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           # rows: V = 40 in both input blocks; the output block (40, 25): towers 1 * 40.  cols: 5 * 40, 4 * 40; output block 1 * 25 no
           {ROWS: 2 * 1, COLS: 2 * 2, PWM: 2 + 2}),
    _entry("V70", (8, 10, 70, 8), SMALL, "map2adj tail V <= 64 (input blocks) and T <= 64 (output block), collapse_rows V <= 32, collapse_cols T <= 64 (output block)",
           {A: 0, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           # rows: V = 70; output block 1 * 70 no.  cols: 5 * 70 = 350 no, 4 * 70 = 280; output block T = 70
           {ROWS: 0, COLS: 2 * 1, PWM: 2 + 2}),
    # joints = 24: the towers of the output block (24, output_n) would take collapse_rows (1 * 24) and collapse_cols but for output_n
    _entry("To40", (8, 10, 24, 8), dict(SMALL, To=40), "collapse_rows V <= 32 in the output block",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           # rows: gates | gates + towers | output block V = 40.  cols: 5 * 24, 4 * 24, output block 1 * 40
           {ROWS: 1 + 3, COLS: 2 * 3, PWM: 2 + 2}),
    _entry("To70", (8, 10, 24, 8), dict(SMALL, To=70), "map2adj tail V <= 64 and collapse_rows V <= 32 in the output block",
           {A: 2 * 2, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           # cols: output block 1 * 70 no
           {ROWS: 1 + 3, COLS: 2 * 2, PWM: 2 + 2}),
    _entry("T25", (10, 25, 22, 8), SMALL, "collapse_rows C * T % 4 (10 * 25, 5 * 25), collapse_cols C * V % 4 (5 * 22)",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           {ROWS: 0, COLS: 0, PWM: 1 + 1}),               # 10 -> 10 -> 10: no residual maps
    _entry("TV-odd", (6, 9, 9, 8), dict(SMALL, To=9), "pointwise_maps / tower_maps H * W even (9 * 9), every % 4 condition",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           {ROWS: 0, COLS: 0, PWM: 0}),                   # 90, 45 | 54, 27 | 9: nothing divides by four
    _entry("hidden96", (8, 10, 22, 8), dict(SMALL, hidden=96), "context_heads hidden <= 64",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 0, F: 0, R1: 0},
           {ROWS: 1 + 3, COLS: 2 * 1, PWM: 2 + 2}),
    _entry("C72", (72, 10, 22, 8), SMALL, "dstd tail C <= 64, gate head C <= 64, rows_gate 2 * out_channels <= 64, pointwise_maps rows (inside the stage limit)",
           {A: 2 * 3, D: 4 * 2, S: 2 * 3, G: 1 * 2, I: 1 * 2, X: 1, F: 0, R1: 0},            # 10 -> 72 leaves the tail and the gate head
           # rows: 10 -> 72: stacked gates 72 rows no, towers 50 no | 72 -> 10: gates + towers (36 * 10).  cols: 36 * 22.
           # maps: 10 -> 72: towers, residual maps of 72 rows no | 72 -> 10: towers 4 * 48 rows no, one residual group
           {ROWS: 0 + 3, COLS: 2 * 1, PWM: 1 + 1}),
    _entry("C130", (130, 10, 22, 8), SMALL, "fused stage Cin, Cout <= 128, collapse O <= 64, pointwise_maps C <= 128",
           {A: 2 * 3, D: 4 * 2, S: 2 * 1, G: 1 * 2, I: 1 * 2, X: 1, F: 0, R1: 0},            # the fused stage: the output block only
           # rows: 130 -> 10: stacked gates (1300, 10 rows); towers of 65 channels no.  maps: the towers of 10 -> 130 only
           {ROWS: 1, COLS: 0, PWM: 1}),
    _entry("T100-C64", (64, 100, 22, 8), SMALL, "gate head S <= 192 (2 + 2 * 100), map2adj tail T <= 64; the stage kernel near its LDS limit",
           {A: 2 * 1, D: 4 * 3, S: 2 * 3, G: 1 * 1, I: 1 * 2, X: 1, F: 0, R1: 0},
           # maps: 10 -> 64: towers + two residual groups (64 + 64 | 64 rows); 64 -> 10: towers (4 * 32 rows) + one group
           {ROWS: 3 + 3, COLS: 0, PWM: 3 + 2}, stage_geometry=True),
    _entry("widths-8-24-16", (8, 10, 22, 8), dict(widths=(8, 24, 16), txc=1), "nothing new alone: every block changes its width (10 -> 8 -> 24 -> 16 -> 10)",
           {A: 2 * 5, D: 4 * 5, S: 2 * 5, G: 1 * 5, I: 1 * 4, X: 1, F: 0, R1: 0},
           # rows: gates | 3 | 3 | 3.  cols: 110 no | 88 | 264 | 176.  maps: towers + one residual group (3 * 32 rows at most) per block
           {ROWS: 1 + 3 + 3 + 3, COLS: 2 * 3, PWM: 2 * 4}),
    _entry("fpn-joints22", (8, 10, 22, 8), dict(blocks=1, txc=2), "ops._FPN_MIN_BATCH (patched to 1): the whole-sample dilated convolutions run",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 1 * 2, R1: 0},
           {ROWS: 1 + 3, COLS: 2 * 1, PWM: 2 + 2}, patch={"_FPN_MIN_BATCH": 1}),
    _entry("fpn-joints28", (8, 10, 28, 8), dict(blocks=1, txc=2), "cg_fpn_conv_supported H * W <= 256 (10 * 28) while the batch threshold says yes",
           {A: 2 * 3, D: 4 * 3, S: 2 * 3, G: 1 * 3, I: 1 * 2, X: 1, F: 0, R1: 0},
           # rows: gates | 3 | the towers of the output block (1 * 28, V = 25).  cols: 5 * 28, 4 * 28
           {ROWS: 1 + 3 + 2, COLS: 2 * 2, PWM: 2 + 2}, patch={"_FPN_MIN_BATCH": 1}),
)
BY_NAME = {e["name"]: e for e in PLANS}
assert len(BY_NAME) == len(PLANS)
# additionally in train mode with dropout 0.1: the site numbering of the fallback paths against the masks of the kernels
DROPOUT_PLANS = ("T70", "C72")


def expected_counts(entry, stack_all):
    want = {k: entry["plan"][k] for k in ALWAYS}
    want.update({k: entry["stacked"][k] if stack_all else 0 for k in STACKED})
    return want


def assert_plan(entry, stack_all, launches):
    """`launches` (loop_shapes.counted_calls) of ONE forward of the entry's model against the hand-written plan"""
    want = expected_counts(entry, stack_all)
    got = {k: launches.get(k, 0) for k in want}
    print("plan %s stack_all=%s (flips %s): %s; cg_contract_many %d" % (entry["name"], stack_all, entry["flips"], got, launches.get("cg_contract_many", 0)))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, "launch plan of %s (stack_all=%s): forward launches (ran, expected) %s - a limit of a shape predicate moved, or a fallback is no longer reached" % (entry["name"], stack_all, wrong)


def stage_kernels(entry):
    """what the fused ST-GCN stage launches for every layer of the entry's input blocks: asked from the library (cg_stgcn_domain_geometry, the
    predicate the launchers use), printed by check_model_plan"""
    import ctypes
    import loop_shapes as L
    C, T, V, B = entry["shape"]
    widths = [10] + list(entry["cfg"].get("widths", [C] * entry["cfg"].get("blocks", 4))) + [10]
    lines = []
    for cin, cout in zip(widths[:-1], widths[1:]):
        wide = cin >= 16 or cout >= 16
        for dom in (0, 1):
            for bwd in (0, 1):
                ntiles, total, per, nwg, grid, planes = L._geom("cg_stgcn_domain_geometry", B, cin, cout, T, V, dom, bwd, 0, n=6)
                mfma = _lib.lib().cg_stgcn_domain_geometry(B, cin, cout, T, V, dom, bwd, 1, (ctypes.c_int * 6)()) == 0
                # the dispatch of cg_stgcn_domain_fwd / _bwd: the plane kernels where the batch-size switch says so; then, for wide layers, the
                # matrix-core kernels (forward: time domain only; graph side J <= 64) where their geometry takes the shape; else the tile kernels
                J = V if dom else T
                kernel = "plane" if planes else "matrix-core" if wide and J <= 64 and (dom == 1 or bwd) and mfma else "tile (VALU)"
                lines.append("stgcn_domain %d -> %d T%d V%d %s %s: %s kernels; tile geometry: %d tiles per sample, %d per workgroup, grid %d"
                             % (cin, cout, T, V, "time" if dom else "space", "backward" if bwd else "forward", kernel, ntiles, per, grid))
    return lines
