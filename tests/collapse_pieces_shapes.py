"""Shapes of the collapse-pieces tests (CPU shim and MI355X) and the properties they are chosen for, asked from the library's own
geometry query.  (B, C, T, V, O); tower: (B, Cin, (M_i), T, V, O)."""
from loop_shapes import _geom, _ranges

ROWS = (
    (805, 6, 14, 7, 5),      # K = 84: two K ranges, the last short; three samples per slice, short last slice; odd V <= 16
    (5, 12, 6, 17, 33),      # K = 72; the second column tile holds one column; O = 33 (three output tiles, the last of one row)
    (3, 8, 16, 32, 64),      # two full ranges; V = 32 and O = 64, the limits
    (2, 4, 1, 16, 16),       # T = 1, K = 4
)
COLS = (
    (805, 12, 5, 6, 5),      # two K ranges, three samples per slice; planes of 30 floats: 8-byte aligned
    (3, 4, 3, 5, 3),         # planes of 15 floats: 4-byte aligned
    (5, 10, 20, 10, 33),     # K = 100; two frame tiles
    (2, 8, 64, 16, 64),      # T = 64 and O = 64, the limits
    (3, 6, 33, 22, 20),      # three ranges, the last of four rows; T = 33
)
TOWER = ((805, 10, (6, 12), 14, 6, 5),)      # transform on load, both axes with two K ranges and three samples per slice


def ident(shape):
    return "-".join(str(s) if not isinstance(s, tuple) else "x".join(map(str, s)) for s in shape)


def _loop_properties(shape, cols):
    """two or more K ranges with a short last one, three or more samples per slice, a short last slice, odd B"""
    B, C, T, V, O = shape
    kranges, slices, per = _geom("cg_collapse_geometry", B, C, T, V, O, 1 if cols else 0, n=3)
    last = _ranges("collapse pieces %s" % (shape,), B, per, slices)
    K = C * (V if cols else T)
    print("collapse pieces %s %s: %d K ranges x %d slices of %d samples, last slice %d" % ("cols" if cols else "rows", shape, kranges, slices, per, last))
    # a range is a whole number of 16-row matrix-core tiles: with K no multiple of 16 the last range is short and its last tile partial
    assert kranges >= 2 and K % 16 != 0, "%s: no short last K range (K = %d, %d ranges)" % (shape, K, kranges)
    assert per >= 3 and last < per and B % 2 == 1, "%s: needs three samples per slice, a short last slice, odd B" % (shape,)


def assert_properties():
    _loop_properties(ROWS[0], cols=False)
    _loop_properties(COLS[0], cols=True)
    B, C, Ms, T, V, O = TOWER[0]
    _loop_properties((B, Ms[0], T, V, O), cols=False)
    _loop_properties((B, Ms[1], T, V, O), cols=True)
    for shape, cols in ((ROWS[2], False), (COLS[4], True)):
        B, C, T, V, O = shape
        kranges = _geom("cg_collapse_geometry", B, C, T, V, O, 1 if cols else 0, n=3)[0]
        assert kranges >= 2, "%s: one K range" % (shape,)
    assert (COLS[0][2] * COLS[0][3]) % 4 == 2 and (COLS[1][2] * COLS[1][3]) % 2 == 1      # plane alignment: 8 and 4 bytes
