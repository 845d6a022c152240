"""CPU guard of the key-switch shape table (tests/tfhe_ks_shapes.py): the table, taken together, holds every path of
tfhe_keyswitch_kernel's loops that the shapes of tests/test_gpu_tfhe_bootstrap.py leave out, and those shapes do leave them
out.  The grouping rule is recomputed here as DESIGN.md §13 states it (ki * ell <= 64, at most 8 mask words per group);
nothing is imported from the library, and nothing needs a GPU."""
import tfhe_edge_words
from tfhe_ks_shapes import (KS_EDGE_SHAPES, KS_TILE_BATCH, KS_TILE_COLS, KS_UNROLL, group_rows, group_words)

# ki and the key rows of every group as they were worked out by hand when the table was written, entry by entry
EXPECTED = [(8, [24, 15]), (8, [15]), (8, [3]), (8, [40, 40, 5]), (8, [48, 6]), (5, [55, 44]), (8, [56, 56, 21]),
            (7, [63, 36]), (6, [60, 60, 10]), (4, [60, 30]), (3, [51, 51, 17]), (3, [63, 63, 63, 21]), (1, [33] * 5)]


def test_grouping_rule():
    """ki = max(1, min(64 / ell, 8)): the largest group whose digits fit the LDS, one thread per (ciphertext, mask word)"""
    for ell in range(1, 65):
        ki = group_words(ell)
        assert 1 <= ki <= 8
        assert ki * ell <= 64 or ki == 1
        assert ki == 8 or (ki + 1) * ell > 64
    assert [group_words(ell) for ell in (1, 8, 9, 10, 11, 12, 13, 16, 17, 21, 22, 32, 33, 64)] == \
        [8, 8, 7, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1]
    assert group_rows(13, 3) == [24, 15] and group_rows(8, 3) == [24] and group_rows(5, 33) == [33] * 5


def test_table_entries_are_valid_and_as_worked_out():
    assert len(EXPECTED) == len(KS_EDGE_SHAPES)
    for (bits, in_dim, out_dim, lb, ell, batch), (ki, rows) in zip(KS_EDGE_SHAPES, EXPECTED):
        assert bits in (32, 64) and 0 < lb < bits and 0 < ell <= bits // lb        # ApproxSignedBasis::new accepts it
        assert tfhe_edge_words.shape(bits, lb, ell) == (ell, bits - ell * lb)
        assert in_dim > 0 and out_dim > 0 and batch > 0
        assert group_words(ell) == ki and group_rows(in_dim, ell) == rows, (bits, in_dim, out_dim, lb, ell)
        assert sum(rows) == in_dim * ell


def test_table_holds_every_path_of_the_key_switch_loops():
    shapes = [(bits, in_dim, out_dim, ell, batch, group_words(ell), group_rows(in_dim, ell))
              for bits, in_dim, out_dim, _, ell, batch in KS_EDGE_SHAPES]
    groups = [r for s in shapes for r in s[6]]
    # the remainder loop behind the unrolled one, with every count of left-over rows; and alone
    assert {r % KS_UNROLL for r in groups} >= {1, 2, 3}
    assert any(r < KS_UNROLL for r in groups)
    for rem in (1, 2, 3):
        assert any(r > KS_UNROLL and r % KS_UNROLL == rem for r in groups), rem
    # every group size, the non-powers of two among them (threadIdx.x % ki, threadIdx.x / ki)
    assert {s[5] for s in shapes} >= {1, 3, 4, 5, 6, 7, 8}
    # a short last group behind at least one full group; and a mask shorter than one group
    assert any(len(rows) >= 2 and rows[-1] < rows[0] for *_, rows in shapes)
    for want_ki in (3, 5, 6, 7, 8):
        assert any(ki == want_ki and len(rows) >= 2 and rows[-1] < rows[0] for *_, ki, rows in shapes), want_ki
    assert any(in_dim < ki for _, in_dim, _, _, _, ki, _ in shapes)
    # the column clamp and the second blockIdx.x: one and two full tiles of columns, and one column more
    assert {out_dim + 1 for _, _, out_dim, *_ in shapes} >= {KS_TILE_COLS, KS_TILE_COLS + 1, 2 * KS_TILE_COLS,
                                                            2 * KS_TILE_COLS + 1}
    # the tile of ciphertexts: one short of it, it, one more
    assert {batch for *_, batch, _, _ in shapes} >= {KS_TILE_BATCH - 1, KS_TILE_BATCH, KS_TILE_BATCH + 1}
    assert {s[0] for s in shapes} == {32, 64}


def test_earlier_shapes_never_reach_the_remainder_loop():
    """why the table exists: at every key-switch shape of tests/test_gpu_tfhe_bootstrap.py the key rows of every group are a
    multiple of four, so `for (; row < rows; ++row)` never ran, and only ki = 1, 2 and 8 did"""
    from test_gpu_tfhe_bootstrap import KS_BASIS, KS_SHAPES
    seen_ki = set()
    for bits in (32, 64):
        for in_dim, out_dim, lb, ell, batch in KS_SHAPES:
            length, _ = tfhe_edge_words.shape(bits, lb, ell)
            seen_ki.add(group_words(length))
            assert all(r % KS_UNROLL == 0 for r in group_rows(in_dim, length)), (bits, in_dim, lb, ell)
            assert in_dim % group_words(length) == 0 or in_dim < group_words(length)      # no short group behind a full one
            assert out_dim + 1 not in (128, 129, 256, 257) and batch not in (31, 32, 33)
    # the handle tests: in_dim = k N, a multiple of 8 at every N >= 8, under KS_BASIS
    lb, ell = KS_BASIS
    seen_ki.add(group_words(ell))
    for in_dim in range(8, 4097, 8):
        assert all(r % KS_UNROLL == 0 for r in group_rows(in_dim, ell)), in_dim
    assert seen_ki == {1, 2, 8}
