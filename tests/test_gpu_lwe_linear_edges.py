"""The linear layer with clear weights at the launch edges tests/test_gpu_lwe_linear.py does not reach, every
word against the integer model (tests/lwe_linear_model.py): more output tiles than one grid dimension holds, so that the
second launch of launch_y_slices runs with a first tile other than 0, in both kernels; the word kernel's remainder of 2 behind
its unroll of 4; the int8 kernel at the ends of a lane's 16-input quarter, of a 64-column tile and of the 32-output tile and
its halves; and the fold of the plane sums with two 16-output halves per workgroup, on weights and words that differ by
output.  The output buffer of run_dev starts at -3, so a tile that is never written is seen."""
import numpy as np
import pytest

import lwe_linear_model as lm
import tfhe_fft_model as m
from test_gpu_lwe_linear import byte_pattern_words, edge_mixed, run_dev, sign_extended
from test_gpu_tfhe_fft import rand_words

pytestmark = pytest.mark.gpu

GRID_Y = 65535                       # launch_y_slices: the output tiles of one launch
MIN_GROUPS = 512                     # pfhe_linear.hip: kLinMinGroups
UNROLL, GROUP = 4, 64                # the word kernel: rows in flight, inputs per staged group (kKsUnroll, kKsMaxRows)


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def outputs_per_thread(row, out_f, batch):
    """linear_rows_per_thread of pfhe_linear.hip, restated: the largest R in 8, 4, 2 whose tile of 4 R outputs is more than
    half used and whose grid (output tiles x batch x column tiles of 128) has 512 workgroups; else 1"""
    groups = batch * ((row + 127) // 128)
    for r in (8, 4, 2):
        tile = 4 * r
        if out_f > tile // 2 and (out_f + tile - 1) // tile * groups >= MIN_GROUPS:
            return r
    return 1


@pytest.mark.parametrize("bits", [32, 64])
def test_more_output_tiles_than_one_launch_holds(p, bits):
    """out_features = 65535 * 32 + 33: 65 537 tiles of 32 outputs in both kernels, so two launches, the second with first
    tile 65535 and two tiles, the last one of a single output; the weights differ by output, so a tile computed from
    another tile's weights or written to another tile's place gives other words"""
    out_f, in_f, row, batch = GRID_Y * 32 + 33, 3, 2, 1
    assert outputs_per_thread(row, out_f, batch) == 8                       # the word kernel's tile: 4 * 8 outputs
    assert out_f > 16                                                       # the int8 kernel's: MT = 2, 32 outputs
    tiles = (out_f + 31) // 32
    assert tiles == GRID_Y + 2 and out_f - (tiles - 1) * 32 == 1
    rng = np.random.default_rng(1000 + bits)
    x = edge_mixed(rng, bits, batch * in_f * row)
    bias = rand_words(rng, bits, out_f)
    for w in (rand_words(rng, bits, out_f * in_f), rng.integers(-128, 128, out_f * in_f).astype(np.int8)):
        want = lm.linear(x, w, bias, row - 1, in_f, out_f, bits)
        got, after = run_dev(p, x, w, bias, row, in_f, out_f, bits)
        assert np.array_equal(got[-34 * row:], want[-34 * row:]), w.dtype        # the second launch, named first
        assert np.array_equal(got, want), w.dtype
        assert np.array_equal(after, x)


@pytest.mark.parametrize("bits", [32, 64])
def test_word_form_at_a_remainder_of_two_behind_the_unroll(p, bits):
    """in_features in {2, 6, 66, 130}: two rows left behind the unroll of 4, alone, after one unrolled step, and after one
    and two whole groups of 64 inputs; row 2 and 129, out_features 1 and 33"""
    rng = np.random.default_rng(1100 + bits)
    for in_f in (2, 6, 66, 130):
        assert in_f % GROUP % UNROLL == 2
        for row in (2, 129):
            for out_f in (1, 33):
                batch = 2
                x = edge_mixed(rng, bits, batch * in_f * row)
                w = edge_mixed(rng, bits, out_f * in_f)
                for bias in (edge_mixed(rng, bits, out_f), None):
                    got, after = run_dev(p, x, w, bias, row, in_f, out_f, bits)
                    assert np.array_equal(got, lm.linear(x, w, bias, row - 1, in_f, out_f, bits)), (in_f, row, out_f)
                    assert np.array_equal(after, x)


# (out_features, in_features, row, batch)
I8_EDGE_CASES = [(31, 2, 63, 1), (32, 15, 64, 3), (47, 16, 65, 1), (48, 17, 128, 1), (49, 31, 63, 3), (64, 33, 64, 1),
                 (65, 47, 65, 1), (31, 48, 128, 3), (32, 49, 63, 1), (48, 127, 64, 1), (65, 128, 65, 3)]


@pytest.mark.parametrize("bits", [32, 64])
def test_i8_form_at_the_ends_of_its_quarters_and_tiles(p, bits):
    """in_features around the ends of a lane's quarter of 16 inputs (where the row index is clamped to in_features - 1) and
    of a step of 64; row around the 64-column tile and at two whole tiles; out_features around the 32-output tile of MT = 2
    and around its second half of 16; against the model and against the word form on the sign-extended weights"""
    rng = np.random.default_rng(1200 + bits)
    assert {c[1] for c in I8_EDGE_CASES} == {2, 15, 16, 17, 31, 33, 47, 48, 49, 127, 128}
    assert {c[2] for c in I8_EDGE_CASES} == {63, 64, 65, 128}
    assert {c[0] for c in I8_EDGE_CASES} == {31, 32, 47, 48, 49, 64, 65} and min(c[0] for c in I8_EDGE_CASES) > 16
    for out_f, in_f, row, batch in I8_EDGE_CASES:
        x = byte_pattern_words(rng, bits, batch * in_f * row)
        w8 = rng.integers(-128, 128, out_f * in_f).astype(np.int8)
        at = rng.permutation(w8.size)[:max(1, w8.size // 2)]
        w8[at] = rng.choice(np.array([-128, -1, 0, 1, 127], np.int8), at.size)
        for bias in (edge_mixed(rng, bits, out_f), None):
            want = lm.linear(x, w8, bias, row - 1, in_f, out_f, bits)
            got, after = run_dev(p, x, w8, bias, row, in_f, out_f, bits)
            word, _ = run_dev(p, x, sign_extended(w8, bits), bias, row, in_f, out_f, bits)
            assert np.array_equal(got, want), (out_f, in_f, row, batch, bias is not None)
            assert np.array_equal(got, word), (out_f, in_f, row, batch, bias is not None)
            assert np.array_equal(after, x)


@pytest.mark.parametrize("bits", [32, 64])
def test_i8_plane_sums_are_folded_in_both_halves_of_a_tile(p, bits):
    """out_features = 33 runs MT = 2: two 16-output halves per workgroup, each with plane sums of its own, and a second
    tile.  Rows 0, 16 and 32 of the weights are all -128 (the first row of either half and of the second tile), the others
    random, so the outputs differ.  in_features 2^16: the fold every 1024 steps lands on the last step and the final fold
    sees cleared planes; 2^16 + 1: one step behind it; 2^17 + 2^11: two folds, and for the -128 rows the unfolded plane sum
    passes 2^31 against words all 0 (the kernel is fed x_b - 128: products of 2^14) and passes -2^31 against words all ones
    (products of -16 256), which is asserted below.  As in test_gpu_lwe_linear.py, a plane sum that wrapped modulo 2^32
    changes no u32 word: the u64 run is the one that tells a wrap, either run an accumulator that saturates or a plane that
    is added twice."""
    rng = np.random.default_rng(1300 + bits)
    out_f, row = 33, 2
    assert out_f > 16                                                             # MT = 2
    top = (1 << bits) - 1
    for in_f, passes in ((1 << 16, False), ((1 << 16) + 1, False), ((1 << 17) + (1 << 11), True)):
        w8 = rng.integers(-128, 128, (out_f, in_f)).astype(np.int8)
        w8[[0, 16, 32]] = -128
        for fill in (0, top, None):
            if fill is None:
                x = byte_pattern_words(rng, bits, in_f * row)
            else:
                x = np.full(in_f * row, fill, np.uint64).astype(m.UINT[bits])
                assert (abs(((fill & 0xff) - 128) * -128 * in_f) > 2 ** 31) == passes        # the unfolded plane sum
            got, _ = run_dev(p, x, w8.reshape(-1), None, row, in_f, out_f, bits)
            want = lm.linear(x, w8.reshape(-1), None, row - 1, in_f, out_f, bits)
            if fill == 0:
                assert not want.any()
            assert np.array_equal(got.reshape(out_f, row)[[0, 16, 32]], want.reshape(out_f, row)[[0, 16, 32]]), (in_f, fill)
            assert np.array_equal(got, want), (in_f, fill)
