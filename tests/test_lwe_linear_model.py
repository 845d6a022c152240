"""The model of the linear layer (tests/lwe_linear_model.py) on the CPU: one 2 x 2 case written out by hand, the int8 weights
as the sign-extended words, chains of add_mul_scalar_assign, the noise bound, and the condition under which the two-layer
network of the GPU test decodes, derived and asserted for both of its shapes."""
import numpy as np
import pytest

import lwe_linear_model as lm
import tfhe_fft_model as m
import tfhe_keygen_model as kg


@pytest.mark.parametrize("bits", [32, 64])
def test_two_by_two_by_hand(bits):
    """dimension 1 (rows of two words), in = out = 2, one vector:
         W = [[3, -1], [2^(BITS-1), 1]],  in = [(5, 7), (2^BITS - 1, 2)],  bias = (10, 2^BITS - 1)
       out[0] = 3 (5, 7) - (2^BITS - 1, 2) + (0, 10) = (15 + 1, 21 - 2 + 10) = (16, 29)
       out[1] = 2^(BITS-1) (5, 7) + (2^BITS - 1, 2) + (0, -1) = (2^(BITS-1) - 1, 2^(BITS-1) + 2 - 1)   (5 and 7 are odd)"""
    top, half = (1 << bits) - 1, 1 << (bits - 1)
    word = lambda *v: np.array(v, dtype=np.uint64).astype(m.UINT[bits])
    out = lm.linear(word(5, 7, top, 2), word(3, top, half, 1), word(10, top), 1, 2, 2, bits)
    assert out.dtype == m.UINT[bits]
    assert [int(v) for v in out] == [16, 29, half - 1, half + 1]
    assert [int(v) for v in lm.linear(word(5, 7, top, 2), word(3, top, half, 1), None, 1, 2, 2, bits)] == \
        [16, 19, half - 1, half + 2]


@pytest.mark.parametrize("bits", [32, 64])
def test_int8_weights_are_the_sign_extended_words_and_the_rule_is_a_chain(bits):
    rng = np.random.default_rng(bits)
    dim, in_f, out_f, batch = 6, 5, 4, 3
    x = rng.integers(0, 2 ** bits, batch * in_f * (dim + 1), dtype=np.uint64).astype(m.UINT[bits])
    w8 = rng.integers(-128, 128, out_f * in_f).astype(np.int8)
    w8[:3] = (-128, -1, 127)
    bias = rng.integers(0, 2 ** bits, out_f, dtype=np.uint64).astype(m.UINT[bits])
    words = w8.astype(np.int64).view(np.uint64).astype(m.UINT[bits])
    got = lm.linear(x, w8, bias, dim, in_f, out_f, bits)
    assert np.array_equal(got, lm.linear(x, words, bias, dim, in_f, out_f, bits))
    # Lwe::add_mul_scalar_assign, one input after the other, in Python integers
    xs, mask = x.reshape(batch, in_f, dim + 1), (1 << bits) - 1
    for e in range(batch):
        for o in range(out_f):
            acc = [0] * dim + [int(bias[o])]
            for i in range(in_f):
                acc = [(a + int(words[o * in_f + i]) * int(v)) & mask for a, v in zip(acc, xs[e, i])]
            assert [int(v) for v in got.reshape(batch, out_f, dim + 1)[e, o]] == acc


def test_linear_bound_is_the_largest_absolute_row_sum():
    assert lm.linear_bound(np.array([[1, -2, 3], [-4, 0, 1]], np.int8), 10.0) == 60.0
    assert lm.linear_bound(np.array([[1, 2 ** 32 - 2]], np.uint64).astype(np.uint32), 1.0) == 3.0     # -2 as a word
    assert lm.linear_bound(np.array([[-128] * 4], np.int8), 0.5) == 256.0


def test_the_clear_network_stays_inside_two_message_bits():
    seen = set()
    for v in range(8):
        s, h, t, y = lm.clear_network([(v >> j) & 1 for j in range(3)])
        assert all(0 <= a < 4 for a in s) and 0 <= t < 4 and 0 <= y < 4
        seen.add((tuple(h), y))
    assert (lm.W1 < 0).any() and len(seen) > 2                         # a negative weight, and not a constant network


@pytest.mark.parametrize("case", lm.DENSE_CASES, ids=lambda c: "u%d" % c[0])
def test_dense_layer_shapes_lie_inside_the_margin(case):
    """For every layer: linear_bound(W, E) 2N / 2^BITS + (n+1)/2 < N / 2^(p+1), E the worst noise of a layer's inputs (a
    bootstrap's output, tfhe_keygen_model.noise_bound, or the fresh noise if that is larger).  The sum's phase is off its
    message by at most linear_bound; the modulus switch scales that to exponents and adds at most half an exponent per
    rounded word; the half-box shift of the test vector leaves half a box, N / 2^(p+1) exponents, either way.  The
    bootstrap's own output must decode too: noise_bound < Delta / 2."""
    bits, log_n, k, n, lb, ell, g, p, noise = case
    assert p == lm.NET_P and g == 0
    bound = kg.noise_bound(bits, log_n, k, n, lb, ell, g, *kg.KS_BASIS, noise)
    assert bound < 2.0 ** (bits - p - 2)
    for weights in (lm.W1, lm.W2):
        assert lm.linear_bound(weights, 1.0) == 3.0
        left, right = lm.dense_margin(case, weights)
        print("u%d: noise bound 2^%.1f, times 3 = 2^%.1f against %.1f exponents = 2^%.1f; %.2f < %g"
              % (bits, np.log2(bound), np.log2(3 * bound), right - (n + 1) / 2,
                 np.log2((right - (n + 1) / 2) * 2.0 ** bits / (2 << log_n)), left, right))
        assert left < right
    if bits == 32:      # the figures of the derivation: about 2^23.7, against 3.5 exponents = 2^26.8
        assert 23.0 < np.log2(bound) < 24.5 and abs(np.log2(3.5 * 2.0 ** 32 / 128) - 26.8) < 0.05
