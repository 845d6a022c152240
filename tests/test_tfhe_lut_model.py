"""CPU checks of the look-up model (tests/tfhe_lut_model.py): (a) with noise-free GGSWs of bits, uniform masks, a basis that
drops no bit and the exact integer schoolbook, the rotation by bits returns X^{-x 2^s} inp word for word in the phase for all
2^r patterns, and the table evaluation returns entry x of every output for all 2^p patterns, on tfhe_lut_table's layout, a
2-word entry included; (b) rule 2 equals its composition: the tree as t calls of the CMUX model, rule 1, extraction; (c) the
derived bound stays below Delta / 2 at every noisy shape of the GPU file.  Nothing here imports the library or needs a GPU."""
import itertools

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cmux_model as xm
import tfhe_fft_model as m
import tfhe_lut_model as lm

FULL = {32: (8, 4), 64: (16, 4)}        # bases that drop no bit: the decomposition is exact modulo 2^BITS


def rand_words(rng, bits, size):
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(m.UINT[bits])


def selectors_of(patterns, z, basis, log_n, k, rng):
    return xm.bit_ggsws([b for pat in patterns for b in pat], z, basis, log_n, k, rng)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_the_rotation_returns_the_input_times_the_inverse_monomial(bits, r, s):
    log_n, k, o = 4, 1, 2
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    assert basis.drop_bits == 0
    rng = np.random.default_rng(1000 * bits + 10 * r + s)
    z = rand_words(rng, bits, k << log_n).reshape(k, -1)            # the identity needs no small key
    glwe = (k + 1) << log_n
    patterns = list(itertools.product((0, 1), repeat=r))
    inp = rand_words(rng, bits, len(patterns) * o * glwe)           # full-range words, uniform masks
    keys = selectors_of(patterns, z, basis, log_n, k, rng)
    out = lm.rotate_by_bits(inp, keys, r, s, o, r, 0, xm.exact_product(basis, log_n, k), bits, log_n, k).reshape(-1, glwe)
    for a, row in enumerate(inp.reshape(-1, glwe)):
        x = xm.leaf_index(patterns[a // o])
        want = lm.mul_monomial(bs.glwe_phase(row, z, bits, log_n, k), (2 << log_n) - (x << s), log_n)
        assert np.array_equal(bs.glwe_phase(out[a], z, bits, log_n, k), want), (a, x)


def test_the_monomial_model_and_first_key():
    bits, log_n, k = 32, 3, 1
    n = 1 << log_n
    p = np.arange(1, n + 1, dtype=np.uint32)
    assert np.array_equal(lm.mul_monomial(p, 0, log_n), p) and np.array_equal(lm.mul_monomial(p, 2 * n, log_n), p)
    assert np.array_equal(lm.mul_monomial(p, n, log_n), (0 - p).astype(np.uint32))
    assert np.array_equal(lm.mul_monomial(p, 1, log_n), np.concatenate([(0 - p[-1:]).astype(np.uint32), p[:-1]]))
    assert np.array_equal(lm.mul_monomial(lm.mul_monomial(p, 2 * n - 3, log_n), 3, log_n), p)
    assert [lm.exponent(j, 1, log_n) for j in range(2)] == [14, 12] and lm.exponent(0, 0, 1) == 3
    # keys_per_input and first_key pick the step's key of the accumulator's input
    basis = m.ApproxSignedBasis(bits, 8, 3)
    rng = np.random.default_rng(3)
    glwe, key_len = (k + 1) << log_n, (k + 1) * 3 * ((k + 1) << log_n)
    product = xm.exact_product(basis, log_n, k)
    inp, keys = rand_words(rng, bits, 6 * glwe), rand_words(rng, bits, 2 * 5 * key_len)
    out = lm.rotate_by_bits(inp, keys, 2, 0, 3, 5, 2, product, bits, log_n, k)
    own = lm.rotate_by_bits(inp, keys.reshape(2, 5, -1)[:, 2:4].reshape(-1), 2, 0, 3, 2, 0, product, bits, log_n, k)
    assert np.array_equal(out, own)
    for a in range(6):
        one = lm.rotate_by_bits(inp.reshape(6, -1)[a], keys.reshape(2, 5, -1)[a // 3, 2:4], 2, 0, 1, 2, 0, product, bits, log_n, k)
        assert np.array_equal(out.reshape(6, -1)[a], one)
    assert np.array_equal(lm.rotate_by_bits(inp, keys[:0], 0, 0, 3, 0, 0, product, bits, log_n, k), inp)     # r = 0: a copy


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("o", [1, 2])
@pytest.mark.parametrize("t, r", [(0, 2), (2, 0), (1, 2), (2, 2)])
def test_the_table_returns_the_entry_of_every_output(bits, k, o, t, r):
    log_n, p = 3, t + r
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(100 * bits + 10 * k + o + 7 * t + 3 * r)
    z = rand_words(rng, bits, k << log_n).reshape(k, -1)
    values = rand_words(rng, bits, o << p).reshape(o, 1 << p)       # full-range entries
    table = lm.lut_table(values, log_n, k, t, r)
    assert table.shape == (o, 1 << t, k + 1, 1 << log_n) and np.count_nonzero(table) <= o << p
    patterns = list(itertools.product((0, 1), repeat=p))
    sel = selectors_of(patterns, z, basis, log_n, k, rng)
    out = lm.lut_eval(table, sel, t, r, 0, o, len(patterns), 1, xm.exact_product(basis, log_n, k), bits, log_n, k)
    phases = bs.lwe_phase(out, bs.flatten_key(z), bits).reshape(len(patterns), o)
    for e, pat in enumerate(patterns):
        assert np.array_equal(phases[e], values[:, xm.leaf_index(pat)]), pat


@pytest.mark.parametrize("bits", [32, 64])
def test_a_two_word_entry_comes_out_at_the_first_two_indices(bits):
    log_n, k, t, r, s, o = 3, 1, 1, 2, 1, 2
    p = t + r
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(bits)
    z = rand_words(rng, bits, k << log_n).reshape(k, -1)
    values = rand_words(rng, bits, (o << p) * 2).reshape(o, 1 << p, 2)
    table = lm.lut_table(values, log_n, k, t, r, s)
    patterns = list(itertools.product((0, 1), repeat=p))
    sel = selectors_of(patterns, z, basis, log_n, k, rng)
    out = lm.lut_eval(table, sel, t, r, s, o, len(patterns), 2, xm.exact_product(basis, log_n, k), bits, log_n, k)
    phases = bs.lwe_phase(out, bs.flatten_key(z), bits).reshape(len(patterns), o, 2)
    for e, pat in enumerate(patterns):
        assert np.array_equal(phases[e], values[:, xm.leaf_index(pat)]), pat


@pytest.mark.parametrize("shared", [True, False])
def test_rule_2_is_its_composition(shared):
    bits, log_n, k, t, r, s, o, batch = 64, 3, 1, 2, 2, 1, 2, 2
    p = t + r
    basis = m.ApproxSignedBasis(bits, 16, 3)
    rng = np.random.default_rng(11)
    glwe, key_len = (k + 1) << log_n, (k + 1) * 3 * ((k + 1) << log_n)
    product = xm.exact_product(basis, log_n, k)
    table = rand_words(rng, bits, (1 if shared else batch) * (o << t) * glwe)
    sel = rand_words(rng, bits, batch * p * key_len)
    # the tree as t calls of the CMUX model with per_key = o 2^(t-1-j) and a key stride of p keys
    nodes = (np.tile(table, batch) if shared else table).reshape(-1, 2, glwe)
    for j in range(t):
        keys = sel.reshape(batch, p, -1)[:, r + j]
        nodes = xm.cmux(nodes[:, 0], nodes[:, 1], keys, o << (t - 1 - j), product, bits, log_n, k)
        nodes = nodes.reshape(-1, 2, glwe) if j + 1 < t else nodes
    assert np.array_equal(nodes, lm.tree_stage(table, sel, t, r, o, batch, product, bits, log_n, k))
    # with o = 1 the tree stage is the CMUX tree of each output on the tree's own keys
    one = lm.tree_stage(table.reshape(-1, o, glwe << t)[:, 0], sel, t, r, 1, batch, product, bits, log_n, k)
    tree_keys = sel.reshape(batch, p, -1)[:, r:].reshape(-1)
    assert np.array_equal(one, xm.tree(table.reshape(-1, o, glwe << t)[:, 0], tree_keys, t, batch, product, bits, log_n, k))
    assert np.array_equal(one.reshape(batch, glwe), nodes.reshape(batch, o, glwe)[:, 0])
    # then rule 1 on the selectors' first r keys per input, then extraction row (e o + u) extract + i
    acc = lm.rotate_by_bits(nodes, sel, r, s, o, p, 0, product, bits, log_n, k)
    assert np.array_equal(acc, lm.lut_eval(table, sel, t, r, s, o, batch, 0, product, bits, log_n, k))
    got = lm.lut_eval(table, sel, t, r, s, o, batch, 2, product, bits, log_n, k).reshape(batch * o, 2, -1)
    for i in range(2):
        assert np.array_equal(got[:, i].reshape(-1), bs.sample_extract(acc, log_n, k, i))
    # every step of rule 1 is the monomial multiplication, then the CMUX with per_key = o
    for j, a, rot, keys, out in lm.rotation_steps(nodes, sel, r, s, o, p, 0, product, bits, log_n, k):
        assert np.array_equal(rot, lm.mul_monomial(a, (2 << log_n) - (1 << (j + s)), log_n))
        assert np.array_equal(keys.reshape(batch, -1), sel.reshape(batch, p, -1)[:, j])
        assert np.array_equal(out, xm.cmux(a, rot, keys, o, product, bits, log_n, k))


@pytest.mark.parametrize("case, t, r", lm.NOISY_LUTS, ids=lambda c: str(c) if isinstance(c, int) else "u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]))
def test_noisy_shapes_stay_below_half_a_step(case, t, r):
    bits, log_n, p = case[0], case[1], case[11]
    assert r <= log_n
    half = 2.0 ** (bits - p - 2)
    bound = lm.noisy_lut_bound(case, t, r)
    print("u%d log_n %d k %d (t, r) = (%d, %d): look-up bound 2^%.2f, Delta/2 2^%d" % (bits, log_n, case[2], t, r, np.log2(bound),
                                                                                     bits - p - 2))
    assert bound < half
    assert bound == (t + r) * xm.noisy_tree_bound(case, 1)
