"""CPU checks of the CMUX model (tests/tfhe_cmux_model.py): (a) with noise-free GGSWs of bits and a basis that drops no bit,
the tree over the exact integer schoolbook returns a ciphertext whose phase is the phase of leaf sum_j m_j 2^j, word for
word, for all 2^d selector patterns, d = 1..4, k = 1 and 2, both widths (the identity is one of wrapping words: it holds on
uniform masks and full-range tables); on trivial GGSWs at u32, where the f64 arithmetic is exact, the Fourier model gives
the same words as the schoolbook; (b) rule 1 tiles per_key as stated and the tree is its d calls; (c) the derived bound
stays below Delta / 2 at every noisy shape of the GPU file.  Nothing here imports the library or needs a GPU."""
import itertools

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_cmux_model as xm
import tfhe_fft_model as m

FULL = {32: (8, 4), 64: (16, 4)}        # bases that drop no bit: the decomposition is exact modulo 2^BITS


def rand_words(rng, bits, size):
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(m.UINT[bits])


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_the_tree_returns_the_phase_of_the_selected_leaf(bits, k, depth):
    log_n = 2
    lb, ell = FULL[bits]
    basis = m.ApproxSignedBasis(bits, lb, ell)
    assert basis.drop_bits == 0
    rng = np.random.default_rng(100 * bits + 10 * k + depth)
    z = rand_words(rng, bits, k << log_n).reshape(k, -1)            # the identity needs no small key
    glwe = (k + 1) << log_n
    table = rand_words(rng, bits, glwe << depth)                    # full-range leaves, shared by the batch
    leaf_phase = [bs.glwe_phase(t, z, bits, log_n, k) for t in table.reshape(-1, glwe)]
    patterns = list(itertools.product((0, 1), repeat=depth))
    selectors = xm.bit_ggsws([b for pat in patterns for b in pat], z, basis, log_n, k, rng)
    out = xm.tree(table, selectors, depth, len(patterns), xm.exact_product(basis, log_n, k), bits, log_n, k)
    for e, pat in enumerate(patterns):
        got = bs.glwe_phase(out.reshape(-1, glwe)[e], z, bits, log_n, k)
        assert np.array_equal(got, leaf_phase[xm.leaf_index(pat)]), (pat, xm.leaf_index(pat))


@pytest.mark.parametrize("depth", [1, 3])
def test_fourier_model_equals_the_schoolbook_in_the_exact_regime(depth):
    """u32, trivial GGSWs of bits: a digit times a gadget word is below 2^31 and a spectrum sums (k+1) ell N of them, far
    below 2^53, so the f64 model is exact and the tree's output IS the leaf"""
    bits, log_n, k = 32, 3, 1
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(depth)
    glwe = (k + 1) << log_n
    table = rand_words(rng, bits, 2 * (glwe << depth))              # a table per input
    msgs = [1, 0, 1, 1, 0, 1][:2 * depth]
    torus = xm.bit_ggsws(msgs, None, basis, log_n, k, rng, trivial=True)
    exact = xm.tree(table, torus, depth, 2, xm.exact_product(basis, log_n, k), bits, log_n, k)
    model = xm.tree(table, xm.to_fourier(torus, bits, log_n), depth, 2, xm.fourier_product(basis, log_n, k), bits, log_n, k)
    assert np.array_equal(model, exact)
    for e in range(2):
        leaf = xm.leaf_index(msgs[e * depth:(e + 1) * depth])
        assert np.array_equal(exact.reshape(2, glwe)[e], table.reshape(2, -1, glwe)[e, leaf])


def test_rule_1_takes_key_i_over_per_key_and_the_tree_is_its_d_calls():
    bits, log_n, k, depth, batch = 64, 2, 1, 3, 2
    basis = m.ApproxSignedBasis(bits, 16, 3)
    rng = np.random.default_rng(5)
    glwe, key_len = (k + 1) << log_n, (k + 1) * 3 * ((k + 1) << log_n)
    product = xm.exact_product(basis, log_n, k)
    d0, d1 = rand_words(rng, bits, 6 * glwe), rand_words(rng, bits, 6 * glwe)
    keys = rand_words(rng, bits, 2 * key_len)
    out = xm.cmux(d0, d1, keys, 3, product, bits, log_n, k).reshape(6, glwe)
    for i in range(6):
        one = xm.cmux(d0.reshape(6, -1)[i], d1.reshape(6, -1)[i], keys.reshape(2, -1)[i // 3], 1, product, bits, log_n, k)
        assert np.array_equal(out[i], one)
    table = rand_words(rng, bits, batch * (glwe << depth))
    sel = rand_words(rng, bits, batch * depth * key_len)
    levels = list(xm.tree_levels(table, sel, depth, batch, product, bits, log_n, k))
    assert [lv[4] for lv in levels] == [4, 2, 1] and [lv[5].size // glwe for lv in levels] == [8, 4, 2]
    for j, d0_j, d1_j, keys_j, per_key, out_j in levels:
        assert np.array_equal(keys_j.reshape(batch, -1), sel.reshape(batch, depth, -1)[:, j])     # a key stride of d
        assert np.array_equal(xm.cmux(d0_j, d1_j, keys_j, per_key, product, bits, log_n, k), out_j)
    # a shared table is the table of every input
    shared = xm.tree(table[:glwe << depth], sel, depth, batch, product, bits, log_n, k)
    tiled = xm.tree(np.tile(table[:glwe << depth], batch), sel, depth, batch, product, bits, log_n, k)
    assert np.array_equal(shared, tiled)


@pytest.mark.parametrize("case, depth", xm.NOISY_TREES, ids=lambda c: str(c) if isinstance(c, int) else "u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]))
def test_noisy_shapes_stay_below_half_a_step(case, depth):
    bits, p = case[0], case[11]
    half = 2.0 ** (bits - p - 2)
    bound = xm.noisy_tree_bound(case, depth)
    print("u%d log_n %d k %d depth %d: tree bound 2^%.2f, Delta/2 2^%d" % (bits, case[1], case[2], depth, np.log2(bound),
                                                                         bits - p - 2))
    assert bound < half
    assert xm.noisy_tree_bound(case, depth) == depth * xm.noisy_tree_bound(case, 1)


def test_the_depths_the_shapes_leave_room_for():
    """u32: one level is 2^26.87, so depth 4 still fits and 6 does not; the circuit bootstrap's own u32 shape does not fit
    depth 2; the two u64 shapes fit depth 8 and 11"""
    u32, a, b = (c for c, _ in xm.NOISY_TREES)
    assert abs(np.log2(xm.noisy_tree_bound(u32, 1)) - 26.87) < 0.01 and abs(np.log2(xm.noisy_tree_bound(u32, 3)) - 28.45) < 0.01
    assert xm.noisy_tree_bound(u32, 4) < 2.0 ** 29 < xm.noisy_tree_bound(u32, 6)
    assert xm.noisy_tree_bound(cm.NOISY_CASES[0], 2) > 2.0 ** 29
    assert xm.noisy_tree_bound(a, 8) < 2.0 ** 61 < xm.noisy_tree_bound(a, 9)
    assert xm.noisy_tree_bound(b, 11) < 2.0 ** 61 < xm.noisy_tree_bound(b, 12)
