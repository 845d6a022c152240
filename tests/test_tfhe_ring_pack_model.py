"""CPU checks of the ring-packing model (tests/tfhe_ring_pack_model.py): (a) with noise-free keys and a basis that drops no
bit, the pack over the exact integer schoolbook has exactly N phi_i at coefficient i N / 2^m and exactly 0 elsewhere, for
log N = 1..4, k = 1 and 2, both widths and counts 1, 2, 3, N - 1 and N, on uniform full-range inputs and keys (an identity
of wrapping words); (b) rule A is S + rule 1(D) for arbitrary key words, and is the doubling-and-cancelling identity on
the phase; (c) a pack whose count is no power of two equals the pack padded with all-zero ciphertexts; (d) the Fourier model
equals the schoolbook in the exact regime; (e) the bound is the full trace's and stays below 2^(BITS-3) at every noisy
shape of the GPU file.  Nothing here imports the library or needs a GPU."""
import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_ring_pack_model as rp
import tfhe_trace_model as tm

FULL = {32: (8, 4), 64: (16, 4)}        # bases that drop no bit: the decomposition is exact modulo 2^BITS


def rand_words(rng, bits, size):
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(m.UINT[bits])


def counts_of(n):
    return sorted({c for c in (1, 2, 3, n - 1, n) if 1 <= c <= n})


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("log_n", [1, 2, 3, 4])
def test_the_pack_puts_n_times_each_phase_at_its_slot_and_clears_the_rest(bits, k, log_n):
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    assert basis.drop_bits == 0
    rng = np.random.default_rng(1000 * bits + 10 * k + log_n)
    n = 1 << log_n
    z = rand_words(rng, bits, k * n).reshape(k, n)                  # the identity needs no small key
    keys = tm.noise_free_gksk(z, z, tm.trace_exponents(log_n), basis, log_n, k, rng)
    product = tm.exact_product(basis, log_n, k)
    for count in counts_of(n):
        lwe = rand_words(rng, bits, 2 * count * (k * n + 1))        # two groups, full-range inputs
        out = rp.pack(lwe, keys, count, product, basis, log_n, k).reshape(2, -1)
        phases = bs.lwe_phase(lwe, bs.flatten_key(z), bits).astype(m.UINT[bits]).reshape(2, count)
        for e in range(2):
            got = bs.glwe_phase(out[e], z, bits, log_n, k).astype(m.UINT[bits])
            assert np.array_equal(got, rp.expected_phase(phases[e], count, bits, log_n)), (count, e)
        slots = [rp.slot(i, count, log_n) for i in range(count)]
        assert slots == [i * (n >> rp.ceil_log2(count)) for i in range(count)] and len(set(slots)) == count


@pytest.mark.parametrize("bits, log_n, k", [(32, 3, 1), (64, 2, 2)])
def test_rule_a_is_an_identity_of_words_for_any_key(bits, log_n, k):
    basis = m.ApproxSignedBasis(bits, 7, 3)                          # drops bits: the identity does not need an exact basis
    rng = np.random.default_rng(bits + log_n)
    n, glwe = 1 << log_n, (k + 1) << log_n
    product = tm.exact_product(basis, log_n, k)
    even, odd = rand_words(rng, bits, 2 * glwe), rand_words(rng, bits, 2 * glwe)
    key = rand_words(rng, bits, tm.key_len(basis, log_n, k))
    for level in range(1, log_n + 1):
        s, t = n >> level, (1 << level) + 1
        shifted = rp.mul_monomial(odd, s, bits, log_n, k)
        for e in range(2):                                           # X^s by hand on one polynomial
            p = odd.reshape(2, k + 1, n)[e, 0]
            want = np.concatenate([(0 - p[n - s:]).astype(m.UINT[bits]), p[:n - s]])
            assert np.array_equal(shifted.reshape(2, k + 1, n)[e, 0], want)
        with np.errstate(over="ignore"):
            d, sm = even - shifted, even + shifted
            want = sm + tm.automorphism(d, key, t, product, basis, log_n, k)
        got = rp.merge(even, odd, key, level, product, basis, log_n, k)
        assert np.array_equal(got, want), level
        dd, ss = rp.merge_parts(even, odd, level, bits, log_n, k)
        assert np.array_equal(dd, d) and np.array_equal(ss, sm)


def test_rule_a_doubles_what_sigma_fixes_and_cancels_what_it_negates():
    bits, log_n, k = 64, 3, 1
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(17)
    n = 1 << log_n
    z = rand_words(rng, bits, k * n).reshape(k, n)
    product = tm.exact_product(basis, log_n, k)
    even, odd = rand_words(rng, bits, (k + 1) * n), rand_words(rng, bits, (k + 1) * n)
    pe, po = (bs.glwe_phase(x, z, bits, log_n, k).astype(np.uint64) for x in (even, odd))
    for level in range(1, log_n + 1):
        s, t = n >> level, (1 << level) + 1
        key = tm.noise_free_gksk(z, z, [t], basis, log_n, k, rng)
        got = bs.glwe_phase(rp.merge(even, odd, key, level, product, basis, log_n, k), z, bits, log_n, k).astype(np.uint64)
        with np.errstate(over="ignore"):
            for j in range(0, n, 2 * s):
                assert got[j] == 2 * pe[j] and got[j + s] == 2 * po[j], (level, j)


@pytest.mark.parametrize("bits, log_n, k, count", [(32, 3, 1, 3), (64, 3, 2, 5), (32, 4, 1, 9)])
def test_a_count_that_is_no_power_of_two_is_the_pack_padded_with_zero_ciphertexts(bits, log_n, k, count):
    basis = m.ApproxSignedBasis(bits, 6, 4)
    rng = np.random.default_rng(count)
    n = 1 << log_n
    product = tm.exact_product(basis, log_n, k)
    keys = rand_words(rng, bits, log_n * tm.key_len(basis, log_n, k))
    lwe = rand_words(rng, bits, count * (k * n + 1))
    full = 1 << rp.ceil_log2(count)
    padded = np.concatenate([lwe, np.zeros((full - count) * (k * n + 1), m.UINT[bits])])
    assert np.array_equal(rp.pack(lwe, keys, count, product, basis, log_n, k),
                          rp.pack(padded, keys, full, product, basis, log_n, k))


def test_the_pack_is_its_levels_and_the_trailing_trace():
    bits, log_n, k, count = 32, 3, 1, 3
    basis = m.ApproxSignedBasis(bits, 7, 3)
    rng = np.random.default_rng(8)
    n = 1 << log_n
    product = tm.exact_product(basis, log_n, k)
    keys = rand_words(rng, bits, log_n * tm.key_len(basis, log_n, k)).reshape(log_n, -1)
    lwe = rand_words(rng, bits, count * (k * n + 1))
    levels = dict(rp.pack_levels(lwe, keys, count, product, basis, log_n, k))
    leaves = tm.embed(lwe, bits, log_n, k).reshape(count, -1)
    zero = np.zeros_like(leaves[0])
    a = rp.merge(leaves[0], leaves[2], keys[log_n - 1], 1, product, basis, log_n, k)     # leaves 0 and 2, t = 3
    b = rp.merge(leaves[1], zero, keys[log_n - 1], 1, product, basis, log_n, k)          # leaf 1 and the absent leaf 3
    assert np.array_equal(levels[1].reshape(-1), np.concatenate([a, b]))
    root = rp.merge(a, b, keys[log_n - 2], 2, product, basis, log_n, k)                  # t = 5
    assert np.array_equal(levels[2].reshape(-1), root)
    want = tm.trace(root, keys[:1].reshape(-1), 1, product, basis, log_n, k)             # the one trailing step, t = N + 1
    assert np.array_equal(levels["out"], want)
    assert np.array_equal(rp.pack(lwe, keys, count, product, basis, log_n, k), want)


def test_fourier_model_equals_the_schoolbook_in_the_exact_regime():
    """u32, keys of small words: digits times key words summed over k ell N terms stay far below 2^53"""
    bits, log_n, k = 32, 3, 1
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(3)
    n = 1 << log_n
    keys = rng.integers(-4, 5, log_n * tm.key_len(basis, log_n, k)).astype(np.int64).view(np.uint64).astype(m.UINT[bits])
    fkeys = tm.to_fourier(keys, bits, log_n)
    for count in (1, 3, n):
        lwe = rand_words(rng, bits, 2 * count * (k * n + 1))
        exact = rp.pack(lwe, keys, count, tm.exact_product(basis, log_n, k), basis, log_n, k)
        model = rp.pack(lwe, fkeys, count, tm.fourier_product(basis, log_n, k), basis, log_n, k)
        assert np.array_equal(model, exact), count


@pytest.mark.parametrize("shape", tm.NOISY_SHAPES, ids=lambda c: "u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]))
def test_the_bound_is_the_full_traces_and_stays_below_half_a_step(shape):
    bits, log_n, k, lb, ell, noise = shape
    bound = rp.ring_pack_bound(noise, *shape)
    print("u%d log_n %d k %d: ring pack bound 2^%.2f, Delta_out/2 2^%d" % (bits, log_n, k, np.log2(bound), bits - 3))
    assert bound == tm.trace_bound(log_n, noise, *shape) == 2.0 ** log_n * noise + (2.0 ** log_n - 1) * tm.ks_bound(*shape)
    assert bound < 2.0 ** (bits - 3)                                # Delta_out = N Delta_in = 2^(BITS-2)
