"""CPU checks of the trace model (tests/tfhe_trace_model.py): (a) sigma_t against the direct evaluation of p(X^t) for every odd
t, its inverse and its multiplicativity; (b) with noise-free keys and a basis that drops no bit, the trace over the exact
integer schoolbook returns exactly 2^m phi at the multiples of 2^m and exactly 0 elsewhere, for m = 1..log N, log N = 1..4,
k = 1 and 2, both widths, on uniform full-range inputs (an identity of wrapping words); (c) the trace is its m calls of
rule 1, rule 1 is the padded-key product; (d) the embedding and its round trip, and embed + full trace; (e) the derived
bound stays below Delta_out / 2 at every noisy shape of the GPU file.  Nothing here imports the library or needs a GPU."""
import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_trace_model as tm

FULL = {32: (8, 4), 64: (16, 4)}        # bases that drop no bit: the decomposition is exact modulo 2^BITS


def rand_words(rng, bits, size):
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(m.UINT[bits])


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [2, 8, 16])
def test_sigma_is_the_evaluation_at_x_to_the_t(bits, n):
    rng = np.random.default_rng(n + bits)
    p, q = rand_words(rng, bits, n), rand_words(rng, bits, n)
    for t in range(1, 2 * n, 2):
        s = tm.sigma(p, t, bits)
        assert np.array_equal(s, tm.sigma_direct(p, t, bits)), t
        assert np.array_equal(tm.sigma(s, pow(t, -1, 2 * n), bits), p), t
        prod = m.negacyclic_u64(p, q).astype(m.UINT[bits])
        want = m.negacyclic_u64(tm.sigma(p, t, bits), tm.sigma(q, t, bits)).astype(m.UINT[bits])
        assert np.array_equal(tm.sigma(prod, t, bits), want), t
    assert np.array_equal(tm.sigma(p, 1, bits), p)


def expected_trace_phase(phi, steps, bits):
    want = np.zeros_like(phi)
    stride = 1 << steps
    with np.errstate(over="ignore"):
        want[::stride] = (phi[::stride].astype(np.uint64) << np.uint64(steps)).astype(m.UINT[bits])
    return want


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("log_n", [1, 2, 3, 4])
def test_the_trace_keeps_the_multiples_of_2_to_the_m_and_clears_the_rest(bits, k, log_n):
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    assert basis.drop_bits == 0
    rng = np.random.default_rng(100 * bits + 10 * k + log_n)
    n, glwe = 1 << log_n, (k + 1) << log_n
    z = rand_words(rng, bits, k * n).reshape(k, n)                 # the identity needs no small key
    ct = rand_words(rng, bits, 2 * glwe)                            # full-range inputs
    product = tm.exact_product(basis, log_n, k)
    for steps in range(1, log_n + 1):
        keys = tm.noise_free_gksk(z, z, tm.trace_exponents(log_n, steps), basis, log_n, k, rng)
        out = tm.trace(ct, keys, steps, product, basis, log_n, k).reshape(2, glwe)
        for e in range(2):
            phi = bs.glwe_phase(ct.reshape(2, glwe)[e], z, bits, log_n, k).astype(m.UINT[bits])
            got = bs.glwe_phase(out[e], z, bits, log_n, k).astype(m.UINT[bits])
            assert np.array_equal(got, expected_trace_phase(phi, steps, bits)), (steps, e)


def test_a_key_switch_changes_the_key_and_keeps_the_phase():
    bits, log_n, k = 64, 3, 2
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(9)
    n = 1 << log_n
    z_in, z_out = rand_words(rng, bits, k * n).reshape(k, n), rand_words(rng, bits, k * n).reshape(k, n)
    ct = rand_words(rng, bits, (k + 1) * n)
    for t in (1, 3, n + 1, 2 * n - 1):
        key = tm.noise_free_gksk(z_in, z_out, [t], basis, log_n, k, rng)
        out = tm.automorphism(ct, key, t, tm.exact_product(basis, log_n, k), basis, log_n, k)
        want = tm.sigma(bs.glwe_phase(ct, z_in, bits, log_n, k), t, bits)
        assert np.array_equal(bs.glwe_phase(out, z_out, bits, log_n, k).astype(m.UINT[bits]), want), t


def test_the_trace_is_its_calls_of_rule_1_and_rule_1_is_the_padded_product():
    bits, log_n, k, steps = 32, 3, 1, 2
    basis = m.ApproxSignedBasis(bits, 7, 3)
    rng = np.random.default_rng(5)
    n, glwe = 1 << log_n, (k + 1) << log_n
    product = tm.exact_product(basis, log_n, k)
    ct = rand_words(rng, bits, 3 * glwe)
    keys = rand_words(rng, bits, steps * tm.key_len(basis, log_n, k))       # the identity is one of words: any key
    levels = list(tm.trace_steps(ct, keys, steps, product, basis, log_n, k))
    assert [lv[1] for lv in levels] == [n + 1, n // 2 + 1] == tm.trace_exponents(log_n, steps)
    acc = ct
    for s, t, before, key, after in levels:
        assert np.array_equal(before, acc) and np.array_equal(key, keys.reshape(steps, -1)[s - 1])
        with np.errstate(over="ignore"):
            acc = acc + tm.automorphism(acc, key, t, product, basis, log_n, k)
        assert np.array_equal(after, acc)
    assert np.array_equal(tm.trace(ct, keys, steps, product, basis, log_n, k), acc)
    # rule 1 by hand: sigma_t of every polynomial, the product against the padded key, the subtraction
    t, key = 3, keys.reshape(steps, -1)[0]
    one = ct[:glwe]
    s = tm.sigma(one.reshape(k + 1, n), t, bits)
    full = tm.pad_key(key, basis, log_n, k)
    assert full.size == (k + 1) * basis.decompose_length * glwe and not full[key.size:].any()
    body = np.concatenate([np.zeros(k * n, m.UINT[bits]), s[k]])
    with np.errstate(over="ignore"):
        want = body - m.schoolbook(s.reshape(-1), full, basis, log_n, k)
    assert np.array_equal(tm.automorphism(one, key, t, product, basis, log_n, k), want)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
def test_embedding_round_trip_and_the_lwe_to_glwe_conversion(bits, k):
    log_n = 3
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(bits + k)
    n = 1 << log_n
    z = rand_words(rng, bits, k * n).reshape(k, n)
    lwe = rand_words(rng, bits, 3 * (k * n + 1))
    glwe = tm.embed(lwe, bits, log_n, k)
    assert np.array_equal(bs.sample_extract(glwe, log_n, k, 0).reshape(-1), lwe)
    phases = bs.lwe_phase(lwe, bs.flatten_key(z), bits).astype(m.UINT[bits])
    for e in range(3):
        ph = bs.glwe_phase(glwe.reshape(3, -1)[e], z, bits, log_n, k).astype(m.UINT[bits])
        assert ph[0] == phases[e]
    keys = tm.noise_free_gksk(z, z, tm.trace_exponents(log_n), basis, log_n, k, rng)
    out = tm.trace(glwe, keys, log_n, tm.exact_product(basis, log_n, k), basis, log_n, k).reshape(3, -1)
    for e in range(3):
        ph = bs.glwe_phase(out[e], z, bits, log_n, k).astype(m.UINT[bits])
        assert int(ph[0]) == (int(phases[e]) * n) % (1 << bits) and not ph[1:].any()


def test_fourier_model_equals_the_schoolbook_in_the_exact_regime():
    """u32, a key of small words: digits times key words summed over k ell N terms stay far below 2^53"""
    bits, log_n, k = 32, 3, 1
    basis = m.ApproxSignedBasis(bits, *FULL[bits])
    rng = np.random.default_rng(3)
    ct = rand_words(rng, bits, 2 * ((k + 1) << log_n))
    keys = rng.integers(-4, 5, log_n * tm.key_len(basis, log_n, k)).astype(np.int64).view(np.uint64).astype(m.UINT[bits])
    exact = tm.trace(ct, keys, log_n, tm.exact_product(basis, log_n, k), basis, log_n, k)
    model = tm.trace(ct, tm.to_fourier(keys, bits, log_n), log_n, tm.fourier_product(basis, log_n, k), basis, log_n, k)
    assert np.array_equal(model, exact)


@pytest.mark.parametrize("shape", tm.NOISY_SHAPES, ids=lambda c: "u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]))
def test_noisy_shapes_stay_below_half_a_step(shape):
    bits, log_n, k, lb, ell, noise = shape
    half = 2.0 ** (bits - 3)                                         # Delta_out = N Delta_in = 2^(BITS-2)
    bound = tm.trace_bound(log_n, noise, *shape)
    ks = tm.ks_bound(*shape)
    print("u%d log_n %d k %d: ks bound 2^%.2f, trace bound 2^%.2f, Delta_out/2 2^%d" % (bits, log_n, k, np.log2(ks),
                                                                                      np.log2(bound), bits - 3))
    assert bound < half / 2.0 ** 10                                  # by hand: tens of bits below
    assert bound == 2.0 ** log_n * noise + (2.0 ** log_n - 1) * ks
    for steps in range(1, log_n):
        assert tm.trace_bound(steps, noise, *shape) < bound
