"""The numpy model of the multi-bit blind rotation (tests/tfhe_multibit_model.py) against what it has to mean: M(r) is the
transform of the monomial, indicator keys rotate a message by X^{sum a_i s_i}, the combined key of g = 1 is
K_0 + X^a K_1, and on full-torus keys the model's own error against the exact integer step is printed per shape (the
quantity the GPU tests' error rule is relative to)."""
import itertools

import numpy as np
import pytest

import tfhe_blindrot_model as bm
import tfhe_fft_model as m
import tfhe_multibit_model as mbm


@pytest.mark.parametrize("log_n", [1, 2, 6])
def test_monomial_spectrum_is_the_forward_transform_of_the_monomial(log_n):
    n = 1 << log_n
    fft = m.FullComplex64FftTable(log_n)
    worst = 0.0
    for r in range(2 * n):
        want = fft.forward(mbm.monomial(r, log_n, 32), 32)
        got = mbm.monomial_spectrum(r, log_n)
        worst = max(worst, float(np.abs(got - want).max()))
        # Hermitian symmetry in the full layout: M[(1 - k) mod N] = conj(M[k])
        k = np.arange(n)
        assert np.abs(got[(1 - k) % n] - np.conj(got)).max() < 1e-15
    print(f"N {n}: max |M(r) - forward(X^r)| = {worst:.3g}")
    assert worst < 1e-13
    assert np.array_equal(mbm.monomial_spectrum(2 * n + 3, log_n), mbm.monomial_spectrum(3, log_n))


@pytest.mark.parametrize("bits,log_n,lb,ell", [(32, 6, 10, 2), (64, 6, 15, 2)])
@pytest.mark.parametrize("g", [1, 2, 3])
def test_indicator_keys_rotate_the_message_for_every_key_pattern(bits, log_n, lb, ell, g):
    n, k = 1 << log_n, 1
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + g)
    for pattern in itertools.product((0, 1), repeat=2 * g):       # two groups: every pattern of each
        exps = np.array([0, n, 2 * n - 1, n + 1, 5, 2 * n - 3][:2 * g], np.uint32)
        exps[-1] = rng.integers(0, 2 * n)
        bsk = mbm.fourier(mbm.multibit_indicator_bsk(basis, log_n, k, pattern, g), log_n, bits)
        msg = rng.integers(0, 1 << bm.PLAINTEXT_BITS, n)
        acc = bm.encode([msg], bits, log_n, k)
        out = mbm.rotate_loop(acc, bsk, exps, g, basis, log_n, k)
        mask_err, got = bm.decode(out, bits, log_n, k)
        total = sum(int(a) * s for a, s in zip(exps, pattern))
        assert mask_err == 0.0, pattern
        assert got == bm.expected_decode(msg, total, n), (pattern, total)


@pytest.mark.parametrize("bits,log_n", [(32, 5), (64, 7)])
def test_combined_key_of_one_element_is_k0_plus_the_rotated_k1(bits, log_n):
    n = 1 << log_n
    rng = np.random.default_rng(bits)
    k0, k1 = (rng.integers(-1024, 1025, 8 * n).astype(m.UINT[bits]) for _ in range(2))
    for a in (0, 1, n - 1, n, 2 * n - 1, 3 * n + 2):
        got = mbm.combine_key(mbm.fourier([k0, k1], log_n, bits), [a], log_n)
        want = mbm.fourier([bm.add(k0, bm.rotate(k1, a, n))], log_n, bits)
        assert np.abs(got - want).max() < 1e-7, a                 # entries up to N 2^11: f64 keeps them to ~1e-10
        assert np.array_equal(mbm.exact_key([k0, k1], [a], log_n), bm.add(k0, bm.rotate(k1, a, n)))


MODEL_SHAPES = [(32, 6, 1, 7, 3, 2), (32, 8, 1, 7, 3, 3), (32, 10, 1, 10, 2, 4), (64, 6, 1, 15, 2, 2), (64, 10, 1, 15, 2, 2),
                (32, 6, 2, 7, 3, 2)]


@pytest.mark.parametrize("bits,log_n,k,lb,ell,g", MODEL_SHAPES)
def test_model_error_against_the_exact_group_on_full_torus_keys(bits, log_n, k, lb, ell, g):
    """the model's own error: zero where f64 holds every accumulator (u32), a few times the single product's at u64 (the
    combined key is a sum of 2^g full-torus keys).  The bound is the f64 budget of the sum: 2^g keys of N (k+1) ell terms of
    magnitude 2^(BITS-1) 2^(logB-1) each, relative 2^-53 per operation of a log2(N)-deep transform."""
    n = 1 << log_n
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + log_n + g)
    keys = [rng.integers(0, 2 ** bits, (k + 1) * ell * (k + 1) * n, dtype=np.uint64).astype(m.UINT[bits]) for _ in range(1 << g)]
    exps = [int(x) for x in rng.integers(0, 2 * n, g)]
    acc = rng.integers(0, 2 ** bits, (k + 1) * n, dtype=np.uint64).astype(m.UINT[bits])
    model = mbm.step(acc, mbm.fourier(keys, log_n, bits), exps, basis, log_n, k)
    exact = mbm.exact_group(acc, keys, exps, basis, log_n, k)
    err = float(m.centred_error(model, exact, bits).max())
    single, _ = m.external_product(acc, mbm.fourier(keys[:1], log_n, bits), basis, log_n, k)
    single_err = float(m.centred_error(single, m.schoolbook(acc, keys[0], basis, log_n, k), bits).max())
    print(f"bits {bits} N 2^{log_n} k {k} logB {lb} ell {ell} g {g}: model_err {err:.3g} (single product {single_err:.3g})")
    budget = (1 << g) * n * (k + 1) * ell * 2.0 ** (bits - 1) * 2.0 ** (lb - 1) * 2.0 ** -53 * 4 * log_n
    assert err <= max(1.0, budget)
