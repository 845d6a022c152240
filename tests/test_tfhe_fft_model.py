"""CPU checks of the torus-FFT / TFHE reference model (tests/tfhe_fft_model.py) the GPU parity tests rely on: the
reference's own tests (primus_fft/tests/{roundtrip,negacyclic}.rs, primus_lattice/tests/{tfhe_external_product,
fourier_convert}.rs) recreated against the model, the two half-spectrum identities and the Hermitian-part inverse the kernels
rest on, and the edge values of the torus conversion."""
import numpy as np
import pytest

import tfhe_fft_model as m
from tfhe_edge_words import edge_words

PATTERN = [0, 1, -1, 2, -2]


def pattern(n, bits):
    return np.array([PATTERN[i % 5] for i in range(n)], np.int64).astype(m.UINT[bits])


def naive_negacyclic(a, b, bits):
    return m.negacyclic_u64(a.astype(m.SINT[bits]).astype(np.int64).view(np.uint64),
                            b.astype(m.SINT[bits]).astype(np.int64).view(np.uint64)).astype(m.UINT[bits])


@pytest.mark.parametrize("bits,max_log_n", [(32, 6), (64, 4)])
def test_roundtrip_patterns(bits, max_log_n):
    """roundtrip.rs: small centred values, monomials, zero and one round-trip exactly"""
    for log_n in range(1, max_log_n + 1):
        t = m.FullComplex64FftTable(log_n)
        n = t.n
        cases = [pattern(n, bits), np.zeros(n, m.UINT[bits]), np.eye(1, n, 0, dtype=m.UINT[bits])[0]]
        cases += [np.eye(1, n, pos, dtype=m.UINT[bits])[0] for pos in (0, 1, n // 2, n - 1)]
        for x in cases:
            assert np.array_equal(t.inverse(t.forward(x, bits), bits), x), log_n


def test_negacyclic_products():
    """negacyclic.rs: pointwise products of forward transforms invert to the negacyclic convolution"""
    rng = np.random.default_rng(1)
    for log_n in range(1, 7):
        t = m.FullComplex64FftTable(log_n)
        a = rng.integers(-50, 50, t.n).astype(np.uint32)
        b = rng.integers(-50, 50, t.n).astype(np.uint32)
        got = t.inverse(t.forward(a, 32) * t.forward(b, 32), 32)
        assert np.array_equal(got, naive_negacyclic(a, b, 32))
        mono = np.eye(1, t.n, t.n - 1, dtype=np.uint32)[0]  # X^{N-1} * a = rotation with one sign flip
        assert np.array_equal(t.inverse(t.forward(a, 32) * t.forward(mono, 32), 32), naive_negacyclic(a, mono, 32))


@pytest.mark.parametrize("bits", [32, 64])
def test_half_spectrum_identities(bits):
    rng = np.random.default_rng(bits)
    for log_n in range(1, 11):
        t = m.FullComplex64FftTable(log_n)
        n = t.n
        x = rng.integers(0, 2 ** bits, n, dtype=np.uint64).astype(m.UINT[bits])
        y = t.forward(x, bits)
        k = np.arange(n)
        scale = 1e-13 * n * 2.0 ** (bits - 1)
        assert np.max(np.abs(y[(1 - k) % n] - np.conj(y))) <= scale
        assert np.max(np.abs(y[0::2] - m.folded_forward(x, bits))) <= scale
        # the reference's inverse (Re of the full inverse) equals the folded inverse of the Hermitian part, on any spectrum
        z = (rng.normal(size=n) + 1j * rng.normal(size=n)) * 2.0 ** 20
        assert np.max(np.abs(t.inverse_f64(z) - m.folded_inverse_f64(m.hermitian_even(z)))) <= 1e-9
        assert np.allclose(m.folded_inverse_f64(m.hermitian_even(y)), m.centred(x, bits), rtol=0, atol=scale)


def test_conversion_edge_values():
    f = m.from_f64_wrapping_rounded
    assert f(2.0 ** 64 + 2.0 ** 40, 64)[0] == 2 ** 40
    assert f(2.0 ** 40 + 5, 32)[0] == 5
    assert f(2.0 ** 70, 32)[0] == 0xFFFFFFFF and f(-2.0 ** 70, 32)[0] == 0
    assert f(2.0 ** 63, 32)[0] == 0xFFFFFFFF and f(-2.0 ** 63, 32)[0] == 0
    assert f(2.0 ** 127, 64)[0] == 2 ** 64 - 1 and f(-2.0 ** 127, 64)[0] == 0
    assert f(-(2.0 ** 64) - 2.0 ** 12, 64)[0] == 2 ** 64 - 2 ** 12
    assert list(f(np.array([2.5, -2.5, 0.49999999999999994, -0.5]), 64)) == [3, 2 ** 64 - 3, 0, 2 ** 64 - 1]
    assert f(np.nan, 32)[0] == 0
    # a constant spectrum V inverts to V at word 0
    t = m.FullComplex64FftTable(4)
    for v, bits, want in ((2.0 ** 64 + 2.0 ** 40, 64, 2 ** 40), (2.0 ** 40 + 5, 32, 5), (2.0 ** 70, 32, 0xFFFFFFFF)):
        assert t.inverse(np.full(16, v, np.complex128), bits)[0] == want


def test_basis_digits_recompose():
    rng = np.random.default_rng(3)
    for bits, lb, length in ((32, 4, 2), (32, 7, 3), (32, 8, None), (32, 1, 8), (64, 23, 1), (64, 15, 2), (64, 1, None)):
        b = m.ApproxSignedBasis(bits, lb, length)
        x = rng.integers(0, 2 ** bits, 4096, dtype=np.uint64).astype(m.UINT[bits])
        digits = b.digits(x)
        assert len(digits) == b.decompose_length
        lo = 0 if lb == 1 else -(1 << (lb - 1))
        assert all(d.min() >= lo and d.max() <= (1 if lb == 1 else (1 << (lb - 1))) for d in digits)
        # sum d_l B^l 2^drop is x rounded to the kept bits (mod 2^BITS), for every word
        half = (1 << (b.drop_bits - 1)) if b.drop_bits else 0
        for j, xi in enumerate(int(v) for v in x):
            approx = sum(int(dd[j]) << (b.drop_bits + i * lb) for i, dd in enumerate(digits))
            rounded = ((xi + half) >> b.drop_bits) << b.drop_bits
            assert approx % (1 << bits) == rounded % (1 << bits), (bits, lb, length, hex(xi))
    with pytest.raises(AssertionError):
        m.ApproxSignedBasis(32, 0)
    with pytest.raises(AssertionError):
        m.ApproxSignedBasis(32, 8, 5)


EDGE_BASES = [  # bits, log_basis, reverse_length (None = full), edge words
    (32, 7, 3, 1373), (32, 10, 2, 197), (32, 8, None, 100), (32, 1, 8, 73), (32, 31, 1, 14),
    (64, 15, 2, 197), (64, 23, 1, 29), (64, 1, 10, 89), (64, 21, 3, 686),
]


@pytest.mark.parametrize("bits,lb,length,count", EDGE_BASES)
def test_digits_of_every_edge_word(bits, lb, length, count):
    """Every edge word (tests/tfhe_edge_words.py) against Python integers: each digit in [-B/2, B/2 - 1] ({0, 1} for
    log B = 1) and sum d_l 2^(drop + l log B) = ((x + 2^(drop-1)) >> drop) << drop mod 2^BITS (no rounding term when
    drop = 0).  ell digits of that range represent at most B^ell = 2^(BITS - drop) values, one per residue, so range and
    recomposition determine the digits: this pins the model without restating its branches."""
    words = edge_words(bits, lb, length)
    assert words.dtype == m.UINT[bits] and len(words) == count
    assert np.array_equal(words, np.unique(words))
    assert {0, 1, (1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1} <= {int(w) for w in words}
    b = m.ApproxSignedBasis(bits, lb, length)
    ell, drop = b.decompose_length, b.drop_bits
    digits = b.digits(words)
    assert len(digits) == ell and all(d.shape == words.shape for d in digits)
    lo, hi = (0, 1) if lb == 1 else (-(1 << (lb - 1)), (1 << (lb - 1)) - 1)
    half = (1 << (drop - 1)) if drop else 0
    seen = set()
    for j, x in enumerate(int(w) for w in words):
        ds = [int(d[j]) for d in digits]
        assert all(lo <= d <= hi for d in ds), (hex(x), ds)
        approx = sum(d << (drop + l * lb) for l, d in enumerate(ds))
        assert approx % (1 << bits) == (((x + half) >> drop) << drop) % (1 << bits), (hex(x), ds)
        seen.update(ds)
    # the list does reach what it is for: both ends of the digit range and, through a carry, a zero digit above B - 1
    assert {lo, hi, 0} <= seen


def test_reference_external_product_smoke():
    """tfhe_external_product.rs: N = 8, k = 1, ell = 2, log B = 4 bit-exact to the schoolbook, and zero in gives zero out"""
    log_n, k, n = 3, 1, 8
    b = m.ApproxSignedBasis(32, 4, 2)
    g = np.array([(i % 7) - 3 for i in range(64)], np.int64).astype(np.uint32)
    inp = np.array([(i % 5) - 2 for i in range(16)], np.int64).astype(np.uint32)
    t = m.FullComplex64FftTable(log_n)
    key = t.forward(g.reshape(-1, n), 32).reshape(-1)
    out, _ = m.external_product(inp, key, b, log_n, k)
    assert np.array_equal(out, m.schoolbook(inp, g, b, log_n, k))
    # the reference's input decomposes to zero digits at these parameters; a full-range one exercises the product
    rng = np.random.default_rng(0)
    inp2 = rng.integers(0, 2 ** 32, 16, dtype=np.uint64).astype(np.uint32)
    out2, _ = m.external_product(inp2, key, b, log_n, k)
    assert np.array_equal(out2, m.schoolbook(inp2, g, b, log_n, k)) and out2.any()
    z, _ = m.external_product(np.zeros(8, np.uint32), np.ones(16, np.complex128), m.ApproxSignedBasis(32, 8, 1), 2, 1)
    assert not z.any()


@pytest.mark.parametrize("bits,log_n,k,lb,length", [(32, 6, 1, 7, 3), (32, 5, 2, 4, None), (64, 6, 1, 15, 2),
                                                     (64, 5, 1, 1, 20)])
def test_model_product_is_exact_on_small_keys(bits, log_n, k, lb, length):
    rng = np.random.default_rng(log_n + lb)
    b = m.ApproxSignedBasis(bits, lb, length)
    n = 1 << log_n
    g = rng.integers(-1024, 1025, (k + 1) * b.decompose_length * (k + 1) * n).astype(m.UINT[bits])
    key = m.FullComplex64FftTable(log_n).forward(g.reshape(-1, n), bits).reshape(-1)
    inp = rng.integers(0, 2 ** bits, (k + 1) * n, dtype=np.uint64).astype(m.UINT[bits])
    out, _ = m.external_product(inp, key, b, log_n, k)
    assert np.array_equal(out, m.schoolbook(inp, g, b, log_n, k))


def test_fourier_convert_roundtrips():
    """fourier_convert.rs: GLWE / GLev / GGSW write_fourier_form then write_torus_form round-trip (polynomial by
    polynomial, which is why the containers are one batched transform)"""
    for bits, max_log_n, k in ((32, 4, 2), (64, 3, 1)):
        for log_n in range(1, max_log_n + 1):
            t = m.FullComplex64FftTable(log_n)
            for polys in (k + 1, 2 * (k + 1), (k + 1) * 2 * (k + 1)):
                x = pattern(polys * t.n, bits).reshape(polys, t.n)
                assert np.array_equal(t.inverse(t.forward(x, bits), bits), x)
