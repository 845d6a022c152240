"""Reference model of the packing key switch in the Fourier domain (include/pfhe.h, pfhe_tfhe{,32}_packfft_*,
_pack_keyswitch_fft*), shared by the CPU model test and the GPU tests.  numpy f64 on tests/tfhe_fft_model.py
(folded_forward / folded_inverse_f64 / from_f64_wrapping_rounded, ApproxSignedBasis.digits) beside the exact
tests/tfhe_pack_model.py:

    D_{j,l}(X) = sum_{i<count} d_l(a_{e,i,j}) X^i                              (real, zero from count on)
    ACC_c      = sum_slices sum_{j in slice} sum_l FFT(D_{j,l}) * fkey[j][l][c]         c = 0..k
    out_e      = (0, .., 0, sum_i b_{e,i} X^i) - to_torus(IFFT(ACC_c))          mod 2^BITS, X^N + 1

with fkey the half spectrum of every key polynomial (the even entries of its negacyclic transform, which for a real
polynomial are its Hermitian part).  The mask words are summed slice by slice and the slices in ascending order, as the
kernels do; the slice width is a parameter here and a constant of the build there.
"""
import functools
import zlib

import numpy as np

import tfhe_fft_model as m
import tfhe_pack_model as pm

SLICE = 4     # mask words per slice in csrc/pfhe_pack_fft.hip (kPackFftSlice)


def half_spectrum_key(pksk, bits: int, log_n: int) -> np.ndarray:
    """the Fourier packing key: polynomial after polynomial, N/2 complex values each"""
    n = 1 << log_n
    return m.folded_forward(np.asarray(pksk).astype(m.UINT[bits]).reshape(-1, n), bits)


def pack_keyswitch_fft(lwe_in, fkey, in_dim: int, count: int, basis: m.ApproxSignedBasis, log_n: int, k: int,
                       slice_width: int = SLICE) -> np.ndarray:
    """batch x count x (in_dim + 1) words -> batch x (k + 1) x N words"""
    bits, ell, n = basis.bits, basis.decompose_length, 1 << log_n
    h = n // 2
    assert 1 <= count <= n
    x = np.asarray(lwe_in).astype(m.UINT[bits]).reshape(-1, count, in_dim + 1)
    key = np.asarray(fkey, np.complex128).reshape(in_dim, ell, k + 1, h)
    out = np.zeros((x.shape[0], k + 1, n), m.UINT[bits])
    with np.errstate(over="ignore"):
        for e in range(x.shape[0]):
            digits = basis.digits(x[e, :, :in_dim])                       # ell arrays of count x in_dim signed digits
            d = np.zeros((in_dim, ell, n), m.UINT[bits])
            for l in range(ell):
                d[:, l, :count] = digits[l].astype(np.int64).view(np.uint64).astype(m.UINT[bits]).T
            spec = m.folded_forward(d, bits)                              # in_dim x ell x N/2
            acc = np.zeros((k + 1, h), np.complex128)
            for j0 in range(0, in_dim, slice_width):
                part = np.zeros((k + 1, h), np.complex128)
                for j in range(j0, min(in_dim, j0 + slice_width)):
                    for l in range(ell):
                        part += spec[j, l][None, :] * key[j, l]
                acc += part
            v = m.folded_inverse_f64(acc)                                 # (k + 1) x N
            body = np.zeros((k + 1, n), m.UINT[bits])
            body[k, :count] = x[e, :, in_dim]
            out[e] = body - m.from_f64_wrapping_rounded(v, bits).reshape(k + 1, n)
    return out.reshape(-1)


# ---------------- the cases both tests run ----------------

# (bits, log_n, k, in_dimension, log_basis, ell, count): keys of words in [-2^10, 2^10] and
# n ell N 2^(logB-1) 2^10 <= 2^40, under which the f64 sums are exact and the route equals the integer one bit for bit
EXACT_CASES = [
    (32, 5, 1, 12, 4, 6, 32),
    (64, 6, 2, 9, 7, 3, 5),
    (64, 11, 1, 8, 4, 2, 2048),
    (32, 10, 1, 20, 4, 3, 1000),
    (32, 1, 1, 3, 3, 2, 2),
    (64, 3, 3, 5, 2, 4, 8),
]

# full-torus keys: the route is approximate; the model's own distance from the exact result is the yardstick
FULL_TORUS_CASES = [
    (32, 5, 1, 12, 4, 6, 32),
    (32, 6, 2, 9, 7, 3, 5),
    (32, 10, 1, 24, 4, 3, 1024),
    (64, 5, 1, 10, 15, 3, 32),
    (64, 4, 1, 7, 8, 8, 16),
    (64, 11, 1, 12, 4, 3, 2048),
]


def exact_regime_holds(case) -> bool:
    _, log_n, _, n, lb, ell, _ = case
    return n * ell * (1 << log_n) * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40


def case_inputs(case, small_keys: bool, batch: int = 1):
    """(basis, pksk, lwe) of a case, the same words wherever it is asked for"""
    bits, log_n, k, n, lb, ell, count = case
    rng = np.random.default_rng(zlib.crc32(repr((case, small_keys, batch)).encode()))
    basis = m.ApproxSignedBasis(bits, lb, ell)
    words = n * ell * (k + 1) << log_n
    if small_keys:
        pksk = rng.integers(-2 ** 10, 2 ** 10 + 1, words).astype(np.int64).view(np.uint64).astype(m.UINT[bits])
    else:
        pksk = rng.integers(0, 2 ** bits, words, dtype=np.uint64).astype(m.UINT[bits])
    lwe = rng.integers(0, 2 ** bits, batch * count * (n + 1), dtype=np.uint64).astype(m.UINT[bits])
    return basis, pksk, lwe


def model_error(case, lwe, pksk, exact) -> float:
    """the largest centred distance of the model's result from `exact` (the integer route's words)"""
    bits, log_n, k, n, lb, ell, count = case
    basis = m.ApproxSignedBasis(bits, lb, ell)
    got = pack_keyswitch_fft(lwe, half_spectrum_key(pksk, bits, log_n), n, count, basis, log_n, k)
    return float(m.centred_error(got, exact, bits).max())


@functools.lru_cache(maxsize=None)
def full_torus_model_error(case) -> float:
    """the model against tfhe_pack_model.pack_keyswitch on the case's own inputs, computed once"""
    bits, log_n, k, n, lb, ell, count = case
    basis, pksk, lwe = case_inputs(case, small_keys=False)
    return model_error(case, lwe, pksk, pm.pack_keyswitch(lwe, pksk, n, count, basis, log_n, k))
