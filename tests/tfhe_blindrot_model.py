"""Reference model of the batched blind rotation over the TFHE product (include/pfhe.h, pfhe_tfhe{,32}_blindrot_*), shared
by the CPU model test and the GPU parity tests.  Built on tests/tfhe_fft_model.py.

One step per ciphertext, with its own exponent r and the step's key (torus words, wrapping arithmetic modulo 2^BITS):
    D   = X^r * ACC - ACC
    E   = external_product_to(D, BSK_i)
    ACC = ACC + E
exact_rotate carries the product out as the exact integer schoolbook on a coefficient-domain key.
"""
import numpy as np

import tfhe_fft_model as m

PLAINTEXT_BITS = 4


def rotate(x: np.ndarray, r: int, n: int) -> np.ndarray:
    """x * X^r (negacyclic: X^N = -1) for a flat array of torus polynomials of n words, wrapping modulo 2^BITS"""
    polys = x.reshape(-1, n)
    with np.errstate(over="ignore"):
        full = np.concatenate([polys, (0 - polys).astype(x.dtype)], axis=1)  # one period of X^j * p
    return np.roll(full, r % (2 * n), axis=1)[:, :n].reshape(-1).copy()


def sub(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (a - b).astype(a.dtype)


def add(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (a + b).astype(a.dtype)


def exact_rotate(acc_e: np.ndarray, keys_coeff, exps_e, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """the loop for ONE ciphertext with the product as the exact schoolbook; keys_coeff[i]: step i's key in the coefficient
    domain ((k+1)*ell*(k+1)*N words)"""
    n = 1 << log_n
    acc = acc_e.copy()
    for g, r in zip(keys_coeff, exps_e):
        d = sub(rotate(acc, int(r), n), acc)
        acc = add(acc, m.schoolbook(d, g, basis, log_n, k).astype(acc.dtype))
    return acc


def trivial_ggsw(basis: m.ApproxSignedBasis, log_n: int, k: int, s: int) -> np.ndarray:
    """s * G as a trivially encrypted torus GGSW in the coefficient domain ((k+1) x ell x (k+1) x N words): entry
    [r][l][r] holds s * 2^(drop_bits + l * log_basis) at coefficient 0, everything else is zero"""
    n, ell = 1 << log_n, basis.decompose_length
    out = np.zeros((k + 1, ell, k + 1, n), m.UINT[basis.bits])
    if s:
        for r in range(k + 1):
            for l in range(ell):
                out[r, l, r, 0] = s << (basis.drop_bits + l * basis.log_basis)
    return out.reshape(-1)


def encode(messages, bits: int, log_n: int, k: int) -> np.ndarray:
    """batch accumulators (0, ..., 0, Delta * m) with Delta = 2^(BITS - PLAINTEXT_BITS); messages: batch x N values below
    2^PLAINTEXT_BITS"""
    n = 1 << log_n
    out = np.zeros((len(messages), k + 1, n), m.UINT[bits])
    for e, msg in enumerate(messages):
        out[e, k] = (np.asarray(msg, np.uint64) << np.uint64(bits - PLAINTEXT_BITS)).astype(m.UINT[bits])
    return out.reshape(-1)


def decode(acc_e: np.ndarray, bits: int, log_n: int, k: int):
    """(largest centred distance of a mask word from zero, round(body / Delta) mod 2^PLAINTEXT_BITS per coefficient)"""
    n = 1 << log_n
    a = acc_e.reshape(k + 1, n)
    shift = bits - PLAINTEXT_BITS
    body = a[k].astype(np.uint64)
    mask = (1 << bits) - 1
    msg = [(((int(v) + (1 << (shift - 1))) & mask) >> shift) for v in body]
    return float(m.centred_error(a[:k], np.zeros_like(a[:k]), bits).max()), msg


def expected_decode(msg, total: int, n: int):
    """coefficients of X^total * msg (negacyclic), negated wrap-arounds taken mod 2^PLAINTEXT_BITS"""
    total %= 2 * n
    out = [0] * n
    for j, v in enumerate(msg):
        d = j + total
        sign = -1 if (d // n) % 2 else 1
        out[d % n] = (sign * int(v)) % (1 << PLAINTEXT_BITS)
    return out
