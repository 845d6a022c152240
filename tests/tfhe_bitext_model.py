"""Reference model of bit extraction on the torus side (include/pfhe.h, pfhe_bitext{,32}_*; DESIGN.md
§24), shared by the CPU model test and the GPU parity tests.  Exact, wrapping numpy; composed from
tfhe_bootstrap_model.keyswitch, modulus_switch and sample_extract and tfhe_blindrot_model.exact_rotate.

Conventions: the phase is b - <a,s>; bit 0 is the least significant.  The input is an LWE ciphertext of k N + 1 words under
the extracted GLWE key whose phase is m 2^delta + e; bit i of input e leaves at row e bits + i as an LWE ciphertext of
n + 1 words under the LWE key whose phase is m_i 2^(BITS-1) plus noise.  With c_0 the input, for i = 0 .. bits-1:
  out[e][i] = keyswitch(c_i << sigma_i), sigma_i = BITS - 1 - delta - i, every word shifted as a wrapping word;
  unless i = bits-1: the modulus switch of (a, b + 2^(BITS-2)) of that output, ACC = X^{neg_b} TV_i with TV_i the trivial
  GLWE whose body is -2^(delta+i-1) on every coefficient, exact_rotate over the n keys, extraction at index 0 with
  2^(delta+i-1) added to the body, and c_{i+1} = c_i minus that: the extracted phase is m_i 2^(delta+i) plus noise.
"""
import numpy as np

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg


def shift_words(words, sigma: int, bits: int) -> np.ndarray:
    """every word shifted left by sigma as a wrapping word"""
    x = np.asarray(words).astype(np.uint64)
    with np.errstate(over="ignore"):
        return ((x << np.uint64(sigma)) & np.uint64((1 << bits) - 1)).astype(m.UINT[bits])


def offset_body(lwe, n: int, bits: int) -> np.ndarray:
    """(a, b + 2^(BITS-2)): what the modulus switch sees"""
    x = np.asarray(lwe).astype(m.UINT[bits]).reshape(-1, n + 1).copy()
    with np.errstate(over="ignore"):
        x[:, n] += m.UINT[bits](1 << (bits - 2))
    return x.reshape(-1)


def bit_test_vector(half_shift: int, bits: int, log_n: int, k: int) -> np.ndarray:
    """TV_i: the trivial GLWE whose body has -2^half_shift on every coefficient"""
    tv = np.zeros((k + 1, 1 << log_n), m.UINT[bits])
    tv[k] = (-(1 << half_shift)) % (1 << bits)
    return tv.reshape(-1)


def clear_bit(run, switched, keys_coeff, basis, log_n: int, k: int, n: int, half_shift: int, rotate=bm.exact_rotate):
    """step 2 of the rule on a batch: run (batch x (k N + 1)) minus the extraction of the rotated X^{neg_b} TV_i.  Returns
    (the new running ciphertexts, exps, neg_b)."""
    bits, big_n = basis.bits, 1 << log_n
    exps, neg_b = bs.modulus_switch(offset_body(switched, n, bits), n, bits, log_n)
    tv = bit_test_vector(half_shift, bits, log_n, k)
    accs = [rotate(bm.rotate(tv, int(neg_b[e]), big_n), keys_coeff, exps[e], basis, log_n, k) for e in range(exps.shape[0])]
    lwe = bs.sample_extract(np.concatenate(accs), log_n, k, 0).reshape(-1, k * big_n + 1)
    with np.errstate(over="ignore"):
        lwe[:, k * big_n] += m.UINT[bits](1 << half_shift)
        out = np.asarray(run).astype(m.UINT[bits]).reshape(-1, k * big_n + 1) - lwe
    return out.reshape(-1), exps, neg_b


def extract_bits(lwe_in, keys_coeff, ksk, basis, ks_basis, log_n: int, k: int, n: int, delta_log: int, nbits: int,
                 rotate=bm.exact_rotate) -> np.ndarray:
    """batch x (k N + 1) words -> batch x nbits x (n + 1) words; keys_coeff: the n coefficient-domain GGSW keys"""
    bits, ext = basis.bits, (k << log_n) + 1
    assert 1 <= delta_log and 1 <= nbits and delta_log + nbits <= bits
    run = np.asarray(lwe_in).astype(m.UINT[bits]).reshape(-1)
    batch = run.size // ext
    out = np.zeros((batch, nbits, n + 1), m.UINT[bits])
    for i in range(nbits):
        sigma = bits - 1 - delta_log - i
        switched = bs.keyswitch(shift_words(run, sigma, bits), ksk, ext - 1, n, ks_basis)
        out[:, i] = switched.reshape(batch, n + 1)
        if i + 1 < nbits:
            run, _, _ = clear_bit(run, switched, keys_coeff, basis, log_n, k, n, delta_log + i - 1, rotate)
    return out.reshape(-1)


def decode_bits(phases, bits: int):
    """round(phase / 2^(BITS-1)) modulo 2 per phase"""
    return [((int(v) + (1 << (bits - 2))) >> (bits - 1)) & 1 for v in phases]


# ---------------- the bound ----------------

def ks_terms(bits, log_n, k, ks_lb, ks_ell, noise) -> float:
    """what the key switch adds: k N ell_ks (B_ks/2) E + k N 2^(drop_ks-1), the last term 0 at drop 0"""
    ks_basis = m.ApproxSignedBasis(bits, ks_lb, ks_ell)
    half = 2.0 ** (ks_basis.drop_bits - 1) if ks_basis.drop_bits else 0.0
    return (k << log_n) * ks_basis.decompose_length * 2.0 ** (ks_lb - 1) * noise + (k << log_n) * half


def bit_bound(bits, log_n, k, n, lb, ell, ks_lb, ks_ell, noise, e_in, delta_log, i) -> float:
    """The worst case of |phase of bit i's ciphertext - m_i 2^(BITS-1) - (higher bits, multiples of 2^BITS)| for binary
    keys and |e| <= noise on every key row.  The running ciphertext before bit i is off by at most e_in plus i rotations of n
    steps each (tfhe_keygen_model.step_bound; the accumulator starts trivial every time, so nothing else is carried); the
    shift multiplies that by 2^sigma_i; the key switch adds its own terms."""
    sigma = bits - 1 - delta_log - i
    return (e_in + i * n * kg.step_bound(bits, log_n, k, lb, ell, noise)) * 2.0 ** sigma + \
        ks_terms(bits, log_n, k, ks_lb, ks_ell, noise)


def margin(bits: int) -> float:
    """a bit ciphertext decodes, and the quarter turn of the next step lands in the right half, while the error is below a
    quarter of the torus"""
    return 2.0 ** (bits - 2)


def bit_fits(bits, log_n, k, n, lb, ell, ks_lb, ks_ell, noise, e_in, delta_log, i) -> bool:
    """the bit is right while bit_bound, scaled to exponents modulo 2N, plus the modulus switch's (n + 1)/2 stays below N/2"""
    big_n = 1 << log_n
    b = bit_bound(bits, log_n, k, n, lb, ell, ks_lb, ks_ell, noise, e_in, delta_log, i)
    return b * (2 * big_n) / 2.0 ** bits + (n + 1) / 2 < big_n / 2


def all_bits_fit(bits, log_n, k, n, lb, ell, ks_lb, ks_ell, noise, e_in, delta_log, nbits) -> bool:
    return all(bit_fits(bits, log_n, k, n, lb, ell, ks_lb, ks_ell, noise, e_in, delta_log, i) for i in range(nbits))


# ---------------- the noisy shapes of the GPU tests ----------------

# (message bits, delta_log as BITS - that) of the meaning test, on the first three shapes of tfhe_keygen_model.NOISY_CASES
MEANING_BITS = ((3, 3), (5, 6))


def meaning_shapes():
    """(bits, log_n, k, n, lb, ell, noise, nbits, delta_log) of every case of the GPU meaning test"""
    out = []
    for bits, log_n, k, n, lb, ell, _g, _p, noise in kg.NOISY_CASES[:3]:
        for nbits, below in MEANING_BITS:
            out.append((bits, log_n, k, n, lb, ell, noise, nbits, bits - below))
    return out


# The chain on the shapes of tfhe_lut_model.NOISY_LUTS needs every bit of a fresh encryption to fit; where the shape's own
# noise does not, the test runs it at the noise listed here instead (index into NOISY_LUTS -> noise), and says so.
CHAIN_NOISE = {}
