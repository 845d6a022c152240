"""Reference model of packing on the torus side (include/pfhe.h, pfhe_tfhe{,32}_pack_keyswitch*, _pksk_generate_dev,
_sample_extract_first_few*, _multimsg_extract*), shared by the CPU model test and the GPU parity tests.  Exact, wrapping
numpy; built on tests/tfhe_fft_model.py, tests/tfhe_bootstrap_model.py and tests/tfhe_keygen_model.py.

  - pack_keyswitch: out_e = (0, .., 0, sum_i b_{e,i} X^i) - sum_i X^i sum_j sum_l d_l(a_{e,i,j}) PKSK[j][l] modulo 2^BITS
    and X^N + 1, the digits those of ApproxSignedBasis.digits.  The sum over i is taken first, per key row, as the digit
    polynomial D_{j,l} = sum_i d_l(a_{e,i,j}) X^i, which then meets the row in one negacyclic product;
  - generate_pksk: the GLWE body call on every row, then key_in[j] 2^(drop_bits + l log_basis) on coefficient 0 of the body;
  - extract_first_few: Rlwe::extract_first_few_lwe (primus_lattice/src/rlwe/coeff.rs:231-260) per mask polynomial;
  - multimsg_extract: MultiMsgLwe::extract_rlwe_mode (lwe/multiple_message.rs:250-263) per mask polynomial, every index.
"""
import numpy as np

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg


def negacyclic(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """tfhe_fft_model.negacyclic_u64 through one wrapping uint64 convolution (the CPU test holds the two together)"""
    n = a.size
    with np.errstate(over="ignore"):
        full = np.convolve(a.astype(np.uint64), b.astype(np.uint64))
        out = full[:n].copy()
        out[:n - 1] -= full[n:]
    return out


def pack_keyswitch(lwe_in, pksk, in_dim: int, count: int, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """batch x count x (in_dim + 1) words -> batch x (k + 1) x N words"""
    bits, ell, n = basis.bits, basis.decompose_length, 1 << log_n
    assert 1 <= count <= n
    x = np.asarray(lwe_in).astype(m.UINT[bits]).reshape(-1, count, in_dim + 1)
    key = np.asarray(pksk).astype(np.uint64).reshape(in_dim, ell, k + 1, n)
    out = np.zeros((x.shape[0], k + 1, n), np.uint64)
    with np.errstate(over="ignore"):
        for e in range(x.shape[0]):
            digits = basis.digits(x[e, :, :in_dim])                       # ell arrays of count x in_dim signed digits
            out[e, k, :count] = x[e, :, in_dim].astype(np.uint64)
            for l in range(ell):
                d = np.zeros((in_dim, n), np.uint64)
                d[:, :count] = digits[l].astype(np.int64).view(np.uint64).T
                for j in range(in_dim):
                    if not d[j].any():
                        continue
                    for c in range(k + 1):
                        out[e, c] -= negacyclic(d[j], key[j, l, c])
    return out.astype(m.UINT[bits]).reshape(-1)


def generate_pksk(rand, key_in, z, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """row (j, l): B += sum_r A_r z_r, and key_in[j] 2^(drop_bits + l log_basis) on coefficient 0; rand holds the randomness"""
    bits, ell, n = basis.bits, basis.decompose_length, 1 << log_n
    out = kg.glwe_body_mac(rand, z, bits, log_n, k).astype(np.uint64).reshape(len(key_in), ell, k + 1, n)
    scale = np.array([1 << (basis.drop_bits + l * basis.log_basis) for l in range(ell)], np.uint64)
    with np.errstate(over="ignore"):
        out[:, :, k, 0] += np.asarray(key_in).astype(np.uint64)[:, None] * scale[None, :]
    return out.astype(m.UINT[bits]).reshape(-1)


def extract_first_few(glwe, log_n: int, k: int, count: int) -> np.ndarray:
    """batch GLWE ciphertexts -> batch MultiMsgLwe layouts of k N + count words"""
    n = 1 << log_n
    g = np.asarray(glwe).reshape(-1, k + 1, n)
    out = np.zeros((g.shape[0], k * n + count), g.dtype)
    with np.errstate(over="ignore"):
        for j in range(k):
            out[:, j * n] = g[:, j, 0]
            out[:, j * n + 1:(j + 1) * n] = (0 - g[:, j, :0:-1]).astype(g.dtype)      # -a_{N-1}, ..., -a_1
    out[:, k * n:] = g[:, k, :count]
    return out.reshape(-1)


def multimsg_extract(multi, log_n: int, k: int, count: int) -> np.ndarray:
    """batch layouts -> batch x count LWE ciphertexts of k N + 1 words: rotate_right(h), the first h words negated, body b_h"""
    n = 1 << log_n
    x = np.asarray(multi).reshape(-1, k * n + count)
    out = np.zeros((x.shape[0], count, k * n + 1), x.dtype)
    with np.errstate(over="ignore"):
        for h in range(count):
            for j in range(k):
                data = np.roll(x[:, j * n:(j + 1) * n], h, axis=1)
                data[:, :h] = (0 - data[:, :h]).astype(x.dtype)
                out[:, h, j * n:(j + 1) * n] = data
            out[:, h, k * n] = x[:, k * n + h]
    return out.reshape(-1)


def extracted_key_rows(pksk, log_n: int, k: int) -> np.ndarray:
    """the LWE key-switch key whose rows are the index-0 extractions of the packing key's rows"""
    return bs.sample_extract(np.asarray(pksk), log_n, k, 0)


# ---------------- the round trip on noisy keys ----------------

def noise_bound(bits, n, lb, ell, count, noise) -> float:
    """|phase - Delta m| of a packed coefficient for binary keys, |e| <= noise on every key row, noise-free inputs and
    digits of magnitude at most B/2: every one of the count n ell digit-times-row-noise products can land on the
    coefficient, and every mask word loses at most 2^(drop_bits - 1) to the decomposition's rounding, once per set key bit:
        count n ell (B/2) E + n 2^(drop_bits - 1)          (the second term 0 at drop_bits 0)"""
    basis = m.ApproxSignedBasis(bits, lb, ell)
    half = 2.0 ** (basis.drop_bits - 1) if basis.drop_bits else 0.0
    return count * n * basis.decompose_length * 2.0 ** (lb - 1) * noise + n * half


# (bits, log_n, k, n, lb, ell, count, noise, p)
NOISY_CASES = [
    (32, 5, 1, 12, 4, 6, 32, 4, 2),
    (32, 6, 2, 9, 7, 3, 5, 16, 2),
    (64, 5, 1, 10, 15, 3, 32, 2 ** 20, 2),
    (64, 4, 1, 7, 8, 8, 16, 2 ** 10, 3),
]


def noisy_case(bits, log_n, k, n, lb, ell, count, noise, p, seed, batch=2):
    """Binary keys, the randomness of a noisy packing key and noise-free inputs of p-bit messages under one padding bit
    (Delta = 2^(BITS - p - 1)).  Host arrays; rand_pksk is the buffer the generation call takes."""
    big_n = 1 << log_n
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, n).astype(m.UINT[bits])
    z = rng.integers(0, 2, (k, big_n)).astype(m.UINT[bits])
    rand_pksk = kg.glwe_randomness(rng, bits, log_n, k, n * ell, noise)
    msgs = rng.integers(0, 1 << p, batch * count)
    delta = 1 << (bits - p - 1)
    lwe = bs.lwe_encrypt(msgs.astype(np.uint64) * np.uint64(delta), s, bits, rng)
    return dict(basis=basis, s=s, z=z, rand_pksk=rand_pksk, msgs=msgs, delta=delta, lwe=lwe, batch=batch)


def message_error(phases, msgs, delta: int, bits: int) -> float:
    """the largest centred distance of a phase from Delta m"""
    want = (np.asarray(msgs).astype(np.uint64) * np.uint64(delta)).astype(m.UINT[bits])
    return float(m.centred_error(np.asarray(phases).astype(m.UINT[bits]), want, bits).max())
