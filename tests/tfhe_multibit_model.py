"""Reference model of the multi-bit blind rotation over the TFHE product (include/pfhe.h, pfhe_tfhe{,32}_mbrot_*), shared by
the CPU model test and the GPU parity tests.  Built on tests/tfhe_fft_model.py and tests/tfhe_blindrot_model.py.

The mask is consumed g elements at a time; group t has 2^g keys, key j for the pattern j of the group's (binary) key bits.
For one ciphertext and one group, with the group's exponents a_0 .. a_{g-1}:
    r_j = (sum of a_b over the set bits b of j) mod 2N,   r_0 = 0
    K   = sum_j M(r_j) (.) BSK[t][j]        M(r)[k'] = root[(r (1 - 2k')) mod 2N], the spectrum of X^r in the full layout
    ACC = external_product_to(ACC, K)       the product itself, no "+ ACC"
exact_group carries the same step out in integers: the schoolbook against the coefficient-domain key sum_j X^{r_j} K_j
(wrapping rotation and sum).
"""
import numpy as np

import tfhe_blindrot_model as bm
import tfhe_fft_model as m


def root(log_n: int) -> np.ndarray:
    """cis(pi i / N) for i < 2N from the table's N twiddles: root[i] = tw[i] for i < N, -tw[i - N] otherwise"""
    tw = m.twist(log_n)
    return np.concatenate([tw, -tw])


def monomial_spectrum(r: int, log_n: int) -> np.ndarray:
    """M(r): the spectrum of X^r (r taken modulo 2N) in the table's full layout, entry k' = root[(r (1 - 2k')) mod 2N]"""
    n = 1 << log_n
    k = np.arange(n, dtype=np.int64)
    return root(log_n)[((r % (2 * n)) * (1 - 2 * k)) % (2 * n)]


def monomial(r: int, log_n: int, bits: int) -> np.ndarray:
    """X^r as a torus polynomial of N words (X^N = -1)"""
    n = 1 << log_n
    r %= 2 * n
    out = np.zeros(n, m.UINT[bits])
    out[r % n] = 1 if r < n else (1 << bits) - 1
    return out


def subset_sums(exps_group, n: int):
    """r_j for j = 0 .. 2^g - 1"""
    g = len(exps_group)
    return [sum(int(exps_group[b]) % (2 * n) for b in range(g) if (j >> b) & 1) % (2 * n) for j in range(1 << g)]


def combine_key(keys_fourier: np.ndarray, exps_group, log_n: int) -> np.ndarray:
    """K = sum_j M(r_j) (.) K_j for the 2^g Fourier keys of one group (2^g x key_len complex values), j ascending"""
    n = 1 << log_n
    keys = np.asarray(keys_fourier, np.complex128).reshape(1 << len(exps_group), -1, n)
    out = keys[0].copy()
    for j, r in enumerate(subset_sums(exps_group, n)):
        if j:
            out = out + monomial_spectrum(r, log_n)[None, :] * keys[j]
    return out.reshape(-1)


def step(acc_e: np.ndarray, keys_fourier: np.ndarray, exps_group, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """one group for ONE ciphertext in the f64 model"""
    out, _ = m.external_product(acc_e, combine_key(keys_fourier, exps_group, log_n), basis, log_n, k)
    return out


def rotate_loop(acc_e: np.ndarray, bsk_fourier: np.ndarray, exps_e, g: int, basis: m.ApproxSignedBasis, log_n: int,
                k: int) -> np.ndarray:
    """the whole loop for ONE ciphertext: bsk_fourier groups x 2^g keys end to end, exps_e groups*g exponents"""
    groups = len(exps_e) // g
    keys = np.asarray(bsk_fourier, np.complex128).reshape(groups, -1)
    acc = np.asarray(acc_e).copy()
    for t in range(groups):
        acc = step(acc, keys[t], exps_e[t * g:(t + 1) * g], basis, log_n, k)
    return acc


def exact_key(keys_coeff, exps_group, log_n: int) -> np.ndarray:
    """sum_j X^{r_j} K_j in the coefficient domain, wrapping; keys_coeff: the group's 2^g keys as word arrays"""
    n = 1 << log_n
    out = np.zeros_like(keys_coeff[0])
    for key, r in zip(keys_coeff, subset_sums(exps_group, n)):
        out = bm.add(out, bm.rotate(key, r, n))
    return out


def exact_group(acc_e: np.ndarray, keys_coeff, exps_group, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """one group for ONE ciphertext with the product as the exact integer schoolbook"""
    return m.schoolbook(acc_e, exact_key(keys_coeff, exps_group, log_n), basis, log_n, k).astype(acc_e.dtype)


def exact_rotate_loop(acc_e: np.ndarray, keys_coeff, exps_e, g: int, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """the whole loop for ONE ciphertext in integers: exact_group over the groups.  keys_coeff: groups * 2^g coefficient-domain
    keys, group after group; exps_e: groups * g exponents, each taken modulo 2N (device-form words of 2N and more allowed)"""
    assert len(exps_e) % g == 0 and len(keys_coeff) == (len(exps_e) // g) << g
    acc = np.asarray(acc_e).copy()
    for t in range(len(exps_e) // g):
        acc = exact_group(acc, keys_coeff[t << g:(t + 1) << g], exps_e[t * g:(t + 1) * g], basis, log_n, k)
    return acc


def indicator_keys(basis: m.ApproxSignedBasis, log_n: int, k: int, key_bits) -> list:
    """the 2^g trivially encrypted keys of one group: key j is G when the group's key bits equal pattern j, 0 otherwise"""
    g = len(key_bits)
    pattern = sum(int(s) << b for b, s in enumerate(key_bits))
    return [bm.trivial_ggsw(basis, log_n, k, int(j == pattern)) for j in range(1 << g)]


def multibit_indicator_bsk(basis: m.ApproxSignedBasis, log_n: int, k: int, secret, g: int) -> list:
    """coefficient-domain keys of a whole multi-bit bootstrapping key, group after group, for a binary secret"""
    assert len(secret) % g == 0
    out = []
    for t in range(len(secret) // g):
        out += indicator_keys(basis, log_n, k, secret[t * g:(t + 1) * g])
    return out


def fourier(keys_coeff, log_n: int, bits: int) -> np.ndarray:
    """write_fourier_form of a list of coefficient-domain keys, end to end"""
    n = 1 << log_n
    fft = m.FullComplex64FftTable(log_n)
    return np.concatenate([fft.forward(g.reshape(-1, n), bits).reshape(-1) for g in keys_coeff])
