"""Reference model of key generation, encryption and phase for the TFHE bootstrap (include/pfhe.h,
pfhe_tfhe{,32}_lwe_body_mac*, _glwe_body_mac*, _ggsw_add_gadget_dev, _bsk_generate_dev, _ksk_generate_dev), shared by the CPU
model test and the GPU parity tests.  Exact, wrapping numpy; built on tests/tfhe_fft_model.py, tests/tfhe_blindrot_model.py
and tests/tfhe_bootstrap_model.py.

No function here draws a random number for the arithmetic under test: as on the device, the caller's buffers hold the
randomness (mask slots the uniform words, body slots noise + message) and the calls are deterministic.
  - lwe_body_mac / glwe_body_mac: Lwe / Rlwe::generate_random_zero_sample (lwe/single_message.rs:94-125,
    rlwe/coeff.rs:92-121) without their sampling, and the phase with the opposite sign;
  - ggsw_add_gadget: tfhe_blindrot_model.trivial_ggsw's rule on any buffer;
  - bsk / ksk: the layouts the rotation, the multi-bit rotation and the key switch take.
"""
import numpy as np

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_multibit_model as mb


def lwe_body_mac(lwe: np.ndarray, key: np.ndarray, bits: int, subtract: bool = False) -> np.ndarray:
    """b_e +- <a_e, key> for a batch of LWE ciphertexts of len(key) + 1 words; returns the new batch"""
    dim = len(key)
    x = np.asarray(lwe).astype(np.uint64).reshape(-1, dim + 1).copy()
    with np.errstate(over="ignore"):
        dot = x[:, :dim] @ np.asarray(key).astype(np.uint64)
        x[:, dim] = x[:, dim] - dot if subtract else x[:, dim] + dot
    return x.astype(m.UINT[bits]).reshape(-1)


def glwe_body_mac(glwe: np.ndarray, key: np.ndarray, bits: int, log_n: int, k: int, subtract: bool = False) -> np.ndarray:
    """B_e +- sum_j A_{e,j} * z_j (negacyclic, exact) for a batch of GLWE ciphertexts; key: k x N words"""
    n = 1 << log_n
    g = np.asarray(glwe).astype(np.uint64).reshape(-1, k + 1, n).copy()
    z = np.asarray(key).astype(np.uint64).reshape(k, n)
    with np.errstate(over="ignore"):
        for e in range(g.shape[0]):
            for j in range(k):
                prod = m.negacyclic_u64(z[j], g[e, j])
                g[e, k] = g[e, k] - prod if subtract else g[e, k] + prod
    return g.astype(m.UINT[bits]).reshape(-1)


def ggsw_add_gadget(ggsw: np.ndarray, messages, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """m 2^(drop_bits + l log_basis) onto coefficient 0 of component r of row (r, l) of every GGSW of the batch"""
    n, ell, bits = 1 << log_n, basis.decompose_length, basis.bits
    out = np.asarray(ggsw).astype(np.uint64).reshape(-1, k + 1, ell, k + 1, n).copy()
    assert out.shape[0] == len(messages)
    with np.errstate(over="ignore"):
        for q, msg in enumerate(messages):
            for r in range(k + 1):
                for l in range(ell):
                    out[q, r, l, r, 0] += np.uint64((int(msg) << (basis.drop_bits + l * basis.log_basis)) % (1 << 64))
    return out.astype(m.UINT[bits]).reshape(-1)


def ggsw_encrypt(rand: np.ndarray, messages, z: np.ndarray, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """torus-form GGSWs of `messages` under the GLWE key z from the randomness in `rand`: the body call on every row,
    then the gadget term"""
    return ggsw_add_gadget(glwe_body_mac(rand, z, basis.bits, log_n, k), messages, basis, log_n, k)


def indicator_messages(s, g: int, bits: int):
    """message of key [t][j] of a multi-bit key: prod_b (bit b of j ? s_{tg+b} : 1 - s_{tg+b}) in wrapping words"""
    assert len(s) % g == 0
    mod = 1 << bits
    out = []
    for t in range(len(s) // g):
        for j in range(1 << g):
            v = 1
            for b in range(g):
                sb = int(s[t * g + b])
                v = v * (sb if (j >> b) & 1 else 1 - sb) % mod
            out.append(v)
    return out


def bsk_messages(s, g: int, bits: int):
    """g = 0: the classic key's messages s_i; g >= 1: the multi-bit key's"""
    return [int(v) % (1 << bits) for v in s] if g == 0 else indicator_messages(s, g, bits)


def bsk(rand: np.ndarray, s, z: np.ndarray, basis: m.ApproxSignedBasis, log_n: int, k: int, g: int = 0) -> np.ndarray:
    """the torus-form bootstrapping key: n GGSWs (g = 0) or (n / g) 2^g (g >= 1), end to end"""
    return ggsw_encrypt(rand, bsk_messages(s, g, basis.bits), z, basis, log_n, k)


def ksk(rand: np.ndarray, s_in, s_out, basis: m.ApproxSignedBasis) -> np.ndarray:
    """row (i, j): b += <a, s_out> + s_in[i] 2^(drop_bits + j log_basis), rows of len(s_out) + 1 words in `rand`"""
    bits, ell = basis.bits, basis.decompose_length
    out = lwe_body_mac(rand, s_out, bits).astype(np.uint64).reshape(len(s_in) * ell, len(s_out) + 1)
    scale = np.array([1 << (basis.drop_bits + j * basis.log_basis) for j in range(ell)], np.uint64)
    with np.errstate(over="ignore"):
        out[:, len(s_out)] += (np.asarray(s_in).astype(np.uint64)[:, None] * scale[None, :]).reshape(-1)
    return out.astype(m.UINT[bits]).reshape(-1)


# ---------------- randomness for the tests ----------------

def uniform_words(rng, bits: int, size: int) -> np.ndarray:
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(m.UINT[bits])


def bounded_noise(rng, bits: int, size: int, bound: int) -> np.ndarray:
    """integers uniform in [-bound, bound] as torus words"""
    return rng.integers(-bound, bound + 1, size).astype(np.int64).view(np.uint64).astype(m.UINT[bits])


def glwe_randomness(rng, bits: int, log_n: int, k: int, count: int, bound: int) -> np.ndarray:
    """count GLWE ciphertexts: mask polynomials uniform, body polynomial noise"""
    n = 1 << log_n
    out = uniform_words(rng, bits, count * (k + 1) * n).reshape(count, k + 1, n)
    out[:, k] = bounded_noise(rng, bits, count * n, bound).reshape(count, n)
    return out.reshape(-1)


def lwe_randomness(rng, bits: int, dim: int, count: int, bound: int) -> np.ndarray:
    """count LWE ciphertexts: masks uniform, body slots noise"""
    out = uniform_words(rng, bits, count * (dim + 1)).reshape(count, dim + 1)
    out[:, dim] = bounded_noise(rng, bits, count, bound)
    return out.reshape(-1)


# ---------------- meaning on noisy keys ----------------

def noise_bound(bits, log_n, k, n, lb, ell, g, ks_lb, ks_ell, noise) -> float:
    """The worst case of |output phase - Delta f(m)| for binary keys, |e| <= noise on every key row, digits of magnitude at
    most B/2:
      steps [(k+1) ell N (B/2) E c + (1 + k N) 2^(drop-1)] + k N ell_ks (B_ks/2) E + k N 2^(ks_drop-1)
    steps = n and c = 1 for the classic rotation, n/g and 2^g for the multi-bit one (its combined key sums 2^g rotated keys);
    a 2^(drop-1) term is 0 at drop 0.  Per step: every one of the (k+1) ell N digit-times-row-noise products, and the
    rounding the decomposition drops, once on the body and once per key coefficient of the k N mask words.  The input's own
    noise does not appear: the test vector is trivially encrypted and condition (a) keeps the switched phase in its box."""
    big_n = 1 << log_n
    ks_basis = m.ApproxSignedBasis(bits, ks_lb, ks_ell)
    steps, c = (n, 1) if g == 0 else (n // g, 1 << g)
    ks_half = 2.0 ** (ks_basis.drop_bits - 1) if ks_basis.drop_bits else 0.0
    return steps * step_bound(bits, log_n, k, lb, ell, noise, c) + \
        k * big_n * ks_basis.decompose_length * 2.0 ** (ks_lb - 1) * noise + k * big_n * ks_half


def step_bound(bits, log_n, k, lb, ell, noise, c=1) -> float:
    """the per-step term of noise_bound"""
    basis = m.ApproxSignedBasis(bits, lb, ell)
    half = 2.0 ** (basis.drop_bits - 1) if basis.drop_bits else 0.0
    return (k + 1) * basis.decompose_length * (1 << log_n) * 2.0 ** (lb - 1) * noise * c + (1 + k * (1 << log_n)) * half


# the six shapes of the noisy bootstrap: (bits, log_n, k, n, lb, ell, g, p, noise); the key switch's basis is KS_BASIS
KS_BASIS = (4, 6)
NOISY_CASES = [
    (32, 6, 1, 8, 7, 3, 0, 2, 64),
    (64, 6, 1, 8, 15, 2, 0, 2, 2 ** 20),
    (32, 6, 2, 6, 7, 3, 0, 1, 64),
    (32, 6, 1, 8, 7, 3, 2, 2, 16),
    (64, 6, 1, 6, 15, 2, 3, 1, 2 ** 18),
    (32, 10, 1, 8, 7, 3, 0, 2, 4),
]


def noisy_case(bits, log_n, k, n, lb, ell, g, p, noise, seed):
    """Keys, the randomness of both generated keys and noisy inputs: binary LWE and GLWE keys, bounded uniform noise on
    every key row and on the inputs, the half-box LUT, every p-bit message twice.  Returns host arrays; nothing is
    encrypted yet (rand_* are the buffers the generation calls take)."""
    big_n = 1 << log_n
    basis, ks_basis = m.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, n).astype(m.UINT[bits])
    z = rng.integers(0, 2, (k, big_n)).astype(m.UINT[bits])
    keys = (n // g) << g if g else n
    rand_bsk = glwe_randomness(rng, bits, log_n, k, keys * (k + 1) * ell, noise)
    rand_ksk = lwe_randomness(rng, bits, n, k * big_n * ks_basis.decompose_length, noise)
    msgs = np.tile(np.arange(1 << p), 2)
    delta = 1 << (bits - p - 1)
    lwe = lwe_randomness(rng, bits, n, len(msgs), noise).reshape(len(msgs), n + 1)
    with np.errstate(over="ignore"):
        lwe[:, n] += (msgs.astype(np.uint64) * np.uint64(delta)).astype(m.UINT[bits])
    tv = bs.lut_test_vector(bs.lut(p), p, bits, log_n, k)
    return dict(basis=basis, ks_basis=ks_basis, s=s, z=z, msgs=msgs, delta=delta, rand_bsk=rand_bsk, rand_ksk=rand_ksk,
                lwe_rand=lwe.reshape(-1), tv=tv, keys=keys)


def exact_bootstrap(lwe_in, keys_coeff, tv, ksk_words, basis, ks_basis, log_n, k, n, g):
    """the whole bootstrap in exact integers: tfhe_bootstrap_model.bootstrap for g = 0, the same stages around
    tfhe_multibit_model.exact_group for g >= 1"""
    if g == 0:
        return bs.bootstrap(lwe_in, keys_coeff, tv, ksk_words, basis, ks_basis, log_n, k, n)
    bits, big_n = basis.bits, 1 << log_n
    exps, neg_b = bs.modulus_switch(lwe_in, n, bits, log_n)
    tv = np.asarray(tv).astype(m.UINT[bits])
    accs = []
    for e in range(exps.shape[0]):
        acc = bm.rotate(tv, int(neg_b[e]), big_n)
        for t in range(n // g):
            acc = mb.exact_group(acc, keys_coeff[t << g:(t + 1) << g], exps[e, t * g:(t + 1) * g], basis, log_n, k)
        accs.append(acc)
    lwe = bs.sample_extract(np.concatenate(accs), log_n, k, 0)
    return bs.keyswitch(lwe, ksk_words, k * big_n, n, ks_basis)


def phase_error(phases, msgs, p: int, bits: int) -> float:
    """the largest centred distance of an output phase from Delta f(m)"""
    delta = 1 << (bits - p - 1)
    want = np.array([(delta * bs.lut(p)(int(v))) % (1 << bits) for v in msgs], dtype=np.uint64).astype(m.UINT[bits])
    return float(m.centred_error(np.asarray(phases).astype(m.UINT[bits]), want, bits).max())
