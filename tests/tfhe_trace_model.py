"""Reference model of the GLWE automorphism with its key switch, the homomorphic trace, their keys and the LWE embedding
(include/pfhe.h, pfhe_tfhe{,32}_glwe_trace_*, _glwe_automorphism*, _gksk_generate_dev, _lwe_embed*), shared by the CPU model
test and the GPU tests.  Wrapping numpy, built on tests/tfhe_fft_model.py: a `product(ct, key)` argument is, as in
tests/tfhe_cmux_model.py, the f64 Fourier model on a Fourier key or the exact integer schoolbook on a torus-form key, both
on a FULL key of (k+1) ell rows: rule 1 hands it the key padded with ell zero body rows.

  sigma_t  p(X) -> p(X^t) mod X^N + 1, t odd: sigma_t(p)[i] = p[u] for u < N, -p[u - N] otherwise, u = i t^-1 mod 2N
  rule 1   out = (0, .., 0, sigma_t(B)) - product(sigma_t(ct), pad(key))                                    modulo 2^BITS
  rule 2   ACC_0 = ct, ACC_s = ACC_{s-1} + rule 1(ACC_{s-1}, keys[s-1], t_s), t_s = 2^(log N - s + 1) + 1, s = 1..m
  rule 3   row (j, l) of key x: B += sum_c A_c (*) key_out_c, B += g_l sigma_{t_x}(key_in_j)
  rule 4   A_j[0] = a[jN], A_j[N - i] = -a[jN + i] (i >= 1), B = (b, 0, .., 0)
"""
import numpy as np

import tfhe_fft_model as m
import tfhe_keygen_model as kg


def fourier_product(basis: m.ApproxSignedBasis, log_n: int, k: int):
    return lambda ct, key: m.external_product(ct, key, basis, log_n, k)[0]


def exact_product(basis: m.ApproxSignedBasis, log_n: int, k: int):
    return lambda ct, key: m.schoolbook(ct, key, basis, log_n, k)


# ---------------- sigma_t ----------------

def sigma(p, t: int, bits: int) -> np.ndarray:
    """sigma_t on the last axis (N words), by the gather rule"""
    p = np.asarray(p).astype(m.UINT[bits])
    n = p.shape[-1]
    assert t % 2 == 1 and 0 < t < 2 * n
    u = (np.arange(n) * pow(t, -1, 2 * n)) % (2 * n)
    with np.errstate(over="ignore"):
        return np.where(u < n, p[..., u % n], (0 - p[..., u % n]).astype(m.UINT[bits])).astype(m.UINT[bits])


def sigma_direct(p, t: int, bits: int) -> np.ndarray:
    """p(X^t) mod X^N + 1 evaluated term by term: coefficient j goes to j t mod 2N, negated past N"""
    p = [int(v) for v in p]
    n, mod = len(p), 1 << bits
    out = [0] * n
    for j, v in enumerate(p):
        e = (j * t) % (2 * n)
        out[e % n] = (out[e % n] + (v if e < n else -v)) % mod
    return np.array(out, dtype=np.uint64).astype(m.UINT[bits])


# ---------------- rules 1 and 2 ----------------

def key_len(basis: m.ApproxSignedBasis, log_n: int, k: int) -> int:
    return k * basis.decompose_length * ((k + 1) << log_n)


def pad_key(key, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """the key of k ell rows as a key of (k+1) ell rows: ell all-zero body rows behind it (torus or Fourier form)"""
    key = np.asarray(key).reshape(-1)
    assert key.size == key_len(basis, log_n, k)
    return np.concatenate([key, np.zeros(basis.decompose_length * ((k + 1) << log_n), key.dtype)])


def automorphism(ct, key, t: int, product, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """rule 1 on a batch of ciphertexts against one key"""
    bits, n = basis.bits, 1 << log_n
    x = np.asarray(ct).astype(m.UINT[bits]).reshape(-1, k + 1, n)
    full = pad_key(key, basis, log_n, k)
    out = np.empty_like(x)
    with np.errstate(over="ignore"):
        for e in range(x.shape[0]):
            s = sigma(x[e], t, bits)
            body = np.zeros_like(s)
            body[k] = s[k]
            out[e] = body - np.asarray(product(s.reshape(-1), full)).astype(m.UINT[bits]).reshape(k + 1, n)
    return out.reshape(-1)


def trace_exponents(log_n: int, steps=None):
    steps = log_n if steps is None else steps
    assert 1 <= steps <= log_n
    return [(1 << (log_n - s + 1)) + 1 for s in range(1, steps + 1)]


def trace_steps(ct, keys, steps: int, product, basis: m.ApproxSignedBasis, log_n: int, k: int):
    """rule 2 as its calls of rule 1: yields (s, t_s, ACC_{s-1}, key s-1, ACC_s)"""
    bits = basis.bits
    acc = np.asarray(ct).astype(m.UINT[bits]).reshape(-1)
    keys = np.asarray(keys).reshape(steps, -1)
    for s, t in enumerate(trace_exponents(log_n, steps), 1):
        with np.errstate(over="ignore"):
            nxt = (acc + automorphism(acc, keys[s - 1], t, product, basis, log_n, k)).astype(m.UINT[bits])
        yield s, t, acc, keys[s - 1], nxt
        acc = nxt


def trace(ct, keys, steps: int, product, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    out = None
    for *_, out in trace_steps(ct, keys, steps, product, basis, log_n, k):
        pass
    return out


# ---------------- rule 3 ----------------

def gksk(rand, key_in, key_out, exponents, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """the torus-form keys from the randomness in `rand` (len(exponents) x k ell GLWE rows); keys: k x N words"""
    bits, n, ell = basis.bits, 1 << log_n, basis.decompose_length
    out = kg.glwe_body_mac(rand, key_out, bits, log_n, k).astype(np.uint64).reshape(len(exponents), k, ell, k + 1, n).copy()
    z_in = np.asarray(key_in).astype(m.UINT[bits]).reshape(k, n)
    with np.errstate(over="ignore"):
        for x, t in enumerate(exponents):
            for j in range(k):
                msg = sigma(z_in[j], t, bits).astype(np.uint64)
                for l in range(ell):
                    out[x, j, l, k] += msg << np.uint64(basis.drop_bits + l * basis.log_basis)
    return out.reshape(-1).astype(m.UINT[bits])


def noise_free_gksk(key_in, key_out, exponents, basis: m.ApproxSignedBasis, log_n: int, k: int, rng) -> np.ndarray:
    rows = len(exponents) * k * basis.decompose_length
    return gksk(kg.glwe_randomness(rng, basis.bits, log_n, k, rows, 0), key_in, key_out, exponents, basis, log_n, k)


def to_fourier(torus, bits: int, log_n: int) -> np.ndarray:
    """write_fourier_form: polynomial after polynomial"""
    return m.FullComplex64FftTable(log_n).forward(np.asarray(torus).reshape(-1, 1 << log_n), bits).reshape(-1)


# ---------------- rule 4 ----------------

def embed(lwe, bits: int, log_n: int, k: int) -> np.ndarray:
    n = 1 << log_n
    x = np.asarray(lwe).astype(m.UINT[bits]).reshape(-1, k * n + 1)
    out = np.zeros((x.shape[0], k + 1, n), m.UINT[bits])
    a = x[:, :k * n].reshape(-1, k, n)
    with np.errstate(over="ignore"):
        out[:, :k, 0] = a[:, :, 0]
        out[:, :k, 1:] = (0 - a[:, :, :0:-1]).astype(m.UINT[bits])      # A_j[N - i] = -a[jN + i]
    out[:, k, 0] = x[:, k * n]
    return out.reshape(-1)


# ---------------- the bound on noisy keys ----------------

def f64_error(bits, log_n, k, lb, ell) -> float:
    """A priori size of the f64 product's error on one output word before rounding: an accumulator sums k ell N products of
    a digit (at most B/2) and a key word (at most 2^(BITS-1)); every butterfly level of the forward and of the inverse
    transform and the multiply-accumulate round at 2^-53 relative to such a sum: (2 log N + 2) roundings."""
    return k * ell * (1 << log_n) * 2.0 ** (lb - 1) * 2.0 ** (bits - 1) * 2.0 ** -53 * (2 * log_n + 2)


def ks_bound(bits, log_n, k, lb, ell, noise) -> float:
    """|coefficient of the phase of rule 1's output - sigma_t(phase of the input)| for binary keys and |e| <= noise on every
    key row:  k ell N (B/2) E  +  k N 2^(drop-1)  +  (1 + k N) (4 f64_error + 2).
    The phase of row (j, l) is g_l sigma(z_j) + e_{j,l}, and sum_l d_l g_l = sigma(A_j) - r_j with |r_j| <= 2^(drop-1) (0 at
    drop 0), so the output's phase is sigma(B) - sum_j sigma(A_j) sigma(z_j) + sum_j r_j sigma(z_j) - sum_{j,l} d_l e_{j,l}:
    k ell N digit-times-noise products of at most (B/2) E per coefficient, and k N rounding terms weighted by a key bit (the
    body is not decomposed).  The last term is the f64 arithmetic in the form of DESIGN section 19's allowance: each of the
    1 + k N words that meet in a phase coefficient is off by the product's f64 error and half a word of rounding."""
    basis = m.ApproxSignedBasis(bits, lb, ell)
    n = 1 << log_n
    half = 2.0 ** (basis.drop_bits - 1) if basis.drop_bits else 0.0
    return k * ell * n * 2.0 ** (lb - 1) * noise + k * n * half + (1 + k * n) * (4 * f64_error(bits, log_n, k, lb, ell) + 2)


def trace_bound(steps: int, e0: float, bits, log_n, k, lb, ell, noise) -> float:
    """|coefficient of the phase of the trace's output - its noise-free value| for an input whose phase is off by at most
    e0: e_s <= 2 e_{s-1} + ks_bound (ACC + sigma(ACC) doubles the error, the key switch adds its own), so
    e_m <= 2^m e0 + (2^m - 1) ks_bound"""
    return 2.0 ** steps * e0 + (2.0 ** steps - 1) * ks_bound(bits, log_n, k, lb, ell, noise)


# (bits, log_n, k, lb, ell, noise E): binary keys, an input LWE of a 1-bit message at Delta_in = 2^(BITS-2) / N
NOISY_SHAPES = [
    (32, 4, 1, 4, 8, 2),
    (64, 6, 1, 8, 5, 2 ** 20),
    (64, 5, 2, 8, 5, 2 ** 20),
]
