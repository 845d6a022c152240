"""Reference model of the steps of a TFHE programmable bootstrap around the blind rotation (include/pfhe.h,
pfhe_tfhe{,32}_modswitch_dev, _sample_extract*, _keyswitch*, _bootstrap_*), shared by the CPU model test and the GPU parity
tests.  Built on tests/tfhe_fft_model.py and tests/tfhe_blindrot_model.py.

  - the modulus switch is the project's own rule (the reference has none): sw(w) = (((w >> (shift-1)) + 1) >> 1) & (2N-1),
    shift = BITS - log_n - 1;
  - sample extraction is Rlwe::extract_lwe_with_index (primus_lattice/src/rlwe/coeff.rs:194-227) per mask polynomial;
  - the key switch is a sequence of Lwe::add_mul_scalar_assign (lwe/single_message.rs:262-268) with the signed digits of
    the power-of-two ApproxSignedBasis, everything modulo 2^BITS;
  - the bootstrap composes them around tfhe_blindrot_model.exact_rotate (the product as the exact integer schoolbook).
An LWE ciphertext is a[0..dim) then b, b = <a,s> + e + m (lwe/single_message.rs:94-125).
"""
import numpy as np

import tfhe_blindrot_model as bm
import tfhe_fft_model as m


# ---------------- modulus switch ----------------

def sw(w: int, bits: int, log_n: int) -> int:
    """one word, in Python integers"""
    shift = bits - log_n - 1
    return (((int(w) >> (shift - 1)) + 1) >> 1) & ((2 << log_n) - 1)


def boundary_words(bits: int, log_n: int):
    """0, 1, all-ones, 2^(BITS-1), and m 2^shift +- 2^(shift-1) with its neighbours for several m (the ties and both
    sides of them), wrapped to the word"""
    shift = bits - log_n - 1
    words = {0, 1, (1 << bits) - 1, 1 << (bits - 1)}
    two_n = 2 << log_n
    for mm in sorted({0, 1, 2, 3, two_n // 2 - 1, two_n // 2, two_n - 2, two_n - 1}):
        for half in (-(1 << (shift - 1)), 1 << (shift - 1)):
            for d in (-2, -1, 0, 1, 2):
                words.add((mm * (1 << shift) + half + d) % (1 << bits))
    return sorted(words)


def modulus_switch(lwe: np.ndarray, n: int, bits: int, log_n: int):
    """(exps: batch x n, neg_b: batch) as uint32"""
    x = np.asarray(lwe).astype(np.uint64).reshape(-1, n + 1)
    shift, mask = np.uint64(bits - log_n - 1), np.uint64((2 << log_n) - 1)
    v = (((x >> (shift - np.uint64(1))) + np.uint64(1)) >> np.uint64(1)) & mask
    neg_b = (np.uint64(2 << log_n) - v[:, n]) & mask
    return v[:, :n].astype(np.uint32), neg_b.astype(np.uint32)


# ---------------- sample extraction ----------------

def sample_extract(glwe: np.ndarray, log_n: int, k: int, h: int) -> np.ndarray:
    """batch GLWE ciphertexts ((k+1) x N words each) -> batch LWE ciphertexts of k N + 1 words"""
    n = 1 << log_n
    g = np.asarray(glwe).reshape(-1, k + 1, n)
    out = np.zeros((g.shape[0], k * n + 1), g.dtype)
    i = np.arange(n)
    with np.errstate(over="ignore"):
        for j in range(k):
            a = g[:, j]
            out[:, j * n:(j + 1) * n] = np.where(i <= h, a[:, (h - i) % n], (0 - a[:, (n + h - i) % n]).astype(g.dtype))
    out[:, k * n] = g[:, k, h]
    return out.reshape(-1)


def flatten_key(z: np.ndarray) -> np.ndarray:
    """the LWE key of an extracted sample: the k GLWE key polynomials end to end"""
    return np.asarray(z).reshape(-1)


def glwe_phase(glwe_e: np.ndarray, z: np.ndarray, bits: int, log_n: int, k: int) -> np.ndarray:
    """B - sum_j A_j z_j (negacyclic) of ONE ciphertext, N words; z: k x N small key polynomials"""
    n = 1 << log_n
    g = np.asarray(glwe_e).reshape(k + 1, n).astype(np.uint64)
    ph = g[k].copy()
    with np.errstate(over="ignore"):
        for j in range(k):
            ph -= m.negacyclic_u64(np.asarray(z[j]).astype(np.uint64), g[j])
    return ph.astype(m.UINT[bits])


def lwe_phase(lwe: np.ndarray, s: np.ndarray, bits: int) -> np.ndarray:
    """b - <a,s> per ciphertext of a batch"""
    dim = len(s)
    x = np.asarray(lwe).astype(np.uint64).reshape(-1, dim + 1)
    with np.errstate(over="ignore"):
        return (x[:, dim] - x[:, :dim] @ np.asarray(s).astype(np.uint64)).astype(m.UINT[bits])


# ---------------- key switch ----------------

def keyswitch(lwe_in: np.ndarray, ksk: np.ndarray, in_dim: int, out_dim: int, basis: m.ApproxSignedBasis) -> np.ndarray:
    """out[e][c] = [c == out_dim] b_e - sum_i sum_j d_{e,i,j} ksk[(i ell + j)(out_dim + 1) + c] modulo 2^BITS"""
    bits, ell = basis.bits, basis.decompose_length
    x = np.asarray(lwe_in).astype(m.UINT[bits]).reshape(-1, in_dim + 1)
    key = np.asarray(ksk).astype(np.uint64).reshape(in_dim * ell, out_dim + 1)
    digits = np.stack(basis.digits(x[:, :in_dim]), axis=-1)                 # batch x in_dim x ell, signed int64
    d = digits.reshape(x.shape[0], in_dim * ell).view(np.uint64)
    with np.errstate(over="ignore"):
        out = (0 - d @ key).astype(np.uint64)
        out[:, out_dim] += x[:, in_dim].astype(np.uint64)
    return out.astype(m.UINT[bits]).reshape(-1)


def noise_free_ksk(s_in: np.ndarray, s_out: np.ndarray, basis: m.ApproxSignedBasis, rng) -> np.ndarray:
    """row (i, j): a uniformly random mask and b = <a, s_out> + s_in[i] * 2^(drop_bits + j log_basis)"""
    bits, ell = basis.bits, basis.decompose_length
    rows = len(s_in) * ell
    a = rng.integers(0, 2 ** bits, (rows, len(s_out)), dtype=np.uint64)
    scale = np.array([1 << (basis.drop_bits + j * basis.log_basis) for j in range(ell)], np.uint64)
    with np.errstate(over="ignore"):
        msg = (np.asarray(s_in).astype(np.uint64)[:, None] * scale[None, :]).reshape(rows)
        b = a @ np.asarray(s_out).astype(np.uint64) + msg
    return np.concatenate([a, b[:, None]], axis=1).astype(m.UINT[bits]).reshape(-1)


# ---------------- the whole bootstrap ----------------

def bootstrap(lwe_in, keys_coeff, tv, ksk, basis: m.ApproxSignedBasis, ks_basis, log_n: int, k: int, n: int,
              rotate=bm.exact_rotate) -> np.ndarray:
    """modulus switch, ACC = X^{neg_b} TV, exact_rotate over the n coefficient-domain keys, extraction at index 0 and,
    when ksk is not None, the key switch from k N to n.  tv: (k+1) N words shared by the batch, or one per ciphertext.
    rotate(acc_e, keys_coeff, exps_e, basis, log_n, k) is the rotation of one ciphertext: another one (a closure over
    tfhe_multibit_model.exact_rotate_loop and its grouping factor) models the handle over the multi-bit rotation."""
    bits, big_n = basis.bits, 1 << log_n
    glwe = (k + 1) * big_n
    exps, neg_b = modulus_switch(lwe_in, n, bits, log_n)
    tv = np.asarray(tv).astype(m.UINT[bits])
    accs = []
    for e in range(exps.shape[0]):
        t = tv if tv.size == glwe else tv[e * glwe:(e + 1) * glwe]
        accs.append(rotate(bm.rotate(t, int(neg_b[e]), big_n), keys_coeff, exps[e], basis, log_n, k))
    lwe = sample_extract(np.concatenate(accs), log_n, k, 0)
    return lwe if ksk is None else keyswitch(lwe, ksk, k * big_n, n, ks_basis)


def lwe_encrypt(values: np.ndarray, s: np.ndarray, bits: int, rng) -> np.ndarray:
    """noise-free LWE ciphertexts of the torus words `values` under the binary key s, uniformly random masks"""
    a = rng.integers(0, 2 ** bits, (len(values), len(s)), dtype=np.uint64)
    with np.errstate(over="ignore"):
        b = a @ np.asarray(s).astype(np.uint64) + np.asarray(values).astype(np.uint64)
    return np.concatenate([a, b[:, None]], axis=1).astype(m.UINT[bits]).reshape(-1)


def lut_test_vector(f, p: int, bits: int, log_n: int, k: int) -> np.ndarray:
    """the half-box-shifted LUT of f on p-bit messages under one padding bit, trivially encrypted: (0, ..., 0, tv) with
    tv[j] = Delta f(floor((j + N/2^(p+1)) 2^p / N)), and -Delta f(0) on the last half box, which wraps negacyclically"""
    n = 1 << log_n
    box = n >> p
    assert box >= 2
    delta = 1 << (bits - p - 1)
    tv = np.zeros((k + 1, n), m.UINT[bits])
    for j in range(n):
        idx = (j + box // 2) // box
        v = delta * f(idx) if idx < (1 << p) else -delta * f(0)
        tv[k, j] = v % (1 << bits)
    return tv.reshape(-1)


def decode(phases: np.ndarray, p: int, bits: int):
    """round(phase / Delta) modulo 2^(p+1)"""
    shift = bits - p - 1
    return [((int(v) + (1 << (shift - 1))) >> shift) % (2 << p) for v in phases]


def lut(p):
    return lambda v: (3 * v + 1) % (1 << p)


def meaning_case(bits, log_n, p, n, k, lb, ell, ks_lb, ks_ell, seed, repeats):
    """every p-bit message `repeats` times under fresh masks; trivial bootstrapping keys, a noise-free key-switch key"""
    big_n = 1 << log_n
    # the switched phase is off by at most (n + 1) / 2 (one half per rounded word); it stays inside the message's box of
    # N / 2^p exponents, centred by the half-box shift, as long as that is below half a box
    assert (n + 1) / 2 < big_n / 2 ** (p + 1)
    basis, ks_basis = m.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, ks_lb, ks_ell)
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, n)
    s[0] = 1
    z = rng.integers(0, 2, (k, big_n))
    msgs = np.tile(np.arange(1 << p), repeats)
    delta = 1 << (bits - p - 1)
    lwe = lwe_encrypt(msgs.astype(np.uint64) * np.uint64(delta), s, bits, rng)
    keys = [bm.trivial_ggsw(basis, log_n, k, int(si)) for si in s]
    tv = lut_test_vector(lut(p), p, bits, log_n, k)
    ksk = noise_free_ksk(flatten_key(z), s, ks_basis, rng)
    return dict(basis=basis, ks_basis=ks_basis, s=s, z=z, msgs=msgs, lwe=lwe, keys=keys, tv=tv, ksk=ksk)
