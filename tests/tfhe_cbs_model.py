"""Reference model of the circuit bootstrap on the torus side (include/pfhe.h, pfhe_tfhe{,32}_private_keyswitch*,
_pfksk_generate_dev, _cbs_*), shared by the CPU model test and the GPU parity tests.  Exact, wrapping numpy; built on
tests/tfhe_fft_model.py, tests/tfhe_blindrot_model.py, tests/tfhe_bootstrap_model.py and tests/tfhe_keygen_model.py.

Conventions: the phase is b - <a,s>; g_l = 2^(drop_bits + l log_basis), levels least significant first; a torus-form GGSW
is [(k+1) rows r][ell levels l][(k+1) components][N]; row (r, l) of a GGSW of m is a GLWE ciphertext of f_r(m g_l) with
f_r(x) = -z_r x for r < k and x on coefficient 0 for r = k.

  - private_keyswitch: out[e][u][l] = - sum_{j <= in_dim} sum_t d_t(c_{e,l,j}) PFKSK[u][j][t] modulo 2^BITS, c = (a, b): the
    body word is decomposed as one more mask word (its key is -1), the digits those of ApproxSignedBasis.digits;
  - generate_pfksk: the GLWE body call on every row, then s'_j g_t on coefficient 0 of the body of row (k, j, t) and
    -s'_j g_t z_u[i] on every body coefficient of row (u, j, t), u < k, with s' = (key_in, -1);
  - circuit_bootstrap: per input e and level l of cbs_basis, the modulus switch of (a, b + 2^(BITS-2)), ACC = X^{neg_b} TV_l
    with TV_l = (0, .., 0, -g_l/2 on every coefficient), tfhe_blindrot_model.exact_rotate, extraction at index 0, g_l/2
    added to the body, and private_keyswitch with levels = ell_cb and in_dim = k N.
"""
import numpy as np

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_ks_shapes as ks


# ---------------- rule 1: the private functional key switch ----------------

def private_keyswitch(lwe_in, pfksk, in_dim: int, levels: int, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """batch x levels x (in_dim + 1) words -> batch x (k + 1) x levels x (k + 1) N words"""
    bits, ell, cols = basis.bits, basis.decompose_length, (k + 1) << log_n
    x = np.asarray(lwe_in).astype(m.UINT[bits]).reshape(-1, levels, in_dim + 1)
    key = np.asarray(pfksk).astype(np.uint64).reshape(k + 1, (in_dim + 1) * ell, cols)
    digits = np.stack(basis.digits(x), axis=-1)                              # batch x levels x (in_dim + 1) x ell, signed
    d = digits.reshape(x.shape[0], levels, (in_dim + 1) * ell).astype(np.int64).view(np.uint64)
    out = np.zeros((x.shape[0], k + 1, levels, cols), np.uint64)
    with np.errstate(over="ignore"):
        for u in range(k + 1):
            out[:, u] = 0 - d @ key[u]
    return out.astype(m.UINT[bits]).reshape(-1)


def gadget(basis: m.ApproxSignedBasis) -> np.ndarray:
    """g_t as uint64 words (of the basis's width)"""
    return np.array([(1 << (basis.drop_bits + t * basis.log_basis)) % (1 << basis.bits)
                     for t in range(basis.decompose_length)], np.uint64)


def rounded_words(words, basis: m.ApproxSignedBasis) -> np.ndarray:
    """sum_t d_t(w) g_t modulo 2^BITS: the word as the decomposition sees it"""
    g = gadget(basis)
    with np.errstate(over="ignore"):
        return sum(d.astype(np.int64).view(np.uint64) * g[t] for t, d in enumerate(basis.digits(np.asarray(words))))


def rounded_phase(lwe_in, s, basis: m.ApproxSignedBasis) -> np.ndarray:
    """phi~ = sum_t d_t(b) g_t - sum_j s_j sum_t d_t(a_j) g_t per ciphertext, as words of the basis's width"""
    dim = len(s)
    r = rounded_words(np.asarray(lwe_in).astype(m.UINT[basis.bits]).reshape(-1, dim + 1), basis)
    with np.errstate(over="ignore"):
        return (r[:, dim] - r[:, :dim] @ np.asarray(s).astype(np.uint64)).astype(m.UINT[basis.bits])


def f_row(u: int, x: int, z, bits: int, log_n: int, k: int) -> np.ndarray:
    """f_u(x) as N words: -z_u x for u < k, x on coefficient 0 for u = k"""
    n = 1 << log_n
    with np.errstate(over="ignore"):
        if u == k:
            out = np.zeros(n, np.uint64)
            out[0] = np.uint64(int(x) % (1 << 64))
        else:
            out = 0 - np.asarray(z).astype(np.uint64).reshape(k, n)[u] * np.uint64(int(x) % (1 << 64))
    return out.astype(m.UINT[bits])


# ---------------- rule 2: its key ----------------

def pfksk_messages(key_in, z, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """the message polynomials of the rows, (k + 1) x (in_dim + 1) x ell x N words: f_u(s'_j g_t)"""
    n, ell, in_dim = 1 << log_n, basis.decompose_length, len(key_in)
    sp = np.concatenate([np.asarray(key_in).astype(np.uint64), np.array([2 ** 64 - 1], np.uint64)])     # s' = (s, -1)
    zz = np.asarray(z).astype(np.uint64).reshape(k, n)
    with np.errstate(over="ignore"):
        scal = sp[:, None] * gadget(basis)[None, :]                          # (in_dim + 1) x ell
        msg = np.zeros((k + 1, in_dim + 1, ell, n), np.uint64)
        msg[k, :, :, 0] = scal
        for u in range(k):
            msg[u] = 0 - scal[:, :, None] * zz[u][None, None, :]
    return msg


def generate_pfksk(rand, key_in, z, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """rand holds the randomness of (k + 1) x (in_dim + 1) x ell GLWE rows; every row gets B += sum_r A_r z_r and its message"""
    bits, ell, n = basis.bits, basis.decompose_length, 1 << log_n
    out = kg.glwe_body_mac(rand, z, bits, log_n, k).astype(np.uint64).reshape(k + 1, len(key_in) + 1, ell, k + 1, n)
    with np.errstate(over="ignore"):
        out[:, :, :, k, :] += pfksk_messages(key_in, z, basis, log_n, k)
    return out.astype(m.UINT[bits]).reshape(-1)


def noise_free_pfksk(key_in, z, basis: m.ApproxSignedBasis, log_n: int, k: int, rng) -> np.ndarray:
    """uniform masks, bodies without noise"""
    rows = (k + 1) * (len(key_in) + 1) * basis.decompose_length
    return generate_pfksk(kg.glwe_randomness(rng, basis.bits, log_n, k, rows, 0), key_in, z, basis, log_n, k)


# ---------------- rule 3: the circuit bootstrap ----------------

def offset_inputs(lwe_in, n: int, bits: int) -> np.ndarray:
    """(a, b + 2^(BITS-2)): what the modulus switch sees"""
    x = np.asarray(lwe_in).astype(m.UINT[bits]).reshape(-1, n + 1).copy()
    with np.errstate(over="ignore"):
        x[:, n] += m.UINT[bits](1 << (bits - 2))
    return x.reshape(-1)


def half_gadget(cbs_basis: m.ApproxSignedBasis, level: int) -> int:
    assert cbs_basis.drop_bits >= 1, "g_l / 2 must be a word"
    return 1 << (cbs_basis.drop_bits + level * cbs_basis.log_basis - 1)


def level_test_vector(cbs_basis: m.ApproxSignedBasis, level: int, log_n: int, k: int) -> np.ndarray:
    """TV_l: the trivial GLWE whose body has -g_l/2 on every coefficient"""
    tv = np.zeros((k + 1, 1 << log_n), m.UINT[cbs_basis.bits])
    tv[k] = (-half_gadget(cbs_basis, level)) % (1 << cbs_basis.bits)
    return tv.reshape(-1)


def extracted(lwe_in, keys_coeff, basis, cbs_basis, log_n: int, k: int, n: int) -> np.ndarray:
    """stages 1-4: batch x ell_cb LWE ciphertexts of k N + 1 words whose phase is m g_l plus the rotation's noise"""
    bits, big_n, levels = basis.bits, 1 << log_n, cbs_basis.decompose_length
    exps, neg_b = bs.modulus_switch(offset_inputs(lwe_in, n, bits), n, bits, log_n)
    accs = []
    for e in range(exps.shape[0]):
        for l in range(levels):
            acc = bm.rotate(level_test_vector(cbs_basis, l, log_n, k), int(neg_b[e]), big_n)
            accs.append(bm.exact_rotate(acc, keys_coeff, exps[e], basis, log_n, k))
    lwe = bs.sample_extract(np.concatenate(accs), log_n, k, 0).reshape(-1, levels, k * big_n + 1)
    with np.errstate(over="ignore"):
        for l in range(levels):
            lwe[:, l, k * big_n] += m.UINT[bits](half_gadget(cbs_basis, l))
    return lwe.reshape(-1)


def circuit_bootstrap(lwe_in, keys_coeff, pfksk, basis, cbs_basis, pfks_basis, log_n: int, k: int, n: int) -> np.ndarray:
    """batch x (n + 1) words -> batch torus-form GGSWs in cbs_basis, (k + 1) x ell_cb x (k + 1) x N words each"""
    lwe = extracted(lwe_in, keys_coeff, basis, cbs_basis, log_n, k, n)
    return private_keyswitch(lwe, pfksk, k << log_n, cbs_basis.decompose_length, pfks_basis, log_n, k)


def ggsw_row_phases(ggsw, z, bits: int, log_n: int, k: int) -> np.ndarray:
    """the phase polynomial of every GLWE row of a flat array of rows: rows x N words"""
    rows = np.asarray(ggsw).reshape(-1, (k + 1) << log_n)
    return np.stack([bs.glwe_phase(r, np.asarray(z).reshape(k, -1), bits, log_n, k) for r in rows])


def expected_row_phases(msgs, z, cbs_basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """f_r(m g_l) for every input, row and level, in the order of the output's rows"""
    g = gadget(cbs_basis)
    return np.stack([f_row(r, int(msg) * int(g[l]), z, cbs_basis.bits, log_n, k)
                     for msg in msgs for r in range(k + 1) for l in range(cbs_basis.decompose_length)])


# ---------------- the bounds on noisy keys ----------------

def row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell) -> float:
    """|coefficient of the phase of row (r, l) - f_r(m g_l)| for binary keys and |e| <= noise on every row of both keys:

        n step_bound(rotation basis, E) + (k N + 1) ell_pf (B_pf / 2) E + (k N + 1) 2^(drop_pf - 1)

    The accumulator starts as a trivial ciphertext, so the extracted phase is m g_l + e_rot exactly, with |e_rot| at most n
    times tfhe_keygen_model.step_bound (one rotation step's worst case, at any coefficient).  The key switch sees every one
    of the k N + 1 words (body included) rounded to a multiple of 2^drop_pf, each off by at most 2^(drop_pf - 1) and each
    weighted by a key word of magnitude at most 1 (a key bit, or the -1 of the body): phi~ = m g_l + e_rot + e_round.  Row u
    then holds f_u(phi~) plus sum_j sum_t d_t e_{u,j,t}: (k N + 1) ell_pf digits of magnitude at most B_pf / 2 against row
    noises of at most E, per coefficient.  f_k leaves the scalar error on coefficient 0; f_u, u < k, multiplies it by one
    key bit per coefficient: the same expression holds for every row.  The last term is 0 at drop_pf 0."""
    pf = m.ApproxSignedBasis(bits, pf_lb, pf_ell)
    words = k * (1 << log_n) + 1
    half = 2.0 ** (pf.drop_bits - 1) if pf.drop_bits else 0.0
    return n * kg.step_bound(bits, log_n, k, lb, ell, noise) + words * pf.decompose_length * 2.0 ** (pf_lb - 1) * noise + \
        words * half


def product_bound(bits, log_n, k, cb_lb, cb_ell, row_noise) -> float:
    """|coefficient of the phase of d0 + (d1 - d0) (x) GGSW - d_m| for noise-free d0, d1: one product step on cbs_basis
    against rows that are off by at most row_noise, which is tfhe_keygen_model.step_bound with that noise (the digits of
    d1 - d0 against the rows' errors, and the rounding of the decomposition, once on the body and once per key bit)"""
    return kg.step_bound(bits, log_n, k, cb_lb, cb_ell, row_noise)


# (bits, log_n, k, n, rotation lb, ell, noise E, pfks lb, ell, cbs lb, ell, p)
NOISY_CASES = [
    (32, 4, 1, 4, 8, 4, 4, 4, 8, 4, 2, 1),
    (64, 6, 1, 8, 15, 2, 2 ** 20, 8, 5, 4, 3, 1),
    (64, 5, 2, 6, 15, 2, 2 ** 20, 8, 5, 4, 3, 1),
]


def noisy_case(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, p, seed):
    """Binary keys, the randomness of both generated keys (|e| <= noise on every row), both bits twice as noise-free
    inputs m 2^(BITS-1), and two noise-free GLWE ciphertexts d0, d1 of p-bit messages under one padding bit"""
    big_n = 1 << log_n
    basis = m.ApproxSignedBasis(bits, lb, ell)
    pfks_basis, cbs_basis = m.ApproxSignedBasis(bits, pf_lb, pf_ell), m.ApproxSignedBasis(bits, cb_lb, cb_ell)
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, n).astype(m.UINT[bits])
    z = rng.integers(0, 2, (k, big_n)).astype(m.UINT[bits])
    rand_bsk = kg.glwe_randomness(rng, bits, log_n, k, n * (k + 1) * ell, noise)
    rand_pfksk = kg.glwe_randomness(rng, bits, log_n, k, (k + 1) * (k * big_n + 1) * pf_ell, noise)
    msgs = np.array([0, 1, 1, 0])
    lwe = bs.lwe_encrypt(msgs.astype(np.uint64) << np.uint64(bits - 1), s, bits, rng)
    delta = 1 << (bits - p - 1)
    data = rng.integers(0, 1 << p, (2, big_n))
    glwe = kg.glwe_randomness(rng, bits, log_n, k, 2, 0).reshape(2, k + 1, big_n)
    with np.errstate(over="ignore"):
        glwe[:, k] += (data.astype(np.uint64) * np.uint64(delta)).astype(m.UINT[bits])
    return dict(basis=basis, pfks_basis=pfks_basis, cbs_basis=cbs_basis, s=s, z=z, rand_bsk=rand_bsk, rand_pfksk=rand_pfksk,
                msgs=msgs, lwe=lwe, delta=delta, data=data, glwe_rand=glwe.reshape(-1))


# ---------------- the shapes at which the key switch's tiling takes its other paths ----------------

# The tile is the LWE key switch's (tests/tfhe_ks_shapes.py), walked over in_dim + 1 words: the body is decomposed too.
PF_UNROLL = ks.KS_UNROLL            # key rows in flight
PF_TILE_ROWS = ks.KS_TILE_BATCH     # input ciphertexts (batch x levels) of one workgroup
PF_TILE_COLS = ks.KS_TILE_COLS      # output columns of one workgroup, two per lane 64 apart

# bits, in_dim, log_n, k, log_basis, ell, levels, batch                 what it reaches
PFKS_EDGE_SHAPES = [
    (32, 12, 6, 1, 4, 3, 1, 33),      # rows 24, 15; 128 columns exactly; two batch tiles
    (32, 2, 1, 1, 5, 5, 1, 31),       # 4 columns
    (32, 1, 1, 1, 4, 1, 1, 1),        # 2 rows: the unrolled loop never runs
    (32, 16, 6, 2, 6, 5, 3, 11),      # rows 40, 40, 5; 192 columns; M = 33; three key blocks
    (64, 18, 7, 1, 9, 7, 2, 1),       # rows 56, 56, 21
    (64, 10, 5, 2, 5, 9, 4, 8),       # ki = 7; rows 63, 36; M = 32 exactly; 96 columns
    (64, 4, 8, 1, 1, 33, 1, 9),       # ki = 1
    (64, 6, 2, 3, 3, 17, 2, 3),       # four key blocks; 16 columns
]


group_words = ks.group_words           # ki: input words per group


def group_rows(in_dim: int, ell: int):
    """key rows of every group, in the order the kernel walks them; the body is word in_dim"""
    return ks.group_rows(in_dim + 1, ell)
