"""Reference model of the batched blind rotation (include/pfhe.h, pfhe_blindrot_*), shared by the CPU model test and the
GPU parity tests.

One step per ciphertext e, with its own exponent r = exps[e*n_steps+i] and the shared key BSK_i:
    D   = mul_monic_monomial(ACC, r) - ACC     (CrtGlwe::mul_monic_monomial_assign, sub_element_wise_assign)
    E   = coeff_form(mul_dcrt_ggsw_to(D, BSK_i))
    ACC = ACC + E
Built from the oracle's own restatements (orc.CrtPolyOps, orc.mul_dcrt_ggsw_to / mul_dcrt32_ggsw_to and the oracle
tables' inverse_transform_slice); the u32 rotate / subtract / add are exact integer operations done in numpy.
"""
import numpy as np

PLAINTEXT_BITS = 8


def rotate_np(x: np.ndarray, r: int, n: int, moduli) -> np.ndarray:
    """x * X^r (negacyclic: X^N = -1) for a flat array of RNS polynomials with moduli below 2^62 that fit int64 sums
    (the u32 words; modulus-major, L x N words per unit)."""
    L = len(moduli)
    polys = x.reshape(-1, L, n).astype(np.int64)
    q = np.array([int(m) for m in moduli], np.int64).reshape(1, L, 1)
    full = np.concatenate([polys, -polys], axis=2)  # one period of X^j * p: index N + j holds -p[j]
    return (np.roll(full, r % (2 * n), axis=2)[..., :n] % q).astype(x.dtype).reshape(-1)


def sub_np(a, b, moduli, n):
    q = np.repeat(np.array([int(m) for m in moduli], np.int64), n)
    q = np.tile(q, a.size // q.size)
    return ((a.astype(np.int64) - b.astype(np.int64)) % q).astype(a.dtype)


def add_np(a, b, moduli, n):
    q = np.repeat(np.array([int(m) for m in moduli], np.int64), n)
    q = np.tile(q, a.size // q.size)
    return ((a.astype(np.int64) + b.astype(np.int64)) % q).astype(a.dtype)


def oracle_rotate(orc, ot, ob, obasis, moduli, n, k, acc_e, bsk, exps_e):
    """The u64 composition for ONE ciphertext (acc_e: (k+1)*L*N words); returns the new accumulator."""
    ops = orc.CrtPolyOps(moduli, n)
    ggsw = bsk.size // len(exps_e) if len(exps_e) else 0
    acc = acc_e.copy()
    for i, r in enumerate(exps_e):
        rot = acc.copy()
        ops.mul_monomial_assign(rot, int(r))
        d = ops.sub_to(rot, acc)
        e = orc.mul_dcrt_ggsw_to(ot, ob, obasis, k, d, bsk[i * ggsw:(i + 1) * ggsw].copy())
        ot.inverse_transform_slice(e)
        acc = ops.add_to(acc, e)
    return acc


def oracle_rotate32(orc, ot, ob, obasis, moduli, n, k, acc_e, bsk, exps_e):
    """The u32 composition for ONE ciphertext: the oracle's product, numpy rotate / subtract / add."""
    ggsw = bsk.size // len(exps_e) if len(exps_e) else 0
    acc = acc_e.copy()
    for i, r in enumerate(exps_e):
        d = sub_np(rotate_np(acc, int(r), n, moduli), acc, moduli, n)
        e = orc.mul_dcrt32_ggsw_to(ot, ob, obasis, k, d, bsk[i * ggsw:(i + 1) * ggsw].copy())
        ot.inverse_transform_slice(e)
        acc = add_np(acc, e, moduli, n)
    return acc


def trivial_ggsw(scalars_residue, moduli, n, k, ell, s: int, dtype=np.uint64):
    """s * G as a trivially encrypted DcrtGgsw (rows x levels x components x L x N): row j, level l holds the constant
    s * g_l (constant in every NTT slot) in component j and zero elsewhere.  scalars_residue: [level][limb]."""
    L = len(moduli)
    out = np.zeros(((k + 1), ell, (k + 1), L, n), dtype=dtype)
    if s:
        for j in range(k + 1):
            for lv in range(ell):
                for li in range(L):
                    out[j, lv, j, li, :] = int(scalars_residue[lv * L + li]) % int(moduli[li])
    return out.reshape(-1)


def big_q(moduli):
    Q = 1
    for m in moduli:
        Q *= int(m)
    return Q


def trivial_acc(moduli, n, k, messages, dtype=np.uint64):
    """batch accumulators (0, ..., 0, TV) with TV = Delta * m, Delta = Q / 2^8 (messages: batch x N values < 2^8)."""
    L = len(moduli)
    delta = big_q(moduli) >> PLAINTEXT_BITS
    out = np.zeros((len(messages), k + 1, L, n), dtype=dtype)
    for e, m in enumerate(messages):
        for li, q in enumerate(moduli):
            out[e, k, li, :] = [(delta * int(v)) % int(q) for v in m]
    return out.reshape(-1)


def decode(acc_e, moduli, n, k):
    """(mask is all zero, round(body / Delta) mod 2^8 per coefficient) of one accumulator."""
    L = len(moduli)
    a = acc_e.reshape(k + 1, L, n)
    Q, delta = big_q(moduli), big_q(moduli) >> PLAINTEXT_BITS
    crt = [(Q // int(q)) * pow(Q // int(q), -1, int(q)) for q in moduli]
    body = []
    for c in range(n):
        x = sum(int(a[k, li, c]) * crt[li] for li in range(L)) % Q
        body.append(((x + delta // 2) // delta) % (1 << PLAINTEXT_BITS))
    return not a[:k].any(), body


def expected_decode(m, total, n):
    """coefficients of X^total * m (total mod 2N, negacyclic), negated wrap-arounds taken mod 2^8"""
    total %= 2 * n
    out = [0] * n
    for j, v in enumerate(m):
        d = j + total
        sign = -1 if (d // n) % 2 else 1
        out[d % n] = (sign * int(v)) % (1 << PLAINTEXT_BITS)
    return out


def special_exponents(rng, n, count):
    """0, 1, N-1, N, N+1, 2N-1 first, then random ones in [0, 2N)"""
    base = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    return np.array((base + [int(x) for x in rng.integers(0, 2 * n, max(0, count - len(base)))])[:count], np.uint32)
