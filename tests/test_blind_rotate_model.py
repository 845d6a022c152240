"""CPU check of the reference model the GPU blind-rotation tests rely on (tests/blindrot_model.py): the oracle composition
monomial -> subtract -> external product -> coefficient form -> add, run with trivially encrypted keys BSK_i = s_i * G,
decodes to X^{sum_i exps_i * s_i} * m.  A wrong model (sign of the wrap-around, exponent order, key layout) cannot then make
the GPU parity tests pass."""
import numpy as np
import pytest

import blindrot_model as bm
from pyref import Q61

Q30 = [1073479681, 1071513601, 1070727169]


@pytest.mark.parametrize("moduli,log_basis", [(Q61, 30), (Q61[:1], 10)])
def test_trivial_keys_rotate_the_test_vector(orc, moduli, log_basis):
    log_n, k, n_steps, batch = 10, 1, 4, 2
    n = 1 << log_n
    rng = np.random.default_rng(log_basis)
    ot, ob = orc.U64DcrtTable(log_n, moduli), orc.RNSBase(moduli)
    obasis = orc.BigUintApproxSignedBasis(ob, log_basis)
    ell = obasis.decompose_length
    secret = [int(x) for x in rng.integers(0, 2, n_steps)]
    secret[0] = 1  # at least one key that rotates
    bsk = np.concatenate([bm.trivial_ggsw(obasis.scalars_residue, moduli, n, k, ell, s) for s in secret])
    msgs = [rng.integers(0, 256, n) for _ in range(batch)]
    acc = bm.trivial_acc(moduli, n, k, msgs)
    exps = np.concatenate([bm.special_exponents(rng, n, n_steps), rng.integers(0, 2 * n, n_steps).astype(np.uint32)])
    W = (k + 1) * len(moduli) * n
    for e in range(batch):
        ex = exps[e * n_steps:(e + 1) * n_steps]
        out = bm.oracle_rotate(orc, ot, ob, obasis, moduli, n, k, acc[e * W:(e + 1) * W], bsk, ex)
        mask_zero, body = bm.decode(out, moduli, n, k)
        assert mask_zero
        assert body == bm.expected_decode(msgs[e], sum(int(r) * s for r, s in zip(ex, secret)), n)


def test_trivial_keys_u32(orc):
    log_n, k, n_steps = 10, 1, 3
    n = 1 << log_n
    rng = np.random.default_rng(7)
    ot, ob = orc.U32DcrtTable(log_n, Q30), orc.RNSBase32(Q30)
    obasis = orc.BigUintApproxSignedBasis32(ob, 15)
    ell = obasis.decompose_length
    secret = [1, 0, 1]
    bsk = np.concatenate([bm.trivial_ggsw(obasis.scalars_residue, Q30, n, k, ell, s, np.uint32) for s in secret])
    m = rng.integers(0, 256, n)
    acc = bm.trivial_acc(Q30, n, k, [m], np.uint32)
    ex = bm.special_exponents(rng, n, 6)[3:]  # N, N+1, 2N-1
    out = bm.oracle_rotate32(orc, ot, ob, obasis, Q30, n, k, acc, bsk, ex)
    mask_zero, body = bm.decode(out, Q30, n, k)
    assert mask_zero
    assert body == bm.expected_decode(m, sum(int(r) * s for r, s in zip(ex, secret)), n)


def test_numpy_rotation_matches_the_oracle(orc):
    """the u32 tests' numpy X^r equals the oracle's mul_monomial_assign on the same words"""
    n, moduli = 64, Q30
    rng = np.random.default_rng(3)
    ops = orc.CrtPolyOps(moduli, n)
    x = np.concatenate([rng.integers(0, q, n, dtype=np.uint64) for _ in range(2) for q in moduli])
    for r in bm.special_exponents(rng, n, 10):
        want = x.copy()
        ops.mul_monomial_assign(want, int(r))
        assert np.array_equal(bm.rotate_np(x.astype(np.uint32), int(r), n, moduli), want.astype(np.uint32))
