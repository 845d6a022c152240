"""Batched blind rotation over the RNS external product (include/pfhe.h, pfhe_blindrot_* / pfhe_blindrot32_*) and the
per-ciphertext monomial product (pfhe_dcrt*_mul_monomial_each_to_dev), checked bit-exactly against the oracle composition
of tests/blindrot_model.py (whose meaning tests/test_blind_rotate_model.py checks on the CPU)."""
import os
import threading

import numpy as np
import pytest

import blindrot_model as bm
from gpu_util import rand_rns, to_dev, to_host
from pyref import Q61

pytestmark = pytest.mark.gpu

Q30 = [1073479681, 1071513601, 1070727169]
GENERIC = [1125899906826241, 562949953392641]  # not pseudo-Mersenne: the table's Montgomery / Shoup arithmetic


@pytest.fixture(scope="module")
def pf():
    import primus_fhe_amd as p
    return p


def exps_dev(exps: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(exps, np.uint32).view(np.int32)).cuda()


def rand32(rng, moduli, n, batch=1):
    return np.concatenate([rng.integers(0, q, n, dtype=np.uint64).astype(np.uint32) for _ in range(batch) for q in moduli])


def to_dev32(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def to_host32(t) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint32)


def make_exps(rng, n, batch, n_steps):
    """batch x n_steps exponents; the first ones are 0, 1, N-1, N, N+1, 2N-1"""
    return bm.special_exponents(rng, n, batch * n_steps)


def ctx64(pf, log_n, moduli, log_basis, chunk=0, plain=False):
    t, base = pf.U64DcrtTable(log_n, moduli), pf.RNSBase(moduli)
    if plain:
        os.environ["PFHE_DISABLE_FUSED_EXTPROD"] = "1"  # read when the handle's plan is created
    try:
        return pf.BlindRotateContext(t, base, pf.BigUintApproxSignedBasis(base, log_basis), 1, chunk)
    finally:
        os.environ.pop("PFHE_DISABLE_FUSED_EXTPROD", None)


def oracle64(orc, log_n, moduli, log_basis):
    ot, ob = orc.U64DcrtTable(log_n, moduli), orc.RNSBase(moduli)
    return ot, ob, orc.BigUintApproxSignedBasis(ob, log_basis)


def run_u64_case(pf, orc, log_n, moduli, log_basis, batch, n_steps, samples=None, seed=0):
    k, n, L = 1, 1 << log_n, len(moduli)
    rng = np.random.default_rng(seed + log_n + L)
    ctx = ctx64(pf, log_n, moduli, log_basis)
    G = ctx.ggsw_len()
    W = ctx.glwe_len()
    acc = rand_rns(rng, moduli, n, batch * (k + 1))
    bsk = rand_rns(rng, moduli, n, n_steps * G // (L * n))
    exps = make_exps(rng, n, batch, n_steps)
    dacc = to_dev(acc)
    pf.blind_rotate_dev(dacc, to_dev(bsk), exps_dev(exps), ctx)
    got = to_host(dacc)
    ot, ob, obasis = oracle64(orc, log_n, moduli, log_basis)
    for e in (range(batch) if samples is None else samples):
        want = bm.oracle_rotate(orc, ot, ob, obasis, moduli, n, k, acc[e * W:(e + 1) * W], bsk,
                                exps[e * n_steps:(e + 1) * n_steps])
        assert np.array_equal(got[e * W:(e + 1) * W], want), e
    return acc, bsk, exps, got


@pytest.mark.parametrize("log_n,moduli,log_basis,batch,n_steps", [
    (10, Q61, 30, 4, 3), (11, Q61, 30, 4, 3),      # small rings below the fused threshold: product + glue
    (12, Q61, 30, 2, 3), (16, Q61, 30, 2, 2),       # the two-pass product
    (10, GENERIC, 13, 3, 3),                       # generic primes
])
def test_oracle_parity_u64(pf, orc, log_n, moduli, log_basis, batch, n_steps):
    run_u64_case(pf, orc, log_n, moduli, log_basis, batch, n_steps)


@pytest.mark.parametrize("log_n,moduli,log_basis", [(10, Q61[:1], 10), (11, Q61[:2], 20), (10, GENERIC, 13)])
def test_small_ring_fused_rotation(pf, orc, log_n, moduli, log_basis):
    """>= 1024 (ciphertext, limb) pairs: two launches per step (digits of X^r ACC - ACC, product adding into ACC).  The whole
    batch equals a handle created under PFHE_DISABLE_FUSED_EXTPROD (product + glue kernel), sampled ciphertexts the
    oracle."""
    k, batch, n_steps = 1, 1100, 3
    n = 1 << log_n
    acc, bsk, exps, got = run_u64_case(pf, orc, log_n, moduli, log_basis, batch, n_steps, samples=(0, 1, 517, batch - 1))
    plain = ctx64(pf, log_n, moduli, log_basis, plain=True)
    dacc = to_dev(acc)
    pf.blind_rotate_dev(dacc, to_dev(bsk), exps_dev(exps), plain)
    assert np.array_equal(to_host(dacc), got)
    assert n == 1 << log_n and k == 1


@pytest.mark.parametrize("log_n,batch,n_steps", [(11, 3, 3), (16, 4, 2)])
def test_oracle_parity_u32(pf, orc, log_n, batch, n_steps):
    k, n, L, log_basis = 1, 1 << log_n, len(Q30), 15
    rng = np.random.default_rng(log_n)
    t, base = pf.U32DcrtTable(log_n, Q30), pf.RNSBase32(Q30)
    ctx = pf.BlindRotateContext32(t, base, pf.BigUintApproxSignedBasis32(base, log_basis), k)
    W, G = ctx.glwe_len(), ctx.ggsw_len()
    acc = rand32(rng, Q30, n, batch * (k + 1))
    bsk = rand32(rng, Q30, n, n_steps * G // (L * n))
    exps = make_exps(rng, n, batch, n_steps)
    dacc = to_dev32(acc)
    pf.blind_rotate_dev(dacc, to_dev32(bsk), exps_dev(exps), ctx)
    got = to_host32(dacc)
    ot, ob = orc.U32DcrtTable(log_n, Q30), orc.RNSBase32(Q30)
    obasis = orc.BigUintApproxSignedBasis32(ob, log_basis)
    for e in (0, batch - 1):
        want = bm.oracle_rotate32(orc, ot, ob, obasis, Q30, n, k, acc[e * W:(e + 1) * W], bsk,
                                  exps[e * n_steps:(e + 1) * n_steps])
        assert np.array_equal(got[e * W:(e + 1) * W], want), e


def test_trivial_keys_decode_u64(pf):
    """meaning: with BSK_i = s_i * G (trivial) the rotation takes (0, Delta*m) to (0, Delta * X^{sum exps_i s_i} * m)"""
    log_n, moduli, log_basis, k, batch, n_steps = 10, Q61, 30, 1, 3, 5
    n = 1 << log_n
    rng = np.random.default_rng(11)
    ctx = ctx64(pf, log_n, moduli, log_basis)
    ell = ctx.basis.decompose_length()
    sr = ctx.basis.scalars_residue()
    secret = [1, 0, 1, 1, 0]
    bsk = np.concatenate([bm.trivial_ggsw(sr, moduli, n, k, ell, s) for s in secret])
    msgs = [rng.integers(0, 256, n) for _ in range(batch)]
    acc = bm.trivial_acc(moduli, n, k, msgs)
    exps = make_exps(rng, n, batch, n_steps)
    dacc = to_dev(acc)
    pf.blind_rotate_dev(dacc, to_dev(bsk), exps_dev(exps), ctx)
    got, W = to_host(dacc), ctx.glwe_len()
    for e in range(batch):
        mask_zero, body = bm.decode(got[e * W:(e + 1) * W], moduli, n, k)
        assert mask_zero
        total = sum(int(r) * s for r, s in zip(exps[e * n_steps:(e + 1) * n_steps], secret))
        assert body == bm.expected_decode(msgs[e], total, n)


def test_trivial_keys_decode_u32(pf):
    log_n, k, batch, n_steps = 11, 1, 2, 4
    n = 1 << log_n
    rng = np.random.default_rng(12)
    t, base = pf.U32DcrtTable(log_n, Q30), pf.RNSBase32(Q30)
    basis = pf.BigUintApproxSignedBasis32(base, 15)
    ctx = pf.BlindRotateContext32(t, base, basis, k)
    sr, ell = basis.scalars_residue(), basis.decompose_length()
    secret = [0, 1, 1, 1]
    bsk = np.concatenate([bm.trivial_ggsw(sr, Q30, n, k, ell, s, np.uint32) for s in secret])
    msgs = [rng.integers(0, 256, n) for _ in range(batch)]
    acc = bm.trivial_acc(Q30, n, k, msgs, np.uint32)
    exps = make_exps(rng, n, batch, n_steps)
    pf.blind_rotate(acc, bsk, exps, ctx)  # the host form
    W = ctx.glwe_len()
    for e in range(batch):
        mask_zero, body = bm.decode(acc[e * W:(e + 1) * W], Q30, n, k)
        assert mask_zero
        total = sum(int(r) * s for r, s in zip(exps[e * n_steps:(e + 1) * n_steps], secret))
        assert body == bm.expected_decode(msgs[e], total, n)


def test_chunked_handle_equals_one_chunk(pf):
    log_n, moduli, log_basis, batch, n_steps = 11, Q61, 30, 7, 3
    n = 1 << log_n
    rng = np.random.default_rng(5)
    one, chunked = ctx64(pf, log_n, moduli, log_basis), ctx64(pf, log_n, moduli, log_basis, chunk=3)
    acc = rand_rns(rng, moduli, n, batch * 2)
    bsk = rand_rns(rng, moduli, n, n_steps * one.ggsw_len() // (len(moduli) * n))
    exps = make_exps(rng, n, batch, n_steps)
    a1, a2 = to_dev(acc), to_dev(acc)
    pf.blind_rotate_dev(a1, to_dev(bsk), exps_dev(exps), one)
    pf.blind_rotate_dev(a2, to_dev(bsk), exps_dev(exps), chunked)
    assert np.array_equal(to_host(a1), to_host(a2))
    assert not np.array_equal(to_host(a1), acc)


@pytest.mark.parametrize("log_n,batch", [(10, 3), (10, 1100), (12, 2)])
def test_one_step_equals_public_calls(pf, log_n, batch):
    """n_steps = 1 gives the words of the loop built from public calls: per-ciphertext monomial, sub_to, the product in
    coefficient form, add_to"""
    import torch
    moduli = Q61[:1] if batch > 1024 else Q61
    log_basis = 10 if batch > 1024 else 30
    n = 1 << log_n
    rng = np.random.default_rng(log_n + batch)
    t, base = pf.U64DcrtTable(log_n, moduli), pf.RNSBase(moduli)
    basis = pf.BigUintApproxSignedBasis(base, log_basis)
    ctx = pf.BlindRotateContext(t, base, basis, 1)
    prod = pf.DcrtGlevContext(t, base, basis, 1)
    acc = rand_rns(rng, moduli, n, batch * 2)
    bsk = rand_rns(rng, moduli, n, ctx.ggsw_len() // (len(moduli) * n))
    exps = rng.integers(0, 2 * n, batch).astype(np.uint32)
    dacc, dk, de = to_dev(acc), to_dev(bsk), exps_dev(exps)
    rot, d, e = torch.empty_like(dacc), torch.empty_like(dacc), torch.empty_like(dacc)
    t.mul_monomial_each_to_dev(dacc, de, 2, rot)
    t.sub_to_dev(rot, dacc, d)
    pf.mul_dcrt_ggsw_to_dev(d, dk, e, prod, into_coeff_form=True)
    want = torch.empty_like(dacc)
    t.add_to_dev(dacc, e, want)
    pf.blind_rotate_dev(dacc, dk, de, ctx)
    assert torch.equal(dacc, want)


@pytest.mark.parametrize("log_n,moduli,ppe", [(10, Q61, 2), (12, Q61[:2], 1)])
def test_monomial_each_matches_oracle(pf, orc, log_n, moduli, ppe):
    import torch
    n, L, elems = 1 << log_n, len(moduli), 8
    rng = np.random.default_rng(log_n)
    t = pf.U64DcrtTable(log_n, moduli)
    a = rand_rns(rng, moduli, n, elems * ppe)
    exps = bm.special_exponents(rng, n, elems)
    out = torch.empty(a.size, dtype=torch.int64, device="cuda")
    t.mul_monomial_each_to_dev(to_dev(a), exps_dev(exps), ppe, out)
    got = to_host(out)
    ops, U = orc.CrtPolyOps(moduli, n), ppe * L * n
    for e in range(elems):
        want = a[e * U:(e + 1) * U].copy()
        ops.mul_monomial_assign(want, int(exps[e]))
        assert np.array_equal(got[e * U:(e + 1) * U], want), e
    # the device form takes exponents modulo 2N
    t.mul_monomial_each_to_dev(to_dev(a), exps_dev(exps + np.uint32(2 * n)), ppe, out)
    assert np.array_equal(to_host(out), got)


def test_monomial_each_u32_matches_oracle(pf, orc):
    import torch
    log_n, ppe, elems = 11, 2, 8
    n, L = 1 << log_n, len(Q30)
    rng = np.random.default_rng(9)
    t = pf.U32DcrtTable(log_n, Q30)
    a = rand32(rng, Q30, n, elems * ppe)
    exps = bm.special_exponents(rng, n, elems)
    out = torch.empty(a.size, dtype=torch.int32, device="cuda")
    t.mul_monomial_each_to_dev(to_dev32(a), exps_dev(exps), ppe, out)
    got = to_host32(out)
    ops, U = orc.CrtPolyOps(Q30, n), ppe * L * n
    for e in range(elems):
        want = a[e * U:(e + 1) * U].astype(np.uint64)
        ops.mul_monomial_assign(want, int(exps[e]))
        assert np.array_equal(got[e * U:(e + 1) * U], want.astype(np.uint32)), e


@pytest.mark.parametrize("log_n,moduli,log_basis,batch", [(11, Q61, 30, 3), (10, Q61[:1], 10, 1100)])
def test_rotation_in_a_graph(pf, log_n, moduli, log_basis, batch):
    """one whole rotation captured in torch.cuda.graph (linear: one stream) and replayed on a fresh copy of ACC"""
    import torch
    n, n_steps = 1 << log_n, 4
    rng = np.random.default_rng(21)
    ctx = ctx64(pf, log_n, moduli, log_basis)
    acc = rand_rns(rng, moduli, n, batch * 2)
    dk = to_dev(rand_rns(rng, moduli, n, n_steps * ctx.ggsw_len() // (len(moduli) * n)))
    de = exps_dev(make_exps(rng, n, batch, n_steps))
    s = torch.cuda.Stream()
    work = to_dev(acc)
    with torch.cuda.stream(s):
        pf.blind_rotate_dev(work, dk, de, ctx, stream=s)  # eager reference
    s.synchronize()
    ref = work.clone()
    work.copy_(to_dev(acc))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pf.blind_rotate_dev(work, dk, de, ctx, stream=s)
    for _ in range(2):
        work.copy_(to_dev(acc))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(work, ref)


def test_errors(pf):
    import torch
    log_n, moduli = 10, Q61
    n = 1 << log_n
    rng = np.random.default_rng(1)
    ctx = ctx64(pf, log_n, moduli, 30)
    W, G = ctx.glwe_len(), ctx.ggsw_len()
    acc = rand_rns(rng, moduli, n, 2 * 2)
    bsk = rand_rns(rng, moduli, n, 2 * G // (len(moduli) * n))
    exps = np.zeros(4, np.uint32)
    dacc, dk = to_dev(acc), to_dev(bsk)
    for bad_acc, bad_k, bad_e in ((dacc[:W + 1], dk, exps), (dacc, dk[:G + 5], exps), (dacc, dk, exps[:3])):
        with pytest.raises(pf.PfheError) as e:
            pf.blind_rotate_dev(bad_acc, bad_k, exps_dev(bad_e), ctx)
        assert e.value.kind == "BadLength"
    host = acc.copy()
    with pytest.raises(pf.PfheError) as e:
        pf.blind_rotate(host, bsk, np.array([0, 1, 2 * n, 3], np.uint32), ctx)
    assert e.value.kind == "BadArgument"
    assert np.array_equal(host, acc)
    # n_steps == 0: no-op
    pf.blind_rotate_dev(dacc, dk[:0], exps_dev(exps[:0]), ctx)
    assert np.array_equal(to_host(dacc), acc)
    pf.blind_rotate(host, bsk[:0], exps[:0], ctx)
    assert np.array_equal(host, acc)
    torch.cuda.synchronize()


def test_second_thread_is_refused_while_a_call_holds_the_handle(pf):
    """one holder at a time: while a long host-form rotation runs on one thread, a call from another gets Busy"""
    log_n, moduli, n_steps, batch = 16, Q61, 8, 4
    n = 1 << log_n
    rng = np.random.default_rng(2)
    ctx = ctx64(pf, log_n, moduli, 30)
    acc = rand_rns(rng, moduli, n, batch * 2)
    bsk = rand_rns(rng, moduli, n, n_steps * ctx.ggsw_len() // (len(moduli) * n))
    exps = rng.integers(0, 2 * n, batch * n_steps).astype(np.uint32)
    small = to_dev(rand_rns(rng, moduli, n, 2))
    done, seen = threading.Event(), []

    def long_call():
        try:
            pf.blind_rotate(acc, bsk, exps, ctx)
        finally:
            done.set()

    th = threading.Thread(target=long_call)
    th.start()
    while not done.is_set():
        if ctx.in_use():
            with pytest.raises(pf.PfheError) as e:
                pf.blind_rotate_dev(small, small[:0], exps_dev(exps[:0]), ctx)
            seen.append(e.value.kind)
            break
    th.join()
    assert seen == ["Busy"]
    assert not ctx.in_use()
