"""GPU parity of the batched blind rotation over the TFHE product (include/pfhe.h, pfhe_tfhe{,32}_blindrot_* and
pfhe_tfhe{,32}_mul_monomial_each_to_dev) against the numpy model (tests/tfhe_blindrot_model.py), against the same loop
built from public calls, and between its two forms (the whole-loop kernel and the per-step form)."""
import os
import threading

import numpy as np
import pytest

import blindrot_model
import tfhe_blindrot_model as bm
import tfhe_fft_model as m
from test_gpu_tfhe_fft import EXACT, REALISTIC, TORCH_INT, dev_complex, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

SWITCH = "PFHE_DISABLE_FUSED_TFHE_BLINDROT"


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def per_step_context(p, *args, **kw):
    """a handle forced to the per-step form (the switch is read when the handle is created)"""
    os.environ[SWITCH] = "1"
    try:
        return p.TfheBlindRotateContext(*args, **kw)
    finally:
        os.environ.pop(SWITCH, None)


def dev_exps(exps):
    import torch
    return torch.from_numpy(np.ascontiguousarray(exps, np.uint32).view(np.int32)).cuda()


def rotate_dev(p, ctx, acc, bsk, exps, bits):
    """acc: host words, bsk: host complex (all steps), exps: batch x n_steps; returns the new accumulators"""
    a = dev_words(acc, bits)
    p.tfhe_blind_rotate_dev(a, bsk if hasattr(bsk, "is_cuda") else dev_complex(bsk), dev_exps(exps), ctx)
    return host_words(a, bits)


def fourier_keys(coeff_keys, log_n, bits):
    n = 1 << log_n
    fft = m.FullComplex64FftTable(log_n)
    return np.concatenate([fft.forward(g.reshape(-1, n), bits).reshape(-1) for g in coeff_keys])


def whole_loop_shape(log_n, k):
    return k == 1 and log_n <= 11


# ---------------- bit-exact, multi-step, exact regime ----------------

EXACT_CASES = [(32, 10, 1, 7, 3), (64, 11, 1, 15, 2),      # whole-loop form
               (32, 12, 1, 7, 3), (32, 10, 2, 7, 3),       # per-step form
               (32, 10, 1, 8, None),                       # drop_bits = 0
               (32, 10, 1, 1, 8)]                          # log B = 1


@pytest.mark.parametrize("bits,log_n,k,lb,ell", EXACT_CASES)
def test_exact_regime_equals_the_integer_loop(p, bits, log_n, k, lb, ell):
    """key words |g| <= 2^10 and (k+1) ell N 2^(logB-1) 2^10 <= 2^40: every product of the loop is the integer schoolbook
    (what test_product_exact_regime requires of the product on these shapes), so the loop is exact word for word"""
    assert (bits, log_n, k, lb, ell) in EXACT
    n = 1 << log_n
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    L = b.decompose_length()
    assert (k + 1) * L * n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    rng = np.random.default_rng(log_n * 100 + lb + k)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBlindRotateContext(fft, b, k)
    assert (ctx.scratch_bytes() == 0) == whole_loop_shape(log_n, k)
    n_steps, batch = 3, 3
    keys = [rng.integers(-1024, 1025, (k + 1) * L * (k + 1) * n).astype(m.UINT[bits]) for _ in range(n_steps)]
    import torch
    bsk = torch.empty(n_steps * ctx.key_len(), dtype=torch.complex128, device="cuda")
    for i, g in enumerate(keys):    # write_fourier_form through the device forward, as the product's exact test
        fft.forward_torus_dev(dev_words(g, bits), bsk[i * ctx.key_len():(i + 1) * ctx.key_len()])
    exps = blindrot_model.special_exponents(rng, n, batch * n_steps).reshape(batch, n_steps)
    W = (k + 1) * n
    assert ctx.glwe_len() == W
    acc = rand_words(rng, bits, batch * W)
    out = rotate_dev(p, ctx, acc, bsk, exps, bits)
    for e in range(batch):
        want = bm.exact_rotate(acc[e * W:(e + 1) * W], keys, exps[e], mb, log_n, k)
        assert np.array_equal(out[e * W:(e + 1) * W], want), e


# ---------------- bit-equal to the loop built from public calls ----------------

def public_loop(p, fft, pctx, acc, bsk, exps, bits, k):
    import torch
    a = dev_words(acc, bits)
    key = dev_complex(bsk)
    n_steps = exps.shape[1]
    klen = pctx.key_len()
    rot, e = torch.empty_like(a), torch.empty_like(a)
    for i in range(n_steps):
        fft.mul_monomial_each_to_dev(a, dev_exps(exps[:, i]), rot, polys_per_exp=k + 1)
        d = rot - a
        p.tfhe_external_product_to_dev(d, key[i * klen:(i + 1) * klen], e, pctx)
        a = a + e
    return host_words(a, bits)


@pytest.mark.parametrize("bits,log_n,k,lb,ell", REALISTIC)
def test_equals_the_loop_of_public_calls(p, bits, log_n, k, lb, ell):
    """full-torus keys, 4 steps: both forms give, word for word, what mul_monomial_each + subtract + the product on a
    TfheFftContext of the same shape + add give — one differing digit would spread over the whole ciphertext"""
    n = 1 << log_n
    b = p.ApproxSignedBasis(bits, lb, ell)
    L = b.decompose_length()
    rng = np.random.default_rng(log_n * 11 + lb + bits + k)
    fft = p.FullComplex64FftTable(log_n)
    n_steps, batch = 4, 5
    bsk = fourier_keys([rand_words(rng, bits, (k + 1) * L * (k + 1) * n) for _ in range(n_steps)], log_n, bits)
    exps = blindrot_model.special_exponents(rng, n, batch * n_steps).reshape(batch, n_steps)
    acc = rand_words(rng, bits, batch * (k + 1) * n)
    want = public_loop(p, fft, p.TfheFftContext(fft, b, k), acc, bsk, exps, bits, k)
    ctx, stepwise = p.TfheBlindRotateContext(fft, b, k), per_step_context(p, fft, b, k)
    assert stepwise.scratch_bytes() > 0 and (ctx.scratch_bytes() == 0) == whole_loop_shape(log_n, k)
    got_steps = rotate_dev(p, stepwise, acc, bsk, exps, bits)
    assert np.array_equal(got_steps, want)
    got = rotate_dev(p, ctx, acc, bsk, exps, bits)
    assert np.array_equal(got, got_steps)
    assert np.array_equal(got, want)


# ---------------- one step against the model ----------------

@pytest.mark.parametrize("bits,log_n,k,lb,ell", REALISTIC)
def test_one_step_within_the_products_error_rule(p, bits, log_n, k, lb, ell):
    n = 1 << log_n
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    L = b.decompose_length()
    rng = np.random.default_rng(log_n * 13 + lb + bits)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBlindRotateContext(fft, b, k)
    g = rand_words(rng, bits, (k + 1) * L * (k + 1) * n)
    key = fourier_keys([g], log_n, bits)
    batch = 2
    W = (k + 1) * n
    acc = rand_words(rng, bits, batch * W)
    exps = np.array([[n + 5], [3]], np.uint32)
    out = rotate_dev(p, ctx, acc, key, exps, bits)
    for e in range(batch):
        a = acc[e * W:(e + 1) * W]
        d = bm.sub(bm.rotate(a, int(exps[e, 0]), n), a)
        exact = m.schoolbook(d, g, mb, log_n, k)
        model, _ = m.external_product(d, key, mb, log_n, k)
        model_err = m.centred_error(model, exact, bits).max()
        gpu_err = m.centred_error(bm.sub(out[e * W:(e + 1) * W], a), exact, bits).max()
        print(f"bits {bits} log_n {log_n} k {k}: gpu_err {gpu_err} model_err {model_err}")
        assert gpu_err <= 4 * model_err + 2, (e, gpu_err, model_err)


# ---------------- meaning ----------------

@pytest.mark.parametrize("bits,log_n,lb,ell,host", [(32, 10, 10, 2, False), (64, 11, 15, 2, True), (64, 12, 15, 2, False)])
def test_trivial_keys_rotate_the_message(p, bits, log_n, lb, ell, host):
    n, k = 1 << log_n, 1
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    assert mb.drop_bits <= bits - bm.PLAINTEXT_BITS
    rng = np.random.default_rng(bits + log_n)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBlindRotateContext(fft, b, k)
    secret = [1, 0, 1, 1, 0, 1, 1]
    bsk = fourier_keys([bm.trivial_ggsw(mb, log_n, k, s) for s in secret], log_n, bits)
    batch = 3
    msgs = rng.integers(0, 1 << bm.PLAINTEXT_BITS, (batch, n))
    acc = bm.encode(msgs, bits, log_n, k)
    exps = blindrot_model.special_exponents(rng, n, batch * len(secret)).reshape(batch, len(secret))
    if host:
        out = acc.copy()
        p.tfhe_blind_rotate(out, bsk, np.ascontiguousarray(exps), ctx)
    else:
        out = rotate_dev(p, ctx, acc, bsk, exps, bits)
    W = (k + 1) * n
    for e in range(batch):
        mask_err, got = bm.decode(out[e * W:(e + 1) * W], bits, log_n, k)
        total = sum(int(a) * s for a, s in zip(exps[e], secret))
        assert mask_err < 2.0 ** (bits - bm.PLAINTEXT_BITS - 2), (e, mask_err)
        assert got == bm.expected_decode(msgs[e], total, n), (e, total)


# ---------------- the per-ciphertext monomial product ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("polys", [1, 2])
def test_mul_monomial_each_matches_numpy(p, bits, polys):
    import torch
    log_n, n = 9, 512
    rng = np.random.default_rng(bits + polys)
    fft = p.FullComplex64FftTable(log_n)
    elements = 8
    x = rand_words(rng, bits, elements * polys * n)
    exps = blindrot_model.special_exponents(rng, n, elements)
    a = dev_words(x, bits)
    out, out2 = torch.empty_like(a), torch.empty_like(a)
    fft.mul_monomial_each_to_dev(a, dev_exps(exps), out, polys_per_exp=polys)
    fft.mul_monomial_each_to_dev(a, dev_exps(exps + np.uint32(2 * n)), out2, polys_per_exp=polys)
    want = np.concatenate([bm.rotate(x[e * polys * n:(e + 1) * polys * n], int(exps[e]), n) for e in range(elements)])
    assert np.array_equal(host_words(out, bits), want)
    assert torch.equal(out, out2)
    with pytest.raises(p.PfheError) as e:
        fft.mul_monomial_each_to_dev(a, dev_exps(exps), a, polys_per_exp=polys)   # in place
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        fft.mul_monomial_each_to_dev(a[:n + 4], dev_exps(exps), out[:n + 4], polys_per_exp=polys)
    assert e.value.kind == "BadLength"


# ---------------- chunking, determinism, graphs ----------------

@pytest.mark.parametrize("bits,log_n,k", [(32, 10, 1), (64, 11, 1), (32, 12, 1), (64, 10, 2)])
def test_chunking_and_repeat_calls(p, bits, log_n, k):
    n = 1 << log_n
    rng = np.random.default_rng(21 + log_n)
    fft = p.FullComplex64FftTable(log_n)
    b = p.ApproxSignedBasis(bits, 7 if bits == 32 else 15, 3 if bits == 32 else 2)
    n_steps, batch = 3, 7
    bsk = fourier_keys([rand_words(rng, bits, (k + 1) * b.decompose_length() * (k + 1) * n) for _ in range(n_steps)],
                       log_n, bits)
    exps = rng.integers(0, 2 * n, (batch, n_steps)).astype(np.uint32)
    acc = rand_words(rng, bits, batch * (k + 1) * n)
    big, small = p.TfheBlindRotateContext(fft, b, k), p.TfheBlindRotateContext(fft, b, k, chunk=3)
    want = rotate_dev(p, big, acc, bsk, exps, bits)
    assert np.array_equal(rotate_dev(p, small, acc, bsk, exps, bits), want)
    assert np.array_equal(rotate_dev(p, small, acc, bsk, exps, bits), want)
    assert np.array_equal(rotate_dev(p, big, acc, bsk, exps, bits), want)
    W = (k + 1) * n
    assert np.array_equal(rotate_dev(p, small, acc[2 * W:3 * W], bsk, exps[2:3], bits), want[2 * W:3 * W])
    small_steps = per_step_context(p, fft, b, k, chunk=3)
    assert np.array_equal(rotate_dev(p, small_steps, acc, bsk, exps, bits), want)


@pytest.mark.parametrize("log_n", [10, 12])
def test_graph_capture_replays_the_eager_rotation(p, log_n):
    """a linear capture on one stream, replayed twice on a fresh accumulator"""
    import torch
    n, bits, k = 1 << log_n, 32, 1
    rng = np.random.default_rng(22)
    fft = p.FullComplex64FftTable(log_n)
    b = p.ApproxSignedBasis(32, 10, 2)
    ctx = p.TfheBlindRotateContext(fft, b, k)
    n_steps, batch = 3, 4
    bsk = dev_complex(fourier_keys([rand_words(rng, bits, 8 * n) for _ in range(n_steps)], log_n, bits))
    exps = dev_exps(rng.integers(0, 2 * n, (batch, n_steps)))
    fresh = dev_words(rand_words(rng, bits, batch * 2 * n), bits)
    eager = fresh.clone()
    p.tfhe_blind_rotate_dev(eager, bsk, exps, ctx)
    torch.cuda.synchronize()
    acc = fresh.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.tfhe_blind_rotate_dev(acc, bsk, exps, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        acc.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(acc, eager)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    log_n, n = 10, 1024
    fft = p.FullComplex64FftTable(log_n)
    b = p.ApproxSignedBasis(32, 10, 2)
    for ctx in (p.TfheBlindRotateContext(fft, b, 1), per_step_context(p, fft, b, 1)):
        assert ctx.glwe_len() == 2 * n and ctx.key_len() == 8 * n and not ctx.in_use()
        acc = torch.zeros(2 * 2 * n + 4, dtype=torch.int32, device="cuda")
        bsk = torch.zeros(3 * ctx.key_len(), dtype=torch.complex128, device="cuda")
        exps = torch.zeros(6, dtype=torch.int32, device="cuda")
        for a, k_, x in ((acc, bsk, exps),                       # not a whole number of ciphertexts
                         (acc[:4 * n], bsk[:100], exps),          # not a whole number of keys
                         (acc[:4 * n], bsk, exps[:5])):           # not batch * n_steps exponents
            with pytest.raises(p.PfheError) as e:
                p.tfhe_blind_rotate_dev(a, k_, x, ctx)
            assert e.value.kind == "BadLength"
        with pytest.raises(p.PfheError) as e:
            p.tfhe_blind_rotate_dev(acc[1:4 * n + 1], bsk, exps, ctx)   # misaligned
        assert e.value.kind == "BadArgument"
        # n_steps = 0 is a no-op
        one = torch.ones(4 * n, dtype=torch.int32, device="cuda")
        p.tfhe_blind_rotate_dev(one, bsk[:0], exps[:0], ctx)
        torch.cuda.synchronize()
        assert bool((one == 1).all())
        # the host form refuses an exponent of 2N and leaves ACC alone
        rng = np.random.default_rng(23)
        host_acc = rand_words(rng, 32, 4 * n)
        before = host_acc.copy()
        host_key = np.zeros(3 * ctx.key_len(), np.complex128)
        host_exps = np.array([0, 1, 2 * n, 3, 4, 5], np.uint32)
        with pytest.raises(p.PfheError) as e:
            p.tfhe_blind_rotate(host_acc, host_key, host_exps, ctx)
        assert e.value.kind == "BadArgument" and np.array_equal(host_acc, before)
        host_exps[2] = 2 * n - 1
        p.tfhe_blind_rotate(host_acc, host_key, host_exps, ctx)      # zero keys: E = 0
        assert np.array_equal(host_acc, before)
        with pytest.raises(p.PfheError) as e:
            p.tfhe_blind_rotate(host_acc[:4 * n - 1], host_key, host_exps, ctx)
        assert e.value.kind == "BadLength"
    with pytest.raises(p.PfheError) as e:
        p.TfheBlindRotateContext(fft, b, 65)
    assert e.value.kind == "Unsupported"


def test_second_thread_gets_busy(p):
    n = 1 << 13
    rng = np.random.default_rng(24)
    fft = p.FullComplex64FftTable(13)
    b = p.ApproxSignedBasis(64, 15, 2)
    ctx = p.TfheBlindRotateContext(fft, b, 1)
    n_steps, batch = 2, 512
    key = np.zeros(n_steps * ctx.key_len(), np.complex128)
    acc = rand_words(rng, 64, batch * 2 * n)
    before = acc.copy()
    exps = rng.integers(0, 2 * n, batch * n_steps).astype(np.uint32)
    seen = {}

    def worker():
        p.tfhe_blind_rotate(acc, key, exps, ctx)

    t = threading.Thread(target=worker)
    t.start()
    small_acc, small_exps = np.zeros(2 * n, np.uint64), np.zeros(n_steps, np.uint32)
    while t.is_alive() and "kind" not in seen:
        if ctx.in_use():
            try:
                p.tfhe_blind_rotate(small_acc, key, small_exps, ctx)
                seen["kind"] = "ok"
            except p.PfheError as e:
                seen["kind"] = e.kind
    t.join()
    assert seen.get("kind") == "Busy", seen
    assert not ctx.in_use() and np.array_equal(acc, before)      # zero keys: the rotation adds nothing
