"""GPU parity of the TFHE external product and the blind rotation over it (pfhe_fft.hip, pfhe_fft_device.hpp) where random
words at log N >= 10 do not reach: the edge words of the signed decomposition (tests/tfhe_edge_words.py), every N from 2 to
512, GLWE dimensions 2 and 3, the product in place, exponents above 2N and the u32 host form of the rotation.

Every assertion is bit for bit against the exact integer schoolbook (tfhe_fft_model.schoolbook,
tfhe_blindrot_model.exact_rotate): key words are integers in [-gmax, gmax] sent through the device forward, and every case
asserts the exact-regime rule of test_product_exact_regime, generalised in gmax:
    (k+1) * ell * N * 2^(logB-1) * gmax <= 2^40.
Only the in-place test and the exponent test take full-torus keys; they compare two runs of the kernels on different
arguments that must give the same words, not a kernel with itself on the same arguments.

What the file was seen to catch on an MI355X, with two changes of values (never of an index, bound or barrier) built
into a copy of the library:
  - digit_step's carry mask reduced to B/2 for log B > 1 (a field sum of B then yields the digit B and no carry): the
    edge-word product fails on every row but the log B = 1 one, the rows at log B = 15 and 23 included, and so does the
    register-path test; on random words test_product_exact_regime[64-10-1-15-2], [64-11-1-15-2] and [64-9-2-15-2] still
    pass, as do the 64-bit small-N cases here except the two at k = 3, N = 512;
  - fused_inverse_rows scaling by 1 / (2 m) where N/2 < 256: the fused product and both k = 1 rotations fail at every
    log N from 1 to 8, while of the earlier tests only the N = 8 host call notices.
"""
import numpy as np
import pytest

import blindrot_model
import tfhe_blindrot_model as bm
import tfhe_fft_model as m
from test_gpu_tfhe_blind_rotate import per_step_context, rotate_dev, whole_loop_shape
from test_gpu_tfhe_fft import dev_complex, dev_words, host_words, make_key, rand_words, run_product
from tfhe_edge_words import edge_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def bases(p, bits, lb, ell, log_n, k, gmax):
    """the device basis, the model's, and the exact-regime rule for keys in [-gmax, gmax]"""
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    assert b.decompose_length() == mb.decompose_length and b.drop_bits() == mb.drop_bits
    assert (k + 1) * mb.decompose_length * (1 << log_n) * 2 ** (lb - 1) * gmax <= 2 ** 40
    return b, mb


def small_key(rng, bits, log_n, k, ell, gmax):
    return rng.integers(-gmax, gmax + 1, (k + 1) * ell * (k + 1) * (1 << log_n)).astype(m.UINT[bits])


def fused_shape(log_n, k):
    return k == 1 and log_n <= 11


def shifted_tiling(words, polys, n):
    """`words` repeated to polys * n words, polynomial r rolled by r positions"""
    x = np.resize(words, polys * n).reshape(polys, n)
    return np.stack([np.roll(row, r) for r, row in enumerate(x)]).reshape(-1)


def assert_product_is_schoolbook(out, inp, g, mb, log_n, k):
    W = (k + 1) << log_n
    for e in range(inp.size // W):
        want = m.schoolbook(inp[e * W:(e + 1) * W], g, mb, log_n, k)
        assert np.array_equal(out[e * W:(e + 1) * W], want), e


# ---------------- a. the product over the edge words ----------------

EDGE_PRODUCT = [  # bits, log_n, k, log_basis, ell (None = full), gmax
    (32, 10, 1, 7, 3, 1024), (64, 11, 1, 15, 2, 1024), (32, 9, 1, 10, 2, 1024), (64, 5, 1, 23, 1, 1024),
    (32, 3, 1, 31, 1, 1), (64, 4, 1, 32, None, 1), (32, 5, 1, 16, None, 16), (64, 8, 1, 1, 10, 1024),
    (64, 2, 2, 21, 3, 64), (32, 4, 3, 7, 3, 1024), (64, 3, 3, 15, 2, 1024),
    (32, 12, 1, 10, 2, 64),     # the general form at a base the fused form is tested with
]


@pytest.mark.parametrize("bits,log_n,k,lb,ell,gmax", EDGE_PRODUCT)
def test_product_over_edge_words(p, bits, log_n, k, lb, ell, gmax):
    """every edge word of the basis, tiled over the batch with each polynomial shifted by one more position, so that a word
    sits in both coefficient halves (i < N/2, i >= N/2) and in several per-thread slots"""
    n = 1 << log_n
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    words = edge_words(bits, lb, ell)
    W = (k + 1) * n
    batch = -(-len(words) // W) + 1
    tiled = shifted_tiling(words, batch * (k + 1), n)
    # where N is small next to the list the tiling wraps too rarely for that, so the same ciphertexts follow once more with
    # the halves of every polynomial exchanged
    inp = np.concatenate([tiled, np.roll(tiled.reshape(-1, n), n // 2, axis=1).reshape(-1)])
    halves = inp.reshape(-1, 2, n // 2)
    assert set(words.tolist()) <= set(halves[:, 0].reshape(-1).tolist())
    assert set(words.tolist()) <= set(halves[:, 1].reshape(-1).tolist())
    rng = np.random.default_rng(1000 * bits + 10 * log_n + lb)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheFftContext(fft, b, k)
    assert (ctx.scratch_bytes() == 0) == fused_shape(log_n, k)
    g = small_key(rng, bits, log_n, k, mb.decompose_length, gmax)
    out = run_product(p, ctx, inp, make_key(p, fft, g, bits), bits)
    assert_product_is_schoolbook(out, inp, g, mb, log_n, k)


# ---------------- b. every small N ----------------

SMALL_SHAPES = [(32, 1, 7, 3), (64, 1, 15, 2), (32, 2, 7, 3), (64, 3, 15, 2)]   # bits, k, log_basis, ell
SMALL_LOG_N = list(range(1, 10))


@pytest.mark.parametrize("log_n", SMALL_LOG_N)
@pytest.mark.parametrize("bits,k,lb,ell", SMALL_SHAPES)
def test_product_at_every_small_n(p, bits, k, lb, ell, log_n):
    """N/2 < 256: most or all threads of a workgroup own no slot; log N = 1 transforms one point in zero stages"""
    n, gmax, batch = 1 << log_n, 1024, 5
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    rng = np.random.default_rng(2000 * bits + 100 * k + log_n)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheFftContext(fft, b, k)
    if k == 1:
        assert ctx.scratch_bytes() == 0
    else:
        assert ctx.scratch_bytes() > 0
    g = small_key(rng, bits, log_n, k, ell, gmax)
    inp = rand_words(rng, bits, batch * (k + 1) * n)
    out = run_product(p, ctx, inp, make_key(p, fft, g, bits), bits)
    assert_product_is_schoolbook(out, inp, g, mb, log_n, k)


# ---------------- c. in place ----------------

@pytest.mark.parametrize("bits,log_n,k,lb,ell,chunk", [(32, 10, 1, 7, 3, 0), (64, 6, 1, 15, 2, 0), (32, 12, 1, 10, 2, 0),
                                                        (64, 10, 2, 15, 2, 3)])
def test_product_in_place(p, bits, log_n, k, lb, ell, chunk):
    """product_dev allows in == out: the buffer must end as the out-of-place call leaves a separate output"""
    import torch
    n, batch = 1 << log_n, 7
    b = p.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(3000 + bits + log_n)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheFftContext(fft, b, k, chunk=chunk)
    key = dev_complex(m.FullComplex64FftTable(log_n).forward(
        rand_words(rng, bits, (k + 1) * ell * (k + 1) * n).reshape(-1, n), bits).reshape(-1))
    x = dev_words(rand_words(rng, bits, batch * (k + 1) * n), bits)
    src = x.clone()
    want = torch.full_like(x, 5)
    p.tfhe_external_product_to_dev(src, key, want, ctx)
    torch.cuda.synchronize()
    assert torch.equal(src, x)          # the out-of-place call leaves its input alone
    p.tfhe_external_product_to_dev(x, key, x, ctx)
    torch.cuda.synchronize()
    assert np.array_equal(host_words(x, bits), host_words(want, bits))
    assert not np.array_equal(host_words(x, bits), host_words(src, bits))


# ---------------- d. blind rotation at small N ----------------

def device_keys(p, fft, ctx, keys, bits):
    """the Fourier keys of all steps, end to end, through the device forward (as test_product_exact_regime's key)"""
    import torch
    klen = ctx.key_len()
    bsk = torch.empty(len(keys) * klen, dtype=torch.complex128, device="cuda")
    for i, g in enumerate(keys):
        fft.forward_torus_dev(dev_words(g, bits), bsk[i * klen:(i + 1) * klen])
    return bsk


def rotation_handles(p, fft, b, log_n, k):
    """the default handle and, where that is the whole-loop kernel, the per-step form next to it"""
    ctx = p.TfheBlindRotateContext(fft, b, k)
    assert (ctx.scratch_bytes() == 0) == whole_loop_shape(log_n, k)
    if not whole_loop_shape(log_n, k):
        return [ctx]
    stepwise = per_step_context(p, fft, b, k)
    assert stepwise.scratch_bytes() > 0
    return [ctx, stepwise]


def assert_rotation_is_exact(p, handles, acc, bsk, exps, keys, mb, log_n, k, bits):
    W = (k + 1) << log_n
    want = np.concatenate([bm.exact_rotate(acc[e * W:(e + 1) * W], keys, exps[e], mb, log_n, k)
                           for e in range(acc.size // W)])
    got = [rotate_dev(p, h, acc, bsk, exps, bits) for h in handles]
    for form, out in enumerate(got):
        for e in range(acc.size // W):
            assert np.array_equal(out[e * W:(e + 1) * W], want[e * W:(e + 1) * W]), (form, e)
    for out in got[1:]:
        assert np.array_equal(out, got[0])


STEP_CASES = [(log_n, 3) for log_n in SMALL_LOG_N] + [(4, 1), (4, 2), (4, 9)]   # both ping-pong parities, a longer loop


@pytest.mark.parametrize("log_n,n_steps", STEP_CASES)
@pytest.mark.parametrize("bits,k,lb,ell", SMALL_SHAPES)
def test_blind_rotation_at_small_n(p, bits, k, lb, ell, log_n, n_steps):
    """batch 3: with three steps the exponents are 0, 1, N-1, N, N+1 and 2N-1, then random ones"""
    n, gmax, batch = 1 << log_n, 1024, 3
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    rng = np.random.default_rng(4000 * bits + 100 * k + 10 * log_n + n_steps)
    fft = p.FullComplex64FftTable(log_n)
    handles = rotation_handles(p, fft, b, log_n, k)
    keys = [small_key(rng, bits, log_n, k, ell, gmax) for _ in range(n_steps)]
    bsk = device_keys(p, fft, handles[0], keys, bits)
    exps = blindrot_model.special_exponents(rng, n, batch * n_steps).reshape(batch, n_steps)
    acc = rand_words(rng, bits, batch * (k + 1) * n)
    assert_rotation_is_exact(p, handles, acc, bsk, exps, keys, mb, log_n, k, bits)


# ---------------- e. the edge words through the loop's register path ----------------

@pytest.mark.parametrize("bits,log_n,lb,ell", [(32, 10, 7, 3), (64, 11, 15, 2)])
def test_edge_words_through_the_rotated_difference(p, bits, log_n, lb, ell):
    """The whole-loop kernel decomposes D = X^r ACC - ACC from registers, never ACC.  With r = 1, D[j] = ACC[j-1] - ACC[j]
    for j >= 1, so ACC[j] = ACC[j-1] - D[j] from a random ACC[0] puts the edge list into D; D[0] = -ACC[N-1] - ACC[0] is
    what the wrap forces.  Two steps with random exponents follow."""
    n, k, gmax, n_steps = 1 << log_n, 1, 1024, 3
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    words = edge_words(bits, lb, ell)
    batch = -(-len(words) // (2 * (n - 1))) + 1
    polys = 2 * batch
    d_want = shifted_tiling(words, polys, n).reshape(polys, n)
    rng = np.random.default_rng(5000 + bits)
    acc = np.empty((polys, n), m.UINT[bits])
    acc[:, 0] = rand_words(rng, bits, polys)
    with np.errstate(over="ignore"):
        for j in range(1, n):
            acc[:, j] = acc[:, j - 1] - d_want[:, j]
    acc = acc.reshape(-1)
    # the point of the test, checked on the host: step 0 decomposes the edge list, bar the forced word of each polynomial
    d = bm.sub(bm.rotate(acc, 1, n), acc).reshape(polys, n)
    assert np.array_equal(d[:, 1:], d_want[:, 1:])
    assert len(set(words.tolist()) - set(d.reshape(-1).tolist())) <= polys
    exps = np.concatenate([np.ones((batch, 1), np.uint32), rng.integers(0, 2 * n, (batch, 2)).astype(np.uint32)], axis=1)
    fft = p.FullComplex64FftTable(log_n)
    handles = rotation_handles(p, fft, b, log_n, k)
    assert len(handles) == 2
    keys = [small_key(rng, bits, log_n, k, ell, gmax) for _ in range(n_steps)]
    bsk = device_keys(p, fft, handles[0], keys, bits)
    assert_rotation_is_exact(p, handles, acc, bsk, exps, keys, mb, log_n, k, bits)


# ---------------- f. exponents of 2N and more; the u32 host form ----------------

@pytest.mark.parametrize("bits,log_n,lb,ell", [(32, 9, 10, 2), (64, 12, 15, 2)])
def test_device_exponents_are_taken_modulo_2n(p, bits, log_n, lb, ell):
    """full-torus keys: e + 2N j, still below 2^32, rotates exactly as e does, in both forms"""
    n, k, batch, n_steps = 1 << log_n, 1, 4, 3
    b = p.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(6000 + bits)
    fft = p.FullComplex64FftTable(log_n)
    bsk = dev_complex(np.concatenate([
        m.FullComplex64FftTable(log_n).forward(rand_words(rng, bits, 4 * ell * n).reshape(-1, n), bits).reshape(-1)
        for _ in range(n_steps)]))
    exps = blindrot_model.special_exponents(rng, n, batch * n_steps).reshape(batch, n_steps)
    acc = rand_words(rng, bits, batch * 2 * n)
    ctx, stepwise = p.TfheBlindRotateContext(fft, b, k), per_step_context(p, fft, b, k)
    assert (ctx.scratch_bytes() == 0) == whole_loop_shape(log_n, k) and stepwise.scratch_bytes() > 0
    base = rotate_dev(p, ctx, acc, bsk, exps, bits)
    assert np.array_equal(rotate_dev(p, stepwise, acc, bsk, exps, bits), base)
    assert not np.array_equal(base, acc)
    for j in (1, 3, 2 ** 31 // (2 * n) - 1):
        big = exps.astype(np.uint64) + 2 * n * j
        assert big.max() < 2 ** 32 and big.min() >= 2 * n
        for h in (ctx, stepwise):
            assert np.array_equal(rotate_dev(p, h, acc, bsk, big.astype(np.uint32), bits), base), j


def test_u32_host_rotation_with_non_zero_keys(p):
    """tfhe_blind_rotate on host arrays, u32 accumulators: the staged form of the same loop"""
    bits, log_n, k, lb, ell, gmax = 32, 8, 1, 7, 3, 1024
    n, batch, n_steps = 1 << log_n, 3, 3
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    rng = np.random.default_rng(7000)
    fft = p.FullComplex64FftTable(log_n)
    keys = [small_key(rng, bits, log_n, k, ell, gmax) for _ in range(n_steps)]
    exps = blindrot_model.special_exponents(rng, n, batch * n_steps).reshape(batch, n_steps)
    acc = rand_words(rng, bits, batch * 2 * n)
    W = 2 * n
    want = np.concatenate([bm.exact_rotate(acc[e * W:(e + 1) * W], keys, exps[e], mb, log_n, k) for e in range(batch)])
    for ctx in rotation_handles(p, fft, b, log_n, k):
        bsk = device_keys(p, fft, ctx, keys, bits).cpu().numpy()
        out = acc.copy()
        p.tfhe_blind_rotate(out, bsk, np.ascontiguousarray(exps), ctx)
        assert np.array_equal(out, want)
