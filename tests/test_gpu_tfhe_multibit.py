"""GPU parity of the multi-bit blind rotation (include/pfhe.h, pfhe_tfhe{,32}_mbrot_*, pfhe_tfhe_mb_combine_key_dev and
pfhe_tfhe{,32}_bootstrap_create_multibit) against the numpy model (tests/tfhe_multibit_model.py): one group within the
product's error rule, its three forms word for word, what it means on indicator keys, the bootstrap handle over it
against the same stages as public calls, and the handle's behaviour (chunks, repeats, graphs, errors, the lease)."""
import os
import threading

import numpy as np
import pytest

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_multibit_model as mbm
from test_gpu_tfhe_blind_rotate import dev_exps
from test_gpu_tfhe_bootstrap import KS_BASIS, composition, empty_exps, empty_words, handle_run
from test_gpu_tfhe_fft import dev_complex, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

SWITCH = "PFHE_DISABLE_FUSED_TFHE_BLINDROT"


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def forced_per_group(make):
    """a handle forced to the per-group form (the switch is read when the handle is created)"""
    os.environ[SWITCH] = "1"
    try:
        return make()
    finally:
        os.environ.pop(SWITCH, None)


def whole_loop_shape(log_n, k):
    return k == 1 and log_n <= 11


def rotate_dev(p, ctx, acc, bsk, exps, bits):
    a = dev_words(acc, bits)
    p.tfhe_multibit_blind_rotate_dev(a, bsk if hasattr(bsk, "is_cuda") else dev_complex(bsk), dev_exps(exps), ctx)
    return host_words(a, bits)


def full_torus_keys(rng, bits, log_n, k, ell, count):
    return [rand_words(rng, bits, (k + 1) * ell * (k + 1) << log_n) for _ in range(count)]


def edge_exponents(rng, n, batch, n_mask, g):
    """per ciphertext n_mask exponents: row 0 cycles through 0, N, 2N-1; row 1 is all 2N-1 (for g >= 2 every subset sum
    of two or more wraps past 2N); row 2 holds device-form words of 2N and more; the rest is random below 2N"""
    exps = rng.integers(0, 2 * n, (batch, n_mask)).astype(np.uint32)
    exps[0] = [(0, n, 2 * n - 1)[i % 3] for i in range(n_mask)]
    exps[1] = 2 * n - 1
    if batch > 2:
        exps[2] = [2 * n + 3 + i * (6 * n + 1) for i in range(n_mask)]
        exps[2, 0] = 0xFFFFFFFF
    return exps


# ---------------- one group within the product's error rule ----------------

ONE_GROUP = [(32, 10, 1, 7, 3, 2), (64, 11, 1, 15, 2, 2), (32, 11, 1, 10, 2, 3), (64, 10, 1, 23, 1, 4),
             (64, 12, 1, 15, 2, 2),      # per-group form
             (32, 9, 2, 7, 3, 2)]        # k = 2


def one_group_check(p, bits, log_n, k, lb, ell, g, key_fn):
    n = 1 << log_n
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(log_n * 17 + lb + bits + g)
    fft = p.FullComplex64FftTable(log_n)
    keys = full_torus_keys(rng, bits, log_n, k, ell, 1 << g)
    bsk = key_fn(rng, mbm.fourier(keys, log_n, bits).reshape(-1, n)).reshape(-1)
    batch, W = 3, (k + 1) * n
    acc = rand_words(rng, bits, batch * W)
    exps = edge_exponents(rng, n, batch, g, g)
    ctx = p.TfheMultiBitBlindRotateContext(fft, b, g, k)
    forced = forced_per_group(lambda: p.TfheMultiBitBlindRotateContext(fft, b, g, k))
    assert (ctx.scratch_bytes() == 0) == whole_loop_shape(log_n, k) and forced.scratch_bytes() > 0
    outs = {"default": rotate_dev(p, ctx, acc, bsk, exps, bits), "per-group": rotate_dev(p, forced, acc, bsk, exps, bits)}
    for e in range(batch):
        a = acc[e * W:(e + 1) * W]
        exact = mbm.exact_group(a, keys, exps[e], mb, log_n, k)
        model_err = m.centred_error(mbm.step(a, bsk, exps[e], mb, log_n, k), exact, bits).max()
        for form, out in outs.items():
            gpu_err = m.centred_error(out[e * W:(e + 1) * W], exact, bits).max()
            print(f"bits {bits} log_n {log_n} k {k} g {g} {form} e {e}: gpu_err {gpu_err} model_err {model_err}")
            assert gpu_err <= 4 * model_err + 2, (form, e, gpu_err, model_err)


@pytest.mark.parametrize("bits,log_n,k,lb,ell,g", ONE_GROUP)
def test_one_group_within_the_products_error_rule(p, bits, log_n, k, lb, ell, g):
    one_group_check(p, bits, log_n, k, lb, ell, g, lambda rng, key: key)


def test_one_group_does_not_see_a_non_hermitian_part(p):
    """K_j + A_j with A_j[(1-i) mod N] = -conj(A_j[i]) has the Hermitian part of K_j (test_non_hermitian_key's perturbation)"""
    def perturb(rng, key):
        n = key.shape[-1]
        j = np.arange(n)
        a = (rng.normal(size=key.shape) + 1j * rng.normal(size=key.shape)) * np.abs(key).max()
        return key + (a - np.conj(a[..., (1 - j) % n])) / 2
    one_group_check(p, 32, 10, 1, 7, 3, 2, perturb)


# ---------------- the three forms word for word ----------------

def composed_loop(p, fft, pctx, acc, bsk, exps, bits, k, ell, g):
    """per group and ciphertext: tfhe_multibit_combine_key_dev, then tfhe_external_product_to_dev on a TfheFftContext"""
    import torch
    a = dev_words(acc, bits)
    key = dev_complex(bsk)
    x = dev_exps(exps)
    batch, n_mask = exps.shape
    W, klen = a.numel() // batch, pctx.key_len()
    combined = torch.empty(klen, dtype=torch.complex128, device="cuda")
    for t in range(n_mask // g):
        group = key[(t << g) * klen:((t + 1) << g) * klen]
        for e in range(batch):
            p.tfhe_multibit_combine_key_dev(group, x[e, t * g:(t + 1) * g], combined, fft, ell, g, k)
            p.tfhe_external_product_to_dev(a[e * W:(e + 1) * W], combined, a[e * W:(e + 1) * W], pctx)
    return host_words(a, bits)


SMALL_N = [(32 if log_n % 2 else 64, log_n, 1, 1 + log_n % 4) for log_n in range(1, 10)]     # N = 2 .. 512, one g each
WORD_FOR_WORD = [(32, 10, 1, 2), (64, 11, 1, 3)] + SMALL_N + [(32, 9, 2, 2)]                 # ..., and k = 2


@pytest.mark.parametrize("bits,log_n,k,g", WORD_FOR_WORD)
def test_forms_agree_word_for_word(p, bits, log_n, k, g):
    """full-torus keys, 3 groups, batch 3: the whole-loop kernel (where the shape has one), the forced per-group form and
    the loop composed from the combined-key call and the product agree in every word.  N = 2 has a single half-spectrum
    slot, N = 512 one per thread, N = 1024 / 2048 two and four."""
    n = 1 << log_n
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    b = p.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(log_n * 19 + bits + g + k)
    fft = p.FullComplex64FftTable(log_n)
    groups, batch = 3, 3
    bsk = mbm.fourier(full_torus_keys(rng, bits, log_n, k, ell, groups << g), log_n, bits)
    exps = edge_exponents(rng, n, batch, groups * g, g)
    acc = rand_words(rng, bits, batch * (k + 1) * n)
    want = composed_loop(p, fft, p.TfheFftContext(fft, b, k), acc, bsk, exps, bits, k, ell, g)
    forced = forced_per_group(lambda: p.TfheMultiBitBlindRotateContext(fft, b, g, k))
    assert forced.scratch_bytes() > 0
    got_groups = rotate_dev(p, forced, acc, bsk, exps, bits)
    assert np.array_equal(got_groups, want)
    ctx = p.TfheMultiBitBlindRotateContext(fft, b, g, k)
    assert (ctx.scratch_bytes() == 0) == whole_loop_shape(log_n, k)
    got = rotate_dev(p, ctx, acc, bsk, exps, bits)
    assert np.array_equal(got, got_groups)
    assert np.array_equal(got, want)


# ---------------- meaning ----------------

@pytest.mark.parametrize("bits,log_n,lb,ell,g,host", [(32, 10, 10, 2, 1, False), (64, 11, 15, 2, 2, True), (32, 10, 10, 2, 3, True),
                                                      (64, 11, 15, 2, 4, False), (64, 12, 15, 2, 2, False)])
def test_indicator_keys_rotate_the_message(p, bits, log_n, lb, ell, g, host):
    """indicator keys of random key bits, n_mask = 4g: the result decodes to X^{sum a_i s_i} m with the bound of
    test_trivial_keys_rotate_the_message"""
    n, k = 1 << log_n, 1
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    assert mb.drop_bits <= bits - bm.PLAINTEXT_BITS
    rng = np.random.default_rng(bits + log_n + g)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheMultiBitBlindRotateContext(fft, b, g, k)
    secret = [int(s) for s in rng.integers(0, 2, 4 * g)]
    secret[0], secret[-1] = 1, 0
    bsk = mbm.fourier(mbm.multibit_indicator_bsk(mb, log_n, k, secret, g), log_n, bits)
    batch = 3
    msgs = rng.integers(0, 1 << bm.PLAINTEXT_BITS, (batch, n))
    acc = bm.encode(msgs, bits, log_n, k)
    exps = edge_exponents(rng, n, batch, len(secret), g)
    if host:
        exps[2] = rng.integers(0, 2 * n, len(secret))
        out = acc.copy()
        p.tfhe_multibit_blind_rotate(out, bsk, np.ascontiguousarray(exps), ctx)
    else:
        out = rotate_dev(p, ctx, acc, bsk, exps, bits)
    W = (k + 1) * n
    for e in range(batch):
        mask_err, got = bm.decode(out[e * W:(e + 1) * W], bits, log_n, k)
        total = sum((int(a) % (2 * n)) * s for a, s in zip(exps[e], secret))
        assert mask_err < 2.0 ** (bits - bm.PLAINTEXT_BITS - 2), (e, mask_err)
        assert got == bm.expected_decode(msgs[e], total, n), (e, total)


# ---------------- the bootstrap handle over the multi-bit rotation ----------------

def multibit_composition(p, fft, rot, lwe, bsk, tv, ksk, bits, log_n, k, n, ks_basis):
    """test_gpu_tfhe_bootstrap's composition with the multi-bit rotation in the middle"""
    big_n = 1 << log_n
    glwe = (k + 1) * big_n
    batch = lwe.numel() // (n + 1)
    exps, neg_b = empty_exps(batch * n), empty_exps(batch)
    p.lwe_modulus_switch_dev(lwe, n, log_n, exps, neg_b)
    tvb = tv if tv.numel() == batch * glwe else tv.repeat(batch)
    acc = empty_words(batch * glwe, bits)
    fft.mul_monomial_each_to_dev(tvb, neg_b, acc, polys_per_exp=k + 1)
    p.tfhe_multibit_blind_rotate_dev(acc, bsk, exps, rot)
    ext = empty_words(batch * (k * big_n + 1), bits)
    p.glwe_sample_extract_dev(acc, ext, fft, k, 0)
    if ksk is None:
        return ext
    out = empty_words(batch * (n + 1), bits)
    p.lwe_keyswitch_dev(ext, ksk, out, k * big_n, n, ks_basis)
    return out


@pytest.mark.parametrize("bits,log_n,g", [(32, 10, 2), (64, 12, 3)])
def test_bootstrap_handle_equals_the_composition_of_public_calls(p, bits, log_n, g):
    """full-torus keys and random everything, with and without the key switch, shared and per-ciphertext test vectors"""
    import torch
    k, n, batch, big_n = 1, 6, 4, 1 << log_n
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(bits + log_n + g)
    fft = p.FullComplex64FftTable(log_n)
    rot = p.TfheMultiBitBlindRotateContext(fft, basis, g, k)
    assert (rot.scratch_bytes() == 0) == whole_loop_shape(log_n, k)
    glwe = (k + 1) * big_n
    bsk = dev_complex(mbm.fourier(full_torus_keys(rng, bits, log_n, k, ell, (n // g) << g), log_n, bits))
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, k * big_n * KS_BASIS[1] * (n + 1)), bits)
    tvs = {"shared": dev_words(rand_words(rng, bits, glwe), bits), "each": dev_words(rand_words(rng, bits, batch * glwe), bits)}
    for with_ks in (True, False):
        ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis if with_ks else None, grouping_factor=g)
        assert ctx.bsk_len() == bsk.numel() and ctx.scratch_bytes() > rot.scratch_bytes()
        for name, tv in tvs.items():
            want = multibit_composition(p, fft, rot, lwe, bsk, tv, ksk if with_ks else None, bits, log_n, k, n, ks_basis)
            got = handle_run(p, ctx, lwe, bsk, tv, ksk if with_ks else None, bits)
            assert torch.equal(got, want), (with_ks, name)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, grouping_factor=g)       # the host form, once
    host_out = np.zeros(batch * (n + 1), m.UINT[bits])
    p.tfhe_bootstrap(host_words(lwe, bits), bsk.cpu().numpy(), host_words(tvs["shared"], bits), host_words(ksk, bits), host_out, ctx)
    want = multibit_composition(p, fft, rot, lwe, bsk, tvs["shared"], ksk, bits, log_n, k, n, ks_basis)
    assert np.array_equal(host_out, host_words(want, bits))


@pytest.mark.parametrize("bits,g", [(32, 2), (64, 3)])
@pytest.mark.parametrize("log_n,pbits,n,repeats", [(6, 2, 6, 6), (10, 3, 18, 3)])
def test_multibit_bootstrap_evaluates_the_lut(p, bits, g, log_n, pbits, n, repeats):
    """the construction of tests/test_tfhe_bootstrap_model.py (its exactness condition is asserted by meaning_case) with
    the trivial keys replaced by trivial indicator keys of the same secret; lwe_dimension a multiple of g"""
    k = 1
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    assert n % g == 0
    c = bs.meaning_case(bits, log_n, pbits, n, k, lb, ell, *KS_BASIS, seed=bits + log_n, repeats=repeats)
    fft = p.FullComplex64FftTable(log_n)
    ks_basis = p.ApproxSignedBasis(bits, *KS_BASIS)
    bsk = dev_complex(mbm.fourier(mbm.multibit_indicator_bsk(c["basis"], log_n, k, [int(s) for s in c["s"]], g), log_n, bits))
    want = [bs.lut(pbits)(int(v)) for v in c["msgs"]]
    for with_ks in (True, False):
        ctx = p.TfheBootstrapContext(fft, p.ApproxSignedBasis(bits, lb, ell), n, k, ks_basis if with_ks else None,
                                     grouping_factor=g)
        out = handle_run(p, ctx, dev_words(c["lwe"], bits), bsk, dev_words(c["tv"], bits),
                         dev_words(c["ksk"], bits) if with_ks else None, bits)
        key = c["s"] if with_ks else bs.flatten_key(c["z"])
        assert bs.decode(bs.lwe_phase(host_words(out, bits), key, bits), pbits, bits) == want, with_ks


def test_a_handle_of_the_old_create_gives_the_old_words(p):
    import torch
    from test_gpu_tfhe_blind_rotate import fourier_keys
    bits, log_n, k, n, batch = 32, 10, 1, 5, 3
    big_n = 1 << log_n
    basis, ks_basis = p.ApproxSignedBasis(bits, 7, 3), p.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(41)
    fft = p.FullComplex64FftTable(log_n)
    rot = p.TfheBlindRotateContext(fft, basis, k)
    bsk = dev_complex(fourier_keys(full_torus_keys(rng, bits, log_n, k, 3, n), log_n, bits))
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, k * big_n * KS_BASIS[1] * (n + 1)), bits)
    tv = dev_words(rand_words(rng, bits, 2 * big_n), bits)
    want = composition(p, fft, rot, lwe, bsk, tv, ksk, bits, log_n, k, n, ks_basis)
    for ctx in (p.TfheBootstrapContext(fft, basis, n, k, ks_basis), p.TfheBootstrapContext(fft, basis, n, k, ks_basis, 0, 1)):
        assert ctx.grouping_factor == 1 and ctx.bsk_len() == n * ctx.key_len()
        assert torch.equal(handle_run(p, ctx, lwe, bsk, tv, ksk, bits), want)


# ---------------- chunking, determinism, graphs ----------------

@pytest.mark.parametrize("bits,log_n,k,g", [(32, 10, 1, 2), (64, 12, 1, 2), (32, 9, 2, 3)])
def test_chunking_and_repeat_calls(p, bits, log_n, k, g):
    n = 1 << log_n
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    rng = np.random.default_rng(51 + log_n)
    fft = p.FullComplex64FftTable(log_n)
    b = p.ApproxSignedBasis(bits, lb, ell)
    groups, batch = 2, 5
    bsk = mbm.fourier(full_torus_keys(rng, bits, log_n, k, ell, groups << g), log_n, bits)
    exps = rng.integers(0, 2 * n, (batch, groups * g)).astype(np.uint32)
    acc = rand_words(rng, bits, batch * (k + 1) * n)
    big, small = p.TfheMultiBitBlindRotateContext(fft, b, g, k), p.TfheMultiBitBlindRotateContext(fft, b, g, k, chunk=2)
    want = rotate_dev(p, big, acc, bsk, exps, bits)
    assert np.array_equal(rotate_dev(p, small, acc, bsk, exps, bits), want)
    assert np.array_equal(rotate_dev(p, small, acc, bsk, exps, bits), want)
    assert np.array_equal(rotate_dev(p, big, acc, bsk, exps, bits), want)
    W = (k + 1) * n
    assert np.array_equal(rotate_dev(p, small, acc[2 * W:3 * W], bsk, exps[2:3], bits), want[2 * W:3 * W])
    forced = forced_per_group(lambda: p.TfheMultiBitBlindRotateContext(fft, b, g, k, chunk=2))
    assert np.array_equal(rotate_dev(p, forced, acc, bsk, exps, bits), want)


@pytest.mark.parametrize("log_n", [10, 12])
def test_graph_capture_replays_the_eager_rotation(p, log_n):
    """a linear capture on one stream, replayed twice on a fresh accumulator"""
    import torch
    n, bits, k, g = 1 << log_n, 32, 1, 2
    rng = np.random.default_rng(52)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheMultiBitBlindRotateContext(fft, p.ApproxSignedBasis(32, 10, 2), g, k)
    groups, batch = 2, 4
    bsk = dev_complex(mbm.fourier(full_torus_keys(rng, bits, log_n, k, 2, groups << g), log_n, bits))
    exps = dev_exps(rng.integers(0, 2 * n, (batch, groups * g)))
    fresh = dev_words(rand_words(rng, bits, batch * 2 * n), bits)
    eager = fresh.clone()
    p.tfhe_multibit_blind_rotate_dev(eager, bsk, exps, ctx)
    torch.cuda.synchronize()
    acc = fresh.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            p.tfhe_multibit_blind_rotate_dev(acc, bsk, exps, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        acc.copy_(fresh)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(acc, eager)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    log_n, n, g = 10, 1024, 2
    fft = p.FullComplex64FftTable(log_n)
    b = p.ApproxSignedBasis(32, 10, 2)
    for bad in (0, 5):
        with pytest.raises(p.PfheError) as e:
            p.TfheMultiBitBlindRotateContext(fft, b, bad)
        assert e.value.kind == "BadArgument" and "grouping_factor" in str(e.value)
        with pytest.raises(p.PfheError) as e:
            p.TfheBootstrapContext(fft, b, 20, 1, None, grouping_factor=bad)
        assert e.value.kind == "BadArgument" and "grouping_factor" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheBootstrapContext(fft, b, 7, 1, None, grouping_factor=2)              # lwe_dimension % g
    assert e.value.kind == "BadArgument" and "multiple" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheMultiBitBlindRotateContext(fft, b, 2, 65)
    assert e.value.kind == "Unsupported"
    for ctx in (p.TfheMultiBitBlindRotateContext(fft, b, g), forced_per_group(lambda: p.TfheMultiBitBlindRotateContext(fft, b, g))):
        assert ctx.glwe_len() == 2 * n and ctx.key_len() == 8 * n and ctx.group_len() == 32 * n and not ctx.in_use()
        acc = torch.zeros(2 * 2 * n + 4, dtype=torch.int32, device="cuda")
        bsk = torch.zeros(3 * ctx.group_len(), dtype=torch.complex128, device="cuda")
        exps = torch.zeros(2 * 3 * g, dtype=torch.int32, device="cuda")
        for a, k_, x in ((acc, bsk, exps),                                       # not a whole number of ciphertexts
                         (acc[:4 * n], bsk[:ctx.key_len()], exps),               # not a whole number of groups of keys
                         (acc[:4 * n], bsk, exps[:2 * 3 * g - 1]),               # not batch * groups * g exponents
                         (acc[:4 * n], bsk, exps[:2 * 3])):                      # batch * groups: the classic count
            with pytest.raises(p.PfheError) as e:
                p.tfhe_multibit_blind_rotate_dev(a, k_, x, ctx)
            assert e.value.kind == "BadLength"
        with pytest.raises(p.PfheError) as e:
            p.tfhe_multibit_blind_rotate_dev(acc[1:4 * n + 1], bsk, exps, ctx)   # misaligned
        assert e.value.kind == "BadArgument"
        one = torch.ones(4 * n, dtype=torch.int32, device="cuda")                # no groups: a no-op
        p.tfhe_multibit_blind_rotate_dev(one, bsk[:0], exps[:0], ctx)
        torch.cuda.synchronize()
        assert bool((one == 1).all())
        # the host form refuses an exponent of 2N and leaves ACC alone
        rng = np.random.default_rng(53)
        host_acc = rand_words(rng, 32, 4 * n)
        before = host_acc.copy()
        host_key = np.zeros(3 * ctx.group_len(), np.complex128)
        host_exps = np.arange(2 * 3 * g, dtype=np.uint32)
        host_exps[5] = 2 * n
        with pytest.raises(p.PfheError) as e:
            p.tfhe_multibit_blind_rotate(host_acc, host_key, host_exps, ctx)
        assert e.value.kind == "BadArgument" and np.array_equal(host_acc, before)
        host_exps[5] = 2 * n - 1
        with pytest.raises(p.PfheError) as e:
            p.tfhe_multibit_blind_rotate(host_acc[:4 * n - 1], host_key, host_exps, ctx)
        assert e.value.kind == "BadLength" and np.array_equal(host_acc, before)
        p.tfhe_multibit_blind_rotate(host_acc, host_key, host_exps, ctx)           # zero keys: the product is zero
        assert not host_acc.any()
    # the combined-key call
    keys = torch.zeros(4 * 8 * n, dtype=torch.complex128, device="cuda")
    out = torch.zeros(8 * n, dtype=torch.complex128, device="cuda")
    x = torch.zeros(2, dtype=torch.int32, device="cuda")
    p.tfhe_multibit_combine_key_dev(keys, x, out, fft, 2, 2)
    for args in ((keys[:-1], x, out, fft, 2, 2), (keys, x[:1], out, fft, 2, 2), (keys, x, out[:-2], fft, 2, 2),
                 (keys, x, out, fft, 2, 3)):
        with pytest.raises(p.PfheError) as e:
            p.tfhe_multibit_combine_key_dev(*args)
        assert e.value.kind == "BadLength"
    for args in ((keys, x, out, fft, 2, 0), (keys, x, out, fft, 2, 5), (keys, x, out, fft, 0, 2), (keys, x, keys[:8 * n], fft, 2, 2)):
        with pytest.raises(p.PfheError) as e:
            p.tfhe_multibit_combine_key_dev(*args)
        assert e.value.kind == "BadArgument"


def test_second_thread_gets_busy(p):
    n = 1 << 13
    rng = np.random.default_rng(54)
    fft = p.FullComplex64FftTable(13)
    ctx = p.TfheMultiBitBlindRotateContext(fft, p.ApproxSignedBasis(64, 15, 2), 1)
    groups, batch = 2, 512
    key = np.zeros(groups * ctx.group_len(), np.complex128)
    acc = rand_words(rng, 64, batch * 2 * n)
    exps = rng.integers(0, 2 * n, batch * groups).astype(np.uint32)
    seen = {}

    def worker():
        p.tfhe_multibit_blind_rotate(acc, key, exps, ctx)

    t = threading.Thread(target=worker)
    t.start()
    small_acc, small_exps = np.zeros(2 * n, np.uint64), np.zeros(groups, np.uint32)
    while t.is_alive() and "kind" not in seen:
        if ctx.in_use():
            try:
                p.tfhe_multibit_blind_rotate(small_acc, key, small_exps, ctx)
                seen["kind"] = "ok"
            except p.PfheError as e:
                seen["kind"] = e.kind
    t.join()
    assert seen.get("kind") == "Busy", seen
    assert not ctx.in_use() and not acc.any()            # zero keys: the product is zero
