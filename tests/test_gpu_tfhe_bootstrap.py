"""GPU parity of the bootstrap around the TFHE blind rotation (include/pfhe.h, pfhe_tfhe{,32}_modswitch_dev,
_sample_extract*, _keyswitch*, _bootstrap_*): every stateless step bit for bit against the integer model
(tests/tfhe_bootstrap_model.py), the handle word for word against the same stages run as public calls and, where the
product is exact, against the model; then what a bootstrap means, chunking, graph replay, errors and the lease."""
import threading

import numpy as np
import pytest

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_edge_words
import tfhe_fft_model as m
from test_gpu_tfhe_blind_rotate import EXACT_CASES, fourier_keys
from test_gpu_tfhe_fft import EXACT, TORCH_INT, dev_complex, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

BASES = {32: (7, 3), 64: (15, 2)}      # the product's (log B, ell) per width
KS_BASIS = (4, 3)                      # the key switch's


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def empty_words(size, bits):
    import torch
    return torch.empty(size, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")


def empty_exps(size):
    import torch
    return torch.empty(size, dtype=torch.int32, device="cuda")


def host_exps(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------- modulus switch ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n", [1, 2, 9, 10, 14])
def test_modulus_switch_matches_the_model(p, bits, log_n):
    rng = np.random.default_rng(bits + log_n)
    edge = np.array(bs.boundary_words(bits, log_n), m.UINT[bits])
    for n in (1, 5, 63, 64, 65, 130):
        for batch in (1, 3, 65):
            size = batch * (n + 1)
            lwe = rand_words(rng, bits, size)
            at = rng.permutation(size)[:min(size, edge.size)]       # the boundary words at random places, b's included
            lwe[at] = edge[:at.size]
            if size >= 2:
                lwe[n], lwe[0] = edge[-1], edge[0]
            exps, neg_b = empty_exps(batch * n), empty_exps(batch)
            p.lwe_modulus_switch_dev(dev_words(lwe, bits), n, log_n, exps, neg_b)
            want_exps, want_neg_b = bs.modulus_switch(lwe, n, bits, log_n)
            assert np.array_equal(host_exps(exps), want_exps.reshape(-1)), (n, batch)
            assert np.array_equal(host_exps(neg_b), want_neg_b), (n, batch)


# ---------------- sample extraction ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n", [1, 3, 9, 11])
def test_sample_extract_matches_the_model(p, bits, log_n):
    n, batch = 1 << log_n, 3
    rng = np.random.default_rng(bits + log_n)
    fft = p.FullComplex64FftTable(log_n)
    for k in (1, 2, 3):
        glwe = rand_words(rng, bits, batch * (k + 1) * n)
        g = dev_words(glwe, bits)
        for h in sorted({0, 1, n // 2, n - 1}):
            want = bs.sample_extract(glwe, log_n, k, h)
            out = empty_words(batch * (k * n + 1), bits)
            p.glwe_sample_extract_dev(g, out, fft, k, h)
            assert np.array_equal(host_words(out, bits), want), (k, h)
            host_out = np.zeros(want.size, m.UINT[bits])
            p.glwe_sample_extract(glwe, host_out, fft, k, h)
            assert np.array_equal(host_out, want), (k, h)


# ---------------- key switch ----------------

KS_SHAPES = [(4, 1, 8, None, 1), (16, 5, 1, None, 3), (64, 63, 7, 3, 17), (512, 64, 4, 3, 65), (1024, 130, 2, 8, 5)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("in_dim,out_dim,lb,ell,batch", KS_SHAPES)
def test_key_switch_matches_the_integer_model(p, bits, in_dim, out_dim, lb, ell, batch):
    """full-range random key words; mask words from the digit rule's edge words plus random ones"""
    rng = np.random.default_rng(bits + in_dim + lb)
    basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    L = basis.decompose_length()
    edge = tfhe_edge_words.edge_words(bits, lb, ell)
    lwe = rand_words(rng, bits, batch * (in_dim + 1))
    at = rng.permutation(lwe.size)[:min(lwe.size - 1, edge.size)]
    lwe[at] = rng.permutation(edge)[:at.size]
    ksk = rand_words(rng, bits, in_dim * L * (out_dim + 1))
    want = bs.keyswitch(lwe, ksk, in_dim, out_dim, mb)
    out = empty_words(batch * (out_dim + 1), bits)
    out.fill_(-1)                                         # the output may hold anything
    d_lwe, d_ksk = dev_words(lwe, bits), dev_words(ksk, bits)
    p.lwe_keyswitch_dev(d_lwe, d_ksk, out, in_dim, out_dim, basis)
    assert np.array_equal(host_words(out, bits), want)
    p.lwe_keyswitch_dev(d_lwe, d_ksk, out, in_dim, out_dim, basis)      # repeatable
    assert np.array_equal(host_words(out, bits), want)
    if in_dim == 64:
        host_out = np.zeros(want.size, m.UINT[bits])
        p.lwe_keyswitch(lwe, ksk, host_out, in_dim, out_dim, basis)
        assert np.array_equal(host_out, want)


# ---------------- the handle against the same stages as public calls ----------------

def composition(p, fft, rot, lwe, bsk, tv, ksk, bits, log_n, k, n, ks_basis):
    """lwe_modulus_switch_dev -> mul_monomial_each_to_dev on a broadcast TV -> tfhe_blind_rotate_dev ->
    glwe_sample_extract_dev -> lwe_keyswitch_dev, on device tensors"""
    big_n = 1 << log_n
    glwe = (k + 1) * big_n
    batch = lwe.numel() // (n + 1)
    exps, neg_b = empty_exps(batch * n), empty_exps(batch)
    p.lwe_modulus_switch_dev(lwe, n, log_n, exps, neg_b)
    tvb = tv if tv.numel() == batch * glwe else tv.repeat(batch)
    acc = empty_words(batch * glwe, bits)
    fft.mul_monomial_each_to_dev(tvb, neg_b, acc, polys_per_exp=k + 1)
    p.tfhe_blind_rotate_dev(acc, bsk, exps, rot)
    ext = empty_words(batch * (k * big_n + 1), bits)
    p.glwe_sample_extract_dev(acc, ext, fft, k, 0)
    if ksk is None:
        return ext
    out = empty_words(batch * (n + 1), bits)
    p.lwe_keyswitch_dev(ext, ksk, out, k * big_n, n, ks_basis)
    return out


def handle_run(p, ctx, lwe, bsk, tv, ksk, bits, stream=None):
    batch = lwe.numel() // (ctx.lwe_dimension + 1)
    out = empty_words(batch * ctx.out_len(), bits)
    p.tfhe_bootstrap_dev(lwe, bsk, tv, ksk, out, ctx, stream)
    return out


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k", [(10, 1), (9, 2), (12, 1)])
def test_handle_equals_the_composition_of_public_calls(p, bits, log_n, k):
    """full-torus keys and random everything: one differing word anywhere would spread over the whole output"""
    import torch
    n, batch, big_n = 5, 5, 1 << log_n
    lb, ell = BASES[bits]
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(bits + log_n + k)
    fft = p.FullComplex64FftTable(log_n)
    rot = p.TfheBlindRotateContext(fft, basis, k)
    assert (rot.scratch_bytes() == 0) == (k == 1 and log_n <= 11)     # the whole-loop shape and the per-step shapes
    glwe = (k + 1) * big_n
    bsk = dev_complex(fourier_keys([rand_words(rng, bits, (k + 1) * ell * glwe) for _ in range(n)], log_n, bits))
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, k * big_n * KS_BASIS[1] * (n + 1)), bits)
    tvs = {"shared": dev_words(rand_words(rng, bits, glwe), bits), "each": dev_words(rand_words(rng, bits, batch * glwe), bits)}
    for with_ks in (True, False):
        ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis if with_ks else None)
        assert ctx.out_len() == (n + 1 if with_ks else k * big_n + 1) and ctx.scratch_bytes() > rot.scratch_bytes()
        for name, tv in tvs.items():
            want = composition(p, fft, rot, lwe, bsk, tv, ksk if with_ks else None, bits, log_n, k, n, ks_basis)
            got = handle_run(p, ctx, lwe, bsk, tv, ksk if with_ks else None, bits)
            assert torch.equal(got, want), (with_ks, name)
    # the host form, once
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis)
    host_out = np.zeros(batch * (n + 1), m.UINT[bits])
    p.tfhe_bootstrap(host_words(lwe, bits), bsk.cpu().numpy(), host_words(tvs["shared"], bits), host_words(ksk, bits),
                     host_out, ctx)
    want = composition(p, fft, rot, lwe, bsk, tvs["shared"], ksk, bits, log_n, k, n, ks_basis)
    assert np.array_equal(host_out, host_words(want, bits))


# ---------------- exact regime: the integer model word for word ----------------

@pytest.mark.parametrize("bits,log_n,k,lb,ell", EXACT_CASES)
def test_exact_regime_equals_the_integer_model(p, bits, log_n, k, lb, ell):
    """key words |g| <= 2^10 and (k+1) ell N 2^(logB-1) 2^10 <= 2^40, as test_exact_regime_equals_the_integer_loop: every
    product of the rotation is the integer schoolbook, and every other stage is integer arithmetic anyway"""
    import torch
    assert (bits, log_n, k, lb, ell) in EXACT
    n, batch, big_n = 3, 2, 1 << log_n
    basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    ks_basis, ks_mb = p.ApproxSignedBasis(bits, *KS_BASIS), m.ApproxSignedBasis(bits, *KS_BASIS)
    L = basis.decompose_length()
    assert (k + 1) * L * big_n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    rng = np.random.default_rng(log_n * 100 + lb + k + bits)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis)
    keys = [rng.integers(-1024, 1025, (k + 1) * L * (k + 1) * big_n).astype(m.UINT[bits]) for _ in range(n)]
    bsk = torch.empty(n * ctx.key_len(), dtype=torch.complex128, device="cuda")
    for i, g in enumerate(keys):
        fft.forward_torus_dev(dev_words(g, bits), bsk[i * ctx.key_len():(i + 1) * ctx.key_len()])
    lwe = rand_words(rng, bits, batch * (n + 1))
    tv = rand_words(rng, bits, ctx.glwe_len())
    ksk = rand_words(rng, bits, ctx.ksk_len())
    got = handle_run(p, ctx, dev_words(lwe, bits), bsk, dev_words(tv, bits), dev_words(ksk, bits), bits)
    want = bs.bootstrap(lwe, keys, tv, ksk, mb, ks_mb, log_n, k, n)
    assert np.array_equal(host_words(got, bits), want)


# ---------------- meaning ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,pbits,n,repeats", [(6, 2, 7, 6), (10, 3, 20, 3)])
def test_bootstrap_evaluates_the_lut_on_the_device(p, bits, log_n, pbits, n, repeats):
    """the CPU meaning test's construction (trivial bootstrapping keys, a noise-free key-switch key, the half-box-shifted
    LUT, every message) through the handle"""
    k = 1
    lb, ell = BASES[bits]
    c = bs.meaning_case(bits, log_n, pbits, n, k, lb, ell, *KS_BASIS, seed=bits + log_n, repeats=repeats)
    fft = p.FullComplex64FftTable(log_n)
    ks_basis = p.ApproxSignedBasis(bits, *KS_BASIS)
    bsk = dev_complex(fourier_keys(c["keys"], log_n, bits))
    want = [bs.lut(pbits)(int(v)) for v in c["msgs"]]
    for with_ks in (True, False):
        ctx = p.TfheBootstrapContext(fft, p.ApproxSignedBasis(bits, lb, ell), n, k, ks_basis if with_ks else None)
        out = handle_run(p, ctx, dev_words(c["lwe"], bits), bsk, dev_words(c["tv"], bits),
                         dev_words(c["ksk"], bits) if with_ks else None, bits)
        key = c["s"] if with_ks else bs.flatten_key(c["z"])
        assert bs.decode(bs.lwe_phase(host_words(out, bits), key, bits), pbits, bits) == want, with_ks


# ---------------- chunking, determinism, graphs ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k", [(10, 1), (9, 2)])
def test_chunking_and_repeat_calls(p, bits, log_n, k):
    import torch
    n, batch, big_n = 4, 5, 1 << log_n
    lb, ell = BASES[bits]
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(31 + bits + log_n)
    fft = p.FullComplex64FftTable(log_n)
    glwe = (k + 1) * big_n
    bsk = dev_complex(fourier_keys([rand_words(rng, bits, (k + 1) * ell * glwe) for _ in range(n)], log_n, bits))
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, k * big_n * KS_BASIS[1] * (n + 1)), bits)
    tv = dev_words(rand_words(rng, bits, batch * glwe), bits)
    big, small = p.TfheBootstrapContext(fft, basis, n, k, ks_basis), p.TfheBootstrapContext(fft, basis, n, k, ks_basis, chunk=2)
    assert small.scratch_bytes() < big.scratch_bytes()
    want = handle_run(p, big, lwe, bsk, tv, ksk, bits)
    assert torch.equal(handle_run(p, small, lwe, bsk, tv, ksk, bits), want)
    assert torch.equal(handle_run(p, small, lwe, bsk, tv, ksk, bits), want)
    assert torch.equal(handle_run(p, big, lwe, bsk, tv, ksk, bits), want)
    one = handle_run(p, small, lwe[2 * (n + 1):3 * (n + 1)].clone(), bsk, tv[2 * glwe:3 * glwe].clone(), ksk, bits)
    assert torch.equal(one, want[2 * (n + 1):3 * (n + 1)])


@pytest.mark.parametrize("log_n", [10, 12])
def test_graph_capture_replays_the_eager_bootstrap(p, log_n):
    """a linear capture on one stream, replayed twice on fresh inputs"""
    import torch
    bits, k, n, batch, big_n = 32, 1, 3, 4, 1 << log_n
    lb, ell = BASES[bits]
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(32)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, chunk=3)       # two chunks in the graph
    glwe = 2 * big_n
    bsk = dev_complex(fourier_keys([rand_words(rng, bits, 2 * ell * glwe) for _ in range(n)], log_n, bits))
    fresh = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, ctx.ksk_len()), bits)
    tv = dev_words(rand_words(rng, bits, glwe), bits)
    eager = handle_run(p, ctx, fresh, bsk, tv, ksk, bits)
    torch.cuda.synchronize()
    lwe, out = fresh.clone(), torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.tfhe_bootstrap_dev(lwe, bsk, tv, ksk, out, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        lwe.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    bits, log_n, k, n, big_n = 32, 10, 1, 4, 1024
    fft = p.FullComplex64FftTable(log_n)
    basis, ks_basis = p.ApproxSignedBasis(32, 7, 3), p.ApproxSignedBasis(32, 4, 3)
    ctx, bare = p.TfheBootstrapContext(fft, basis, n, k, ks_basis), p.TfheBootstrapContext(fft, basis, n, k)
    assert ctx.key_len() == 12 * big_n and ctx.ksk_len() == big_n * 3 * (n + 1) and bare.ksk_len() == 0
    assert not ctx.in_use()
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")
    lwe, tv, ksk, out = z(2 * (n + 1)), z(2 * big_n), z(ctx.ksk_len()), z(2 * (n + 1))
    bsk = torch.zeros(n * ctx.key_len(), dtype=torch.complex128, device="cuda")
    p.tfhe_bootstrap_dev(lwe, bsk, tv, ksk, out, ctx)                      # the lengths that fit
    for args in ((z(2 * (n + 1) + 1), bsk, tv, ksk, out),                  # not a whole number of ciphertexts
                 (lwe, bsk[:-1], tv, ksk, out),                            # not n keys
                 (lwe, bsk, z(3 * big_n), ksk, out),                       # neither one test vector nor one each
                 (lwe, bsk, tv, ksk[:-1], out),                            # a key-switch key of another shape
                 (lwe, bsk, tv, ksk, z(2 * (big_n + 1))),                  # the output of a handle without a key switch
                 (lwe, bsk, tv, ksk, out[:-1])):
        with pytest.raises(p.PfheError) as e:
            p.tfhe_bootstrap_dev(*args, ctx)
        assert e.value.kind == "BadLength"
    with pytest.raises(p.PfheError) as e:
        p.tfhe_bootstrap_dev(lwe, bsk, tv, ksk, out, bare)                 # a key for a handle that switches no key
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        p.tfhe_bootstrap_dev(lwe, bsk, tv, None, out, ctx)                 # no key for a handle that does
    assert e.value.kind == "BadLength"
    p.tfhe_bootstrap_dev(lwe, bsk, tv, None, z(2 * (big_n + 1)), bare)
    # the output overlapping an input
    both = z(4 * (n + 1))
    with pytest.raises(p.PfheError) as e:
        p.tfhe_bootstrap_dev(both[:2 * (n + 1)], bsk, tv, ksk, both[n + 1:3 * (n + 1)], ctx)
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        p.tfhe_bootstrap_dev(lwe, bsk, ksk[:2 * big_n], ksk, ksk[big_n:big_n + 2 * (n + 1)], ctx)
    assert e.value.kind == "BadArgument"
    ext = z(2 * (big_n + 1))
    with pytest.raises(p.PfheError) as e:
        p.lwe_keyswitch_dev(ext, ksk, ext[:2 * (n + 1)], big_n, n, ks_basis)
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        p.glwe_sample_extract_dev(tv, tv[:big_n + 1], fft, 1, 0)
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        p.glwe_sample_extract_dev(tv, ext[:big_n + 1], fft, 1, big_n)      # index N
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        p.glwe_sample_extract_dev(tv, ext[:big_n + 2], fft, 1, 0)
    assert e.value.kind == "BadLength"
    # create: the rotation's statuses first, then the bootstrap's own
    with pytest.raises(p.PfheError) as e:
        p.TfheBootstrapContext(fft, basis, n, 65, ks_basis)
    assert e.value.kind == "Unsupported"
    for args in ((fft, basis, 0, 1, ks_basis), (fft, basis, n, 0, ks_basis)):
        with pytest.raises(p.PfheError) as e:
            p.TfheBootstrapContext(*args)
        assert e.value.kind == "BadArgument"
    lib = p.lib()
    import ctypes as C
    h = C.c_void_p()
    for ks_lb, ks_len in ((0, 0), (32, 0), (10, 4)):                       # ApproxSignedBasis::new on the key switch's basis
        assert lib.pfhe_tfhe32_bootstrap_create(fft._h, 1, 7, 3, n, ks_lb, ks_len, 1, 0, C.byref(h)) == 33 and not h.value
    torch.cuda.synchronize()


def test_second_thread_gets_busy(p):
    log_n, n, batch = 13, 2, 512
    big_n = 1 << log_n
    rng = np.random.default_rng(34)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBootstrapContext(fft, p.ApproxSignedBasis(64, 15, 2), n, 1)
    bsk = np.zeros(n * ctx.key_len(), np.complex128)
    lwe = rand_words(rng, 64, batch * (n + 1))
    tv = rand_words(rng, 64, batch * 2 * big_n)
    out = np.zeros(batch * (big_n + 1), np.uint64)
    seen = {}

    def worker():
        p.tfhe_bootstrap(lwe, bsk, tv, None, out, ctx)

    t = threading.Thread(target=worker)
    t.start()
    small_out = np.zeros(big_n + 1, np.uint64)
    while t.is_alive() and "kind" not in seen:
        if ctx.in_use():
            try:
                p.tfhe_bootstrap(lwe[:n + 1], bsk, tv[:2 * big_n], None, small_out, ctx)
                seen["kind"] = "ok"
            except p.PfheError as e:
                seen["kind"] = e.kind
    t.join()
    assert seen.get("kind") == "Busy", seen
    assert not ctx.in_use()
    # zero keys: the rotation adds nothing, so the output is the extraction of X^{neg_b} TV
    _, neg_b = bs.modulus_switch(lwe, n, 64, log_n)
    acc = np.concatenate([bm.rotate(tv[e * 2 * big_n:(e + 1) * 2 * big_n], int(neg_b[e]), big_n) for e in range(batch)])
    assert np.array_equal(out, bs.sample_extract(acc, log_n, 1, 0))
