"""GPU parity of the many-LUT steps (include/pfhe.h, pfhe_tfhe{,32}_modswitch_stride_dev, _bootstrap_create_many_lut,
_cbs_create_with): rule 1, the strided modulus switch, bit for bit against the model
(tests/tfhe_manylut_model.py); rule 2, the many-LUT bootstrap, word for word against the same stages run as public calls;
rule 3, the circuit bootstrap with its options, against its composition, against the existing handle where the options
change nothing, and against the exact model at small N and at the branch points of the patterned accumulator; then what
the shared handle's output means on noisy keys, all on the device; then chunking, errors, the lease and the stream order.
Every comparison is bit for bit unless it is a bound."""
import threading

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_fft_model as m
import tfhe_manylut_model as ml
from test_gpu_tfhe_bootstrap_edges import assert_same_rows
from test_gpu_tfhe_cbs import device_randomness, handle_run, product_model_error
from test_gpu_tfhe_cbs_edges import fourier_form, one_stream_after_another
from test_gpu_tfhe_edges import SMALL_SHAPES, bases, device_keys, small_key
from test_gpu_tfhe_fft import TORCH_INT, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

BASES = {32: (7, 3), 64: (15, 2)}      # the rotation's (log B, ell) per width
KS_BASIS = (4, 6)
PFKS_BASIS = (5, 4)
CBS_LOG_BASIS = 4


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


_TABLES = {}


def table(p, log_n):
    if log_n not in _TABLES:
        _TABLES[log_n] = p.FullComplex64FftTable(log_n)
    return _TABLES[log_n]


def empty_words(size, bits):
    import torch
    return torch.empty(size, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")


def empty_exps(size):
    import torch
    return torch.empty(size, dtype=torch.int32, device="cuda")


def signed(value: int, bits: int) -> int:
    """a torus word as the two's-complement integer torch takes"""
    value %= 1 << bits
    return value - (1 << bits) if value >> (bits - 1) else value


def rotation(p, fft, basis, k, g):
    """the stand-alone rotation handle of a composition and its call"""
    if g == 1:
        return p.TfheBlindRotateContext(fft, basis, k), p.tfhe_blind_rotate_dev
    return p.TfheMultiBitBlindRotateContext(fft, basis, g, k), p.tfhe_multibit_blind_rotate_dev


def random_bsk(p, rng, fft, bits, log_n, k, ell, n, g):
    """full-torus Fourier keys: n of them, or (n / g) 2^g"""
    keys = n if g == 1 else (n // g) << g
    return fourier_form(p, fft, dev_words(rand_words(rng, bits, keys * (k + 1) * ell * ((k + 1) << log_n)), bits))


# ---------------- rule 1: the strided switch ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n", [1, 4, 11])
def test_strided_switch_matches_the_model(p, bits, log_n):
    """the edge words (0, all ones, exact ties, words that round up to 2N, b words that wrap under an offset) in mask and
    body positions; v = 0 is the plain switch's words"""
    rng = np.random.default_rng(bits + log_n)
    for v in sorted({0, 1, log_n}):
        edges = np.array(ml.strided_edge_words(bits, log_n, v), np.uint64).astype(m.UINT[bits])
        for n in (1, 5, 33):
            for batch in (1, 67):
                lwe = rand_words(rng, bits, batch * (n + 1)).reshape(batch, n + 1)
                at = rng.permutation(lwe.size)[:min(lwe.size, edges.size)]
                lwe.reshape(-1)[at] = rng.permutation(edges)[:at.size]
                rows = rng.permutation(batch)[:max(1, batch // 2)]
                lwe[rows, n] = np.resize(rng.permutation(edges), rows.size)
                want_e, want_b = ml.modulus_switch_strided(lwe, n, bits, log_n, v)
                exps, neg_b = empty_exps(batch * n), empty_exps(batch)
                p.lwe_modulus_switch_strided_dev(dev_words(lwe.reshape(-1), bits), n, log_n, v, exps, neg_b)
                what = (bits, log_n, v, n, batch)
                assert np.array_equal(exps.cpu().numpy().view(np.uint32), want_e.reshape(-1)), what
                assert np.array_equal(neg_b.cpu().numpy().view(np.uint32), want_b), what
                if v == 0:
                    plain_e, plain_b = empty_exps(batch * n), empty_exps(batch)
                    p.lwe_modulus_switch_dev(dev_words(lwe.reshape(-1), bits), n, log_n, plain_e, plain_b)
                    assert np.array_equal(plain_e.cpu().numpy(), exps.cpu().numpy()), what
                    assert np.array_equal(plain_b.cpu().numpy(), neg_b.cpu().numpy()), what
    with pytest.raises(p.PfheError) as e:
        p.lwe_modulus_switch_strided_dev(dev_words(lwe.reshape(-1), bits), n, log_n, log_n + 1, exps, neg_b)
    assert e.value.kind == "BadArgument" and "log_stride" in str(e.value)


# ---------------- rule 2: the many-LUT bootstrap against the same stages as public calls ----------------

def many_lut_composition(p, fft, rot, rotate, lwe, bsk, tv, ksk, bits, log_n, k, n, v, ks_basis):
    """lwe_modulus_switch_strided_dev with v; mul_monomial_each_to_dev on the test vector; the rotation; glwe_sample_extract_dev
    at every index i < 2^v, output (e, i) at e 2^v + i; lwe_keyswitch_dev over all of them"""
    import torch
    big_n = 1 << log_n
    glwe, ext, luts = (k + 1) * big_n, k * big_n + 1, 1 << v
    batch = lwe.numel() // (n + 1)
    exps, neg_b = empty_exps(batch * n), empty_exps(batch)
    p.lwe_modulus_switch_strided_dev(lwe, n, log_n, v, exps, neg_b)
    tvb = tv if tv.numel() == batch * glwe else tv.repeat(batch)
    acc = empty_words(batch * glwe, bits)
    fft.mul_monomial_each_to_dev(tvb, neg_b, acc, polys_per_exp=k + 1)
    rotate(acc, bsk, exps, rot)
    rows = empty_words(batch * luts * ext, bits).view(batch, luts, ext)
    one = empty_words(batch * ext, bits)
    for i in range(luts):
        p.glwe_sample_extract_dev(acc, one, fft, k, i)
        rows[:, i] = one.view(batch, ext)
    if ksk is None:
        return rows.reshape(-1)
    out = empty_words(batch * luts * (n + 1), bits)
    p.lwe_keyswitch_dev(rows.reshape(-1).contiguous(), ksk, out, k * big_n, n, ks_basis)
    return out


def bootstrap_run(p, ctx, lwe, bsk, tv, ksk, bits, stream=None):
    import torch
    batch = lwe.numel() // (ctx.lwe_dimension + 1)
    out = torch.full(((batch << ctx.log_luts) * ctx.out_len(),), -1, dtype=lwe.dtype, device="cuda")       # uninitialised
    p.tfhe_bootstrap_dev(lwe, bsk, tv, ksk, out, ctx, stream)
    return out


# fused shapes log N 1, 2, 10 and the general (5, k 2), (12, k 1); v = 1, 2 and log N (at log N 1 and 2)
MANY_LUT_SHAPES = [(1, 1, (1,)), (2, 1, (1, 2)), (10, 1, (1, 2)), (5, 2, (1, 2)), (12, 1, (1, 2))]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k,strides", MANY_LUT_SHAPES, ids=["N%d-k%d" % (1 << s[0], s[1]) for s in MANY_LUT_SHAPES])
def test_many_lut_bootstrap_equals_the_composition_of_public_calls(p, bits, log_n, k, strides):
    """full-torus keys and random everything; classic and g = 2, with and without the key switch, a shared and a
    per-ciphertext test vector; the default chunk, chunk 1 and a chunk below the batch; a repeated call; the host form"""
    import torch
    n, batch, big_n = 4, 3, 1 << log_n
    lb, ell = BASES[bits]
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(bits + 10 * log_n + k)
    fft = table(p, log_n)
    glwe = (k + 1) * big_n
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, k * big_n * KS_BASIS[1] * (n + 1)), bits)
    tvs = {"shared": dev_words(rand_words(rng, bits, glwe), bits), "each": dev_words(rand_words(rng, bits, batch * glwe), bits)}
    for g in (1, 2):
        rot, rotate = rotation(p, fft, basis, k, g)
        bsk = random_bsk(p, rng, fft, bits, log_n, k, ell, n, g)
        for v in strides:
            for with_ks in (True, False):
                key = ksk if with_ks else None
                make = lambda chunk: p.TfheBootstrapContext(fft, basis, n, k, ks_basis if with_ks else None, chunk=chunk,  # noqa: E731
                                                            grouping_factor=g, log_luts=v)
                ctx = make(0)
                assert ctx.bsk_len() == bsk.numel() and ctx.log_luts == v
                handles = (("default", ctx), ("repeat", ctx), ("chunk 1", make(1)), ("chunk 2", make(2)))
                for name, tv in tvs.items():
                    want = many_lut_composition(p, fft, rot, rotate, lwe, bsk, tv, key, bits, log_n, k, n, v, ks_basis)
                    assert want.numel() == (batch << v) * ctx.out_len()
                    for what, c in handles:
                        got = bootstrap_run(p, c, lwe, bsk, tv, key, bits)
                        assert torch.equal(got, want), (g, v, with_ks, name, what)
        if g == 1 or log_n == 2:                 # the host form: classic everywhere, g = 2 once per width
            v = strides[-1]
            ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, grouping_factor=g, log_luts=v)
            host_out = np.zeros((batch << v) * (n + 1), m.UINT[bits])
            p.tfhe_bootstrap(host_words(lwe, bits), bsk.cpu().numpy(), host_words(tvs["shared"], bits), host_words(ksk, bits),
                             host_out, ctx)
            want = many_lut_composition(p, fft, rot, rotate, lwe, bsk, tvs["shared"], ksk, bits, log_n, k, n, v, ks_basis)
            assert np.array_equal(host_out, host_words(want, bits)), g
            assert not ctx.in_use()


def test_log_luts_zero_is_the_existing_handle_and_the_helper_interleaves(p):
    import torch
    bits, log_n, k, n, batch = 32, 6, 1, 4, 3
    rng = np.random.default_rng(77)
    fft = table(p, log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, *BASES[bits]), p.ApproxSignedBasis(bits, *KS_BASIS)
    bsk = random_bsk(p, rng, fft, bits, log_n, k, BASES[bits][1], n, 1)
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, (k << log_n) * KS_BASIS[1] * (n + 1)), bits)
    tv = dev_words(rand_words(rng, bits, (k + 1) << log_n), bits)
    old = p.TfheBootstrapContext(fft, basis, n, k, ks_basis)
    new = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, log_luts=0)
    assert torch.equal(bootstrap_run(p, new, lwe, bsk, tv, ksk, bits), bootstrap_run(p, old, lwe, bsk, tv, ksk, bits))
    # tfhe_many_lut_test_vector: TV[c] = tvs[c mod 2^v][c - (c mod 2^v)], on tensors and on a list of them
    tvs = rand_words(rng, bits, 4 * 2 * 64).reshape(4, 2, 64)
    want = ml.many_lut_test_vector(tvs)
    d = dev_words(tvs, bits)
    assert np.array_equal(host_words(p.tfhe_many_lut_test_vector(d), bits), want)
    assert np.array_equal(host_words(p.tfhe_many_lut_test_vector([d[i] for i in range(4)]), bits), want)
    with pytest.raises(ValueError):
        p.tfhe_many_lut_test_vector(d[:3])
    with pytest.raises(p.PfheError) as e:
        p.TfheBootstrapContext(fft, basis, n, k, ks_basis, log_luts=log_n + 1)
    assert e.value.kind == "BadArgument" and "log_luts" in str(e.value)


def test_many_lut_graph_capture_replays_the_eager_call(p):
    """a linear capture on one stream, two chunks in the graph, replayed twice on fresh inputs"""
    import torch
    bits, log_n, k, n, batch, v = 32, 6, 1, 4, 3, 2
    rng = np.random.default_rng(78)
    fft = table(p, log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, *BASES[bits]), p.ApproxSignedBasis(bits, *KS_BASIS)
    bsk = random_bsk(p, rng, fft, bits, log_n, k, BASES[bits][1], n, 1)
    fresh = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    ksk = dev_words(rand_words(rng, bits, (k << log_n) * KS_BASIS[1] * (n + 1)), bits)
    tv = dev_words(rand_words(rng, bits, (k + 1) << log_n), bits)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, chunk=2, log_luts=v)
    eager = bootstrap_run(p, ctx, fresh, bsk, tv, ksk, bits)
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


# ---------------- rule 3: the circuit bootstrap with options against the same stages as public calls ----------------

def cbs_composition(p, fft, rot, rotate, shared, lwe, bsk, pfksk, bits, log_n, k, n, cbs_basis, pfks_basis):
    """shared:  b += 2^(BITS-2); lwe_modulus_switch_strided_dev with v = ceil(log2 ell_cb); mul_monomial_each_to_dev on the
                patterned TV in memory; the rotation on batch accumulators; glwe_sample_extract_dev at every index l;
                body += g_l/2; lwe_private_keyswitch_dev.
       not:     tests/test_gpu_tfhe_cbs.py's composition (one accumulator per level, extraction at index 0) around `rotate`."""
    import torch
    big_n = 1 << log_n
    glwe, ext = (k + 1) * big_n, k * big_n + 1
    batch, levels = lwe.numel() // (n + 1), cbs_basis.decompose_length()
    half = [1 << (cbs_basis.drop_bits() + l * cbs_basis.log_basis() - 1) for l in range(levels)]
    shifted = lwe.clone()
    shifted.view(batch, n + 1)[:, n] += signed(1 << (bits - 2), bits)
    lwe_ext = empty_words(batch * levels * ext, bits).view(batch, levels, ext)
    if shared:
        v = ml.log_stride(levels)
        exps, neg_b = empty_exps(batch * n), empty_exps(batch)
        p.lwe_modulus_switch_strided_dev(shifted, n, log_n, v, exps, neg_b)
        tv = torch.zeros((batch, k + 1, big_n), dtype=lwe.dtype, device="cuda")
        for l in range(levels):
            tv[:, k, l::1 << v] = signed(-half[l], bits)
        acc = empty_words(batch * glwe, bits)
        fft.mul_monomial_each_to_dev(tv.view(-1), neg_b, acc, polys_per_exp=k + 1)
        rotate(acc, bsk, exps, rot)
        one = empty_words(batch * ext, bits)
        for l in range(levels):
            p.glwe_sample_extract_dev(acc, one, fft, k, l)
            lwe_ext[:, l] = one.view(batch, ext)
    else:
        exps, neg_b = empty_exps(batch * n), empty_exps(batch)
        p.lwe_modulus_switch_dev(shifted, n, log_n, exps, neg_b)
        exps = exps.view(batch, n).repeat_interleave(levels, dim=0).contiguous().view(-1)
        neg_b = neg_b.repeat_interleave(levels).contiguous()
        tv = torch.zeros((batch, levels, k + 1, big_n), dtype=lwe.dtype, device="cuda")
        for l in range(levels):
            tv[:, l, k, :] = signed(-half[l], bits)
        acc = empty_words(batch * levels * glwe, bits)
        fft.mul_monomial_each_to_dev(tv.view(-1), neg_b, acc, polys_per_exp=k + 1)
        rotate(acc, bsk, exps, rot)
        p.glwe_sample_extract_dev(acc, lwe_ext.view(-1), fft, k, 0)
    for l in range(levels):
        lwe_ext[:, l, ext - 1] += signed(half[l], bits)
    out = empty_words(batch * (k + 1) * levels * glwe, bits)
    p.lwe_private_keyswitch_dev(lwe_ext.view(-1), pfksk, out, k * big_n, levels, fft, pfks_basis, k)
    return out


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k", [(6, 1), (5, 2)])
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_cbs_with_options_equals_the_composition_of_public_calls(p, bits, log_n, k, levels):
    """every combination of shared_rotation and g in {1, 2}; with both off, and with one level shared, the existing handle's
    words on the same inputs; the host form of the shared handle"""
    import torch
    n, batch = 4, 3
    lb, ell = BASES[bits]
    rng = np.random.default_rng(bits + log_n + k + 100 * levels)
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = (p.ApproxSignedBasis(bits, *b) for b in ((lb, ell), (CBS_LOG_BASIS, levels), PFKS_BASIS))
    glwe = (k + 1) << log_n
    pfksk = dev_words(rand_words(rng, bits, (k + 1) * ((k << log_n) + 1) * PFKS_BASIS[1] * glwe), bits)
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    existing = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    for g in (1, 2):
        rot, rotate = rotation(p, fft, basis, k, g)
        bsk = random_bsk(p, rng, fft, bits, log_n, k, ell, n, g)
        for shared in (False, True):
            ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, grouping_factor=g, shared_rotation=shared)
            assert ctx.bsk_len() == bsk.numel() and ctx.ggsw_len() == existing.ggsw_len()
            want = cbs_composition(p, fft, rot, rotate, shared, lwe, bsk, pfksk, bits, log_n, k, n, cbs_basis, pfks_basis)
            got = handle_run(p, ctx, lwe, bsk, pfksk, bits)
            assert torch.equal(got, want), (g, shared)
            if g == 1 and (not shared or levels == 1):
                assert torch.equal(got, handle_run(p, existing, lwe, bsk, pfksk, bits)), shared
            if g == 1 and not shared:            # both options off through the new create entry, not through Python's routing
                import ctypes as C
                h = C.c_void_p()
                lib = p.lib()
                pre = "pfhe_tfhe" + ("" if bits == 64 else "32") + "_cbs"
                assert getattr(lib, pre + "_create_with")(fft._h, k, lb, ell, n, CBS_LOG_BASIS, levels, *PFKS_BASIS, 0, 0, 0,
                                                         C.byref(h)) == 0
                out = torch.full_like(got, -1)
                assert getattr(lib, pre + "_dev")(h, C.c_void_p(lwe.data_ptr()), lwe.numel(),
                                                  C.cast(C.c_void_p(bsk.data_ptr()), C.POINTER(C.c_double)), bsk.numel(),
                                                  C.c_void_p(pfksk.data_ptr()), pfksk.numel(), C.c_void_p(out.data_ptr()),
                                                  out.numel(), None) == 0
                torch.cuda.synchronize()
                assert getattr(lib, pre + "_scratch_bytes")(h) == existing.scratch_bytes()
                getattr(lib, pre + "_destroy")(h)
                assert torch.equal(out, got)
            if shared and g == 1:
                host_out = np.zeros(batch * ctx.ggsw_len(), m.UINT[bits])
                p.tfhe_circuit_bootstrap(host_words(lwe, bits), bsk.cpu().numpy(), host_words(pfksk, bits), host_out, ctx)
                assert np.array_equal(host_out, host_words(want, bits))
            assert not ctx.in_use()


# ---------------- rule 3 at small N and at the branch points, against the exact model ----------------

LWE_DIM = 4
# bits, log_n, k, rotation (log B, ell), output basis
EDGE_CASES = [(bits, log_n, k, lb, ell, cbs) for bits, k, lb, ell in SMALL_SHAPES
              for log_n, cbs in ((1, (4, 2)), (2, (4, 2)), (2, (4, 3)))] + [       # 2^v = N at N = 2 and at N = 4
    (32, 9, 1, 7, 3, (4, 3)), (64, 9, 1, 15, 2, (4, 4)),
    (64, 2, 1, 15, 2, (21, 3)), (64, 3, 1, 15, 2, (21, 3)), (32, 3, 1, 7, 3, (31, 1)),      # drop_bits 1: g_0/2 = 1
]


def crafted_shared_lwe(rng, bits, log_n, n, v):
    """A batch whose switched words, AFTER the handle's offset of 2^(BITS-2), sit on the branch points of the patterned
    accumulator.  With u = 2^(BITS - log N - 1), one exponent: b words r u for r in {0, 2^v, N - 2^v, N, N + 2^v, 2N - 2^v}
    (fewer where they coincide: two at 2^v = N), which switch to r exactly; then a b half a stride above 2N - 2^v, an exact
    tie that rounds up to 2N and wraps to 0; then the all-ones word, which wraps to 0 too; then random rows until the batch is
    no multiple of 3.  Mask words: r u for r in {0, N - 2^v, N, 2N - 2^v} and the all-ones word at random places.  Then
    2^(BITS-2) is subtracted (wrapping) from every b, so that b words wrap when the kernel adds it.  Returns (lwe, the list
    of r, index of the tie, index of the all-ones b)."""
    big_n, stride = 1 << log_n, 1 << v
    two_n, unit = 2 * big_n, 1 << (bits - log_n - 1)
    rs = sorted({0, stride % two_n, big_n - stride, big_n, (big_n + stride) % two_n, two_n - stride})
    batch = len(rs) + 2
    while batch % 3 == 0 or batch < 4:
        batch += 1
    x = rand_words(rng, bits, batch * (n + 1)).astype(np.uint64).reshape(batch, n + 1)
    x[:len(rs), n] = [r * unit for r in rs]
    tie, ones = len(rs), len(rs) + 1
    x[tie, n] = (two_n - stride) * unit + stride * unit // 2
    x[ones, n] = (1 << bits) - 1
    masks = [r * unit for r in (0, big_n - stride, big_n, two_n - stride)] + [(1 << bits) - 1]
    slots = rng.permutation(batch * n)[:len(masks)]
    for slot, w in zip(slots, masks):
        x[slot // n, slot % n] = w
    x = x.astype(m.UINT[bits])
    with np.errstate(over="ignore"):
        x[:, n] -= m.UINT[bits](1 << (bits - 2))
    return x.reshape(-1), rs, tie, ones


@pytest.mark.parametrize("bits,log_n,k,lb,ell,cbs", EDGE_CASES,
                         ids=["u%d-N%d-k%d-cbs%s" % (c[0], 1 << c[1], c[2], c[5]) for c in EDGE_CASES])
def test_shared_handle_at_small_n_and_the_branch_points(p, bits, log_n, k, lb, ell, cbs):
    """keys |g| <= 2^10 under (k+1) ell N 2^(logB-1) 2^10 <= 2^40 and a full-range private-key-switch key: the rotation is the
    integer schoolbook and tfhe_manylut_model.shared_circuit_bootstrap is the reference word for word.  A handle of chunk 3
    and a default one, each called twice into an output of all-ones."""
    n, gmax, big_n = LWE_DIM, 1024, 1 << log_n
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    cbs_b, pfks_b = p.ApproxSignedBasis(bits, *cbs), p.ApproxSignedBasis(bits, *PFKS_BASIS)
    cbs_mb, pfks_mb = m.ApproxSignedBasis(bits, *cbs), m.ApproxSignedBasis(bits, *PFKS_BASIS)
    levels = cbs_mb.decompose_length
    v = ml.log_stride(levels)
    assert (1 << v) <= big_n and cbs_mb.drop_bits >= 1
    if cbs[0] != CBS_LOG_BASIS:
        assert cbs_mb.drop_bits == 1 and cm.half_gadget(cbs_mb, 0) == 1
    rng = np.random.default_rng(9700 * bits + 100 * k + 10 * log_n + cbs[0] + cbs[1])
    lwe, rs, tie, ones = crafted_shared_lwe(rng, bits, log_n, n, v)
    batch = lwe.size // (n + 1)
    # the point of the input, from the model's switch of (a, b + 2^(BITS-2)), before the device is called
    two_n = 2 * big_n
    exps, neg_b = ml.modulus_switch_strided(cm.offset_inputs(lwe, n, bits), n, bits, log_n, v)
    assert neg_b[:len(rs)].tolist() == [(two_n - r) % two_n for r in rs]
    assert {0, big_n} <= set(neg_b.tolist()) and {(two_n - (1 << v)) % two_n, (big_n - (1 << v)) % two_n} <= set(neg_b.tolist())
    assert neg_b[tie] == 0 and neg_b[ones] == 0 and batch % 3 != 0
    assert {0, big_n - (1 << v), big_n, (two_n - (1 << v)) % two_n} <= set(exps.reshape(-1).tolist())
    assert sum(int(w) + (1 << (bits - 2)) >= 1 << bits for w in lwe.reshape(batch, n + 1)[:, n]) >= 1     # b + offset wraps

    fft = table(p, log_n)
    keys = [small_key(rng, bits, log_n, k, mb.decompose_length, gmax) for _ in range(n)]
    pfksk = rand_words(rng, bits, (k + 1) * (k * big_n + 1) * pfks_mb.decompose_length * (k + 1) * big_n)
    want = ml.shared_circuit_bootstrap(lwe, keys, pfksk, mb, cbs_mb, pfks_mb, log_n, k, n)
    rows = f"row r is input r // {(k + 1) * levels}, GGSW row r // {levels} % {k + 1}, level r % {levels}; neg_b {neg_b.tolist()}"
    d_lwe, d_pfksk = dev_words(lwe, bits), dev_words(pfksk, bits)
    bsk = None
    for chunk in (3, 0):
        ctx = p.TfheCircuitBootstrapContext(fft, b, n, k, cbs_b, pfks_b, chunk=chunk, shared_rotation=True)
        assert ctx.pfksk_len() == pfksk.size and batch * ctx.ggsw_len() == want.size
        if bsk is None:
            bsk = device_keys(p, fft, ctx, keys, bits)
        for run in ("first", "repeated"):
            got = handle_run(p, ctx, d_lwe, bsk, d_pfksk, bits)          # into an output of all-ones
            assert_same_rows(host_words(got, bits), want, (k + 1) * big_n, f"chunk {chunk}, {run} call; {rows}")


# ---------------- meaning on noisy keys, all on the device ----------------

@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("case", cm.NOISY_CASES, ids=lambda c: "u%d-N%d-k%d-n%d" % (c[0], 1 << c[1], c[2], c[3]))
def test_noisy_shared_circuit_bootstrap_gives_a_usable_ggsw_on_the_device(p, case, g):
    """tests/test_gpu_tfhe_cbs.py's noisy test through the SHARED handle, over the classic rotation and over the multi-bit
    one with g = 2: binary keys, torus_noise(bound=E) on every row of both generated keys, both bits twice.
      (i)  every coefficient of every row's phase is within tfhe_cbs_model.row_bound of f_r(m g_l) (the accumulator starts
           trivial, so the bound of the existing path holds), plus the rotation's f64 allowance n (1 + k N) (4 model_err + 2);
      (ii) after write_fourier_form, one CMUX d0 + (d1 - d0) (x) GGSW decodes to d_m at every coefficient, within
           tfhe_cbs_model.product_bound of the row allowance plus (1 + k N) (4 model_err + 2).
    The switch's worst-case margin 2^(v-1) (n + 1) < N / 2 is asserted first: a changed shape cannot hide a decode failure."""
    import torch
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, pbits = case
    assert n % g == 0
    big_n = 1 << log_n
    drift, room = ml.switch_margin(n, log_n, ml.log_stride(cb_ell))
    assert drift < room
    c = cm.noisy_case(*case, seed=4000 + bits + log_n + k)
    rng = np.random.default_rng(bits + log_n + g)
    gen = torch.Generator(device="cuda").manual_seed(5000 + bits + log_n + k + g)
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = (p.ApproxSignedBasis(bits, *b) for b in ((lb, ell), (cb_lb, cb_ell), (pf_lb, pf_ell)))
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, grouping_factor=g, shared_rotation=True)
    row = cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell)
    assert cm.product_bound(bits, log_n, k, cb_lb, cb_ell, row) < 2.0 ** (bits - pbits - 2)
    s, z_flat = dev_words(c["s"], bits), dev_words(bs.flatten_key(c["z"]), bits)
    keys = n if g == 1 else (n // g) << g
    torus = device_randomness(p, bits, log_n, k, keys * (k + 1) * ell, noise, gen)
    pfksk = device_randomness(p, bits, log_n, k, (k + 1) * (k * big_n + 1) * pf_ell, noise, gen)
    bsk = p.tfhe_generate_bsk_dev(p.TfheKeyShape(fft, basis, n, k, 0 if g == 1 else g), s, z_flat, torus)
    p.tfhe_generate_pfksk_dev(z_flat, z_flat, fft, pfks_basis, pfksk, k)
    assert bsk.numel() == ctx.bsk_len() and pfksk.numel() == ctx.pfksk_len()
    keys_torus = host_words(torus, bits).reshape(keys, -1)
    ggsw = handle_run(p, ctx, dev_words(c["lwe"], bits), bsk, pfksk, bits)
    # (i)
    phases = ggsw.clone()
    p.glwe_phase_dev(phases, z_flat, fft, k)
    got = host_words(phases, bits).reshape(-1, k + 1, big_n)[:, k]
    err = float(m.centred_error(got, cm.expected_row_phases(c["msgs"], c["z"], c["cbs_basis"], log_n, k), bits).max())
    rot_err = product_model_error(c["basis"], keys_torus[0], bits, log_n, k, rng)
    row_allowed = row + n * (1 + k * big_n) * (4 * rot_err + 2)
    # (ii)
    fourier = torch.empty(ggsw.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(ggsw, fourier, fft)
    plan = p.TfheFftContext(fft, cbs_basis, k)
    d = dev_words(c["glwe_rand"], bits)
    p.glwe_encrypt_dev(d, z_flat, fft, k)
    glwe = (k + 1) * big_n
    d0, d1 = d[:glwe], d[glwe:]
    diff, prod = d1 - d0, empty_words(glwe, bits)
    cb_err = product_model_error(c["cbs_basis"], host_words(ggsw[:ctx.ggsw_len()], bits), bits, log_n, k, rng)
    allowed = cm.product_bound(bits, log_n, k, cb_lb, cb_ell, row_allowed) + (1 + k * big_n) * (4 * cb_err + 2)
    worst = 0.0
    decoded = []
    for e, msg in enumerate(c["msgs"]):
        p.tfhe_external_product_to_dev(diff, fourier[e * ctx.ggsw_len():(e + 1) * ctx.ggsw_len()], prod, plan)
        sel = d0 + prod
        p.glwe_phase_dev(sel, z_flat, fft, k)
        ph = host_words(sel, bits)[k * big_n:]
        want = (c["data"][int(msg)].astype(np.uint64) * np.uint64(c["delta"])).astype(m.UINT[bits])
        worst = max(worst, float(m.centred_error(ph, want, bits).max()))
        decoded.append(bs.decode(ph, pbits, bits) == [int(x) for x in c["data"][int(msg)]])
    print("shared g %d bits %d log_n %d k %d n %d: rows err 2^%.1f bound 2^%.1f allowed 2^%.1f (rotation model_err %g); product "
          "err 2^%.1f allowed 2^%.1f (model_err %g) Delta/2 2^%d" % (g, bits, log_n, k, n, np.log2(max(err, 1)), np.log2(row),
                                                                    np.log2(row_allowed), rot_err, np.log2(max(worst, 1)),
                                                                    np.log2(allowed), cb_err, bits - pbits - 2))
    assert err <= row_allowed, (err, row_allowed)
    assert all(decoded), decoded
    assert worst <= allowed, (worst, allowed)


# ---------------- handle behaviour: chunking, errors, the lease, the stream order ----------------

@pytest.mark.parametrize("bits,log_n,k,g", [(32, 6, 1, 1), (64, 5, 2, 1), (32, 6, 1, 2)])
def test_shared_chunking_repeat_calls_and_scratch(p, bits, log_n, k, g):
    import torch
    n, batch, levels = 4, 5, 3
    lb, ell = BASES[bits]
    rng = np.random.default_rng(131 + bits + log_n + g)
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = (p.ApproxSignedBasis(bits, *b) for b in ((lb, ell), (CBS_LOG_BASIS, levels), PFKS_BASIS))
    bsk = random_bsk(p, rng, fft, bits, log_n, k, ell, n, g)
    make = lambda chunk, shared=True, lv=cbs_basis: p.TfheCircuitBootstrapContext(  # noqa: E731
        fft, basis, n, k, lv, pfks_basis, chunk=chunk, grouping_factor=g, shared_rotation=shared)
    big, one, two = make(0), make(1), make(2)
    pfksk = dev_words(rand_words(rng, bits, big.pfksk_len()), bits)
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    assert one.scratch_bytes() < two.scratch_bytes() < big.scratch_bytes()
    want = handle_run(p, big, lwe, bsk, pfksk, bits)
    for ctx in (one, two, two, big):
        assert torch.equal(handle_run(p, ctx, lwe, bsk, pfksk, bits), want)
    alone = handle_run(p, two, lwe[2 * (n + 1):3 * (n + 1)].clone(), bsk, pfksk, bits)
    assert torch.equal(alone, want[2 * big.ggsw_len():3 * big.ggsw_len()])
    # a shared handle holds chunk accumulators, not chunk * ell_cb: below the unshared one's at the same chunk for ell_cb >= 2
    for lv in (2, 3, 4):
        b_lv = p.ApproxSignedBasis(bits, CBS_LOG_BASIS, lv)
        for chunk in (1, 7):
            assert make(chunk, True, b_lv).scratch_bytes() < make(chunk, False, b_lv).scratch_bytes(), (lv, chunk)
    b1 = p.ApproxSignedBasis(bits, CBS_LOG_BASIS, 1)
    assert make(7, True, b1).scratch_bytes() == make(7, False, b1).scratch_bytes()


def test_errors_behind_the_shared_handle(p):
    import torch
    bits, log_n, k, n, big_n = 32, 5, 1, 4, 32
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = p.ApproxSignedBasis(32, 7, 3), p.ApproxSignedBasis(32, 4, 3), p.ApproxSignedBasis(32, 5, 4)
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, grouping_factor=2, shared_rotation=True)
    assert ctx.bsk_len() == 2 * 4 * ctx.key_len() and ctx.ggsw_len() == 12 * big_n and not ctx.in_use()
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")  # noqa: E731
    lwe, pfksk, out = z(2 * (n + 1)), z(ctx.pfksk_len()), z(2 * ctx.ggsw_len())
    bsk = torch.zeros(ctx.bsk_len(), dtype=torch.complex128, device="cuda")
    p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx)                  # the lengths that fit
    p.tfhe_circuit_bootstrap_dev(z(0), bsk, pfksk, z(0), ctx)                # an empty batch is a no-op
    for args in ((z(2 * (n + 1) + 1), bsk, pfksk, out), (lwe, bsk[:n * ctx.key_len()], pfksk, out),      # the classic key
                 (lwe, bsk, pfksk[:-1], out), (lwe, bsk, pfksk, out[:-1]), (lwe, bsk, pfksk, z(ctx.ggsw_len()))):
        with pytest.raises(p.PfheError) as e:
            p.tfhe_circuit_bootstrap_dev(*args, ctx)
        assert e.value.kind == "BadLength"
    both = z(2 * ctx.ggsw_len() + 2 * (n + 1))
    with pytest.raises(p.PfheError) as e:                                    # the output overlapping an input
        p.tfhe_circuit_bootstrap_dev(both[:2 * (n + 1)], bsk, pfksk, both[n + 1:n + 1 + 2 * ctx.ggsw_len()], ctx)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    with pytest.raises(TypeError):                                           # words of another width
        p.tfhe_circuit_bootstrap_dev(lwe.long(), bsk, pfksk, out, ctx)
    # create: the rotation's statuses first, then the divisibility, then the handle's own, ell_cb above N last
    small = table(p, 1)
    for kwargs, args, kind, text in (
            (dict(grouping_factor=2), (fft, basis, n, 65, cbs_basis, pfks_basis), "Unsupported", ""),
            (dict(grouping_factor=5), (fft, basis, n, k, cbs_basis, pfks_basis), "BadArgument", "grouping_factor"),
            (dict(grouping_factor=2), (fft, basis, 5, k, cbs_basis, pfks_basis), "BadArgument", "multiple of grouping_factor"),
            (dict(shared_rotation=True), (fft, basis, n, k, p.ApproxSignedBasis(32, 4), pfks_basis), "BadArgument", "drop"),
            (dict(shared_rotation=True), (small, basis, n, k, cbs_basis, pfks_basis), "BadArgument", "at most N levels")):
        with pytest.raises(p.PfheError) as e:
            p.TfheCircuitBootstrapContext(*args, **kwargs)
        assert e.value.kind == kind and text in str(e.value), (kwargs, str(e.value))
    p.TfheCircuitBootstrapContext(small, basis, n, k, p.ApproxSignedBasis(32, 4, 2), pfks_basis, shared_rotation=True)   # ell_cb = N
    torch.cuda.synchronize()


def test_second_thread_gets_busy_on_the_shared_handle(p):
    """tests/test_gpu_tfhe_cbs.py's lease test on a shared handle: two threads call the host form until one has been
    refused; every refusal seen is Busy, and the handle still gives the right words afterwards"""
    bits, log_n, k, n, batch = 32, 10, 1, 2, 256
    rng = np.random.default_rng(134)
    fft = table(p, log_n)
    ctx = p.TfheCircuitBootstrapContext(fft, p.ApproxSignedBasis(bits, 7, 3), n, k, p.ApproxSignedBasis(bits, 8, 2),
                                        p.ApproxSignedBasis(bits, 16, 1), shared_rotation=True)
    bsk = np.zeros(ctx.bsk_len(), np.complex128)
    lwe = rand_words(rng, bits, batch * (n + 1))
    pfksk = rand_words(rng, bits, ctx.pfksk_len())
    outs = [np.zeros(batch * ctx.ggsw_len(), np.uint32) for _ in range(2)]
    refused, done = [], threading.Event()

    def caller(out):
        for _ in range(200):
            if done.is_set():
                return
            try:
                p.tfhe_circuit_bootstrap(lwe, bsk, pfksk, out, ctx)
            except p.PfheError as e:
                refused.append(e.kind)
                done.set()

    t = threading.Thread(target=caller, args=(outs[1],))
    t.start()
    caller(outs[0])
    done.set()
    t.join()
    assert refused and set(refused) == {"Busy"}, refused
    assert not ctx.in_use()
    # zero keys: the rotation adds nothing, so every input gives the key switch of the extractions of X^{neg_b} TV + g_l/2
    p.tfhe_circuit_bootstrap(lwe, bsk, pfksk, outs[0], ctx)
    mb, cbs_mb, pfks_mb = m.ApproxSignedBasis(bits, 7, 3), m.ApproxSignedBasis(bits, 8, 2), m.ApproxSignedBasis(bits, 16, 1)
    zero_keys = [np.zeros(ctx.key_len(), np.uint32)] * n
    want = ml.shared_circuit_bootstrap(lwe[:3 * (n + 1)], zero_keys, pfksk, mb, cbs_mb, pfks_mb, log_n, k, n)
    assert np.array_equal(outs[0][:3 * ctx.ggsw_len()], want)


def test_shared_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p):
    """tests/test_gpu_tfhe_cbs_edges.py's stream case on a shared handle: its accumulators, exponents, neg_b and extracted
    ciphertexts are shared by all its calls.  u32, N = 2^8, k = 1, full-torus keys, 256 steps, chunks of 2."""
    bits, log_n, k, n = 32, 8, 1, 256
    rng = np.random.default_rng(9800)
    fft = table(p, log_n)
    basis, cbs_b, pfks_b = (p.ApproxSignedBasis(bits, *b) for b in ((7, 3), (CBS_LOG_BASIS, 3), PFKS_BASIS))
    make = lambda: p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_b, pfks_b, chunk=2, shared_rotation=True)  # noqa: E731
    shape = make()
    bsk = fourier_form(p, fft, dev_words(rand_words(rng, bits, shape.bsk_len()), bits))
    pfksk = dev_words(rand_words(rng, bits, shape.pfksk_len()), bits)

    def inputs(batch):
        lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
        return (lambda ctx, out, stream: p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx, stream)), batch * shape.ggsw_len()

    one_stream_after_another(make, inputs(24), inputs(3), (k + 1) << log_n, bits)
