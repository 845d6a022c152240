"""GPU tests of the packing key switch in the Fourier domain (include/pfhe.h, pfhe_tfhe{,32}_packfft_*, _pack_keyswitch_fft*;
csrc/pfhe_pack_fft.hip) against the exact call lwe_pack_keyswitch_dev on the same device inputs: bit for bit in the exact
regime, within 4 x the numpy model's own error + 2 on full-torus keys (the convention of test_gpu_tfhe_fft.py), identical
words whatever the batch and the chunk, the round trip on noisy keys, a captured graph, the host form and the statuses.

The kernels' edges, and the EXACT case that takes each (slices are 4 mask words, tfhe_pack_fft_model.SLICE):
  - in_dimension below the slice width, one slice: "one-slice-m1"; whole slices only: "whole-slices-idle-threads" (3),
    "all-slots-n2048" (2), "n1024-count-partial" (5), "one-whole-slice-count1" (1); a partial last slice: "partial-slice-k2"
    (9 = 2 * 4 + 1), "k3" (5 = 4 + 1), "carry-mask-drop0" (3 of 4);
  - m = N/2 = 1, no butterfly at all: "one-slice-m1"; threads without a slot at N < 512: every case below N = 2^9; all of
    kFusedPer = 4 slots per thread and more than 64 KiB of LDS for the staged u64 words: "all-slots-n2048";
  - K1 = k + 1 = 2, 3, 4: "partial-slice-k2" is 3, "k3" is 4, the others 2;
  - count = 1: "one-whole-slice-count1"; partial: "partial-slice-k2" (5 of 64), "n1024-count-partial" (1000 of 1024, both
    halves of a slot's pair cut); N: the others;
  - drop_bits = 0 and log B = 1, the carry mask of one bit: "carry-mask-drop0".
"""
import ctypes as C

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_pack_fft_model as fm
import tfhe_pack_model as pm
from test_gpu_tfhe_fft import dev_words, host_words

pytestmark = pytest.mark.gpu

OK, BAD_LENGTH, BAD_ARGUMENT = 0, 32, 33


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


def context(p, case, chunk=0):
    bits, log_n, k, n, lb, ell = case[:6]
    return p.TfhePackFftContext(table(p, log_n), p.ApproxSignedBasis(bits, lb, ell), n, k, chunk)


def fourier_key(p, ctx, d_pksk):
    import torch
    fkey = torch.empty(ctx.fkey_len, dtype=torch.complex128, device="cuda")
    p.tfhe_pack_key_fourier_dev(d_pksk, fkey, ctx)
    return fkey


def fft_pack(p, ctx, d_lwe, fkey, count, stream=None):
    import torch
    batch = d_lwe.numel() // (count * (ctx.in_dimension + 1))
    out = torch.full((batch * ctx.glwe_len(),), -1, dtype=d_lwe.dtype, device="cuda")     # as good as uninitialised
    p.lwe_pack_keyswitch_fft_dev(d_lwe, fkey, out, count, ctx, stream=stream)
    return out


def exact_pack(p, case, d_lwe, d_pksk):
    import torch
    bits, log_n, k, n, lb, ell, count = case[:7]
    batch = d_lwe.numel() // (count * (n + 1))
    out = torch.empty(batch * (k + 1) << log_n, dtype=d_lwe.dtype, device="cuda")
    p.lwe_pack_keyswitch_dev(d_lwe, d_pksk, out, n, count, table(p, log_n), p.ApproxSignedBasis(bits, lb, ell), k)
    return out


def with_edge_words(case, lwe, seed):
    """the basis's digit edge words spread over the masks"""
    bits, _, _, n, lb, ell, count = case[:7]
    rng = np.random.default_rng(seed)
    x = lwe.reshape(-1, n + 1).copy()
    edges = ew.edge_words(bits, lb, ell)
    at = rng.permutation(x.shape[0] * n)[:min(x.shape[0] * n, 2 * edges.size)]
    x[at // n, at % n] = rng.permutation(np.tile(edges, 2))[:at.size]
    return x.reshape(-1)


# (id, (bits, log_n, k, in_dimension, log_basis, ell, count)): tfhe_pack_fft_model.EXACT_CASES, a count of 1 and the carry mask
GPU_EXACT_CASES = [
    ("whole-slices-idle-threads", fm.EXACT_CASES[0]),
    ("partial-slice-k2", fm.EXACT_CASES[1]),
    ("all-slots-n2048", fm.EXACT_CASES[2]),
    ("n1024-count-partial", fm.EXACT_CASES[3]),
    ("one-slice-m1", fm.EXACT_CASES[4]),
    ("k3", fm.EXACT_CASES[5]),
    ("one-whole-slice-count1", (32, 5, 1, 4, 4, 6, 1)),
    ("carry-mask-drop0", (32, 4, 1, 3, 1, 32, 16)),
]


@pytest.mark.parametrize("name,case", GPU_EXACT_CASES, ids=[c[0] for c in GPU_EXACT_CASES])
def test_bit_equal_to_the_exact_call_in_the_exact_regime(p, name, case):
    """keys in [-2^10, 2^10] and n ell N 2^(logB-1) 2^10 <= 2^40: the same device inputs through both calls give the same
    words; the key is the model's half spectrum within the transform's rounding"""
    bits, log_n, k, n, lb, ell, count = case
    assert fm.exact_regime_holds(case)
    _, pksk, lwe = fm.case_inputs(case, small_keys=True, batch=2)
    lwe = with_edge_words(case, lwe, 7)
    d_lwe, d_pksk = dev_words(lwe, bits), dev_words(pksk, bits)
    ctx = context(p, case)
    fkey = fourier_key(p, ctx, d_pksk)
    want_key = fm.half_spectrum_key(pksk, bits, log_n).reshape(-1)
    assert np.abs(fkey.cpu().numpy() - want_key).max() <= 1e-13 * (1 << log_n) * 2.0 ** 10
    got, want = fft_pack(p, ctx, d_lwe, fkey, count), exact_pack(p, case, d_lwe, d_pksk)
    diff = np.nonzero(host_words(got, bits) != host_words(want, bits))[0]
    assert diff.size == 0, (name, diff[:8])


@pytest.mark.parametrize("case", fm.FULL_TORUS_CASES, ids=lambda c: "u%d-logn%d-k%d-n%d-lb%d-ell%d-count%d" % c)
def test_full_torus_keys_within_four_times_the_models_error(p, case):
    """the centred distance from the exact kernel's result is at most 4 x the numpy model's own distance from it + 2"""
    bits, log_n, k, n, lb, ell, count = case
    _, pksk, lwe = fm.case_inputs(case, small_keys=False)
    d_lwe, d_pksk = dev_words(lwe, bits), dev_words(pksk, bits)
    ctx = context(p, case)
    got = host_words(fft_pack(p, ctx, d_lwe, fourier_key(p, ctx, d_pksk), count), bits)
    exact = host_words(exact_pack(p, case, d_lwe, d_pksk), bits)
    model = fm.model_error(case, lwe, pksk, exact)
    err = float(m.centred_error(got, exact, bits).max())
    print(f"{case}: device error 2^{np.log2(max(err, 1)):.1f} model error 2^{np.log2(max(model, 1)):.1f}")
    assert err <= 4 * model + 2


@pytest.mark.parametrize("bits", [32, 64])
def test_a_groups_words_do_not_depend_on_batch_chunk_or_repetition(p, bits):
    """a group alone at batch 1, and the same group as element 3 of a batch of 5 on a plan with chunk 2 (chunks of 2, 2
    and 1): identical words; a second call and a second key conversion repeat theirs"""
    import torch
    case = (bits, 8, 1, 9, 8 if bits == 64 else 4, 3, 200)
    _, log_n, k, n, lb, ell, count = case
    _, pksk, lwe = fm.case_inputs(case, small_keys=False, batch=5)
    d_lwe, d_pksk = dev_words(lwe, bits), dev_words(pksk, bits)
    group = count * (n + 1)
    one, five = context(p, case), context(p, case, chunk=2)
    half = (k + 1) << (log_n - 1)
    assert not five.in_use() and five.scratch_bytes() == 2 * ((n + fm.SLICE - 1) // fm.SLICE) * half * 16
    fkey = fourier_key(p, one, d_pksk)
    assert torch.equal(torch.view_as_real(fkey), torch.view_as_real(fourier_key(p, five, d_pksk)))
    alone = fft_pack(p, one, d_lwe[3 * group:4 * group].clone(), fkey, count)
    batched = fft_pack(p, five, d_lwe, fkey, count)
    assert torch.equal(batched[3 * five.glwe_len():4 * five.glwe_len()], alone)
    assert torch.equal(fft_pack(p, five, d_lwe, fkey, count), batched)
    # and every group of the batch is right, not only the third
    exact = host_words(exact_pack(p, case, d_lwe, d_pksk), bits)
    model = fm.model_error(case, lwe, pksk, exact)
    assert m.centred_error(host_words(batched, bits), exact, bits).max() <= 4 * model + 2


@pytest.mark.parametrize("case", pm.NOISY_CASES, ids=lambda c: "u%d-logn%d-k%d-n%d-lb%d-ell%d-count%d" % c[:7])
def test_round_trip_on_noisy_keys(p, case):
    """All on the device: the packing key generated from binary keys and bounded noise, converted, the inputs packed through
    the Fourier route, the GLWE phase taken.  Every coefficient below count decodes, and the largest centred distance
    from Delta m is at most tfhe_pack_model.noise_bound(...) + 4 x the model's FFT error + 2.
    Measured (MI355X): see DESIGN.md section 18."""
    import torch
    bits, log_n, k, n, lb, ell, count, noise, prec = case
    big_n = 1 << log_n
    bound = pm.noise_bound(bits, n, lb, ell, count, noise)
    c = pm.noisy_case(*case, seed=9, batch=3)
    batch, basis = c["batch"], p.ApproxSignedBasis(bits, lb, ell)
    fft = table(p, log_n)
    rand = dev_words(c["rand_pksk"], bits).reshape(n * ell, k + 1, big_n)
    rand[:, k] = p.torus_noise(n * ell * big_n, bits, bound=noise).reshape(n * ell, big_n)
    pksk = rand.reshape(-1).contiguous()
    d_z = dev_words(c["z"].reshape(-1), bits)
    p.tfhe_generate_pksk_dev(dev_words(c["s"], bits), d_z, fft, basis, pksk, k)
    ctx = context(p, case[:7])
    fkey = fourier_key(p, ctx, pksk)
    d_lwe = dev_words(c["lwe"], bits)
    packed = fft_pack(p, ctx, d_lwe, fkey, count)
    exact = host_words(exact_pack(p, case[:7], d_lwe, pksk), bits)
    model = fm.model_error(case[:7], c["lwe"], host_words(pksk, bits), exact)
    p.glwe_phase_dev(packed, d_z, fft, k)
    phases = host_words(packed, bits).reshape(batch, k + 1, big_n)[:, k, :count].reshape(-1)
    assert bound + 4 * model + 2 < 2.0 ** (bits - prec - 2)
    assert bs.decode(phases, prec, bits) == list(c["msgs"])
    err = pm.message_error(phases, c["msgs"], c["delta"], bits)
    print(f"{case}: err 2^{np.log2(max(err, 1)):.1f} noise bound 2^{np.log2(bound):.1f} model fft error 2^{np.log2(max(model, 1)):.1f}")
    assert err <= bound + 4 * model + 2


def test_graph_capture_replays_the_eager_call(p):
    """one call captured on a single stream (a linear chain: accumulate, finish) and replayed twice"""
    import torch
    case = (32, 9, 1, 10, 4, 3, 512)
    bits, count = case[0], case[6]
    _, pksk, lwe = fm.case_inputs(case, small_keys=False, batch=3)
    d_lwe, d_pksk = dev_words(lwe, bits), dev_words(pksk, bits)
    ctx = context(p, case)
    fkey = fourier_key(p, ctx, d_pksk)
    eager = fft_pack(p, ctx, d_lwe, fkey, count)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            p.lwe_pack_keyswitch_fft_dev(d_lwe, fkey, out, count, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("bits", [32, 64])
def test_host_form_equals_the_device_form(p, bits):
    case = (bits, 6, 2, 9, 7, 3, 37)
    count = case[6]
    _, pksk, lwe = fm.case_inputs(case, small_keys=False, batch=3)
    ctx = context(p, case)
    fkey = fourier_key(p, ctx, dev_words(pksk, bits))
    want = host_words(fft_pack(p, ctx, dev_words(lwe, bits), fkey, count), bits)
    out = np.zeros(want.size, m.UINT[bits])
    p.lwe_pack_keyswitch_fft(lwe, fkey.cpu().numpy(), out, count, ctx)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_calls_refuse_their_arguments_in_the_exact_calls_order(p, w, bits):
    """behind the plan: count, the three lengths, the empty batch as a no-op, null pointers, the overlap (device form only);
    the key conversion: the lengths, null pointers, the overlap"""
    import torch
    lib = p.lib()
    case = (bits, 3, 1, 5, 4, 2, 3)
    _, log_n, k, n, lb, ell, count = case
    big_n, batch = 1 << log_n, 2
    ctx = context(p, case)
    len_in, len_key, len_out = batch * count * (n + 1), ctx.fkey_len, batch * ctx.glwe_len()
    words = torch.zeros(4096, dtype=torch.int64, device="cuda")
    fkey = torch.zeros(len_key, dtype=torch.complex128, device="cuda")
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    fp = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))
    src, dst = vp(words), vp(words, 16384)
    last = lambda: lib.pfhe_last_error().decode(errors="replace")
    host_buf = np.zeros(4096, np.uint64)
    host_key = np.zeros(len_key, np.complex128)
    hp = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    hf = host_key.ctypes.data_as(C.POINTER(C.c_double))
    forms = ((getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_fft_dev"), src, fp(fkey), dst, (None,)),
             (getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_fft"), hp(host_buf), hf, hp(host_buf, 16384), ()))
    for call, a, f, o, tail in forms:
        for bad in (0, big_n + 1, 2 ** 40):
            assert call(ctx._h, None, 7, bad, None, 1, None, 3, *tail) == BAD_ARGUMENT and "count must be in 1..N" in last()
        assert call(ctx._h, a, len_in + 1, count, f, len_key, o, len_out, *tail) == BAD_LENGTH
        assert call(ctx._h, a, len_in, count, f, len_key - 1, o, len_out, *tail) == BAD_LENGTH
        assert call(ctx._h, a, len_in, count, f, 2 * len_key, o, len_out, *tail) == BAD_LENGTH       # the full-layout length
        assert call(ctx._h, a, len_in, count, f, len_key, o, len_out - 1, *tail) == BAD_LENGTH
        assert "batch*count*(in_dimension+1)" in last()
        assert call(ctx._h, None, 0, count, None, len_key, None, 0, *tail) == OK                     # an empty batch is a no-op
        for args in ((None, f, o), (a, None, o), (a, f, None)):
            assert call(ctx._h, args[0], len_in, count, args[1], len_key, args[2], len_out, *tail) == BAD_ARGUMENT
        assert call(ctx._h, a, len_in, count, f, len_key, o, len_out, *tail) == OK
    dev = forms[0][0]
    assert dev(ctx._h, src, len_in, count, fp(fkey), len_key, src, len_out, None) == BAD_ARGUMENT and "overlap" in last()
    assert dev(ctx._h, src, len_in, count, fp(fkey), len_key, vp(fkey), len_out, None) == BAD_ARGUMENT and "overlap" in last()
    assert forms[1][0](ctx._h, hp(host_buf), len_in, count, hf, len_key, hp(host_buf), len_out) == OK   # staged: no overlap
    key = getattr(lib, f"pfhe_tfhe{w}_packfft_key_dev")
    len_pksk = ctx.pksk_len()
    assert key(ctx._h, src, len_pksk + 1, fp(fkey), len_key, None) == BAD_LENGTH
    assert key(ctx._h, src, len_pksk, fp(fkey), 2 * len_key, None) == BAD_LENGTH
    assert key(ctx._h, None, len_pksk, fp(fkey), len_key, None) == BAD_ARGUMENT
    assert key(ctx._h, src, len_pksk, None, len_key, None) == BAD_ARGUMENT
    assert key(ctx._h, src, len_pksk, C.cast(src, C.POINTER(C.c_double)), len_key, None) == BAD_ARGUMENT and "overlap" in last()
    assert key(ctx._h, src, len_pksk, fp(fkey), len_key, None) == OK
    torch.cuda.synchronize()
    assert not ctx.in_use()
