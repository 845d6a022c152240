"""GPU parity of the circuit bootstrap's stages (csrc/pfhe_tfhe_stages.hip: tfhe_modswitch_kernel with the exponents
written once per level, tfhe_const_acc_init_kernel, tfhe_extract_kernel; one kernel per stage for every handle around a
blind rotation) where the random data and comfortable shapes of tests/test_gpu_tfhe_cbs.py do not reach, and the
stream order of the four handles that own device buffers between calls and had no test of it:

  - the handle at N = 2 .. 512 with k up to 3, with inputs whose switched exponents, AFTER the handle's own offset of
    2^(BITS-2), sit on the branch points of the accumulator's first rotation (0, 1, N-1, N, N+1, 2N-1, a rounding tie, the
    all-ones word that wraps to 0): section D of tests/test_gpu_tfhe_bootstrap_edges.py with 2^(BITS-2) subtracted from
    every b word, so that b words wrap when the kernel adds the offset;
  - an output basis of drop_bits 1 (g_l/2 = 1, the smallest the create admits; at u32 it is one level) and a key-switch
    basis of drop_bits 0 inside the handle;
  - one handle used from one stream after another with no event handling by the caller, for the circuit bootstrap (the
    rotation's guard nested in its own), the CMUX tree in both forms (the general form's short call is tfhe_cmux_dev on
    the same handle: it shares D and E with the tree), the trace in both forms and the Fourier packing plan (which calls
    ordered_on itself, from inside stateless_call).

Every comparison is bit for bit.  The handle is compared with the integer model (tests/tfhe_cbs_model.circuit_bootstrap)
under the exact-regime rule of tests/test_gpu_tfhe_edges.py; the stream cases compare with a second handle of the same
shape that ran alone.  N = 2^12 is left out: the private-key-switch key alone would be 2 * 4097 * ell * 8192 words, and
the per-step rotation it would select is reached through k = 2 and k = 3.

What the file was seen to catch on an MI355X, each change built into a copy of the library (none of them moves an access
out of bounds):
  1. the accumulator written from constants (tfhe_const_acc_init_kernel now, then the circuit bootstrap's own copy) with
     `high = r > n` and the rotation still reduced for r >= n (X^N TV_l comes out as +TV_l, the change
     tests/test_gpu_tfhe_bootstrap_edges.py records for tfhe_acc_init_kernel): 20 of the 22 handle cases fail,
     each at exactly the GGSW rows of the inputs with neg_b = N.  The two cases with the output basis of drop_bits 1 pass:
     there +-g_0/2 = +-1 on the extracted body is below what the key switch's basis (5, 4) keeps, so they cannot see the
     sign (they do see change 2).  Of tests/test_gpu_tfhe_cbs.py, 1 of 34 fails (test_exact_regime_equals_the_integer_model
     [64-5-2-15-2], whose random data happens to hold a neg_b of N); 33 pass.
  2. the extraction (then the circuit bootstrap's own copy) taking its level as a / levels instead of a % levels: all 22
     handle cases fail.  tests/test_gpu_tfhe_cbs.py sees this one too: 17 of 34 fail.
  3. ordered_on without its hipStreamWaitEvent: all six stream cases of a form that owns buffers fail (circuit
     bootstrap, CMUX tree fused and general, trace general u32 and u64, packing plan), in 4 runs of 4, in round 0 or 1, at
     ciphertexts of the long call that the short one overtook or at the short call's; the fused trace passes, as it shares
     no buffer between calls.  All 138 tests of test_gpu_tfhe_cbs.py, _cmux.py, _trace.py and _pack_fft.py pass under it.
     This is a race: a failure under the change was seen, not proven to be certain.
     Shapes kept.  At the issue's starting shapes three cases did not see the race: the circuit bootstrap at 32 steps (kept:
     256 steps), the general CMUX tree and the u64 trace at N = 2^5 (kept: N = 2^11, where a launch outlasts its queueing);
     the fused CMUX tree saw it in one run of two at 24 inputs (kept: 96 inputs, 48 chunks).  With ONE pair of streams for
     all rounds, every run still left one case passing, and which one depended on what had run before in the process (the
     whole file: the circuit bootstrap's; the stream cases alone: the fused tree's), while a loop of the fused tree's case
     on its own failed in 17 of 21 repetitions.  Supposed, not shown: the runtime served that pair from one hardware queue,
     which orders the two streams by itself.  Hence a fresh pair of streams in every round (one_stream_after_another).
  4. The index arithmetic of the merged stage kernels, one run each of the 22 handle cases (levels 3, or 1 with the output
     basis of drop_bits 1 at u32; batch 7 to 9; chunk 3 and the default), the unmodified library failing none:
     (a) tfhe_extract_kernel's level as a / level_period instead of a % level_period (change 2 on the merged kernel): all 22
         fail;
     (b) tfhe_const_acc_init_kernel's input as a % per_input instead of a / per_input (the level base kept right): 21 of
         22 fail; u32-N8-k1-cbs(31, 1) passes, the one-level basis whose +-g_0/2 = +-1 the key switch's basis drops (change 1);
     (c) tfhe_modswitch_kernel's copies written at (e + c batch) n instead of (e copies + c) n: 12 of 22 fail: the 10 u32
         cases with 3 levels, u64-N8-k1-cbs(21, 3) and u64-N8-k1-pfks(16, None).  The 8 u64 cases of the shape table, u64-N512
         and the one-level u32 case pass; supposed, not examined: the change hands an accumulator another input's mask
         exponents, and the crafted batches are mostly zero there, so a swap of equal rows is not seen.
     Each is seen by existing cases, so none was added.
Wall time on an MI355X: 4.7 s for the 29 tests of this file, 1.6 s of it the first import; the slowest case 0.63 s (the
circuit bootstrap's stream case), the two N = 512 handle cases 0.5 s each (the integer model), every other below 0.12 s.
"""
import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_fft_model as m
from test_gpu_tfhe_bootstrap_edges import STREAM_ROUNDS, assert_same_rows, crafted_lwe
from test_gpu_tfhe_cbs import CBS_BASIS, PFKS_BASIS, handle_run
from test_gpu_tfhe_edges import SMALL_SHAPES, bases, device_keys, small_key
from test_gpu_tfhe_fft import TORCH_INT, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


# ---------------- A. the handle at small N and at the init's branch points ----------------

LWE_DIM = 4
# bits, log_n, k, rotation (log B, ell), output basis, key-switch basis
CBS_CASES = [(bits, log_n, k, lb, ell, CBS_BASIS, PFKS_BASIS) for bits, k, lb, ell in SMALL_SHAPES for log_n in (1, 2, 3, 6)] + [
    (32, 9, 1, 7, 3, CBS_BASIS, PFKS_BASIS), (64, 9, 1, 15, 2, CBS_BASIS, PFKS_BASIS),
    (32, 3, 1, 7, 3, (31, 1), PFKS_BASIS), (64, 3, 1, 15, 2, (21, 3), PFKS_BASIS),          # drop_bits 1: g_0/2 = 1
    (32, 3, 1, 7, 3, CBS_BASIS, (8, None)), (64, 3, 1, 15, 2, CBS_BASIS, (16, None)),       # the key switch drops nothing
]
HOST_FORM = {(32, 3, 2), (64, 3, 3)}       # (bits, log_n, k): once per width, over the per-step rotation


def crafted_cbs_lwe(rng, bits, log_n, n):
    """crafted_lwe of tests/test_gpu_tfhe_bootstrap_edges.py with 2^(BITS-2) subtracted (wrapping) from every b word: the
    handle's offset puts the switched values back on the branch points.  Returns (lwe, the crafted batch it comes from,
    the r of the crafted b words, index of the tie, index of the all-ones b, the all-ones mask slot)."""
    crafted, rs, tie, wrapped, ones_slot = crafted_lwe(rng, bits, log_n, n)
    x = crafted.reshape(-1, n + 1).copy()
    x[:, n] -= m.UINT[bits](1 << (bits - 2))
    return x.reshape(-1), crafted, rs, tie, wrapped, ones_slot


def assert_inputs_sit_on_the_branch_points(lwe, crafted, rs, tie, wrapped, ones_slot, bits, log_n, n):
    """the point of the input, from the model's modulus switch of (a, b + 2^(BITS-2)), before the device is called"""
    big_n, batch = 1 << log_n, lwe.size // (n + 1)
    two_n = 2 * big_n
    assert batch in (7, 8, 9) and batch % 3 != 0                     # chunk = 3: several chunks, a partial last one
    off = cm.offset_inputs(lwe, n, bits)
    assert np.array_equal(off, crafted)                              # the handle's offset undoes the subtraction
    exps, neg_b = bs.modulus_switch(off, n, bits, log_n)
    assert neg_b[:len(rs)].tolist() == rs == sorted({0, 1, big_n - 1, big_n, big_n + 1, two_n - 1})
    b_off = off.reshape(batch, n + 1)[:, n]
    assert bs.sw(int(b_off[tie]) - 1, bits, log_n) == 1 and neg_b[tie] == two_n - 2                   # ties go up
    assert int(b_off[wrapped]) == 2 ** bits - 1 and neg_b[wrapped] == 0
    assert {0, big_n - 1, big_n, two_n - 1} <= set(exps.reshape(-1).tolist())
    assert int(off.reshape(batch, n + 1)[:, :n].reshape(-1)[ones_slot]) == 2 ** bits - 1 and exps.reshape(-1)[ones_slot] == 0
    assert np.count_nonzero(exps) >= 3
    wraps = sum(int(v) + (1 << (bits - 2)) >= 1 << bits for v in lwe.reshape(batch, n + 1)[:, n])
    assert wraps >= 1                                                # the kernel's b + 2^(BITS-2) overflows the word
    return neg_b


def case_inputs(bits, log_n, k, cbs, pfks):
    """the crafted batch of one case, checked: (rng, lwe, neg_b)"""
    rng = np.random.default_rng(9500 * bits + 100 * k + 10 * log_n + cbs[0] + pfks[0])
    lwe, crafted, rs, tie, wrapped, ones_slot = crafted_cbs_lwe(rng, bits, log_n, LWE_DIM)
    neg_b = assert_inputs_sit_on_the_branch_points(lwe, crafted, rs, tie, wrapped, ones_slot, bits, log_n, LWE_DIM)
    return rng, lwe, neg_b


@pytest.mark.parametrize("bits,log_n,k,lb,ell,cbs,pfks", CBS_CASES,
                         ids=["u%d-N%d-k%d-cbs%s-pfks%s" % (c[0], 1 << c[1], c[2], c[5], c[6]) for c in CBS_CASES])
def test_handle_at_small_n_and_the_branch_points(p, bits, log_n, k, lb, ell, cbs, pfks):
    """keys |g| <= 2^10 under (k+1) ell N 2^(logB-1) 2^10 <= 2^40 and a full-range private-key-switch key: the rotation is the
    integer schoolbook, every other stage is integer arithmetic, and tfhe_cbs_model.circuit_bootstrap is the reference
    word for word.  A handle of chunk 3 and a default one, each called twice into an output of all-ones; rows of (k+1) N
    words, so that a failure names the input, the GGSW row and the level."""
    n, gmax, big_n = LWE_DIM, 1024, 1 << log_n
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    assert (k + 1) * mb.decompose_length * big_n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    cbs_b, pfks_b = p.ApproxSignedBasis(bits, *cbs), p.ApproxSignedBasis(bits, *pfks)
    cbs_mb, pfks_mb = m.ApproxSignedBasis(bits, *cbs), m.ApproxSignedBasis(bits, *pfks)
    assert cbs_b.drop_bits() == cbs_mb.drop_bits >= 1 and pfks_b.drop_bits() == pfks_mb.drop_bits
    if cbs != CBS_BASIS:
        assert cbs_mb.drop_bits == 1 and cm.half_gadget(cbs_mb, 0) == 1
    if pfks != PFKS_BASIS:
        assert pfks_mb.drop_bits == 0
    levels = cbs_mb.decompose_length
    rng, lwe, neg_b = case_inputs(bits, log_n, k, cbs, pfks)
    batch = lwe.size // (n + 1)

    fft = p.FullComplex64FftTable(log_n)
    keys = [small_key(rng, bits, log_n, k, mb.decompose_length, gmax) for _ in range(n)]
    pfksk = rand_words(rng, bits, (k + 1) * (k * big_n + 1) * pfks_mb.decompose_length * (k + 1) * big_n)
    want = cm.circuit_bootstrap(lwe, keys, pfksk, mb, cbs_mb, pfks_mb, log_n, k, n)
    rows = f"row r is input r // {(k + 1) * levels}, GGSW row r // {levels} % {k + 1}, level r % {levels}; neg_b {neg_b.tolist()}"

    d_lwe, d_pfksk = dev_words(lwe, bits), dev_words(pfksk, bits)
    bsk = None
    for chunk in (3, 0):
        ctx = p.TfheCircuitBootstrapContext(fft, b, n, k, cbs_b, pfks_b, chunk=chunk)
        assert ctx.pfksk_len() == pfksk.size and batch * ctx.ggsw_len() == want.size
        if bsk is None:
            bsk = device_keys(p, fft, ctx, keys, bits)
        for run in ("first", "repeated"):
            got = handle_run(p, ctx, d_lwe, bsk, d_pfksk, bits)          # into an output of all-ones
            assert_same_rows(host_words(got, bits), want, (k + 1) * big_n, f"chunk {chunk}, {run} call; {rows}")
    if (bits, log_n, k) in HOST_FORM:
        host_out = np.full(want.size, 2 ** bits - 1, m.UINT[bits])
        p.tfhe_circuit_bootstrap(lwe, bsk.cpu().numpy(), pfksk, host_out, ctx)
        assert_same_rows(host_out, want, (k + 1) * big_n, f"host form; {rows}")


# ---------------- B. one handle, one stream after another ----------------

STREAM_CHUNK, LONG_BATCH, SHORT_BATCH = 2, 24, 3       # the long call is 12 chunks


def zeros(size, bits):
    import torch
    return torch.zeros(size, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")


def fourier_form(p, fft, torus):
    """full-torus Fourier keys from random torus words, through the device forward"""
    import torch
    out = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, out, fft)
    return out


def one_stream_after_another(make, long, short, row_len, bits):
    """long and short: (call(ctx, out, stream), words of the output).  The long call on stream 1, the short one on stream 2
    queued right behind it with nothing in between, and the long one again on stream 1, STREAM_ROUNDS times; every output
    word for word what a second handle from `make` gave that ran alone.  Every round takes another pair of streams: with one
    pair for all rounds a handle whose ordering was taken out could still pass, depending on what the process had run
    before (the module's docstring; two streams that the runtime serves from one hardware queue would run one after the
    other whatever the library does)."""
    import torch
    alone = make()
    want = [zeros(size, bits) for _, size in (long, short)]
    for (call, _), out in zip((long, short), want):
        call(alone, out, None)
    torch.cuda.synchronize()
    want_long, want_short = want
    assert not torch.equal(want_long[:want_short.numel()], want_short) and want_long.any() and want_short.any()
    ctx = make()
    for rnd in range(STREAM_ROUNDS):
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1, o2, o3 = torch.zeros_like(want_long), torch.zeros_like(want_short), torch.zeros_like(want_long)
        torch.cuda.synchronize()
        long[0](ctx, o1, s1.cuda_stream)
        short[0](ctx, o2, s2.cuda_stream)                            # nothing in between
        long[0](ctx, o3, s1.cuda_stream)                             # and back
        s1.synchronize(); s2.synchronize()
        for what, got, ref in (("long", o1, want_long), ("short", o2, want_short), ("long again", o3, want_long)):
            assert_same_rows(host_words(got, bits), host_words(ref, bits), row_len, f"round {rnd}, {what}")
    assert not ctx.in_use()
    return ctx


def test_circuit_bootstrap_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p):
    """The handle's accumulators, exponents, neg_b and extracted ciphertexts are shared by all its calls, and so is the
    rotation it owns, whose guard is taken inside the handle's own.  u32, N = 2^8, k = 1, full-torus keys; 256 steps, so
    that a chunk's rotation outlasts the queueing of the next call."""
    bits, log_n, k, n = 32, 8, 1, 256
    rng = np.random.default_rng(9600)
    fft = p.FullComplex64FftTable(log_n)
    basis, cbs_b, pfks_b = (p.ApproxSignedBasis(bits, *b) for b in ((7, 3), CBS_BASIS, PFKS_BASIS))
    make = lambda: p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_b, pfks_b, chunk=STREAM_CHUNK)
    shape = make()
    bsk = fourier_form(p, fft, dev_words(rand_words(rng, bits, shape.bsk_len()), bits))
    pfksk = dev_words(rand_words(rng, bits, shape.pfksk_len()), bits)

    def inputs(batch):
        lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
        return (lambda ctx, out, stream: p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx, stream)), batch * shape.ggsw_len()

    one_stream_after_another(make, inputs(LONG_BATCH), inputs(SHORT_BATCH), (k + 1) << log_n, bits)


@pytest.mark.parametrize("form", ["fused", "general"])
def test_cmux_tree_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p, form):
    """Both node buffers are shared by all calls of a tree handle; the general form also shares D, E and the product plan.
    fused: u32, N = 2^8, k = 1, depth 4, a table per input, a long call of 96 inputs (one small launch per level and chunk:
    48 chunks keep the device behind the host).  general: u64, N = 2^11, k = 2, depth 3, and the short call is
    tfhe_cmux_dev on the same handle, which writes the D and E the tree's levels use."""
    bits, log_n, k, depth, long_batch = (32, 8, 1, 4, 4 * LONG_BATCH) if form == "fused" else (64, 11, 2, 3, LONG_BATCH)
    rng = np.random.default_rng(9700 + depth)
    fft = p.FullComplex64FftTable(log_n)
    basis = p.ApproxSignedBasis(bits, *((7, 3) if bits == 32 else (15, 2)))
    make = lambda: p.TfheCmuxTreeContext(fft, basis, k, depth, chunk=STREAM_CHUNK)
    shape = make()
    glwe, key_len = shape.glwe_len(), shape.key_len()
    assert shape.scratch_bytes() > 0

    def tree(batch):
        table = dev_words(rand_words(rng, bits, batch * (glwe << depth)), bits)
        selectors = fourier_form(p, fft, dev_words(rand_words(rng, bits, batch * depth * key_len), bits))
        return (lambda ctx, out, stream: p.tfhe_cmux_tree_dev(table, selectors, out, ctx, stream)), batch * glwe

    def cmux(count):
        d0, d1 = (dev_words(rand_words(rng, bits, count * glwe), bits) for _ in range(2))
        keys = fourier_form(p, fft, dev_words(rand_words(rng, bits, count * key_len), bits))
        return (lambda ctx, out, stream: p.tfhe_cmux_dev(d0, d1, keys, out, ctx, 1, stream)), count * glwe

    short = tree(SHORT_BATCH) if form == "fused" else cmux(SHORT_BATCH)
    one_stream_after_another(make, tree(long_batch), short, glwe, bits)


@pytest.mark.parametrize("form,bits,log_n,k", [("general", 32, 12, 1), ("general", 64, 11, 2), ("fused", 32, 10, 1)])
def test_trace_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p, form, bits, log_n, k):
    """The general form shares D, the gathered bodies, E and the product's scratch between its calls, and the chunks of a
    call write their own output in between: the full trace, log N steps.  At the fused shape the handle owns no buffer
    between its calls (scratch_bytes() == 0): there the case pins only that the calls do not disturb each other."""
    rng = np.random.default_rng(9800 + bits + log_n)
    fft = p.FullComplex64FftTable(log_n)
    basis = p.ApproxSignedBasis(bits, *((7, 3) if bits == 32 else (15, 2)))
    make = lambda: p.TfheGlweTraceContext(fft, basis, k, chunk=STREAM_CHUNK)
    shape = make()
    assert (shape.scratch_bytes() == 0) == (form == "fused") == (k == 1 and log_n <= 11)
    glwe = shape.glwe_len()
    keys = fourier_form(p, fft, dev_words(rand_words(rng, bits, log_n * shape.key_len()), bits))

    def inputs(batch):
        inp = dev_words(rand_words(rng, bits, batch * glwe), bits)
        return (lambda ctx, out, stream: p.glwe_trace_dev(inp, keys, out, ctx, None, stream)), batch * glwe

    one_stream_after_another(make, inputs(LONG_BATCH), inputs(SHORT_BATCH), glwe, bits)


def test_packing_plan_used_from_one_stream_after_another_is_ordered_by_the_library(p):
    """The plan's partial spectra are shared by all its calls, and the call reaches ordered_on by a route of its own (from
    inside stateless_call, not through handle_call).  u32, N = 2^10, k = 1, 13 mask words: three whole slices and a partial
    one, 1000 ciphertexts per group."""
    import torch
    bits, log_n, k, in_dim, count = 32, 10, 1, 13, 1000
    rng = np.random.default_rng(9900)
    fft = p.FullComplex64FftTable(log_n)
    basis = p.ApproxSignedBasis(bits, 4, 3)
    make = lambda: p.TfhePackFftContext(fft, basis, in_dim, k, STREAM_CHUNK)
    shape = make()
    assert shape.scratch_bytes() == STREAM_CHUNK * 4 * (k + 1) * (1 << (log_n - 1)) * 16
    fkey = torch.empty(shape.fkey_len, dtype=torch.complex128, device="cuda")
    p.tfhe_pack_key_fourier_dev(dev_words(rand_words(rng, bits, shape.pksk_len()), bits), fkey, shape)

    def inputs(batch):
        lwe = dev_words(rand_words(rng, bits, batch * count * (in_dim + 1)), bits)
        return (lambda ctx, out, stream: p.lwe_pack_keyswitch_fft_dev(lwe, fkey, out, count, ctx, stream)), batch * shape.glwe_len()

    one_stream_after_another(make, inputs(LONG_BATCH), inputs(SHORT_BATCH), shape.glwe_len(), bits)
