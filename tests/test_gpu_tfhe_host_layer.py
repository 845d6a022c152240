"""What the torus entry points (csrc/pfhe_fft.hip, pfhe_bootstrap.hip, pfhe_keygen.hip, pfhe_cbs.hip, pfhe_cmux.hip; for the
allocations also pfhe_trace.hip and pfhe_pack_fft.hip) share on
the host side, pinned where the other torus tests leave it open: every host form against its device form word for word, the status and the
pfhe_last_error() text of every refusal that is decided before a launch (and their order), a zero batch, and what each
handle kind allocates.  All at N = 8 with batch 3 on handles of chunk 2, so every chunk loop runs a full and a short chunk."""
import ctypes as C
import os

import numpy as np
import pytest

import tfhe_fft_model as m
from test_gpu_tfhe_fft import dev_complex, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

LOG_N, N = 3, 8
BASES = {32: (7, 2), 64: (15, 2)}      # the product's (log B, ell) per width
KS = (4, 3)                            # the key switch's
LWE, G, BATCH, CHUNK = 4, 2, 3, 2
SWITCH = "PFHE_DISABLE_FUSED_TFHE_BLINDROT"
BAD_LENGTH, BAD_ARGUMENT = 32, 33


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def forced(make):
    """a handle created with the switch set: the per-step / per-group form on the fused shape"""
    os.environ[SWITCH] = "1"
    try:
        return make()
    finally:
        os.environ.pop(SWITCH, None)


def fourier(rng, size, bits):
    """random spectra large enough that a product of digits and these fills the torus words of either width"""
    return (rng.standard_normal(size) + 1j * rng.standard_normal(size)) * 2.0 ** (bits - 22)


def dev_exps(x):
    import torch
    return torch.from_numpy(x.view(np.int32)).cuda()


def bases(p, bits):
    return p.ApproxSignedBasis(bits, *BASES[bits]), p.ApproxSignedBasis(bits, *KS)


# ---------------- host form = device form ----------------

@pytest.mark.parametrize("bits", [32, 64])
def test_transform_slices_equal_the_device_forms(p, bits):
    import torch
    rng = np.random.default_rng(bits)
    fft = p.FullComplex64FftTable(LOG_N)
    x = rand_words(rng, bits, BATCH * N)
    host_y, dev_y = np.zeros(x.size, np.complex128), torch.zeros(x.size, dtype=torch.complex128, device="cuda")
    fft.forward_torus_slice(x, host_y)
    fft.forward_torus_dev(dev_words(x, bits), dev_y)
    assert np.array_equal(host_y, dev_y.cpu().numpy())
    y = fourier(rng, x.size, bits)                                   # not Hermitian: the inverse forms the Hermitian part
    host_x, dev_x = np.zeros(x.size, m.UINT[bits]), dev_words(np.zeros(x.size, m.UINT[bits]), bits)
    fft.inverse_torus_slice(y, host_x)
    fft.inverse_torus_dev(dev_complex(y), dev_x)
    assert np.array_equal(host_x, host_words(dev_x, bits))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])                          # the fused and the general product
def test_product_host_equals_device(p, bits, k):
    rng = np.random.default_rng(bits + k)
    fft, (basis, _) = p.FullComplex64FftTable(LOG_N), bases(p, bits)
    ctx = p.TfheFftContext(fft, basis, k, chunk=CHUNK)
    inp, key = rand_words(rng, bits, BATCH * ctx.glwe_len()), fourier(rng, ctx.key_len(), bits)
    host_out, dev_out = np.zeros(inp.size, m.UINT[bits]), dev_words(np.zeros(inp.size, m.UINT[bits]), bits)
    p.tfhe_external_product_to(inp, key, host_out, ctx)
    p.tfhe_external_product_to_dev(dev_words(inp, bits), dev_complex(key), dev_out, ctx)
    assert np.array_equal(host_out, host_words(dev_out, bits))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k,per_step", [(1, False), (1, True), (2, True)])     # the whole loop; the per-step / per-group form
@pytest.mark.parametrize("multibit", [False, True])
def test_rotation_host_equals_device(p, bits, k, per_step, multibit):
    rng = np.random.default_rng(bits + 3 * k + multibit)
    fft, (basis, _) = p.FullComplex64FftTable(LOG_N), bases(p, bits)
    if multibit:
        make = lambda: p.TfheMultiBitBlindRotateContext(fft, basis, G, k, chunk=CHUNK)
        keys, rotate, rotate_dev = (LWE // G) << G, p.tfhe_multibit_blind_rotate, p.tfhe_multibit_blind_rotate_dev
    else:
        make = lambda: p.TfheBlindRotateContext(fft, basis, k, chunk=CHUNK)
        keys, rotate, rotate_dev = LWE, p.tfhe_blind_rotate, p.tfhe_blind_rotate_dev
    ctx = forced(make) if per_step else make()
    assert (ctx.scratch_bytes() > 0) == per_step
    acc, bsk = rand_words(rng, bits, BATCH * ctx.glwe_len()), fourier(rng, keys * ctx.key_len(), bits)
    exps = rng.integers(0, 2 * N, BATCH * LWE).astype(np.uint32)
    exps[:3] = (0, N, 2 * N - 1)
    host_acc, dev_acc = acc.copy(), dev_words(acc, bits)
    rotate(host_acc, bsk, exps, ctx)
    rotate_dev(dev_acc, dev_complex(bsk), dev_exps(exps), ctx)
    assert np.array_equal(host_acc, host_words(dev_acc, bits)) and not np.array_equal(host_acc, acc)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
def test_stateless_host_forms_equal_the_device_forms(p, bits, k):
    """sample extraction, the key switch at (4, 3), the LWE and the GLWE body, the packing key switch of 3 ciphertexts
    per GLWE at (4, 3), the first-few extraction and its expansion"""
    rng = np.random.default_rng(bits + 5 * k)
    fft, (_, ks_basis) = p.FullComplex64FftTable(LOG_N), bases(p, bits)
    zeros = lambda size: np.zeros(size, m.UINT[bits])
    glwe = rand_words(rng, bits, BATCH * (k + 1) * N)
    host_lwe, dev_lwe = zeros(BATCH * (k * N + 1)), dev_words(zeros(BATCH * (k * N + 1)), bits)
    p.glwe_sample_extract(glwe, host_lwe, fft, k, N - 1)
    p.glwe_sample_extract_dev(dev_words(glwe, bits), dev_lwe, fft, k, N - 1)
    assert np.array_equal(host_lwe, host_words(dev_lwe, bits))
    ksk = rand_words(rng, bits, k * N * KS[1] * (LWE + 1))
    host_out, dev_out = zeros(BATCH * (LWE + 1)), dev_words(zeros(BATCH * (LWE + 1)), bits)
    p.lwe_keyswitch(host_lwe, ksk, host_out, k * N, LWE, ks_basis)
    p.lwe_keyswitch_dev(dev_lwe, dev_words(ksk, bits), dev_out, k * N, LWE, ks_basis)
    assert np.array_equal(host_out, host_words(dev_out, bits))
    lwe_key, glwe_key = rand_words(rng, bits, LWE), rand_words(rng, bits, k * N)
    for encrypt, encrypt_dev in ((p.lwe_encrypt, p.lwe_encrypt_dev), (p.lwe_phase, p.lwe_phase_dev)):
        host_ct, dev_ct = host_out.copy(), dev_words(host_out, bits)
        encrypt(host_ct, lwe_key)
        encrypt_dev(dev_ct, dev_words(lwe_key, bits))
        assert np.array_equal(host_ct, host_words(dev_ct, bits)) and not np.array_equal(host_ct, host_out)
    for encrypt, encrypt_dev in ((p.glwe_encrypt, p.glwe_encrypt_dev), (p.glwe_phase, p.glwe_phase_dev)):
        host_ct, dev_ct = glwe.copy(), dev_words(glwe, bits)
        encrypt(host_ct, glwe_key, fft, k)
        encrypt_dev(dev_ct, dev_words(glwe_key, bits), fft, k)
        assert np.array_equal(host_ct, host_words(dev_ct, bits)) and not np.array_equal(host_ct, glwe)
    count = 3
    lwe_in, pksk = rand_words(rng, bits, BATCH * count * (LWE + 1)), rand_words(rng, bits, LWE * KS[1] * (k + 1) * N)
    host_glwe, dev_glwe = zeros(BATCH * (k + 1) * N), dev_words(zeros(BATCH * (k + 1) * N), bits)
    p.lwe_pack_keyswitch(lwe_in, pksk, host_glwe, LWE, count, fft, ks_basis, k)
    p.lwe_pack_keyswitch_dev(dev_words(lwe_in, bits), dev_words(pksk, bits), dev_glwe, LWE, count, fft, ks_basis, k)
    assert np.array_equal(host_glwe, host_words(dev_glwe, bits)) and host_glwe.any()
    host_multi, dev_multi = zeros(BATCH * (k * N + count)), dev_words(zeros(BATCH * (k * N + count)), bits)
    p.glwe_sample_extract_first_few(host_glwe, host_multi, fft, count, k)
    p.glwe_sample_extract_first_few_dev(dev_glwe, dev_multi, fft, count, k)
    assert np.array_equal(host_multi, host_words(dev_multi, bits)) and host_multi.any()
    host_each, dev_each = zeros(BATCH * count * (k * N + 1)), dev_words(zeros(BATCH * count * (k * N + 1)), bits)
    p.multimsg_lwe_extract(host_multi, host_each, fft, count, k)
    p.multimsg_lwe_extract_dev(dev_multi, dev_each, fft, count, k)
    assert np.array_equal(host_each, host_words(dev_each, bits)) and host_each.any()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("grouping", [1, G])                   # the classic and the multi-bit rotation
def test_bootstrap_host_equals_device(p, bits, k, grouping):
    rng = np.random.default_rng(bits + 7 * k + grouping)
    fft, (basis, ks_basis) = p.FullComplex64FftTable(LOG_N), bases(p, bits)
    lwe = rand_words(rng, bits, BATCH * (LWE + 1))
    for with_ks in (True, False):
        ctx = p.TfheBootstrapContext(fft, basis, LWE, k, ks_basis if with_ks else None, chunk=CHUNK, grouping_factor=grouping)
        bsk = fourier(rng, ctx.bsk_len(), bits)
        ksk = rand_words(rng, bits, ctx.ksk_len()) if with_ks else None
        for tvs in (1, BATCH):                                 # one test vector for the batch, one per ciphertext
            tv = rand_words(rng, bits, tvs * ctx.glwe_len())
            host_out = np.zeros(BATCH * ctx.out_len(), m.UINT[bits])
            dev_out = dev_words(host_out, bits)
            p.tfhe_bootstrap(lwe, bsk, tv, ksk, host_out, ctx)
            p.tfhe_bootstrap_dev(dev_words(lwe, bits), dev_complex(bsk), dev_words(tv, bits),
                                 None if ksk is None else dev_words(ksk, bits), dev_out, ctx)
            assert np.array_equal(host_out, host_words(dev_out, bits)) and host_out.any(), (with_ks, tvs)


def handle_cases(p, rng, bits, k):
    """(name, host call, device call, input arrays, words of the output) of the circuit bootstrap, the CMUX and the CMUX tree
    on chunk-2 handles.  The CMUX handle of depth 2 launches 4 nodes at a time: 6 nodes with per_key = 3 put the second
    key group across the launch boundary; the tree runs with a table per input and with one for the batch."""
    fft, (basis, ks_basis) = p.FullComplex64FftTable(LOG_N), bases(p, bits)
    cbs = p.TfheCircuitBootstrapContext(fft, basis, LWE, k, basis, ks_basis, chunk=CHUNK)
    yield ("cbs", lambda *a: p.tfhe_circuit_bootstrap(*a, cbs), lambda *a: p.tfhe_circuit_bootstrap_dev(*a, cbs),
           (rand_words(rng, bits, BATCH * (LWE + 1)), fourier(rng, cbs.bsk_len(), bits), rand_words(rng, bits, cbs.pfksk_len())),
           BATCH * cbs.ggsw_len())
    tree = p.TfheCmuxTreeContext(fft, basis, k, 2, chunk=CHUNK)
    glwe, key, count, per_key = tree.glwe_len(), tree.key_len(), 6, 3
    yield ("cmux", lambda *a: p.tfhe_cmux(*a, tree, per_key), lambda *a: p.tfhe_cmux_dev(*a, tree, per_key),
           (rand_words(rng, bits, count * glwe), rand_words(rng, bits, count * glwe), fourier(rng, count // per_key * key, bits)),
           count * glwe)
    for tables in (BATCH, 1):
        yield ("cmux_tree, %d table(s)" % tables, lambda *a: p.tfhe_cmux_tree(*a, tree), lambda *a: p.tfhe_cmux_tree_dev(*a, tree),
               (rand_words(rng, bits, tables * 4 * glwe), fourier(rng, BATCH * 2 * key, bits)), BATCH * glwe)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])                          # the fused and the general form
def test_handle_host_equals_device(p, bits, k):
    rng = np.random.default_rng(bits + 11 * k)
    for name, host_call, dev_call, inputs, out_words in handle_cases(p, rng, bits, k):
        host_out = np.zeros(out_words, m.UINT[bits])
        dev_out = dev_words(host_out, bits)
        host_call(*inputs, host_out)
        dev_call(*[dev_complex(x) if x.dtype == np.complex128 else dev_words(x, bits) for x in inputs], dev_out)
        assert np.array_equal(host_out, host_words(dev_out, bits)) and host_out.any(), name


# ---------------- what each handle kind allocates ----------------
#
# scratch_bytes() and the allocations of a create (as many frees in the destroy), per width, at N = 8 (N/2 = 4 complex
# slots of 16 bytes), ell = 2, chunk 2, lwe_dimension 4, W = 4 or 8 bytes per word:
#   general product, k = 2   spec 2*3*2*4*16 = 768, acc 2*3*4*16 = 384, keyh 3*2*3*4*16 = 1152: three buffers, 2304 bytes
#   per-step glue            three buffers of chunk*(k+1)*N words: 3*2*16*W at k = 1, 3*2*24*W at k = 2
#   per-group multi-bit      the product's three with 2^g = 4 keys' Hermitian parts: k = 1: 512 + 256 + 4*512 = 2816,
#                            k = 2: 768 + 384 + 4*1152 = 5760
#   bootstrap                the rotation's plus acc chunk*(k+1)*N*W, extracted chunk*(k*N+1)*W (with a key switch only),
#                            exps chunk*4*4 = 32 and neg_b chunk*4 = 8: k = 1: 240 / 440 (168 / 296 without), k = 2: 368 / 696
#   many-LUT bootstrap       log_luts = 1: two outputs per input, so extracted holds (chunk*2)*(k*N+1) words; the rest as the
#                            bootstrap's.  k = 1 with a key switch: acc 2*16 W, extracted 4*9 W, exps 32, neg_b 8:
#                            68 W + 40 = 312 / 584, four buffers
#   the fused product and the whole-loop rotations own nothing
# The handles of DESIGN.md §18-21, from the buffer lists in their header comments (csrc/pfhe_pack_fft.hip, pfhe_cbs.hip,
# pfhe_cmux.hip, pfhe_trace.hip), not from the numbers the code gives:
#   circuit bootstrap        output basis = the product's (two levels), so chunk 2 is 4 accumulators, and the rotation it
#                            owns is created for a chunk of 4.  Its own four buffers: acc 4*(k+1)*N*W, extracted
#                            4*(k*N+1)*W, exps 4*4*4 = 64, neg_b 2*4 = 8.
#                            k = 1 (whole loop, nothing more): 64 W + 36 W + 72 = 472 / 872.
#                            k = 2: 96 W + 68 W + 72 = 728 / 1384, plus the per-step rotation at chunk 4: the product's
#                            spec 4*3*2*4*16 = 1536, acc 4*3*4*16 = 768, keyh 1152 = 3456 and three glue buffers of
#                            4*24 W = 1152 / 2304: 5336 / 7144 in 4 + 6 buffers
#                            shared rotation, k = 1: one accumulator per input, so the rotation is created for a chunk of 2;
#                            acc 2*16 W, extracted still 4*9 W, exps 2*4*4 = 32, neg_b 8: 68 W + 40 = 312 / 584 in four
#   CMUX tree                node buffers of chunk*2^(d-1) and chunk*2^(d-2) ciphertexts (depth 1 none, depth 2 one); the
#                            general form adds D and E of chunk*2^(d-1) ciphertexts and a product plan of the DEFAULT chunk
#                            (§11: what fits 256 MiB at (k+1)(ell+1) N/2 = 3*3*4 complex values = 576 bytes a
#                            ciphertext, floor(2^28 / 576) = 466033 of them, and the Hermitian parts of one key, 1152):
#                            PLAN = 466033 * 576 + 1152 = 268436160 in three buffers.
#                            fused (k = 1, 16 words a ciphertext): depth 1 nothing; depth 3: (8 + 4)*16 W = 768 / 1536, two
#                            general (k = 2, 24 words): depth 1: D, E of 2 ciphertexts, 96 W = 384 / 768, + PLAN, 2 + 3;
#                            depth 3: (8 + 4 + 8 + 8)*24 W = 2688 / 5376, + PLAN, 4 + 3
#   trace                    fused: nothing.  general, k = 2: the product's scratch at chunk 2 (the "plan general" row: 2304)
#                            and D 2*2*8 W, the gathered bodies 2*8 W, E 2*24 W = 96 W = 384 / 768: six buffers
#   packing plan             the partial half spectra, chunk x ceil(in_dimension / 4) x (k+1) x N/2 complex values: 5 mask
#                            words are 2 slices, 2*2*2*4*16 = 512, one buffer
CMUX_PLAN = 466033 * 576 + 1152
HANDLES = {
    "plan fused": (lambda p, f, b, ks: p.TfheFftContext(f, b, 1, chunk=CHUNK), False, {32: (0, 0), 64: (0, 0)}),
    "plan general": (lambda p, f, b, ks: p.TfheFftContext(f, b, 2, chunk=CHUNK), False, {32: (2304, 3), 64: (2304, 3)}),
    "rotation whole loop": (lambda p, f, b, ks: p.TfheBlindRotateContext(f, b, 1, chunk=CHUNK), False, {32: (0, 0), 64: (0, 0)}),
    "rotation per step, switch": (lambda p, f, b, ks: p.TfheBlindRotateContext(f, b, 1, chunk=CHUNK), True,
                                  {32: (384, 3), 64: (768, 3)}),
    "rotation per step": (lambda p, f, b, ks: p.TfheBlindRotateContext(f, b, 2, chunk=CHUNK), False,
                          {32: (2304 + 576, 6), 64: (2304 + 1152, 6)}),
    "multi-bit whole loop": (lambda p, f, b, ks: p.TfheMultiBitBlindRotateContext(f, b, G, 1, chunk=CHUNK), False,
                             {32: (0, 0), 64: (0, 0)}),
    "multi-bit per group, switch": (lambda p, f, b, ks: p.TfheMultiBitBlindRotateContext(f, b, G, 1, chunk=CHUNK), True,
                                    {32: (2816, 3), 64: (2816, 3)}),
    "multi-bit per group": (lambda p, f, b, ks: p.TfheMultiBitBlindRotateContext(f, b, G, 2, chunk=CHUNK), False,
                            {32: (5760, 3), 64: (5760, 3)}),
    "bootstrap over the whole loop": (lambda p, f, b, ks: p.TfheBootstrapContext(f, b, LWE, 1, ks, chunk=CHUNK), False,
                                      {32: (240, 4), 64: (440, 4)}),
    "bootstrap without key switch": (lambda p, f, b, ks: p.TfheBootstrapContext(f, b, LWE, 1, None, chunk=CHUNK), False,
                                     {32: (168, 3), 64: (296, 3)}),
    "bootstrap per step": (lambda p, f, b, ks: p.TfheBootstrapContext(f, b, LWE, 2, ks, chunk=CHUNK), False,
                           {32: (2880 + 368, 10), 64: (3456 + 696, 10)}),
    "bootstrap over the multi-bit whole loop": (
        lambda p, f, b, ks: p.TfheBootstrapContext(f, b, LWE, 1, ks, chunk=CHUNK, grouping_factor=G), False,
        {32: (240, 4), 64: (440, 4)}),
    "bootstrap per group": (lambda p, f, b, ks: p.TfheBootstrapContext(f, b, LWE, 2, ks, chunk=CHUNK, grouping_factor=G), False,
                            {32: (5760 + 368, 7), 64: (5760 + 696, 7)}),
    "bootstrap many-LUT": (lambda p, f, b, ks: p.TfheBootstrapContext(f, b, LWE, 1, ks, chunk=CHUNK, log_luts=1), False,
                           {32: (312, 4), 64: (584, 4)}),
    "circuit bootstrap, shared rotation": (
        lambda p, f, b, ks: p.TfheCircuitBootstrapContext(f, b, LWE, 1, b, ks, chunk=CHUNK, shared_rotation=True), False,
        {32: (312, 4), 64: (584, 4)}),
    "circuit bootstrap over the whole loop": (
        lambda p, f, b, ks: p.TfheCircuitBootstrapContext(f, b, LWE, 1, b, ks, chunk=CHUNK), False, {32: (472, 4), 64: (872, 4)}),
    "circuit bootstrap per step": (
        lambda p, f, b, ks: p.TfheCircuitBootstrapContext(f, b, LWE, 2, b, ks, chunk=CHUNK), False,
        {32: (3456 + 1152 + 728, 10), 64: (3456 + 2304 + 1384, 10)}),
    "cmux tree fused, depth 1": (lambda p, f, b, ks: p.TfheCmuxTreeContext(f, b, 1, 1, chunk=CHUNK), False, {32: (0, 0), 64: (0, 0)}),
    "cmux tree fused, depth 3": (lambda p, f, b, ks: p.TfheCmuxTreeContext(f, b, 1, 3, chunk=CHUNK), False,
                                 {32: (768, 2), 64: (1536, 2)}),
    "cmux tree general, depth 1": (lambda p, f, b, ks: p.TfheCmuxTreeContext(f, b, 2, 1, chunk=CHUNK), False,
                                   {32: (384 + CMUX_PLAN, 5), 64: (768 + CMUX_PLAN, 5)}),
    "cmux tree general, depth 3": (lambda p, f, b, ks: p.TfheCmuxTreeContext(f, b, 2, 3, chunk=CHUNK), False,
                                   {32: (2688 + CMUX_PLAN, 7), 64: (5376 + CMUX_PLAN, 7)}),
    "trace fused": (lambda p, f, b, ks: p.TfheGlweTraceContext(f, b, 1, chunk=CHUNK), False, {32: (0, 0), 64: (0, 0)}),
    "trace general": (lambda p, f, b, ks: p.TfheGlweTraceContext(f, b, 2, chunk=CHUNK), False,
                      {32: (2304 + 384, 6), 64: (2304 + 768, 6)}),
    "packing plan": (lambda p, f, b, ks: p.TfhePackFftContext(f, ks, 5, 1, CHUNK), False, {32: (512, 1), 64: (512, 1)}),
}


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", sorted(HANDLES))
def test_handle_scratch_and_allocations(p, bits, kind):
    make, switch, want = HANDLES[kind]
    scratch, allocs = want[bits]
    fft, (basis, ks_basis) = p.FullComplex64FftTable(LOG_N), bases(p, bits)
    count = p.lib().pfhe_debug_alloc_count
    before = count()
    ctx = forced(lambda: make(p, fft, basis, ks_basis)) if switch else make(p, fft, basis, ks_basis)
    created = count()
    assert ctx.scratch_bytes() == scratch and created - before == allocs and not ctx.in_use()
    ctx.__del__()
    assert count() - created == allocs


# ---------------- refusals ----------------

SENTINEL = "FFT tables cover 1 <= log N <= 14 (the N/2-point transform of a polynomial lives in LDS)"
F64P = C.POINTER(C.c_double)

PRODUCT_LEN = ("TFHE external product: input / output must be batch*(k+1)*N words and the key (k+1)*ell*(k+1)*N complex "
               "values")
ROT_LEN = ("TFHE blind rotation: acc must be batch*(k+1)*N words, bsk n_steps*(k+1)*ell*(k+1)*N complex values and exps "
           "batch*n_steps exponents")
MB_LEN = ("TFHE multi-bit blind rotation: acc must be batch*(k+1)*N words, bsk groups*2^g keys of (k+1)*ell*(k+1)*N complex "
          "values and exps batch*groups*g exponents")
EXTRACT_LEN = "sample extraction: glwe must be batch*(k+1)*N words and lwe batch*(k*N+1)"
KS_LEN = ("key switch: lwe_in must be batch*(in_dimension+1) words, ksk in_dimension*ell*(out_dimension+1) and lwe_out "
          "batch*(out_dimension+1)")
BOOT_LEN = ("TFHE bootstrap: lwe_in must be batch*(n+1) words, bsk n*(k+1)*ell*(k+1)*N complex values, tv (k+1)*N or "
            "batch*(k+1)*N words, ksk k*N*ks_ell*(n+1) words (0 without a key switch) and lwe_out batch*(n+1) (batch*(k*N+1) "
            "without)")
BSK_LEN = ("bootstrapping key: glwe_key must be k*N words, ggsw_torus keys*(k+1)*ell*(k+1)*N words and bsk_out as many "
           "complex values, keys = n or (n/g)*2^g")
CBS_LEN = ("TFHE circuit bootstrap: lwe_in must be batch*(n+1) words, bsk n*(k+1)*ell*(k+1)*N complex values, pfksk "
           "(k+1)*(k*N+1)*pfks_ell*(k+1)*N words and ggsw_out batch*(k+1)*cbs_ell*(k+1)*N")
CMUX_LEN = ("TFHE CMUX: d0, d1 and out must be count*(k+1)*N words, count a multiple of per_key, and keys "
            "(count/per_key)*(k+1)*ell*(k+1)*N complex values")
TREE_LEN = ("TFHE CMUX tree: out must be batch*(k+1)*N words, selectors batch*depth keys of (k+1)*ell*(k+1)*N complex values "
            "and table 2^depth or batch*2^depth ciphertexts")


class Bufs:
    """named buffers of one call: pointers and element counts that a case may bend before the arguments are formed"""

    def __init__(self, sizes, on_device):
        import torch
        self.keep, self.ptr, self.len = {}, {}, {}
        for name, (count, elem) in sizes.items():
            fill = 0 if name == "exps" and not on_device else 0xA5      # the host forms read their exponents
            if on_device:
                t = torch.full((count * elem + 64,), fill, dtype=torch.uint8, device="cuda")
                self.keep[name], self.ptr[name] = t, t.data_ptr()
            else:
                a = np.full(count * elem + 64, fill, np.uint8)
                self.keep[name], self.ptr[name] = a, a.ctypes.data
            self.len[name] = count

    def untouched(self, name):
        return bool((self.keep[name] == 0xA5).all())


def entry_points(p, bits):
    """(name, on_device, {buffer: (elements, bytes each)}, arguments, expectations) of every torus entry point, k = 1.
    Expectations: lengths = the message of a wrong length (None: refused without one), null_first = a null pointer is
    refused before a wrong length, overlap = (bent buffer, onto, message), zero = the lengths of an empty batch,
    out = the buffer such a call must leave alone, exps = the message for a host exponent of 2N."""
    w, W = ("32" if bits == 32 else ""), bits // 8
    fft, (basis, ks_basis) = p.FullComplex64FftTable(LOG_N), bases(p, bits)
    lb, ell = BASES[bits]
    glwe, key = 2 * N, 2 * ell * 2 * N
    plan = p.TfheFftContext(fft, basis, 1, chunk=CHUNK)
    rot = p.TfheBlindRotateContext(fft, basis, 1, chunk=CHUNK)
    mb = p.TfheMultiBitBlindRotateContext(fft, basis, G, 1, chunk=CHUNK)
    boot = p.TfheBootstrapContext(fft, basis, LWE, 1, ks_basis, chunk=CHUNK)
    cbs = p.TfheCircuitBootstrapContext(fft, basis, LWE, 1, basis, ks_basis, chunk=CHUNK)
    tree = p.TfheCmuxTreeContext(fft, basis, 1, 2, chunk=CHUNK)
    keep = (fft, plan, rot, mb, boot, cbs, tree)
    f, t = fft._h, "pfhe_tfhe" + w + "_"
    words = lambda count: (count, W)
    out = []

    def add(name, on_device, sizes, args, **expect):
        out.append((name, on_device, sizes, args, expect, keep))

    for form, dev in (("_dev", True), ("_slice", False)):
        tail = [None] if dev else []
        add("pfhe_fft_forward_torus" + w + form, dev, {"in": words(BATCH * N), "out": (BATCH * N, 16)},
            lambda b, tail=tail: [f, b.ptr["in"], b.len["in"], b.ptr["out"], b.len["out"]] + tail,
            lengths="fft forward: input must be count*N words and output count*N complex values" if dev else None,
            null_first=not dev, zero=("in", "out"), out="out")
        add("pfhe_fft_inverse_torus" + w + form, dev, {"in": (BATCH * N, 16), "out": words(BATCH * N)},
            lambda b, tail=tail: [f, b.ptr["in"], b.len["in"], b.ptr["out"], b.len["out"]] + tail,
            lengths="fft inverse: input must be count*N complex values and output count*N words" if dev else None,
            null_first=not dev, zero=("in", "out"), out="out")
    sizes = {"in": words(BATCH * glwe), "key": (key, 16), "out": words(BATCH * glwe)}
    product = lambda b: [plan._h, b.ptr["in"], b.len["in"], b.ptr["key"], b.len["key"], b.ptr["out"], b.len["out"]]
    add(t + "external_product_to_dev", True, sizes, lambda b: product(b) + [None], lengths=PRODUCT_LEN, null_first=False,
        overlap=("out", "in", "TFHE external product: input and output must be the same buffer or disjoint"),
        zero=("in", "out"), out="out")
    add(t + "external_product_to", False, sizes, product, lengths=None, null_first=True, zero=("in", "out"), out="out")
    for h, keys, per_ct, lengths, what in ((rot, LWE, LWE, ROT_LEN, "TFHE blind rotation"),
                                          (mb, (LWE // G) << G, LWE, MB_LEN, "TFHE multi-bit blind rotation")):
        sizes = {"acc": words(BATCH * glwe), "bsk": (keys * key, 16), "exps": (BATCH * per_ct, 4)}
        rotate = lambda b, h=h: [h._h, b.ptr["acc"], b.len["acc"], b.ptr["bsk"], b.len["bsk"], b.ptr["exps"], b.len["exps"]]
        add(h._pre + "rotate_dev", True, sizes, lambda b, rotate=rotate: rotate(b) + [None], lengths=lengths, null_first=False,
            zero=("acc", "exps"), out="acc")
        add(h._pre + "rotate", False, sizes, rotate, lengths=lengths, null_first=True, zero=("acc", "exps"), out="acc",
            exps=what + ": every exponent must be below 2N")
    add(t + "mul_monomial_each_to_dev", True, {"a": words(BATCH * glwe), "exps": (BATCH, 4), "out": words(BATCH * glwe)},
        lambda b: [f, b.ptr["a"], b.len["a"], b.ptr["exps"], 2, b.ptr["out"], None],
        lengths="mul_monomial_each: len must be a whole number of elements of polys_per_exp * N words", null_first=False,
        overlap=("out", "a", "mul_monomial_each_to needs non-overlapping buffers"), zero=("a",), out="out")
    if bits == 64:
        add("pfhe_tfhe_mb_combine_key_dev", True, {"keys": (key << G, 16), "exps": (G, 4), "out": (key, 16)},
            lambda b: [f, 1, ell, G, b.ptr["keys"], b.len["keys"], b.ptr["exps"], b.len["exps"], b.ptr["out"], b.len["out"],
                       None],
            lengths="multi-bit key combination: keys must be 2^g keys of (k+1)*ell*(k+1)*N complex values, exps g exponents "
                    "and out one key", null_first=False,
            overlap=("out", "keys", "multi-bit key combination: the output must not overlap the keys"))
    add(t + "modswitch_dev", True, {"lwe": words(BATCH * (LWE + 1)), "exps": (BATCH * LWE, 4), "neg_b": (BATCH, 4)},
        lambda b: [0, b.ptr["lwe"], b.len["lwe"], LWE, LOG_N, b.ptr["exps"], b.len["exps"], b.ptr["neg_b"], b.len["neg_b"],
                   None],
        lengths="modulus switch: lwe must be batch*(n+1) words, exps batch*n and neg_b batch exponents", null_first=False,
        zero=("lwe", "exps", "neg_b"), out="exps")
    sizes = {"glwe": words(BATCH * glwe), "lwe": words(BATCH * (N + 1))}
    extract = lambda b: [f, 1, b.ptr["glwe"], b.len["glwe"], 0, b.ptr["lwe"], b.len["lwe"]]
    add(t + "sample_extract_dev", True, sizes, lambda b: extract(b) + [None], lengths=EXTRACT_LEN, null_first=False,
        overlap=("lwe", "glwe", "sample extraction: the output must not overlap the input"), zero=("glwe", "lwe"), out="lwe")
    add(t + "sample_extract", False, sizes, extract, lengths=EXTRACT_LEN, null_first=False, zero=("glwe", "lwe"), out="lwe")
    sizes = {"in": words(BATCH * (N + 1)), "ksk": words(N * KS[1] * (LWE + 1)), "out": words(BATCH * (LWE + 1))}
    switch = lambda b: [0, b.ptr["in"], b.len["in"], N, b.ptr["ksk"], b.len["ksk"], LWE, KS[0], KS[1], b.ptr["out"],
                        b.len["out"]]
    add(t + "keyswitch_dev", True, sizes, lambda b: switch(b) + [None], lengths=KS_LEN, null_first=False,
        overlap=("out", "in", "key switch: the output must not overlap an input"), zero=("in", "out"), out="out")
    add(t + "keyswitch", False, sizes, switch, lengths=KS_LEN, null_first=False, zero=("in", "out"), out="out")
    sizes = {"in": words(BATCH * (LWE + 1)), "bsk": (boot.bsk_len(), 16), "tv": words(glwe), "ksk": words(boot.ksk_len()),
             "out": words(BATCH * (LWE + 1))}
    strap = lambda b: [boot._h, b.ptr["in"], b.len["in"], b.ptr["bsk"], b.len["bsk"], b.ptr["tv"], b.len["tv"], b.ptr["ksk"],
                       b.len["ksk"], b.ptr["out"], b.len["out"]]
    add(t + "bootstrap_dev", True, sizes, lambda b: strap(b) + [None], lengths=BOOT_LEN, null_first=False,
        overlap=("out", "in", "TFHE bootstrap: the output must not overlap an input"), zero=("in", "out"), out="out")
    add(t + "bootstrap", False, sizes, strap, lengths=BOOT_LEN, null_first=False, zero=("in", "out"), out="out")
    sizes = {"lwe": words(BATCH * (LWE + 1)), "key": words(LWE)}
    lwe_body = lambda b: [0, b.ptr["lwe"], b.len["lwe"], LWE, b.ptr["key"], b.len["key"], 0]
    lengths = "LWE body: lwe must be batch*(dimension+1) words and key dimension words"
    add(t + "lwe_body_mac_dev", True, sizes, lambda b: lwe_body(b) + [None], lengths=lengths, null_first=False,
        overlap=("key", "lwe", "LWE body: the key must not overlap the ciphertexts"), zero=("lwe",), out="lwe")
    add(t + "lwe_body_mac", False, sizes, lwe_body, lengths=lengths, null_first=False, zero=("lwe",), out="lwe")
    sizes = {"glwe": words(BATCH * glwe), "key": words(N)}
    glwe_body = lambda b: [f, 1, b.ptr["glwe"], b.len["glwe"], b.ptr["key"], b.len["key"], 0]
    lengths = "GLWE body: glwe must be batch*(k+1)*N words and key k*N words"
    add(t + "glwe_body_mac_dev", True, sizes, lambda b: glwe_body(b) + [None], lengths=lengths, null_first=False,
        overlap=("key", "glwe", "GLWE body: the key must not overlap the ciphertexts"), zero=("glwe",), out="glwe")
    add(t + "glwe_body_mac", False, sizes, glwe_body, lengths=lengths, null_first=False, zero=("glwe",), out="glwe")
    add(t + "ggsw_add_gadget_dev", True, {"ggsw": words(BATCH * key), "msgs": words(BATCH)},
        lambda b: [f, 1, lb, ell, b.ptr["ggsw"], b.len["ggsw"], b.ptr["msgs"], b.len["msgs"], None],
        lengths="GGSW gadget: ggsw must be count*(k+1)*ell*(k+1)*N words and messages count words", null_first=False,
        overlap=("msgs", "ggsw", "GGSW gadget: the messages must not overlap the GGSWs"), zero=("ggsw", "msgs"), out="ggsw")
    add(t + "bsk_generate_dev", True, {"ggsw": words(LWE * key), "lwe_key": words(LWE), "glwe_key": words(N), "bsk": (LWE * key, 16)},
        lambda b: [f, 1, lb, ell, 0, b.ptr["lwe_key"], b.len["lwe_key"], b.ptr["glwe_key"], b.len["glwe_key"], b.ptr["ggsw"],
                   b.len["ggsw"], b.ptr["bsk"], b.len["bsk"], None],
        lengths=BSK_LEN, null_first=False,
        overlap=("ggsw", "glwe_key", "bootstrapping key: the outputs must overlap neither each other nor a key"))
    add(t + "ksk_generate_dev", True, {"ksk": words(N * KS[1] * (LWE + 1)), "key_in": words(N), "key_out": words(LWE)},
        lambda b: [0, b.ptr["key_in"], b.len["key_in"], b.ptr["key_out"], b.len["key_out"], KS[0], KS[1], b.ptr["ksk"],
                   b.len["ksk"], None],
        lengths="key-switch key: ksk must be in_dimension*ell*(out_dimension+1) words", null_first=False,
        overlap=("ksk", "key_in", "key-switch key: the keys must not overlap ksk"))
    sizes = {"in": words(BATCH * (LWE + 1)), "bsk": (cbs.bsk_len(), 16), "pfksk": words(cbs.pfksk_len()),
             "out": words(BATCH * cbs.ggsw_len())}
    circuit = lambda b: [cbs._h, b.ptr["in"], b.len["in"], b.ptr["bsk"], b.len["bsk"], b.ptr["pfksk"], b.len["pfksk"],
                         b.ptr["out"], b.len["out"]]
    add(cbs._pre + "_dev", True, sizes, lambda b: circuit(b) + [None], lengths=CBS_LEN, null_first=False,
        overlap=("out", "in", "TFHE circuit bootstrap: the output must not overlap an input"), zero=("in", "out"), out="out")
    add(cbs._pre, False, sizes, circuit, lengths=CBS_LEN, null_first=False, zero=("in", "out"), out="out")
    sizes = {"d0": words(BATCH * glwe), "d1": words(BATCH * glwe), "keys": (BATCH * key, 16), "out": words(BATCH * glwe)}
    cmux = lambda b: [tree._h, b.ptr["d0"], b.len["d0"], b.ptr["d1"], b.len["d1"], b.ptr["keys"], b.len["keys"], 1, b.ptr["out"],
                      b.len["out"]]
    add(t + "cmux_dev", True, sizes, lambda b: cmux(b) + [None], lengths=CMUX_LEN, null_first=False,
        overlap=("out", "d0", "TFHE CMUX: out must be exactly d0, exactly d1, or disjoint from both, and disjoint from the keys"),
        zero=("d0", "d1", "keys", "out"), out="out")
    add(t + "cmux", False, sizes, cmux, lengths=CMUX_LEN, null_first=True, zero=("d0", "d1", "keys", "out"), out="out")
    sizes = {"table": words(4 * glwe), "selectors": (BATCH * 2 * key, 16), "out": words(BATCH * glwe)}
    select = lambda b: [tree._h, b.ptr["table"], b.len["table"], b.ptr["selectors"], b.len["selectors"], b.ptr["out"],
                        b.len["out"]]
    add(tree._pre + "_dev", True, sizes, lambda b: select(b) + [None], lengths=TREE_LEN, null_first=False,
        overlap=("out", "table", "TFHE CMUX tree: the output must not overlap an input"), zero=("table", "selectors", "out"),
        out="out")
    add(tree._pre, False, sizes, select, lengths=TREE_LEN, null_first=True, zero=("table", "selectors", "out"), out="out")
    return out


def refused(p, name, args):
    """(status, pfhe_last_error()) of one call; the text is SENTINEL when the call set none"""
    lib = p.lib()
    assert lib.pfhe_fft_create(0, 0, C.byref(C.c_void_p())) != 0          # leaves SENTINEL as the last error
    fn = getattr(lib, name)
    assert len(args) == len(fn.argtypes), name
    status = fn(*[C.cast(C.c_void_p(a), F64P) if kind == F64P else a for a, kind in zip(args, fn.argtypes)])
    return status, lib.pfhe_last_error().decode()


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals_before_a_launch(p, bits):
    import torch
    seen = 0
    for name, on_device, sizes, args, expect, _keep in entry_points(p, bits):
        first = next(iter(sizes))                              # the buffer whose pointer and length the cases bend
        text = lambda message: SENTINEL if message is None else message
        wrong_length = (BAD_LENGTH, text(expect["lengths"]))

        def case(bend):
            b = Bufs(sizes, on_device)
            bend(b)
            return refused(p, name, args(b)), b

        def null(b):
            b.ptr[first] = None

        def short(b):
            b.len[first] -= 1

        def both(b):
            null(b), short(b)

        assert case(null)[0] == (BAD_ARGUMENT, SENTINEL), name
        assert case(short)[0] == wrong_length, name
        assert case(both)[0] == ((BAD_ARGUMENT, SENTINEL) if expect["null_first"] else wrong_length), name
        if "overlap" in expect:
            bent, onto, message = expect["overlap"]

            def overlap(b):
                b.ptr[bent] = b.ptr[onto] + 16                 # keeps the alignment the device forms ask for

            assert case(overlap)[0] == (BAD_ARGUMENT, message), name
        if "exps" in expect:
            def two_n(b):
                b.keep["exps"][4:8] = np.frombuffer(np.uint32(2 * N).tobytes(), np.uint8)

            assert case(two_n)[0] == (BAD_ARGUMENT, expect["exps"]), name

            def two_n_and_short(b):                            # the exponents are looked at before the lengths
                two_n(b), short(b)

            assert case(two_n_and_short)[0] == (BAD_ARGUMENT, expect["exps"]), name
        if "zero" in expect:
            def empty(b):
                for buf in expect["zero"]:
                    b.len[buf] = 0

            (status, message), b = case(empty)
            torch.cuda.synchronize()
            assert (status, message) == (0, SENTINEL) and b.untouched(expect["out"]), name
        seen += 1
    assert seen == (32 if bits == 64 else 31)
