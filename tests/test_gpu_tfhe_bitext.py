"""GPU tests of bit extraction (include/pfhe.h, pfhe_bitext{,32}_*): the shifted key switch
alone against lwe_keyswitch_dev on the shifted input and against the model, at the shapes that reach every path of the
tile and on the digit rule's edge words; the handle word for word against its composition of public calls, with chunking,
the host form and an unchanged input; the exact regime against the integer model; what it means on noisy generated keys,
within the derived bound; the chain bit extraction -> circuit bootstrap -> look-up on fresh encryptions of integers; graph
capture, the call's refusals in their order, the lease and the stream order."""
import threading

import numpy as np
import pytest

import tfhe_bitext_model as bx
import tfhe_bootstrap_model as bs
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_lut_model as lm
from test_gpu_tfhe_cbs import device_randomness, signed
from test_gpu_tfhe_cbs_edges import one_stream_after_another
from test_gpu_tfhe_fft import TORCH_INT, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

BASES = {32: (7, 3), 64: (15, 2)}      # the rotation's (log B, ell) per width
KS_BASES = {32: (4, 6), 64: (8, 5)}    # the key switch's


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
    return torch.full((size,), -1, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")


def fourier_form(p, fft, torus):
    import torch
    out = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, out, fft)
    return out


def handle_run(p, ctx, lwe, bsk, ksk, delta, nbits, bits, stream=None):
    batch = lwe.numel() // (ctx.extracted_dimension() + 1)
    out = empty_words(batch * nbits * (ctx.lwe_dimension + 1), bits)              # uninitialised
    p.tfhe_extract_bits_dev(lwe, bsk, ksk, out, ctx, delta, nbits, stream)
    return out


def composition(p, fft, rot, lwe_in, bsk, ksk, bits, log_n, k, n, ks_basis, delta, nbits):
    """bit extraction as public calls on device tensors, per bit i with c_0 = lwe_in:
         c_i << (BITS - 1 - delta - i)                                (torch)
         lwe_keyswitch_dev                                            -> out[:, i]
         b += 2^(BITS-2)                                              (torch)
         lwe_modulus_switch_dev                                       -> exps, neg_b
         mul_monomial_each_to_dev on TV_i = (0, .., 0, -2^(delta+i-1)) -> ACC
         tfhe_blind_rotate_dev
         glwe_sample_extract_dev at index 0
         body += 2^(delta+i-1)                                        (torch)
         c_{i+1} = c_i - that                                         (torch)"""
    import torch
    big_n = 1 << log_n
    glwe, ext = (k + 1) * big_n, k * big_n + 1
    batch = lwe_in.numel() // ext
    run = lwe_in.clone()
    out = empty_words(batch * nbits * (n + 1), bits).view(batch, nbits, n + 1)
    for i in range(nbits):
        sigma = bits - 1 - delta - i
        shifted = torch.bitwise_left_shift(run, sigma).contiguous()
        switched = empty_words(batch * (n + 1), bits)
        p.lwe_keyswitch_dev(shifted, ksk, switched, ext - 1, n, ks_basis)
        out[:, i] = switched.view(batch, n + 1)
        if i + 1 == nbits:
            break
        switched.view(batch, n + 1)[:, n] += signed(1 << (bits - 2), bits)
        exps = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        neg_b = torch.empty(batch, dtype=torch.int32, device="cuda")
        p.lwe_modulus_switch_dev(switched, n, log_n, exps, neg_b)
        half = 1 << (delta + i - 1)
        tv = torch.zeros((batch, k + 1, big_n), dtype=lwe_in.dtype, device="cuda")
        tv[:, k, :] = signed(-half, bits)
        acc = empty_words(batch * glwe, bits)
        fft.mul_monomial_each_to_dev(tv.view(-1), neg_b, acc, polys_per_exp=k + 1)
        p.tfhe_blind_rotate_dev(acc, bsk, exps, rot)
        lwe_ext = empty_words(batch * ext, bits)
        p.glwe_sample_extract_dev(acc, lwe_ext, fft, k, 0)
        lwe_ext.view(batch, ext)[:, ext - 1] += signed(half, bits)
        run = run - lwe_ext
    return out.reshape(-1)


def random_case(p, rng, bits, log_n, k, n, batch, ks=None, lwe_words=None):
    """full-torus keys and random everything: (fft, basis, ks_basis, bsk, ksk, lwe)"""
    lb, ell = BASES[bits]
    ks = ks or KS_BASES[bits]
    fft = table(p, log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *ks)
    glwe, ext = (k + 1) << log_n, (k << log_n) + 1
    bsk = fourier_form(p, fft, dev_words(rand_words(rng, bits, n * (k + 1) * ell * glwe), bits))
    ksk = dev_words(rand_words(rng, bits, (ext - 1) * ks[1] * (n + 1)), bits)
    lwe = dev_words(rand_words(rng, bits, batch * ext) if lwe_words is None else lwe_words, bits)
    return fft, basis, ks_basis, bsk, ksk, lwe


# ---------------- the shifted key switch alone ----------------

# batch 1 / 31 / 33 (one row, a tile short of one row, a tile and one row), n + 1 = 127 / 128 / 129 (a column tile short of one,
# exactly one, one more), and (k, log N, ell_ks) whose k N ell_ks rows leave a remainder in the row loop: each value of each
# with each value of the others once (a Latin square)
KS_SHAPES = [(batch, n, shape) for a, batch in enumerate((1, 31, 33)) for b, n in enumerate((126, 127, 128))
             for c, shape in enumerate(((3, 1, 3), (1, 4, 5), (2, 5, 6))) if (a + b + c) % 3 == 0]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("batch,n,shape", KS_SHAPES, ids=lambda v: str(v))
def test_shifted_key_switch_equals_the_key_switch_of_the_shifted_input(p, bits, batch, n, shape):
    """bits = 1 is the shifted key switch and nothing else: word for word lwe_keyswitch_dev on the shifted input and the
    model, at delta = 1 (sigma = BITS - 2) and delta = BITS - 1 (sigma = 0).  The inputs are the edge words of the key
    switch's basis moved right by sigma under random high bits, so that the SHIFTED word is the edge word (its low sigma
    bits cleared) and the digit rule's carries are taken after the shift.  With bits = 2 the second output depends on every
    exponent the kernel wrote behind the first: it is compared with the composition."""
    import torch
    k, log_n, ks_ell = shape
    ks_lb = 4 if bits == 32 else 8
    rng = np.random.default_rng(bits + batch + n + ks_ell)
    ext = (k << log_n) + 1
    edges = ew.edge_words(bits, ks_lb, ks_ell).astype(np.uint64)
    fft, basis, ks_basis, bsk, ksk, _ = random_case(p, rng, bits, log_n, k, n, batch, (ks_lb, ks_ell))
    ks_model = m.ApproxSignedBasis(bits, ks_lb, ks_ell)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis)
    assert ctx.ksk_len() == ksk.numel() and ctx.bsk_len() == bsk.numel() and not ctx.in_use()
    rot = p.TfheBlindRotateContext(fft, basis, k)
    for delta in (1, bits - 1):
        sigma = bits - 1 - delta
        want_shifted = rng.choice(edges, batch * ext)
        high = rand_words(rng, bits, batch * ext).astype(np.uint64)
        words = (want_shifted >> np.uint64(sigma)) | ((high << np.uint64(bits - sigma)) & np.uint64(2 ** bits - 1) if sigma else 0)
        words = np.asarray(words, np.uint64).astype(m.UINT[bits])
        lwe = dev_words(words, bits)
        shifted = torch.bitwise_left_shift(lwe, sigma).contiguous()
        assert np.array_equal(host_words(shifted, bits), bx.shift_words(words, sigma, bits))
        want = empty_words(batch * (n + 1), bits)
        p.lwe_keyswitch_dev(shifted, ksk, want, ext - 1, n, ks_basis)
        got = handle_run(p, ctx, lwe, bsk, ksk, delta, 1, bits)
        assert torch.equal(got, want), delta
        model = bs.keyswitch(bx.shift_words(words, sigma, bits), host_words(ksk, bits), ext - 1, n, ks_model)
        assert np.array_equal(host_words(got, bits), model), delta
        assert np.array_equal(host_words(lwe, bits), words)                   # the input is read only
    for delta in (1, bits - 2):
        lwe = dev_words(rand_words(rng, bits, batch * ext), bits)
        want = composition(p, fft, rot, lwe, bsk, ksk, bits, log_n, k, n, ks_basis, delta, 2)
        assert torch.equal(handle_run(p, ctx, lwe, bsk, ksk, delta, 2, bits), want), delta


# ---------------- the handle against the composition of public calls ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k", [(6, 1), (9, 1), (4, 2)])
def test_handle_equals_the_composition_of_public_calls(p, bits, log_n, k):
    """full-torus random keys; k = 1 runs the rotation's whole-loop kernel, k = 2 its per-step path; bits 1, 2 and 5; batch 3
    under chunk 1, 2 and the default; the host form; the input unchanged; one input alone"""
    import torch
    n, batch = 5, 3
    rng = np.random.default_rng(bits + log_n + k)
    fft, basis, ks_basis, bsk, ksk, lwe = random_case(p, rng, bits, log_n, k, n, batch)
    before = lwe.clone()
    rot = p.TfheBlindRotateContext(fft, basis, k)
    one, two, wide = (p.TfheBitExtractContext(fft, basis, n, k, ks_basis, chunk=c) for c in (1, 2, 0))
    assert one.scratch_bytes() < two.scratch_bytes() < wide.scratch_bytes() and wide.scratch_bytes() > rot.scratch_bytes()
    ext = (k << log_n) + 1
    for nbits, delta in ((1, bits - 1), (2, 1), (5, bits - 5), (5, bits // 2)):
        want = composition(p, fft, rot, lwe, bsk, ksk, bits, log_n, k, n, ks_basis, delta, nbits)
        for ctx in (one, two, wide, two):
            assert torch.equal(handle_run(p, ctx, lwe, bsk, ksk, delta, nbits, bits), want), (nbits, delta)
        assert torch.equal(lwe, before)
        alone = handle_run(p, two, lwe[2 * ext:].clone(), bsk, ksk, delta, nbits, bits)
        assert torch.equal(alone, want[2 * nbits * (n + 1):])
    host_out = np.zeros(batch * 5 * (n + 1), m.UINT[bits])
    p.tfhe_extract_bits(host_words(lwe, bits), bsk.cpu().numpy(), host_words(ksk, bits), host_out, two, bits // 2, 5)
    assert np.array_equal(host_out, host_words(want, bits))
    assert not two.in_use()


# ---------------- the exact regime ----------------

# bits, log_n, k, lb, ell: key words |g| <= 2^10 and (k+1) ell N 2^(logB-1) 2^10 <= 2^40, as test_gpu_tfhe_bootstrap's
EXACT_CASES = [(32, 6, 1, 7, 3), (64, 6, 1, 15, 2), (32, 5, 2, 7, 3), (64, 5, 2, 15, 2), (32, 6, 1, 8, None)]


@pytest.mark.parametrize("bits,log_n,k,lb,ell", EXACT_CASES)
def test_exact_regime_equals_the_integer_model(p, bits, log_n, k, lb, ell):
    """every product of the rotation is the integer schoolbook, and every other stage is integer arithmetic anyway"""
    n, batch, big_n = 3, 2, 1 << log_n
    basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    L = basis.decompose_length()
    assert (k + 1) * L * big_n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    ks_basis, ks_mb = p.ApproxSignedBasis(bits, *KS_BASES[bits]), m.ApproxSignedBasis(bits, *KS_BASES[bits])
    rng = np.random.default_rng(log_n * 100 + lb + k + bits)
    fft = table(p, log_n)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis)
    keys = [rng.integers(-1024, 1025, (k + 1) * L * (k + 1) * big_n).astype(m.UINT[bits]) for _ in range(n)]
    bsk = fourier_form(p, fft, dev_words(np.concatenate(keys), bits))
    lwe = rand_words(rng, bits, batch * (k * big_n + 1))
    ksk = rand_words(rng, bits, ctx.ksk_len())
    for nbits, delta in ((3, bits - 3), (4, 2)):
        got = handle_run(p, ctx, dev_words(lwe, bits), bsk, dev_words(ksk, bits), delta, nbits, bits)
        want = bx.extract_bits(lwe, keys, ksk, mb, ks_mb, log_n, k, n, delta, nbits)
        assert np.array_equal(host_words(got, bits), want), (nbits, delta)


# ---------------- meaning on noisy keys, all on the device ----------------

def noisy_keys(p, bits, log_n, k, n, lb, ell, noise, gen, rng):
    """binary keys; bsk and ksk generated on the device from torus_uniform masks and torus_noise(bound=noise) bodies"""
    big_n = 1 << log_n
    fft = table(p, log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *kg.KS_BASIS)
    s = rng.integers(0, 2, n).astype(m.UINT[bits])
    z = rng.integers(0, 2, (k, big_n)).astype(m.UINT[bits])
    d_s, z_flat = dev_words(s, bits), dev_words(bs.flatten_key(z), bits)
    torus = device_randomness(p, bits, log_n, k, n * (k + 1) * ell, noise, gen)
    bsk = p.tfhe_generate_bsk_dev(p.TfheKeyShape(fft, basis, n, k), d_s, z_flat, torus)
    rows = k * big_n * kg.KS_BASIS[1]
    ksk = p.torus_uniform(rows * (n + 1), bits, generator=gen).view(rows, n + 1)
    ksk[:, n] = p.torus_noise(rows, bits, bound=noise, generator=gen)
    ksk = ksk.view(-1)
    p.tfhe_generate_ksk_dev(z_flat, d_s, ks_basis, ksk)
    return fft, basis, ks_basis, d_s, z_flat, bsk, ksk


def fresh_encryptions(p, values, z_flat, bits, noise, gen):
    """LWE ciphertexts of the torus words `values` under the flattened GLWE key: uniform masks, |e| <= noise"""
    dim = z_flat.numel()
    lwe = p.torus_uniform(len(values) * (dim + 1), bits, generator=gen).view(len(values), dim + 1)
    lwe[:, dim] = p.torus_noise(len(values), bits, bound=noise, generator=gen) + dev_words(np.asarray(values, m.UINT[bits]), bits)
    lwe = lwe.view(-1)
    p.lwe_encrypt_dev(lwe, z_flat)
    return lwe


@pytest.mark.parametrize("case", kg.NOISY_CASES[:3], ids=lambda c: "u%d-N%d-k%d-n%d" % (c[0], 1 << c[1], c[2], c[3]))
def test_every_bit_of_every_message_decodes_on_noisy_keys(p, case):
    """Binary keys, |e| <= E on every row of both generated keys and on the inputs.  Every message of 3 bits at delta =
    BITS - 3 and of 5 bits at delta = BITS - 6 (a bit above the message is left clear), twice; every bit decodes through
    lwe_phase_dev, and the largest distance of a phase from m_i 2^(BITS-1) is under tfhe_bitext_model.bit_bound for its i,
    which tests/test_tfhe_bitext_model.py holds under the margin.  Largest errors seen on the device are in DESIGN.md §24's
    table."""
    import torch
    bits, log_n, k, n, lb, ell, _g, _p, noise = case
    rng = np.random.default_rng(7000 + bits + log_n + k)
    gen = torch.Generator(device="cuda").manual_seed(7100 + bits + log_n + k)
    fft, basis, ks_basis, d_s, z_flat, bsk, ksk = noisy_keys(p, bits, log_n, k, n, lb, ell, noise, gen, rng)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis)
    for nbits, below in bx.MEANING_BITS:
        delta = bits - below
        assert bx.all_bits_fit(bits, log_n, k, n, lb, ell, *kg.KS_BASIS, noise, noise, delta, nbits)
        msgs = list(range(1 << nbits)) * 2
        lwe = fresh_encryptions(p, [(v << delta) % (1 << bits) for v in msgs], z_flat, bits, noise, gen)
        out = handle_run(p, ctx, lwe, bsk, ksk, delta, nbits, bits)
        p.lwe_phase_dev(out, d_s)
        phases = host_words(out, bits).reshape(len(msgs), nbits, n + 1)[:, :, n]
        want = np.array([[(v >> i) & 1 for i in range(nbits)] for v in msgs], np.uint64)
        err = m.centred_error(phases.reshape(-1), (want.reshape(-1) << np.uint64(bits - 1)).astype(m.UINT[bits]), bits)
        err = np.asarray(err, np.float64).reshape(len(msgs), nbits).max(axis=0)
        bounds = [bx.bit_bound(bits, log_n, k, n, lb, ell, *kg.KS_BASIS, noise, noise, delta, i) for i in range(nbits)]
        print("bits %d log_n %d k %d n %d: %d bits at delta %d: worst err 2^%.2f (bit %d) bound there 2^%.2f margin 2^%d"
              % (bits, log_n, k, n, nbits, delta, np.log2(max(err.max(), 1)), int(err.argmax()),
                 np.log2(bounds[int(err.argmax())]), bits - 2))
        assert bx.decode_bits(phases.reshape(-1), bits) == [int(b) for b in want.reshape(-1)]
        for i in range(nbits):
            assert err[i] <= bounds[i], (i, err[i], bounds[i])


# ---------------- the chain: a table on an encrypted integer ----------------

@pytest.mark.parametrize("idx", range(len(lm.NOISY_LUTS)), ids=lambda i: "u%d-N%d-k%d-n%d" % (
    lm.NOISY_LUTS[i][0][0], 1 << lm.NOISY_LUTS[i][0][1], lm.NOISY_LUTS[i][0][2], lm.NOISY_LUTS[i][0][3]))
def test_table_on_an_encrypted_integer_without_a_padding_bit(p, idx):
    """tfhe_lut_on_integer_dev on fresh encryptions (|e| <= E) of every p-bit message at delta = BITS - p, no padding bit:
    bit extraction, circuit bootstrap, look-up with extract = 1 over a shared tfhe_lut_table of random 1-bit entries under one
    padding bit, all keys generated on the device with |e| <= E on every row; every message decodes to its entry.  A shape
    listed in tfhe_bitext_model.CHAIN_NOISE runs at the noise given there, because its own does not fit bit_bound."""
    import torch
    case, t, r = lm.NOISY_LUTS[idx]
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, pbits = case
    noise = bx.CHAIN_NOISE.get(idx, noise)
    big_n, pb = 1 << log_n, t + r
    assert pb == (3 if bits == 32 else 5) and pbits == 1
    assert bx.all_bits_fit(bits, log_n, k, n, lb, ell, *kg.KS_BASIS, noise, noise, bits - pb, pb)
    rng = np.random.default_rng(8000 + bits + log_n + k)
    gen = torch.Generator(device="cuda").manual_seed(8100 + bits + log_n + k)
    fft, basis, ks_basis, d_s, z_flat, bsk, ksk = noisy_keys(p, bits, log_n, k, n, lb, ell, noise, gen, rng)
    cbs_basis, pfks_basis = p.ApproxSignedBasis(bits, cb_lb, cb_ell), p.ApproxSignedBasis(bits, pf_lb, pf_ell)
    pfksk = device_randomness(p, bits, log_n, k, (k + 1) * (k * big_n + 1) * pf_ell, noise, gen)
    p.tfhe_generate_pfksk_dev(z_flat, z_flat, fft, pfks_basis, pfksk, k)
    bitext = p.TfheBitExtractContext(fft, basis, n, k, ks_basis)
    cbs = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    lut = p.TfheLutContext(fft, cbs_basis, k, t, r)
    msgs = list(range(1 << pb))
    delta = bits - pb
    lwe = fresh_encryptions(p, [(v << delta) % (1 << bits) for v in msgs], z_flat, bits, noise, gen)
    data = rng.integers(0, 1 << pbits, (1, 1 << pb))
    values = (data.astype(np.uint64) << np.uint64(bits - pbits - 1)).astype(m.UINT[bits])
    tbl = p.tfhe_lut_table(dev_words(values, bits), log_n, k, t, r)
    out = empty_words(len(msgs) * (k * big_n + 1), bits)
    p.tfhe_lut_on_integer_dev(lwe, bsk, ksk, pfksk, tbl.view(-1), out, bitext, cbs, lut, delta)
    p.lwe_phase_dev(out, z_flat)
    phases = host_words(out, bits).reshape(len(msgs), k * big_n + 1)[:, k * big_n]
    assert bs.decode(phases, pbits, bits) == [int(data[0, v]) for v in msgs]
    # the output is an input of the next such call: k N + 1 words under the extracted key
    assert out.numel() == len(msgs) * (bitext.extracted_dimension() + 1)


# ---------------- graph capture ----------------

def test_graph_capture_replays_the_eager_call(p):
    """a linear capture on one stream, replayed twice on fresh inputs"""
    import torch
    bits, log_n, k, n, batch, delta, nbits = 32, 6, 1, 3, 3, 20, 3
    rng = np.random.default_rng(32)
    fft, basis, ks_basis, bsk, ksk, fresh = random_case(p, rng, bits, log_n, k, n, batch)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis, chunk=2)            # two chunks in the graph
    eager = handle_run(p, ctx, fresh, bsk, ksk, delta, nbits, bits)
    torch.cuda.synchronize()
    lwe, out = fresh.clone(), torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.tfhe_extract_bits_dev(lwe, bsk, ksk, out, ctx, delta, nbits)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        lwe.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------- errors and the lease ----------------

def test_call_refusals_arrive_in_their_order(p):
    """delta_log and bits before anything else of the call; the host form's null pointers before the lengths; the lengths;
    the empty batch; the device form's null pointers, alignment and overlap"""
    import ctypes as C
    import torch
    bits, log_n, k, n = 32, 5, 1, 4
    fft = table(p, log_n)
    basis, ks_basis = p.ApproxSignedBasis(32, 7, 3), p.ApproxSignedBasis(32, 4, 6)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis)
    ext, row = 33, n + 1
    assert ctx.ksk_len() == 32 * 6 * row and ctx.bsk_len() == n * 2 * 3 * 64
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")
    f = lambda size: torch.zeros(size, dtype=torch.complex128, device="cuda")
    lwe, bsk, ksk = z(3 * ext), f(ctx.bsk_len()), z(ctx.ksk_len())
    p.tfhe_extract_bits_dev(lwe, bsk, ksk, z(3 * 2 * row), ctx, 5, 2)              # the lengths that fit
    p.tfhe_extract_bits_dev(lwe, bsk, ksk, z(3 * row), ctx, 31, 1)                 # delta + bits = BITS
    p.tfhe_extract_bits_dev(z(0), bsk, ksk, z(0), ctx, 5, 2)                       # an empty batch is a no-op
    for delta, nbits in ((0, 2), (5, 0), (31, 2), (33, 1), (1, 32), (2 ** 32 - 1, 2)):
        with pytest.raises(p.PfheError) as e:                                      # whatever the lengths are
            p.tfhe_extract_bits_dev(lwe[:-1], bsk[:-1], ksk[:-1], z(5), ctx, delta, nbits)
        assert e.value.kind == "BadArgument" and "delta_log" in str(e.value), (delta, nbits)
    for args in ((lwe[:-1], bsk, ksk, z(3 * 2 * row)),                             # not a whole number of ciphertexts
                 (lwe, bsk, ksk, z(3 * 2 * row - 1)), (lwe, bsk, ksk, z(3 * row)), (lwe, bsk, ksk, z(2 * 2 * row)),
                 (lwe, bsk[:-1], ksk, z(3 * 2 * row)), (lwe, f((n - 1) * 2 * 3 * 64), ksk, z(3 * 2 * row)),
                 (lwe, bsk, ksk[:-1], z(3 * 2 * row)), (lwe, bsk, z(32 * 5 * row), z(3 * 2 * row))):
        with pytest.raises(p.PfheError) as e:
            p.tfhe_extract_bits_dev(*args, ctx, 5, 2)
        assert e.value.kind == "BadLength" and "bits_out" in str(e.value)
    lib = p.lib()
    dev, host = lib.pfhe_bitext32_extract_bits_dev, lib.pfhe_bitext32_extract_bits
    ptr = lambda t: C.c_void_p(t.data_ptr())
    dbl = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))
    out = z(3 * 2 * row)
    BAD_LENGTH, BAD_ARGUMENT = 32, 33
    # the host form refuses a null pointer before the lengths, the device form after them (and after the empty batch)
    arr = np.zeros(3 * ext, np.uint32)
    assert host(ctx._h, None, arr.size - 1, None, 0, None, 0, 5, 2, None, 7) == BAD_ARGUMENT
    assert dev(ctx._h, None, lwe.numel() - 1, dbl(bsk), bsk.numel(), ptr(ksk), ksk.numel(), 5, 2, ptr(out), out.numel(),
               None) == BAD_LENGTH
    assert dev(ctx._h, None, 0, None, bsk.numel(), None, ksk.numel(), 5, 2, None, 0, None) == 0
    for hole in range(4):
        a = [ptr(lwe), dbl(bsk), ptr(ksk), ptr(out)]
        a[hole] = None
        assert dev(ctx._h, a[0], lwe.numel(), a[1], bsk.numel(), a[2], ksk.numel(), 5, 2, a[3], out.numel(), None) == BAD_ARGUMENT
    odd = z(3 * 2 * row + 1)[1:]                                                   # four bytes off: before the overlap
    assert dev(ctx._h, ptr(lwe), lwe.numel(), dbl(bsk), bsk.numel(), ptr(ksk), ksk.numel(), 5, 2, ptr(odd), odd.numel(),
               None) == BAD_ARGUMENT
    assert "16-byte aligned" in lib.pfhe_last_error().decode()
    both = z(3 * ext + 3 * 2 * row + 64)
    with pytest.raises(p.PfheError) as e:                                          # the output inside the input
        p.tfhe_extract_bits_dev(both[:3 * ext], bsk, ksk, both[32:32 + 3 * 2 * row], ctx, 5, 2)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    big = z(ctx.ksk_len() + 64)
    with pytest.raises(p.PfheError) as e:                                          # the output inside the key-switch key
        p.tfhe_extract_bits_dev(lwe, bsk, big[:ctx.ksk_len()], big[64:64 + 3 * 2 * row], ctx, 5, 2)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    with pytest.raises(TypeError):                                                 # words of another width
        p.tfhe_extract_bits_dev(lwe.long(), bsk, ksk, out, ctx, 5, 2)
    with pytest.raises(ValueError):
        p.TfheBitExtractContext(fft, basis, n, k)
    with pytest.raises(p.PfheError) as e:
        p.TfheBitExtractContext(fft, basis, 0, k, ks_basis)
    assert e.value.kind == "BadArgument" and "lwe_dimension" in str(e.value)
    assert not ctx.in_use()
    torch.cuda.synchronize()


def test_second_thread_gets_busy(p):
    """Two threads call the host form of one handle over and over until one of them has been refused: a call that arrives
    while the other thread is inside gets Busy, and a call that arrives in between runs (neither is a failure, so the test
    waits for no timing).  Every refusal seen is Busy, and the handle still gives the right words afterwards."""
    bits, log_n, k, n, batch, delta, nbits = 32, 8, 1, 16, 8, 20, 3
    rng = np.random.default_rng(35)
    fft, basis, ks_basis, bsk, ksk, lwe = random_case(p, rng, bits, log_n, k, n, batch)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis)
    want = host_words(handle_run(p, ctx, lwe, bsk, ksk, delta, nbits, bits), bits)
    h_lwe, h_bsk, h_ksk = host_words(lwe, bits), bsk.cpu().numpy(), host_words(ksk, bits)
    outs = [np.zeros(want.size, np.uint32) for _ in range(2)]
    refused, done = [], threading.Event()

    def caller(out):
        for _ in range(200):
            if done.is_set():
                return
            try:
                p.tfhe_extract_bits(h_lwe, h_bsk, h_ksk, out, ctx, delta, nbits)
            except p.PfheError as e:
                refused.append(e.kind)
                done.set()

    th = threading.Thread(target=caller, args=(outs[1],))
    th.start()
    caller(outs[0])
    done.set()
    th.join()
    assert refused and set(refused) == {"Busy"}, refused
    assert not ctx.in_use()
    p.tfhe_extract_bits(h_lwe, h_bsk, h_ksk, outs[0], ctx, delta, nbits)
    assert np.array_equal(outs[0], want)


def test_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p):
    """The accumulators, the exponents, neg_b and the running ciphertexts are shared by all calls of the handle, and so is the
    rotation it owns.  u32, N = 2^8, k = 1, full-torus keys, 256 steps and two bits, so that a chunk's rotation outlasts the
    queueing of the next call."""
    bits, log_n, k, n, delta, nbits = 32, 8, 1, 256, 12, 2
    rng = np.random.default_rng(9650)
    fft = p.FullComplex64FftTable(log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, 7, 3), p.ApproxSignedBasis(bits, 4, 3)
    make = lambda: p.TfheBitExtractContext(fft, basis, n, k, ks_basis, chunk=2)
    shape = make()
    bsk = fourier_form(p, fft, dev_words(rand_words(rng, bits, shape.bsk_len()), bits))
    ksk = dev_words(rand_words(rng, bits, shape.ksk_len()), bits)

    def inputs(batch):
        lwe = dev_words(rand_words(rng, bits, batch * (shape.extracted_dimension() + 1)), bits)
        return (lambda ctx, out, stream: p.tfhe_extract_bits_dev(lwe, bsk, ksk, out, ctx, delta, nbits, stream)), \
            batch * nbits * (n + 1)

    one_stream_after_another(make, inputs(24), inputs(3), n + 1, bits)
