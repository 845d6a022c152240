"""GPU tests of the GLWE automorphism with its key switch, the trace, their keys and the LWE embedding (include/pfhe.h,
pfhe_tfhe{,32}_glwe_trace_*, _glwe_automorphism*, _gksk_generate_dev, _lwe_embed*): rule 1 word for word against the
composition of public calls (a torch gather for sigma_t, the public product on the zero-padded key, a subtraction) on
full-torus keys, at the shapes where the fused kernel's slot loop and the general form take their paths; rule 2 against its
m calls of rule 1, with chunking, repeat calls, out == inp, the host form and graph replay; bit for bit against the integer
schoolbook where the product is exact, the inputs walking the digit rule's edge words; the keys and the embedding against
the integer model; what embed + trace means on noisy keys, all on the device; errors and the lease."""
import threading

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_trace_model as tm
from test_gpu_tfhe_fft import TORCH_INT, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu


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


def fourier_keys(p, fft, torus):
    import torch
    out = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, out, fft)
    return out


def sigma_dev(x, t, n):
    """the exact permutation sigma_t of every polynomial of N words, as a torch gather"""
    import torch
    u = (torch.arange(n, device="cuda") * pow(t, -1, 2 * n)) % (2 * n)
    g = x.view(-1, n)[:, u % n]
    return torch.where(u < n, g, -g).reshape(-1)


def composition(p, plan, inp, key, t):
    """rule 1 as public calls: sigma_t, the product against the key padded with ell zero body rows, the subtraction"""
    import torch
    k, n = plan.glwe_dimension, plan.fft.poly_length()
    s = sigma_dev(inp, t, n)
    padded = torch.cat([key, torch.zeros(plan.key_len() - key.numel(), dtype=key.dtype, device="cuda")])
    prod = torch.empty_like(s)
    p.tfhe_external_product_to_dev(s, padded, prod, plan)
    body = torch.zeros_like(s).view(-1, k + 1, n)
    body[:, k] = s.view(-1, k + 1, n)[:, k]
    return body.view(-1) - prod


def auto_run(p, ctx, inp, key, t, bits):
    out = empty_words(inp.numel(), bits)
    p.glwe_automorphism_dev(inp, key, out, t, ctx)
    return out


def trace_run(p, ctx, inp, keys, steps, bits, stream=None):
    out = empty_words(inp.numel(), bits)
    p.glwe_trace_dev(inp, keys, out, ctx, steps, stream)
    return out


def trace_by_rule_1(p, ctx, inp, keys, steps, bits):
    acc = inp
    for s, t in enumerate(ctx.trace_exponents(steps)):
        acc = acc + auto_run(p, ctx, acc, keys[s * ctx.key_len():(s + 1) * ctx.key_len()], t, bits)
    return acc


# ---------------- rule 1 against the composition of public calls ----------------

# bits, log_n, k, log_basis, ell (None: the full length, drop_bits 0)
RULE1_CASES = [
    (32, 1, 1, 8, None),       # fused: one slot, 255 idle threads, the only t besides 1 is 3; drop_bits 0
    (64, 2, 1, 15, 2),         # fused: two coefficients per half
    (64, 9, 1, 15, 2),         # fused: exactly one slot per thread
    (32, 10, 1, 7, 3),         # fused: two slots
    (64, 11, 1, 15, 2),        # fused: four slots
    (64, 10, 1, 20, 1),        # ell = 1
    (32, 11, 1, 16, None),     # four slots at u32, drop_bits 0
    (32, 5, 2, 7, 3),          # general
    (64, 5, 2, 20, 1),         # general, ell = 1
    (64, 3, 3, 16, None),      # general, drop_bits 0
    (64, 12, 1, 15, 2),        # general: k = 1 above the fused N
    (32, 12, 1, 10, 1),        # general, ell = 1
]


@pytest.mark.parametrize("bits,log_n,k,lb,ell", RULE1_CASES, ids=lambda v: str(v))
def test_automorphism_equals_the_composition_of_public_calls(p, bits, log_n, k, lb, ell):
    """three ciphertexts at t = 1, 3, N + 1 and 2N - 1, on a default handle (one launch) and on one of chunk 1; the host
    form; one ciphertext alone"""
    import torch
    count, n = 3, 1 << log_n
    rng = np.random.default_rng(bits + 10 * log_n + k)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    plan = p.TfheFftContext(fft, basis, k)
    wide, narrow = p.TfheGlweTraceContext(fft, basis, k), p.TfheGlweTraceContext(fft, basis, k, chunk=1)
    glwe = plan.glwe_len()
    assert wide.glwe_len() == glwe and wide.key_len() * (k + 1) == plan.key_len() * k and not wide.in_use()
    inp = dev_words(rand_words(rng, bits, count * glwe), bits)
    key = fourier_keys(p, fft, dev_words(rand_words(rng, bits, wide.key_len()), bits))
    for t in sorted({1, 3, n + 1, 2 * n - 1}):
        want = composition(p, plan, inp, key, t)
        for ctx in (wide, narrow):
            assert torch.equal(auto_run(p, ctx, inp, key, t, bits), want), (t, ctx is wide)
    t = 2 * n - 1
    want = host_words(composition(p, plan, inp, key, t), bits)
    host = np.zeros(count * glwe, m.UINT[bits])
    p.glwe_automorphism(host_words(inp, bits), key.cpu().numpy(), host, t, wide)
    assert np.array_equal(host, want)
    one = auto_run(p, narrow, inp[glwe:2 * glwe].clone(), key, t, bits)
    assert np.array_equal(host_words(one, bits), want[glwe:2 * glwe])
    ks = empty_words(count * glwe, bits)
    p.glwe_keyswitch_dev(inp, key, ks, wide)                               # the wrapper with t = 1
    assert torch.equal(ks, composition(p, plan, inp, key, 1))
    fused = k == 1 and log_n <= 11
    assert (wide.scratch_bytes() == 0) == fused


# ---------------- rule 2 against its calls of rule 1 ----------------

@pytest.mark.parametrize("bits,log_n,k", [(32, 6, 1), (64, 9, 1), (32, 11, 1), (64, 4, 2), (32, 12, 1)])
def test_trace_equals_its_calls_of_rule_1(p, bits, log_n, k):
    """m = 1, a partial m and log N; chunk 1 and a chunk below the batch; a repeat call; out == inp; the host form"""
    import torch
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    batch = 3
    rng = np.random.default_rng(bits + log_n + k)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    big, one, two = (p.TfheGlweTraceContext(fft, basis, k, chunk=c) for c in (0, 1, 2))
    glwe, key_len = big.glwe_len(), big.key_len()
    inp = dev_words(rand_words(rng, bits, batch * glwe), bits)
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, log_n * key_len), bits))
    assert big.trace_exponents()[0] == (1 << log_n) + 1 and big.trace_exponents()[-1] == 3
    for steps in (1, log_n // 2 + 1, log_n):
        ks = keys[:steps * key_len]
        want = trace_by_rule_1(p, big, inp, ks, steps, bits)
        for ctx in (big, one, two):
            assert torch.equal(trace_run(p, ctx, inp, ks, steps, bits), want), steps
        assert torch.equal(trace_run(p, two, inp, ks, steps, bits), want)                 # a repeat call
        for ctx in (big, two):
            same = inp.clone()
            p.glwe_trace_dev(same, ks, same, ctx, steps)                                  # out is inp
            assert torch.equal(same, want), steps
    full = trace_run(p, big, inp, keys, None, bits)                                       # steps defaults to log N
    assert torch.equal(full, trace_by_rule_1(p, big, inp, keys, log_n, bits))
    host = np.zeros(batch * glwe, m.UINT[bits])
    p.glwe_trace(host_words(inp, bits), keys.cpu().numpy(), host, two)
    assert np.array_equal(host, host_words(full, bits))


def test_graph_capture_replays_the_eager_call(p):
    """a linear capture on one stream, two chunks and all steps in the graph, replayed twice on fresh inputs"""
    import torch
    bits, log_n, k, batch = 32, 8, 1, 3
    rng = np.random.default_rng(77)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, 7, 3)
    ctx = p.TfheGlweTraceContext(fft, basis, k, chunk=2)
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, log_n * ctx.key_len()), bits))
    fresh = dev_words(rand_words(rng, bits, batch * ctx.glwe_len()), bits)
    eager = trace_run(p, ctx, fresh, keys, None, bits)
    torch.cuda.synchronize()
    inp, out = fresh.clone(), torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.glwe_trace_dev(inp, keys, out, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        inp.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------- the exact regime against the integer schoolbook ----------------

@pytest.mark.parametrize("bits,log_n,lb,ell", [(32, 4, 7, 3), (64, 4, 15, 2), (32, 9, 7, 3), (64, 9, 15, 2), (32, 4, 8, None)])
def test_exact_regime_equals_the_integer_schoolbook(p, bits, log_n, lb, ell):
    """key words |g| <= 2^10 and k ell N 2^(logB-1) 2^10 <= 2^40: the f64 product is the integer one.  The inputs are the
    digit rule's edge words, which sigma_t only permutes and negates; rule 1 at t = N + 1 and 3, and a trace of two steps"""
    k, n = 1, 1 << log_n
    mb = m.ApproxSignedBasis(bits, lb, ell)
    assert (k + 1) * mb.decompose_length * n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    rng = np.random.default_rng(bits + log_n + lb)
    glwe = (k + 1) * n
    edges = ew.edge_words(bits, lb, ell)
    count = max(2, -(-edges.size // glwe))                          # every edge word is somewhere in the inputs
    inp = rng.permutation(np.resize(edges, max(edges.size, count * glwe)))[:count * glwe].astype(m.UINT[bits])
    keys = rng.integers(-1024, 1025, 2 * tm.key_len(mb, log_n, k)).astype(np.int64).view(np.uint64).astype(m.UINT[bits])
    fft = table(p, log_n)
    ctx = p.TfheGlweTraceContext(fft, p.ApproxSignedBasis(bits, lb, ell), k)
    fkeys = fourier_keys(p, fft, dev_words(keys, bits))
    product = tm.exact_product(mb, log_n, k)
    for t in (n + 1, 3):
        got = auto_run(p, ctx, dev_words(inp, bits), fkeys[:ctx.key_len()], t, bits)
        assert np.array_equal(host_words(got, bits), tm.automorphism(inp, keys[:ctx.key_len()], t, product, mb, log_n, k)), t
    got = trace_run(p, ctx, dev_words(inp, bits), fkeys, 2, bits)
    assert np.array_equal(host_words(got, bits), tm.trace(inp, keys, 2, product, mb, log_n, k))


# ---------------- rules 3 and 4 against the integer model ----------------

@pytest.mark.parametrize("bits,log_n,k,lb,ell", [(32, 4, 1, 4, 8), (64, 5, 2, 8, 5), (64, 9, 1, 15, 2), (32, 1, 1, 8, None)])
def test_generated_keys_equal_the_model(p, bits, log_n, k, lb, ell):
    import torch
    n = 1 << log_n
    rng = np.random.default_rng(bits + log_n + k)
    fft, basis, mb = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    ctx = p.TfheGlweTraceContext(fft, basis, k)
    z_in, z_out = rand_words(rng, bits, k * n), rand_words(rng, bits, k * n)
    for exps in ([1], ctx.trace_exponents(), sorted({2 * n - 1, 3})):
        rows = len(exps) * k * mb.decompose_length
        rand = kg.glwe_randomness(rng, bits, log_n, k, rows, 5)
        torus = dev_words(rand, bits)
        out = p.tfhe_generate_gksk_dev(dev_words(z_in, bits), dev_words(z_out, bits), fft, basis, torus, exps, k)
        assert out.numel() == len(exps) * ctx.key_len() == torus.numel()
        assert np.array_equal(host_words(torus, bits), tm.gksk(rand, z_in.reshape(k, n), z_out.reshape(k, n), exps, mb, log_n, k))
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(fourier_keys(p, fft, torus)))   # bit for bit


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k", [(1, 1), (5, 1), (9, 1), (4, 3)])
def test_embedding_equals_the_model_and_extracts_back(p, bits, log_n, k):
    import torch
    n, batch = 1 << log_n, 5
    rng = np.random.default_rng(bits + log_n + k)
    fft = table(p, log_n)
    lwe = rand_words(rng, bits, batch * (k * n + 1))
    glwe = empty_words(batch * (k + 1) * n, bits)
    p.lwe_embed_glwe_dev(dev_words(lwe, bits), glwe, fft, k)
    assert np.array_equal(host_words(glwe, bits), tm.embed(lwe, bits, log_n, k))
    back = empty_words(lwe.size, bits)
    p.glwe_sample_extract_dev(glwe, back, fft, k, 0)
    assert np.array_equal(host_words(back, bits), lwe)
    host = np.zeros(batch * (k + 1) * n, m.UINT[bits])
    p.lwe_embed_glwe(lwe, host, fft, k)
    assert np.array_equal(host, host_words(glwe, bits))


# ---------------- meaning on noisy keys, all on the device ----------------

def device_randomness(p, bits, log_n, k, rows, noise, gen):
    """`rows` GLWE rows drawn on the device: torus_uniform masks, torus_noise(bound=noise) bodies"""
    n = 1 << log_n
    rand = p.torus_uniform(rows * (k + 1) * n, bits, generator=gen).view(rows, k + 1, n)
    rand[:, k] = p.torus_noise(rows * n, bits, bound=noise, generator=gen).view(rows, n)
    return rand.view(-1)


@pytest.mark.parametrize("shape", tm.NOISY_SHAPES, ids=lambda c: "u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]))
def test_embed_and_trace_convert_an_lwe_on_noisy_keys(p, shape):
    """Binary keys, torus_noise(bound=E) on every key row and on the inputs.  (i) LWE ciphertexts of a bit at Delta_in =
    2^(BITS-2) / N under the extracted key, embedded, traced in full, read with glwe_phase_dev: coefficient 0 within
    tm.trace_bound of N Delta_in m, every other coefficient within it of 0.  (ii) a partial trace of m steps on GLWE
    ciphertexts whose bits sit at the multiples of 2^m (Delta_in = 2^(BITS-2) / 2^m) and whose other coefficients hold
    full-range words: 2^(BITS-2) bit at the multiples, 0 elsewhere, within tm.trace_bound(m).  Largest errors seen on
    the device are in DESIGN.md section 21's table."""
    import torch
    bits, log_n, k, lb, ell, noise = shape
    n, batch = 1 << log_n, 8
    gen = torch.Generator(device="cuda").manual_seed(4000 + bits + log_n + k)
    rng = np.random.default_rng(bits + log_n + k)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    ctx = p.TfheGlweTraceContext(fft, basis, k)
    dt = getattr(torch, TORCH_INT[bits])
    z = torch.randint(0, 2, (k * n,), generator=gen, device="cuda").to(dt)
    exps = ctx.trace_exponents()
    rand = device_randomness(p, bits, log_n, k, len(exps) * k * ell, noise, gen)
    keys = p.tfhe_generate_gksk_dev(z, z, fft, basis, rand, exps, k)
    bound = tm.trace_bound(log_n, noise, *shape)
    assert bound < 2.0 ** (bits - 3)
    # (i)
    msgs = torch.tensor([i & 1 for i in range(batch)], device="cuda").to(dt)
    lwe = p.torus_uniform(batch * (k * n + 1), bits, generator=gen).view(batch, k * n + 1)
    lwe[:, k * n] = p.torus_noise(batch, bits, bound=noise, generator=gen) + msgs * (1 << (bits - 2 - log_n))
    lwe = lwe.view(-1)
    p.lwe_encrypt_dev(lwe, z)
    glwe = empty_words(batch * ctx.glwe_len(), bits)
    p.lwe_embed_glwe_dev(lwe, glwe, fft, k)
    p.glwe_trace_dev(glwe, keys, glwe, ctx)
    p.glwe_phase_dev(glwe, z, fft, k)
    ph = host_words(glwe, bits).reshape(batch, k + 1, n)[:, k]
    want = np.zeros((batch, n), m.UINT[bits])
    want[:, 0] = (np.arange(batch) & 1).astype(np.uint64) << np.uint64(bits - 2)
    err = float(m.centred_error(ph, want, bits).max())
    # (ii)
    steps = max(1, log_n // 2)
    stride = 1 << steps
    part = tm.trace_bound(steps, noise, *shape)
    data = rng.integers(0, 2, (batch, n // stride))
    body = rand_words(rng, bits, batch * n).reshape(batch, n)
    body[:, ::stride] = (data.astype(np.uint64) << np.uint64(bits - 2 - steps)).astype(m.UINT[bits])
    ct = p.torus_uniform(batch * ctx.glwe_len(), bits, generator=gen).view(batch, k + 1, n)
    ct[:, k] = p.torus_noise(batch * n, bits, bound=noise, generator=gen).view(batch, n) + dev_words(body.reshape(-1), bits).view(batch, n)
    ct = ct.view(-1)
    p.glwe_encrypt_dev(ct, z, fft, k)
    out = trace_run(p, ctx, ct, keys[:steps * ctx.key_len()], steps, bits)
    p.glwe_phase_dev(out, z, fft, k)
    ph2 = host_words(out, bits).reshape(batch, k + 1, n)[:, k]
    want2 = np.zeros((batch, n), m.UINT[bits])
    want2[:, ::stride] = (data.astype(np.uint64) << np.uint64(bits - 2)).astype(m.UINT[bits])
    err2 = float(m.centred_error(ph2, want2, bits).max())
    print("bits %d log_n %d k %d: full trace err 2^%.1f bound 2^%.1f; %d steps err 2^%.1f bound 2^%.1f; Delta_out/2 2^%d"
          % (bits, log_n, k, np.log2(max(err, 1)), np.log2(bound), steps, np.log2(max(err2, 1)), np.log2(part), bits - 3))
    assert err <= bound, (err, bound)
    assert err2 <= part, (err2, part)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    bits, log_n, k = 32, 5, 1
    fft, basis = table(p, log_n), p.ApproxSignedBasis(32, 7, 3)
    ctx = p.TfheGlweTraceContext(fft, basis, k)
    glwe, key_len = ctx.glwe_len(), ctx.key_len()
    assert glwe == 64 and key_len == 3 * 64 and not ctx.in_use()
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")
    f = lambda size: torch.zeros(size, dtype=torch.complex128, device="cuda")
    inp, out, keys = z(4 * glwe), z(4 * glwe), f(log_n * key_len)
    p.glwe_automorphism_dev(inp, keys[:key_len], out, 3, ctx)                # the lengths that fit
    p.glwe_trace_dev(inp, keys, out, ctx)
    p.glwe_trace_dev(inp, keys[:2 * key_len], out, ctx, 2)
    p.glwe_trace_dev(z(0), keys, z(0), ctx)                                  # an empty batch is a no-op
    for args in ((inp[:-1], keys[:key_len], out[:-1]), (inp, keys[:key_len], out[:3 * glwe]), (inp, keys[:key_len - 1], out),
                 (inp, keys[:2 * key_len], out)):
        with pytest.raises(p.PfheError) as e:
            p.glwe_automorphism_dev(*args[:2], args[2], 3, ctx)
        assert e.value.kind == "BadLength", e.value
    for args, steps in (((inp, keys[:-1], out), None), ((inp, keys[:2 * key_len], out), 3),      # keys shorter than m keys
                        ((inp, keys, out), 4), ((inp[:-1], keys, out[:-1]), None), ((inp, keys, out[:glwe]), None)):
        with pytest.raises(p.PfheError) as e:
            p.glwe_trace_dev(*args, ctx, steps)
        assert e.value.kind == "BadLength", (steps, e.value)
    for steps in (0, log_n + 1):
        with pytest.raises(p.PfheError) as e:
            p.glwe_trace_dev(inp, keys, out, ctx, steps)
        assert e.value.kind == "BadArgument" and "steps" in str(e.value)
    for t in (0, 2, 64, 65, 2 ** 31):                                        # even, or outside 1..2N-1
        with pytest.raises(p.PfheError) as e:
            p.glwe_automorphism_dev(inp, keys[:key_len], out, t, ctx)
        assert e.value.kind == "BadArgument" and "odd" in str(e.value), t
    with pytest.raises(TypeError):                                           # words of another width
        p.glwe_automorphism_dev(inp.long(), keys[:key_len], out, 3, ctx)
    both = z(5 * glwe)
    for a, b in ((both[:4 * glwe], both[glwe:]), (inp, inp)):                # rule 1 is a gather: no overlap at all
        with pytest.raises(p.PfheError) as e:
            p.glwe_automorphism_dev(a, keys[:key_len], b, 3, ctx)
        assert e.value.kind == "BadArgument" and "gather" in str(e.value)
    with pytest.raises(p.PfheError) as e:                                    # the trace: exactly inp, or disjoint
        p.glwe_trace_dev(both[:4 * glwe], keys, both[glwe:], ctx)
    assert e.value.kind == "BadArgument" and "exactly in" in str(e.value)
    ptr = lambda t, off=0: (t.data_ptr() + off, t.numel() - (1 if off else 0), "32")
    for args in (((0, inp.numel(), "32"), keys[:key_len], out), (inp, (0, key_len), out), (inp, keys[:key_len], (0, out.numel(), "32"))):
        with pytest.raises(p.PfheError) as e:                                # null pointers, after the lengths
            p.glwe_automorphism_dev(*args, 3, ctx)
        assert e.value.kind == "BadArgument"
    odd_in, odd_out = z(4 * glwe + 1), z(4 * glwe + 1)
    for args in ((ptr(odd_in, 4), keys[:key_len], out), (inp, keys[:key_len], ptr(odd_out, 4))):
        with pytest.raises(p.PfheError) as e:
            p.glwe_automorphism_dev(*args, 3, ctx)
        assert e.value.kind == "BadArgument" and "aligned" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheGlweTraceContext(fft, basis, 65)
    assert e.value.kind == "Unsupported"
    with pytest.raises(p.PfheError) as e:
        p.tfhe_generate_gksk_dev(z(32), z(32), fft, basis, z(key_len), [4], k)
    assert e.value.kind == "BadArgument" and "odd" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.tfhe_generate_gksk_dev(z(32), z(32), fft, basis, z(key_len), [3, 5], k)
    assert e.value.kind == "BadLength"
    torch.cuda.synchronize()


def test_second_thread_gets_busy(p):
    """Two threads call the host form of one handle over and over until one of them has been refused: a call that arrives
    while the other thread is inside gets Busy, and a call that arrives in between runs (neither is a failure, so the test
    waits for no timing).  Every refusal seen is Busy, and the handle still gives the right words afterwards."""
    bits, log_n, k, batch = 32, 10, 1, 16
    rng = np.random.default_rng(34)
    fft = table(p, log_n)
    ctx = p.TfheGlweTraceContext(fft, p.ApproxSignedBasis(bits, 8, 4), k)
    inp = rand_words(rng, bits, batch * ctx.glwe_len())
    keys = np.zeros(log_n * ctx.key_len(), np.complex128)            # zero keys: out = inp + (0, sigma(B)) step by step
    outs = [np.zeros(inp.size, np.uint32) for _ in range(2)]
    refused, done = [], threading.Event()

    def caller(out):
        for _ in range(200):
            if done.is_set():
                return
            try:
                p.glwe_trace(inp, keys, out, ctx)
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
    p.glwe_trace(inp, keys, outs[0], ctx)
    want = tm.trace(inp, np.zeros(log_n * ctx.key_len(), np.uint32), log_n,
                    lambda ct, key: np.zeros(ct.size, np.uint32), m.ApproxSignedBasis(bits, 8, 4), log_n, k)
    assert np.array_equal(outs[0], want)
