"""GPU tests of ring packing by automorphisms (include/pfhe.h, pfhe_ringpack{,32}_*): rule A word for word against its composition of public calls (the monomial
product, a wrapping subtraction and addition, glwe_automorphism_dev, a wrapping addition) on full-torus keys, at the shapes
where the fused kernel's slot loop and the general form take their paths; rule B against the composition of
lwe_embed_glwe_dev, rule A's composition level by level (batched over the nodes) and glwe_trace_dev, over the counts at
which the tree changes shape, with chunking, max_count below N, a repeat call, the host form and graph replay; bit for bit
against the integer schoolbook where the product is exact, the inputs walking the digit rule's edge words; what the pack
means on noisy keys, all on the device; errors and the lease."""
import threading

import numpy as np
import pytest

import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_ring_pack_model as rp
import tfhe_trace_model as tm
from test_gpu_tfhe_fft import TORCH_INT, dev_words, host_words, rand_words
from test_gpu_tfhe_trace import device_randomness, empty_words, fourier_keys, table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def merge_composition(p, trace, even, odd, key, level):
    """rule A as public calls on a batch of pairs"""
    import torch
    fft, k = trace.fft, trace.glwe_dimension
    n = fft.poly_length()
    batch = even.numel() // trace.glwe_len()
    exps = torch.full((batch,), n >> level, dtype=torch.int32, device="cuda")
    shifted = torch.empty_like(odd)
    fft.mul_monomial_each_to_dev(odd, exps, shifted, polys_per_exp=k + 1)
    d, s = even - shifted, even + shifted
    auto = torch.empty_like(d)
    p.glwe_automorphism_dev(d, key, auto, (1 << level) + 1, trace)
    return s + auto


def pack_composition(p, trace, lwe, keys, count):
    """rule B as public calls: the embedding, the levels batched over nodes and groups, the trailing trace"""
    import torch
    fft, k = trace.fft, trace.glwe_dimension
    n, log_n, glwe, key_len = fft.poly_length(), fft.log_n, trace.glwe_len(), trace.key_len()
    batch = lwe.numel() // (count * (k * n + 1))
    mm = rp.ceil_log2(count)
    leaves = torch.empty(batch * count * glwe, dtype=lwe.dtype, device="cuda")
    p.lwe_embed_glwe_dev(lwe, leaves, fft, k)
    nodes = torch.zeros((batch, 1 << mm, glwe), dtype=lwe.dtype, device="cuda")
    nodes[:, :count] = leaves.view(batch, count, glwe)
    for level in range(1, mm + 1):
        half = 1 << (mm - level)
        even, odd = nodes[:, :half].reshape(-1), nodes[:, half:2 * half].reshape(-1)
        key = keys[(log_n - level) * key_len:(log_n - level + 1) * key_len]
        nodes = merge_composition(p, trace, even, odd, key, level).view(batch, half, glwe)
    root = nodes[:, 0].reshape(-1).clone()
    if mm < log_n:
        p.glwe_trace_dev(root, keys[:(log_n - mm) * key_len], root, trace, log_n - mm)
    return root


def merge_run(p, ctx, even, odd, key, level, bits):
    out = empty_words(even.numel(), bits)
    p.glwe_ring_merge_dev(even, odd, key, out, level, ctx)
    return out


def pack_run(p, ctx, lwe, keys, count, bits, stream=None):
    out = empty_words(lwe.numel() // (count * ctx.lwe_len()) * ctx.glwe_len(), bits)
    p.lwe_ring_pack_dev(lwe, keys, out, count, ctx, stream)
    return out


# ---------------- rule A against its composition ----------------

# bits, log_n, k, log_basis, ell (None: the full length, drop_bits 0)
RULE_A_CASES = [
    (32, 1, 1, 8, None),       # fused: one slot, 255 idle threads, s = 1 alone; drop_bits 0
    (64, 2, 1, 15, 2),         # fused: every level
    (64, 9, 1, 20, 1),         # fused: exactly one slot per thread, ell = 1
    (32, 11, 1, 7, 3),         # fused: four slots
    (64, 11, 1, 16, None),     # four slots at u64, drop_bits 0
    (32, 5, 2, 7, 3),          # general
    (64, 3, 3, 16, None),      # general, drop_bits 0
]


@pytest.mark.parametrize("bits,log_n,k,lb,ell", RULE_A_CASES, ids=lambda v: str(v))
def test_merge_equals_the_composition_of_public_calls(p, bits, log_n, k, lb, ell):
    """three pairs on a default handle and on one of chunk 1; out == even; the host form"""
    import torch
    batch = 3
    rng = np.random.default_rng(bits + 10 * log_n + k)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    trace = p.TfheGlweTraceContext(fft, basis, k)
    wide, narrow = p.TfheRingPackContext(fft, basis, k), p.TfheRingPackContext(fft, basis, k, max_count=1, chunk=1)
    glwe = wide.glwe_len()
    assert glwe == trace.glwe_len() and wide.key_len() == trace.key_len() and not wide.in_use()
    assert wide.max_count == 1 << log_n and wide.trace_exponents() == trace.trace_exponents()
    even, odd = (dev_words(rand_words(rng, bits, batch * glwe), bits) for _ in range(2))
    key = fourier_keys(p, fft, dev_words(rand_words(rng, bits, wide.key_len()), bits))
    levels = range(1, log_n + 1) if log_n == 2 else sorted({1, log_n})
    for level in levels:
        want = merge_composition(p, trace, even, odd, key, level)
        for ctx in (wide, narrow):
            assert torch.equal(merge_run(p, ctx, even, odd, key, level, bits), want), (level, ctx is wide)
        for ctx in (wide, narrow):
            same = even.clone()
            p.glwe_ring_merge_dev(same, odd, key, same, level, ctx)              # out is even
            assert torch.equal(same, want), (level, ctx is wide)
    host = np.zeros(batch * glwe, m.UINT[bits])
    p.glwe_ring_merge(host_words(even, bits), host_words(odd, bits), key.cpu().numpy(), host, log_n, narrow)
    assert np.array_equal(host, host_words(merge_composition(p, trace, even, odd, key, log_n), bits))
    assert wide.scratch_bytes() > 0                                              # the node buffer, in either form


# ---------------- rule B against the composition ----------------

# bits, log_n, k, log_basis, ell, counts, batch
RULE_B_CASES = [
    (64, 2, 1, 15, 2, (1, 2, 3, 4), 3),
    (32, 4, 1, 7, 3, (1, 2, 3, 5, 9, 16), 3),
    (32, 10, 1, 7, 3, (1, 2, 3, 5, 513, 1024), 2),
    (64, 10, 1, 15, 2, (5, 1024), 2),
    (64, 11, 1, 20, 1, (2048,), 1),
    (32, 5, 2, 7, 3, (4,), 3),             # general
    (64, 12, 1, 15, 2, (4,), 2),           # general: k = 1 above the fused N
]


@pytest.mark.parametrize("bits,log_n,k,lb,ell,counts,batch", RULE_B_CASES, ids=lambda v: str(v))
def test_pack_equals_the_composition_of_public_calls(p, bits, log_n, k, lb, ell, counts, batch):
    import torch
    n = 1 << log_n
    rng = np.random.default_rng(bits + 10 * log_n + k)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    trace = p.TfheGlweTraceContext(fft, basis, k)
    ctx = p.TfheRingPackContext(fft, basis, k, max_count=max(counts))
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, log_n * ctx.key_len()), bits))
    for count in counts:
        lwe = dev_words(rand_words(rng, bits, batch * count * ctx.lwe_len()), bits)
        want = pack_composition(p, trace, lwe, keys, count)
        assert torch.equal(pack_run(p, ctx, lwe, keys, count, bits), want), count
    if max(counts) >= 3:
        assert [ctx.slot(i, 3) for i in range(3)] == [0, n // 4, n // 2] and ctx.slot(1, 2) == n // 2 and ctx.slot(0, 1) == 0


@pytest.mark.parametrize("bits,log_n,k", [(32, 4, 1), (64, 5, 2)])
def test_pack_in_chunks_below_max_count_twice_and_on_host_arrays(p, bits, log_n, k):
    """batch 3 under chunk 1 and chunk 2, max_count below N, a repeat call, the host form"""
    import torch
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    batch, max_count = 3, 6
    rng = np.random.default_rng(bits + log_n)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    trace = p.TfheGlweTraceContext(fft, basis, k)
    one, two = (p.TfheRingPackContext(fft, basis, k, max_count=max_count, chunk=c) for c in (1, 2))
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, log_n * one.key_len()), bits))
    for count in (6, 5, 1):
        lwe = dev_words(rand_words(rng, bits, batch * count * one.lwe_len()), bits)
        want = pack_composition(p, trace, lwe, keys, count)
        for ctx in (one, two, two):                                              # the last: a repeat call
            assert torch.equal(pack_run(p, ctx, lwe, keys, count, bits), want), count
    host = np.zeros(batch * one.glwe_len(), m.UINT[bits])
    p.lwe_ring_pack(host_words(lwe, bits), keys.cpu().numpy(), host, 1, two)
    assert np.array_equal(host, host_words(want, bits))
    with pytest.raises(p.PfheError) as e:
        pack_run(p, one, dev_words(rand_words(rng, bits, 7 * one.lwe_len()), bits), keys, 7, bits)
    assert e.value.kind == "BadArgument" and "count" in str(e.value)


def test_graph_capture_replays_the_eager_call(p):
    """a linear capture on one stream, two chunks and all levels in the graph, replayed twice on fresh inputs"""
    import torch
    bits, log_n, k, batch, count = 32, 8, 1, 3, 5
    rng = np.random.default_rng(78)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, 7, 3)
    ctx = p.TfheRingPackContext(fft, basis, k, max_count=8, chunk=2)
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, log_n * ctx.key_len()), bits))
    fresh = dev_words(rand_words(rng, bits, batch * count * ctx.lwe_len()), bits)
    eager = pack_run(p, ctx, fresh, keys, count, bits)
    torch.cuda.synchronize()
    inp, out = fresh.clone(), torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.lwe_ring_pack_dev(inp, keys, out, count, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        inp.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------- the exact regime against the integer schoolbook ----------------

@pytest.mark.parametrize("bits,log_n,k,lb,ell", [(32, 4, 1, 7, 3), (64, 4, 1, 15, 2), (32, 3, 2, 7, 3), (64, 3, 2, 15, 2)])
def test_exact_regime_equals_the_integer_schoolbook(p, bits, log_n, k, lb, ell):
    """key words |g| <= 2^10 and (k+1) ell N 2^(logB-1) 2^10 <= 2^40: the f64 product is the integer one.  The LWE inputs are
    the digit rule's edge words; counts N, 3 and 1"""
    n = 1 << log_n
    mb = m.ApproxSignedBasis(bits, lb, ell)
    assert (k + 1) * mb.decompose_length * n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    rng = np.random.default_rng(bits + log_n + lb)
    edges = ew.edge_words(bits, lb, ell)
    keys = rng.integers(-1024, 1025, log_n * tm.key_len(mb, log_n, k)).astype(np.int64).view(np.uint64).astype(m.UINT[bits])
    fft = table(p, log_n)
    ctx = p.TfheRingPackContext(fft, p.ApproxSignedBasis(bits, lb, ell), k)
    fkeys = fourier_keys(p, fft, dev_words(keys, bits))
    product = tm.exact_product(mb, log_n, k)
    for count in (n, 3, 1):
        words = count * (k * n + 1)
        batch = max(2, -(-edges.size // words))                     # every edge word is somewhere in the inputs
        lwe = rng.permutation(np.resize(edges, max(edges.size, batch * words)))[:batch * words].astype(m.UINT[bits])
        got = pack_run(p, ctx, dev_words(lwe, bits), fkeys, count, bits)
        assert np.array_equal(host_words(got, bits), rp.pack(lwe, keys, count, product, mb, log_n, k)), count


# ---------------- meaning on noisy keys, all on the device ----------------

@pytest.mark.parametrize("shape", tm.NOISY_SHAPES, ids=lambda c: "u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]))
def test_pack_on_noisy_keys_puts_every_bit_at_its_slot(p, shape):
    """Binary keys, torus_noise(bound=E) on every key row and on the inputs.  LWE ciphertexts of a bit at Delta_in =
    2^(BITS-2) / N under the extracted key, packed at counts N and 3, read with glwe_phase_dev: coefficient
    ctx.slot(i, count) within rp.ring_pack_bound of 2^(BITS-2) bit_i, every other coefficient within it of 0.  Largest
    errors seen on the device are in DESIGN.md section 28's table."""
    import torch
    bits, log_n, k, lb, ell, noise = shape
    n, batch = 1 << log_n, 4
    gen = torch.Generator(device="cuda").manual_seed(5000 + bits + log_n + k)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    ctx = p.TfheRingPackContext(fft, basis, k)
    dt = getattr(torch, TORCH_INT[bits])
    z = torch.randint(0, 2, (k * n,), generator=gen, device="cuda").to(dt)
    exps = ctx.trace_exponents()
    rand = device_randomness(p, bits, log_n, k, len(exps) * k * ell, noise, gen)
    keys = p.tfhe_generate_gksk_dev(z, z, fft, basis, rand, exps, k)
    bound = rp.ring_pack_bound(noise, *shape)
    assert bound < 2.0 ** (bits - 3)
    for count in (n, 3):
        total = batch * count
        msgs = torch.randint(0, 2, (total,), generator=gen, device="cuda").to(dt)
        lwe = p.torus_uniform(total * (k * n + 1), bits, generator=gen).view(total, k * n + 1)
        lwe[:, k * n] = p.torus_noise(total, bits, bound=noise, generator=gen) + msgs * (1 << (bits - 2 - log_n))
        lwe = lwe.view(-1)
        p.lwe_encrypt_dev(lwe, z)
        out = pack_run(p, ctx, lwe, keys, count, bits)
        p.glwe_phase_dev(out, z, fft, k)
        ph = host_words(out, bits).reshape(batch, k + 1, n)[:, k]
        want = np.zeros((batch, n), m.UINT[bits])
        slots = [ctx.slot(i, count) for i in range(count)]
        want[:, slots] = (host_words(msgs, bits).reshape(batch, count).astype(np.uint64) << np.uint64(bits - 2)).astype(m.UINT[bits])
        err = float(m.centred_error(ph, want, bits).max())
        print("bits %d log_n %d k %d count %d: err 2^%.1f bound 2^%.1f; Delta_out/2 2^%d"
              % (bits, log_n, k, count, np.log2(max(err, 1)), np.log2(bound), bits - 3))
        assert err <= bound, (count, err, bound)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    bits, log_n, k = 32, 5, 1
    fft, basis = table(p, log_n), p.ApproxSignedBasis(32, 7, 3)
    ctx = p.TfheRingPackContext(fft, basis, k, max_count=8)
    glwe, lwe_len, key_len = ctx.glwe_len(), ctx.lwe_len(), ctx.key_len()
    assert glwe == 64 and lwe_len == 33 and key_len == 3 * 64 and not ctx.in_use()
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")
    f = lambda size: torch.zeros(size, dtype=torch.complex128, device="cuda")
    even, odd, out, keys = z(4 * glwe), z(4 * glwe), z(4 * glwe), f(log_n * key_len)
    key = keys[:key_len]
    lwe = z(4 * 8 * lwe_len)
    p.glwe_ring_merge_dev(even, odd, key, out, 3, ctx)                       # the lengths that fit
    p.lwe_ring_pack_dev(lwe, keys, out, 8, ctx)
    p.lwe_ring_pack_dev(lwe[:4 * 3 * lwe_len], keys, out, 3, ctx)
    p.lwe_ring_pack_dev(z(0), keys, z(0), 8, ctx)                            # an empty batch is a no-op
    p.glwe_ring_merge_dev(z(0), z(0), key, z(0), 1, ctx)
    for args in ((even[:-1], odd[:-1], key, out[:-1]), (even, odd[:3 * glwe], key, out), (even, odd, key, out[:3 * glwe]),
                 (even, odd, keys[:key_len - 1], out), (even, odd, keys[:2 * key_len], out)):
        with pytest.raises(p.PfheError) as e:
            p.glwe_ring_merge_dev(*args, 3, ctx)
        assert e.value.kind == "BadLength", e.value
    for args, count in (((lwe[:-1], keys, out), 8), ((lwe, keys[:-1], out), 8), ((lwe, keys[:4 * key_len], out), 8),
                        ((lwe, keys, out[:3 * glwe]), 8), ((lwe, keys, out), 3)):
        with pytest.raises(p.PfheError) as e:
            p.lwe_ring_pack_dev(*args, count, ctx)
        assert e.value.kind == "BadLength", (count, e.value)
    for count in (0, 9, 32):                                                 # 0, above max_count
        with pytest.raises(p.PfheError) as e:
            p.lwe_ring_pack_dev(lwe, keys, out, count, ctx)
        assert e.value.kind == "BadArgument" and "count" in str(e.value)
    for level in (0, log_n + 1, 2 ** 31):
        with pytest.raises(p.PfheError) as e:
            p.glwe_ring_merge_dev(even, odd, key, out, level, ctx)
        assert e.value.kind == "BadArgument" and "level" in str(e.value)
    with pytest.raises(p.PfheError) as e:                                    # the value is judged before the lengths
        p.glwe_ring_merge_dev(even[:-1], odd, key, out, 0, ctx)
    assert e.value.kind == "BadArgument"
    with pytest.raises(TypeError):                                           # words of another width
        p.glwe_ring_merge_dev(even.long(), odd, key, out, 3, ctx)
    both = z(5 * glwe)
    for a, b, c in ((both[:4 * glwe], odd, both[glwe:]), (even, both[:4 * glwe], both[glwe:]), (even, odd, odd)):
        with pytest.raises(p.PfheError) as e:                                # out: exactly even, or disjoint; never odd
            p.glwe_ring_merge_dev(a, b, key, c, 3, ctx)
        assert e.value.kind == "BadArgument" and "exactly even" in str(e.value)
    p.glwe_ring_merge_dev(even, odd, key, even, 3, ctx)
    wide = z(4 * 8 * lwe_len)
    with pytest.raises(p.PfheError) as e:
        p.lwe_ring_pack_dev(wide, keys, wide[:4 * glwe], 8, ctx)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    ptr = lambda t, off=0: (t.data_ptr() + off, t.numel() - (1 if off else 0), "32")
    for args in (((0, even.numel(), "32"), odd, key, out), (even, (0, odd.numel(), "32"), key, out), (even, odd, (0, key_len), out),
                 (even, odd, key, (0, out.numel(), "32"))):
        with pytest.raises(p.PfheError) as e:                                # null pointers, after the lengths
            p.glwe_ring_merge_dev(*args, 3, ctx)
        assert e.value.kind == "BadArgument"
    for args in (((0, lwe.numel(), "32"), keys, out), (lwe, (0, keys.numel()), out), (lwe, keys, (0, out.numel(), "32"))):
        with pytest.raises(p.PfheError) as e:
            p.lwe_ring_pack_dev(*args, 8, ctx)
        assert e.value.kind == "BadArgument"
    odd_in, odd_out = z(4 * glwe + 1), z(4 * glwe + 1)
    for args in ((ptr(odd_in, 4), odd, key, out), (even, ptr(odd_in, 4), key, out), (even, odd, key, ptr(odd_out, 4))):
        with pytest.raises(p.PfheError) as e:
            p.glwe_ring_merge_dev(*args, 3, ctx)
        assert e.value.kind == "BadArgument" and "aligned" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.lwe_ring_pack_dev(lwe, keys, ptr(odd_out, 4), 8, ctx)
    assert e.value.kind == "BadArgument" and "aligned" in str(e.value)
    for bad in (0, 33):
        with pytest.raises(p.PfheError) as e:
            p.TfheRingPackContext(fft, basis, k, max_count=bad)
        assert e.value.kind == "BadArgument" and "max_count" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheRingPackContext(fft, basis, 65)
    assert e.value.kind == "Unsupported"
    torch.cuda.synchronize()


def test_second_thread_gets_busy(p):
    """Two threads call the host form of one handle over and over until one of them has been refused: a call that arrives
    while the other thread is inside gets Busy, and a call that arrives in between runs (neither is a failure, so the test
    waits for no timing).  Every refusal seen is Busy, and the handle still gives the right words afterwards."""
    bits, log_n, k, batch, count = 32, 10, 1, 4, 8
    rng = np.random.default_rng(35)
    fft = table(p, log_n)
    ctx = p.TfheRingPackContext(fft, p.ApproxSignedBasis(bits, 8, 4), k, max_count=count)
    lwe = rand_words(rng, bits, batch * count * ctx.lwe_len())
    keys = np.zeros(log_n * ctx.key_len(), np.complex128)            # zero keys: every product is zero
    outs = [np.zeros(batch * ctx.glwe_len(), np.uint32) for _ in range(2)]
    refused, done = [], threading.Event()

    def caller(out):
        for _ in range(200):
            if done.is_set():
                return
            try:
                p.lwe_ring_pack(lwe, keys, out, count, ctx)
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
    p.lwe_ring_pack(lwe, keys, outs[0], count, ctx)
    want = rp.pack(lwe, np.zeros(log_n * ctx.key_len(), np.uint32), count, lambda ct, key: np.zeros(ct.size, np.uint32),
                   m.ApproxSignedBasis(bits, 8, 4), log_n, k)
    assert np.array_equal(outs[0], want)
