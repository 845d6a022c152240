"""GPU tests of the linear layer with clear weights (include/pfhe.h, pfhe_lwe{,32}_linear*): the word form
word for word against the integer model (tests/lwe_linear_model.py) at the shapes that reach every tile and every edge of
one, the int8 form against the word form on the sign-extended weights and against the model (byte patterns in every plane,
an asymmetric case for the operand maps, the fold of the plane sums), a two-layer network through tfhe_dense_layer_dev on
generated noisy keys, the refusals in their order, graph capture and two streams."""
import ctypes as C

import numpy as np
import pytest

import lwe_linear_model as lm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg
from test_gpu_tfhe_fft import dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

OK, BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE = 0, 32, 33, 34


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def dev_i8(w):
    import torch
    return torch.from_numpy(np.ascontiguousarray(w, np.int8)).cuda()


def edge_mixed(rng, bits, size):
    """random words with the edge words 0, 1, 2^(BITS-1), 2^BITS - 1 (-1 as a word) at random places and at both ends"""
    x = rand_words(rng, bits, size)
    edge = np.array([0, 1, 1 << (bits - 1), (1 << bits) - 1], dtype=np.uint64).astype(m.UINT[bits])
    at = rng.permutation(size)[:max(1, size // 3)]
    x[at] = edge[rng.integers(0, 4, at.size)]
    x[0], x[-1] = edge[3], edge[2]
    return x


def byte_pattern_words(rng, bits, size):
    """words whose bytes come from {0x00, 0x7f, 0x80, 0xff} in every plane, mixed with random words"""
    planes = rng.choice(np.array([0x00, 0x7f, 0x80, 0xff], np.uint8), (size, bits // 8))
    x = np.ascontiguousarray(planes).view(m.UINT[bits]).reshape(-1)
    at = rng.permutation(size)[:size // 4]
    x[at] = rand_words(rng, bits, at.size)
    return x


def sign_extended(w8, bits):
    return np.asarray(w8).astype(np.int64).view(np.uint64).astype(m.UINT[bits])


def run_dev(p, x, w, bias, row, in_f, out_f, bits, stream=None):
    """the device form on fresh device copies; returns (output words, the input words afterwards)"""
    import torch
    d_x = dev_words(x, bits)
    d_w = dev_i8(w) if np.asarray(w).dtype == np.int8 else dev_words(w, bits)
    d_b = dev_words(bias, bits) if bias is not None else None
    batch = x.size // (in_f * row)
    out = torch.full((batch * out_f * row,), -3, dtype=d_x.dtype, device="cuda")     # never zero-initialised
    p.lwe_linear_dev(d_x, d_w, d_b, out, row - 1, in_f, out_f, stream=stream)
    torch.cuda.synchronize()
    return host_words(out, bits), host_words(d_x, bits)


# (row, out_features, in_features, batch): every row / out / in / batch of the lists below at least once.  At these batches
# every grid is short and the kernel keeps one output per thread; the second list reaches the instances of 2, 4 and 8 outputs
# per thread, which run when (output tiles) x batch x (column tiles of 128) is at least 512 workgroups and half the tile
# would not hold the outputs: each at the last out_features of its tile and one past it, at the shortest grid that takes it
# and one workgroup short of it, with ragged columns and a second output tile.
WORD_CASES = [(2, 1, 1, 1), (127, 31, 3, 3), (128, 32, 4, 1), (129, 33, 5, 3), (2, 33, 63, 1), (129, 1, 64, 3),
              (128, 31, 65, 1), (127, 32, 64, 3), (129, 4, 5, 1), (2, 5, 3, 3), (127, 8, 64, 1), (128, 9, 4, 1),
              (129, 16, 65, 1), (2, 17, 1, 3)]
LONG_GRID_CASES = [(2, 5, 3, 512), (2, 8, 3, 512), (2, 9, 4, 512), (2, 16, 1, 512), (2, 17, 1, 512), (2, 17, 1, 511),
                   (129, 33, 5, 128), (128, 32, 4, 512), (127, 31, 65, 256), (129, 8, 64, 256), (129, 8, 3, 255)]


@pytest.mark.parametrize("bits", [32, 64])
def test_word_form_matches_the_model(p, bits):
    """row in {2, 127, 128, 129}, out_features in {1, 31, 32, 33}, in_features in {1, 3, 4, 5, 63, 64, 65}, batch in {1, 3},
    with a bias and without, inputs and weights edge words mixed with random ones; the host form gives the device form's
    words and the input is left as it was"""
    rng = np.random.default_rng(bits)
    assert {c[0] for c in WORD_CASES} == {2, 127, 128, 129} and {1, 31, 32, 33} <= {c[1] for c in WORD_CASES}
    assert {c[2] for c in WORD_CASES} == {1, 3, 4, 5, 63, 64, 65} and {c[3] for c in WORD_CASES} == {1, 3}
    for idx, (row, out_f, in_f, batch) in enumerate(WORD_CASES + LONG_GRID_CASES):
        x = edge_mixed(rng, bits, batch * in_f * row)
        w = edge_mixed(rng, bits, out_f * in_f)
        for bias in (edge_mixed(rng, bits, out_f), None):
            want = lm.linear(x, w, bias, row - 1, in_f, out_f, bits)
            got, after = run_dev(p, x, w, bias, row, in_f, out_f, bits)
            assert np.array_equal(got, want), (row, out_f, in_f, batch, bias is not None)
            assert np.array_equal(after, x)
        if idx % 4 == 1:                                          # the host form, without a bias and with one
            host = np.full(want.size, 7, m.UINT[bits])
            p.lwe_linear(x, w, None, host, row - 1, in_f, out_f)
            assert np.array_equal(host, want), ("host", row, out_f, in_f, batch)
            host_bias = edge_mixed(rng, bits, out_f)
            p.lwe_linear(x, w, host_bias, host, row - 1, in_f, out_f)
            assert np.array_equal(host, lm.linear(x, w, host_bias, row - 1, in_f, out_f, bits)), ("host, bias", row, out_f)


@pytest.mark.parametrize("bits", [32, 64])
def test_more_vectors_than_a_grid_dimension_and_a_glwe_row(p, bits):
    """batch 65 537 at row 2 with both features 1, in both forms; a GLWE row of 2 x 64 words as dimension 2*64 - 1 with a
    null bias"""
    rng = np.random.default_rng(100 + bits)
    batch = 65537
    x = edge_mixed(rng, bits, batch * 2)
    for w in (np.array([(1 << bits) - 3], np.uint64).astype(m.UINT[bits]), np.array([-5], np.int8)):
        bias = rand_words(rng, bits, 1)
        got, _ = run_dev(p, x, w, bias, 2, 1, 1, bits)
        assert np.array_equal(got, lm.linear(x, w, bias, 1, 1, 1, bits))
    row, in_f, out_f = 2 * 64, 3, 2
    x = edge_mixed(rng, bits, 2 * in_f * row)
    w = edge_mixed(rng, bits, out_f * in_f)
    got, _ = run_dev(p, x, w, None, row, in_f, out_f, bits)
    assert np.array_equal(got, lm.linear(x, w, None, row - 1, in_f, out_f, bits))


# (out_features, in_features, row, batch)
I8_CASES = [(1, 1, 15, 1), (15, 63, 16, 3), (16, 64, 17, 1), (17, 65, 129, 3), (33, 129, 15, 1), (33, 64, 129, 1),
            (1, 129, 16, 3), (16, 65, 129, 1)]


@pytest.mark.parametrize("bits", [32, 64])
def test_i8_form_matches_the_word_form_and_the_model(p, bits):
    """out_features in {1, 15, 16, 17, 33}, in_features in {1, 63, 64, 65, 129}, row in {15, 16, 17, 129}; weights from
    {-128, -1, 0, 1, 127} and random; the words' bytes from {0x00, 0x7f, 0x80, 0xff} in every plane and random"""
    rng = np.random.default_rng(200 + bits)
    assert {c[0] for c in I8_CASES} == {1, 15, 16, 17, 33} and {c[1] for c in I8_CASES} == {1, 63, 64, 65, 129}
    assert {c[2] for c in I8_CASES} == {15, 16, 17, 129}
    for out_f, in_f, row, batch in I8_CASES:
        x = byte_pattern_words(rng, bits, batch * in_f * row)
        w8 = rng.integers(-128, 128, out_f * in_f).astype(np.int8)
        at = rng.permutation(w8.size)[:max(1, w8.size // 2)]
        w8[at] = rng.choice(np.array([-128, -1, 0, 1, 127], np.int8), at.size)
        for bias in (edge_mixed(rng, bits, out_f), None):
            want = lm.linear(x, w8, bias, row - 1, in_f, out_f, bits)
            got, after = run_dev(p, x, w8, bias, row, in_f, out_f, bits)
            word, _ = run_dev(p, x, sign_extended(w8, bits), bias, row, in_f, out_f, bits)
            assert np.array_equal(got, word), (out_f, in_f, row, batch, bias is not None)
            assert np.array_equal(got, want), (out_f, in_f, row, batch, bias is not None)
            assert np.array_equal(after, x)
    out_f, in_f, row = I8_CASES[1][:3]
    x = byte_pattern_words(rng, bits, in_f * row)
    w8 = rng.integers(-128, 128, out_f * in_f).astype(np.int8)
    host = np.full(out_f * row, 7, m.UINT[bits])
    for bias in (None, edge_mixed(rng, bits, out_f)):
        p.lwe_linear(x, w8, bias, host, row - 1, in_f, out_f)
        assert np.array_equal(host, lm.linear(x, w8, bias, row - 1, in_f, out_f, bits)), bias is not None


@pytest.mark.parametrize("bits", [32, 64])
def test_i8_operand_maps_on_asymmetric_data(p, bits):
    """identity-like weights, W[o][3 o + 1] = 1 and W[o][3 o + 2] = -2, on words x[i][c] = 256 i + c: out[o][c] is written
    out below, and a swapped or transposed operand or result map gives other words"""
    out_f, in_f, row = 17, 64, 17
    w8 = np.zeros((out_f, in_f), np.int8)
    for o in range(out_f):
        w8[o, 3 * o + 1], w8[o, 3 * o + 2] = 1, -2
    i, c = np.meshgrid(np.arange(in_f), np.arange(row), indexing="ij")
    x = (256 * i + c).astype(m.UINT[bits]).reshape(-1)
    o, c = np.meshgrid(np.arange(out_f), np.arange(row), indexing="ij")
    want = ((256 * (3 * o + 1) + c) - 2 * (256 * (3 * o + 2) + c)).astype(np.int64).view(np.uint64).astype(m.UINT[bits])
    got, _ = run_dev(p, x, w8.reshape(-1), None, row, in_f, out_f, bits)
    assert np.array_equal(got, want.reshape(-1))


@pytest.mark.parametrize("bits", [32, 64])
def test_i8_plane_sums_are_folded_before_they_overflow(p, bits):
    """in_features = 2^17 + 1, weights all -128: against words all 0 the output is all 0, against words all ones it equals
    the model.  The kernel is fed x_b - 128, so with words all 0 every product is (-128)(-128) = 2^14 and an unfolded plane
    sum reaches 2^31 + 2^14: past the top of an i32.  With words all ones the product is 127 (-128) = -16 256 and the sum
    over 2^17 + 1 inputs is -2 130 722 688, still above -2^31; the third case, 2^17 + 2^11 inputs, takes it to
    -2 163 998 720, past the bottom.  A plane sum that wrapped modulo 2^32 would change no u32 word (2^32 2^(8b) = 0 modulo
    2^32) and would change the u64 words of every plane below the fourth, so the u64 run is the one that tells a wrap; either
    run would tell an accumulator that saturates."""
    w_word = lambda n: sign_extended(np.full(n, -128, np.int8), bits)
    top = (1 << bits) - 1
    for in_f, fill, passes in (((1 << 17) + 1, 0, True), ((1 << 17) + 1, top, False), ((1 << 17) + (1 << 11), top, True)):
        assert (abs(((fill & 0xff) - 128) * -128 * in_f) > 2 ** 31) == passes      # the unfolded plane sum
        w8 = np.full(in_f, -128, np.int8)
        x = np.full(in_f * 2, fill, np.uint64).astype(m.UINT[bits])
        got, _ = run_dev(p, x, w8, None, 2, in_f, 1, bits)
        if fill == 0:
            assert not got.any()
        assert np.array_equal(got, lm.linear(x, w8, None, 1, in_f, 1, bits)), (in_f, fill)
        word, _ = run_dev(p, x, w_word(in_f), None, 2, in_f, 1, bits)
        assert np.array_equal(got, word), (in_f, fill)


# ---------------- meaning on generated noisy keys ----------------

@pytest.mark.parametrize("case", lm.DENSE_CASES, ids=lambda c: "u%d-N%d-k%d-n%d" % (c[0], 1 << c[1], c[2], c[3]))
def test_two_layer_network_decodes_on_generated_keys(p, case):
    """The network of tests/lwe_linear_model.py through tfhe_dense_layer_dev, twice: keys generated by the device from
    bounded randomness, the 8 settings of three encrypted bits at Delta = 2^(BITS-3), each twice with fresh noise; every
    decoded output equals the clear network.  The condition on the noise is derived and asserted on the CPU
    (tests/test_lwe_linear_model.py)."""
    bits, log_n, k, n, lb, ell, g, pbits, noise = case
    assert pbits == lm.NET_P
    for weights in (lm.W1, lm.W2):
        left, right = lm.dense_margin(case, weights)
        assert left < right
    c = kg.noisy_case(*case, seed=3000 + bits)
    rng = np.random.default_rng(bits + 7)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *kg.KS_BASIS)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis)
    s, z_flat = dev_words(c["s"], bits), dev_words(bs.flatten_key(c["z"]), bits)
    bsk = p.tfhe_generate_bsk_dev(ctx, s, z_flat, dev_words(c["rand_bsk"], bits))
    ksk = dev_words(c["rand_ksk"], bits)
    p.tfhe_generate_ksk_dev(z_flat, s, ks_basis, ksk)
    delta = 1 << (bits - pbits - 1)
    settings = np.array([[(v >> j) & 1 for j in range(3)] for v in range(8)] * 2)            # 16 vectors of 3 bits
    lwe = kg.lwe_randomness(rng, bits, n, settings.size, noise).reshape(-1, n + 1)
    with np.errstate(over="ignore"):
        lwe[:, n] += (settings.reshape(-1).astype(np.uint64) * np.uint64(delta)).astype(m.UINT[bits])
    d_in = dev_words(lwe.reshape(-1), bits)
    p.lwe_encrypt_dev(d_in, s)
    tv1 = dev_words(bs.lut_test_vector(lm.threshold, pbits, bits, log_n, k), bits)
    tv2 = dev_words(bs.lut_test_vector(bs.lut(pbits), pbits, bits, log_n, k), bits)
    bias1 = dev_words((lm.B1.astype(np.uint64) * np.uint64(delta)).astype(m.UINT[bits]), bits)
    hidden = dev_words(np.zeros(16 * 2 * (n + 1), m.UINT[bits]), bits)
    out = dev_words(np.zeros(16 * (n + 1), m.UINT[bits]), bits)
    # layer 1 with int8 weights, layer 2 with the same weights as words: both forms feed a bootstrap
    p.tfhe_dense_layer_dev(d_in, dev_i8(lm.W1), bias1, bsk, tv1, ksk, hidden, ctx, 3, 2)
    p.tfhe_dense_layer_dev(hidden, dev_words(sign_extended(lm.W2, bits), bits), None, bsk, tv2, ksk, out, ctx, 2, 1)
    clear = [lm.clear_network(x) for x in settings]
    p.lwe_phase_dev(hidden, s)
    assert bs.decode(host_words(hidden, bits).reshape(-1, n + 1)[:, n], pbits, bits) == [h for r in clear for h in r[1]]
    p.lwe_phase_dev(out, s)
    assert bs.decode(host_words(out, bits).reshape(-1, n + 1)[:, n], pbits, bits) == [r[3] for r in clear]


# ---------------- call behaviour ----------------

@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_refusals_arrive_in_order(p, w, bits):
    import torch
    lib = p.lib()
    dim, in_f, out_f, batch = 5, 3, 2, 2
    row = dim + 1
    x = dev_words(np.zeros(batch * in_f * row, m.UINT[bits]), bits)
    wt = dev_words(np.ones(out_f * in_f, m.UINT[bits]), bits)
    w8 = dev_i8(np.ones(out_f * in_f, np.int8))
    bias = dev_words(np.zeros(out_f, m.UINT[bits]), bits)
    out = dev_words(np.zeros(batch * out_f * row, m.UINT[bits]), bits)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for entry, wp in (("linear", wt), ("linear_i8", w8)):
        call = getattr(lib, "pfhe_lwe%s_%s_dev" % (w, entry))
        good = [0, ptr(x), x.numel(), dim, ptr(wp), wp.numel(), in_f, out_f, ptr(bias), out_f, ptr(out), out.numel(), None]

        def with_(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return call(*a)

        assert with_() == OK
        for at in (3, 6, 7):                                              # the ranges, before any length
            for bad in (0, 2 ** 31 - 1):
                assert with_(**{"a%d" % at: bad, "a2": 1, "a5": 0}) == BAD_ARGUMENT
        assert with_(a2=x.numel() - 1) == BAD_LENGTH                      # the lengths, before any pointer
        assert with_(a5=wp.numel() + 1, a1=None) == BAD_LENGTH
        assert with_(a9=1, a4=None) == BAD_LENGTH
        assert with_(a11=out.numel() - row, a10=None) == BAD_LENGTH
        assert with_(a2=0, a11=0, a1=None, a10=None, a0=99) == OK         # the empty batch
        for at in (1, 4, 8, 10):                                          # a null pointer
            assert with_(**{"a%d" % at: None, "a0": 99}) == BAD_ARGUMENT
        assert with_(a9=0, a0=99, a10=C.c_void_p(x.data_ptr() + 8)) == BAD_ARGUMENT      # a bias pointer with no length,
        assert "bias" in lib.pfhe_last_error().decode()                                  # before the overlap
        assert with_(a8=None, a9=0) == OK                                 # no bias
        big = dev_words(np.zeros(batch * in_f * row, m.UINT[bits]), bits)
        assert call(99, ptr(big), big.numel(), dim, ptr(wp), wp.numel(), in_f, out_f, ptr(bias), out_f,
                    C.c_void_p(big.data_ptr() + 8), out.numel(), None) == BAD_ARGUMENT      # the overlap, before the device
        assert "overlap" in lib.pfhe_last_error().decode()
        assert with_(a0=99) == NO_DEVICE
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        p.lwe_linear_dev(x, wt.to(torch.int16), bias, out, dim, in_f, out_f)
    with pytest.raises(ValueError):
        p.lwe_linear_dev(x, wt.double(), bias, out, dim, in_f, out_f)


def dense_case(p, bits):
    """a dense layer of exact words: random keys and inputs (what it means is the network test's business)"""
    import torch
    log_n, k, n, in_f, out_f, batch = 6, 1, 5, 4, 3, 2
    lb, ell = {32: (7, 3), 64: (15, 2)}[bits]
    rng = np.random.default_rng(300 + bits)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *kg.KS_BASIS)
    ctx = p.TfheBootstrapContext(p.FullComplex64FftTable(log_n), basis, n, k, ks_basis)
    bsk = torch.from_numpy(rng.standard_normal(2 * ctx.bsk_len()) * 2.0 ** 10).cuda()
    ksk = dev_words(rand_words(rng, bits, ctx.ksk_len()), bits)
    tv = dev_words(rand_words(rng, bits, (k + 1) << log_n), bits)
    x = dev_words(rand_words(rng, bits, batch * in_f * (n + 1)), bits)
    w8 = dev_i8(rng.integers(-128, 128, out_f * in_f))
    bias = dev_words(rand_words(rng, bits, out_f), bits)
    return ctx, bsk, ksk, tv, x, w8, bias, in_f, out_f, batch * out_f * (n + 1)


def test_graph_capture_of_a_dense_layer_replays_the_eager_call(p):
    import torch
    bits = 32
    ctx, bsk, ksk, tv, x, w8, bias, in_f, out_f, out_len = dense_case(p, bits)
    eager = torch.zeros(out_len, dtype=x.dtype, device="cuda")
    p.tfhe_dense_layer_dev(x, w8, bias, bsk, tv, ksk, eager, ctx, in_f, out_f)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.tfhe_dense_layer_dev(x, w8, bias, bsk, tv, ksk, out, ctx, in_f, out_f, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("bits", [32, 64])
def test_a_call_gives_the_same_words_on_two_streams_in_turn(p, bits):
    import torch
    rng = np.random.default_rng(400 + bits)
    row, in_f, out_f, batch = 129, 65, 33, 2
    x = rand_words(rng, bits, batch * in_f * row)
    bias = rand_words(rng, bits, out_f)
    for w in (rand_words(rng, bits, out_f * in_f), rng.integers(-128, 128, out_f * in_f).astype(np.int8)):
        want = lm.linear(x, w, bias, row - 1, in_f, out_f, bits)
        for _ in range(2):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                got, _ = run_dev(p, x, w, bias, row, in_f, out_f, bits, stream=s)
            assert np.array_equal(got, want)
