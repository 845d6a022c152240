"""GPU parity of the torus FFT tables and the TFHE external product (include/pfhe.h pfhe_fft_*, pfhe_tfhe{,32}_*) against
the numpy model of the reference (tests/tfhe_fft_model.py) and its exact integer schoolbook."""
import threading

import numpy as np
import pytest

import tfhe_fft_model as m

pytestmark = pytest.mark.gpu

TORCH_INT = {32: "int32", 64: "int64"}


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def dev_words(x, bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(m.SINT[bits])).cuda()


def host_words(t, bits):
    return t.cpu().numpy().view(m.UINT[bits])


def dev_complex(y):
    import torch
    return torch.from_numpy(np.ascontiguousarray(y, np.complex128)).cuda()


def rand_words(rng, bits, size):
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(m.UINT[bits])


def device_forward(p, fft, x, bits):
    import torch
    out = torch.empty(x.size, dtype=torch.complex128, device="cuda")
    fft.forward_torus_dev(dev_words(x, bits), out)
    return out.cpu().numpy()


def device_inverse(p, fft, y, bits):
    import torch
    out = torch.empty(y.size, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")
    fft.inverse_torus_dev(dev_complex(y), out)
    return host_words(out, bits)


# ---------------- transforms ----------------

@pytest.mark.parametrize("bits", [32, 64])
def test_forward_matches_model(p, bits):
    rng = np.random.default_rng(bits)
    for log_n in range(1, 15):
        fft = p.FullComplex64FftTable(log_n)
        n = 1 << log_n
        assert fft.poly_length() == n and fft.fourier_length() == n
        x = rand_words(rng, bits, 3 * n)
        got = device_forward(p, fft, x, bits).reshape(3, n)
        want = m.FullComplex64FftTable(log_n).forward(x.reshape(3, n), bits)
        bound = 1e-13 * n * np.max(np.abs(m.centred(x, bits)))
        assert np.max(np.abs(got - want)) <= bound, log_n


@pytest.mark.parametrize("bits", [32, 64])
def test_roundtrip_bit_exact(p, bits):
    rng = np.random.default_rng(bits + 1)
    for log_n in range(1, 15):
        fft = p.FullComplex64FftTable(log_n)
        n = 1 << log_n
        if bits == 32:
            x = rand_words(rng, 32, 2 * n)
        else:
            x = rng.integers(-2 ** 40, 2 ** 40 + 1, 2 * n).astype(np.uint64)
        assert np.array_equal(device_inverse(p, fft, device_forward(p, fft, x, bits), bits), x), log_n


@pytest.mark.parametrize("bits", [32, 64])
def test_inverse_of_non_hermitian_spectra(p, bits):
    rng = np.random.default_rng(bits + 2)
    for log_n in range(1, 15):
        fft = p.FullComplex64FftTable(log_n)
        n = 1 << log_n
        y = (rng.normal(size=2 * n) + 1j * rng.normal(size=2 * n)) * 2.0 ** 30
        got = device_inverse(p, fft, y, bits).reshape(2, n)
        want = m.FullComplex64FftTable(log_n).inverse(y.reshape(2, n), bits)
        err = m.centred_error(got, want, bits)
        assert err.max() <= 1 and (err == 0).mean() > 0.999, log_n


def test_conversion_edge_values(p):
    fft = p.FullComplex64FftTable(4)
    for v, bits, want in ((2.0 ** 64 + 2.0 ** 40, 64, 2 ** 40), (2.0 ** 40 + 5, 32, 5), (2.0 ** 70, 32, 0xFFFFFFFF),
                          (-2.0 ** 70, 32, 0), (2.0 ** 127, 64, 2 ** 64 - 1), (-2.0 ** 127, 64, 0),
                          (-(2.0 ** 64) - 2.0 ** 12, 64, 2 ** 64 - 2 ** 12), (-2.5, 64, 2 ** 64 - 3), (2.5, 32, 3),
                          (2.0 ** 100 + 2.0 ** 60, 64, 2 ** 60)):
        assert int(device_inverse(p, fft, np.full(16, v, np.complex128), bits)[0]) == want, (v, bits)


def test_host_slices_match_device(p):
    rng = np.random.default_rng(5)
    fft = p.FullComplex64FftTable(9)
    for bits in (32, 64):
        x = rand_words(rng, 32, 3 * 512) if bits == 32 else rng.integers(-2 ** 40, 2 ** 40, 3 * 512).astype(np.uint64)
        y = np.empty(x.size, np.complex128)
        fft.forward_torus_slice(x, y)
        assert np.array_equal(y, device_forward(p, fft, x, bits))
        back = np.empty_like(x)
        fft.inverse_torus_slice(y.view(np.float64), back)
        assert np.array_equal(back, x)


def test_reference_transform_tests(p):
    """roundtrip.rs and negacyclic.rs, log N 1..6, through the device transforms"""
    pat = [0, 1, -1, 2, -2]
    rng = np.random.default_rng(6)
    for log_n in range(1, 7):
        fft = p.FullComplex64FftTable(log_n)
        n = 1 << log_n
        for bits in (32, 64):
            cases = [np.array([pat[i % 5] for i in range(n)], np.int64).astype(m.UINT[bits]), np.zeros(n, m.UINT[bits])]
            cases += [np.eye(1, n, pos, dtype=m.UINT[bits])[0] for pos in (0, 1, n // 2, n - 1)]
            for x in cases:
                assert np.array_equal(device_inverse(p, fft, device_forward(p, fft, x, bits), bits), x)
        a = rng.integers(-50, 50, n).astype(np.uint32)
        b = rng.integers(-50, 50, n).astype(np.uint32)
        prod = device_forward(p, fft, a, 32) * device_forward(p, fft, b, 32)
        want = m.negacyclic_u64(a.astype(np.int32).astype(np.int64).view(np.uint64),
                                b.astype(np.int32).astype(np.int64).view(np.uint64)).astype(np.uint32)
        assert np.array_equal(device_inverse(p, fft, prod, 32), want)


def test_write_fourier_form_is_the_batched_forward(p):
    """fourier_convert.rs: GLWE / GLev / GGSW containers are polynomial after polynomial"""
    rng = np.random.default_rng(7)
    fft = p.FullComplex64FftTable(5)
    k, ell = 2, 3
    for polys in (k + 1, ell * (k + 1), (k + 1) * ell * (k + 1)):
        x = rand_words(rng, 32, polys * 32)
        y = np.empty(x.size, np.complex128)
        p.write_fourier_form(x, y, fft)
        assert np.max(np.abs(y.reshape(polys, 32) - m.FullComplex64FftTable(5).forward(x.reshape(polys, 32), 32))) < 1e-3
        back = np.empty_like(x)
        fft.inverse_torus_slice(y, back)
        assert np.array_equal(back, x)


# ---------------- the product ----------------

def make_key(p, fft, g, bits):
    """the Fourier GGSW of a coefficient key g through the device forward (write_fourier_form)"""
    return device_forward(p, fft, g, bits)


def run_product(p, ctx, inp, key, bits):
    import torch
    out = torch.empty(inp.size, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")
    p.tfhe_external_product_to_dev(dev_words(inp, bits), dev_complex(key), out, ctx)
    return host_words(out, bits)


def test_reference_smoke_and_zero(p):
    log_n, k, n = 3, 1, 8
    fft = p.FullComplex64FftTable(log_n)
    b, mb = p.ApproxSignedBasis(32, 4, 2), m.ApproxSignedBasis(32, 4, 2)
    ctx = p.TfheFftContext(fft, b, k)
    g = np.array([(i % 7) - 3 for i in range(64)], np.int64).astype(np.uint32)
    key = make_key(p, fft, g, 32)
    rng = np.random.default_rng(8)
    for inp in (np.array([(i % 5) - 2 for i in range(16)], np.int64).astype(np.uint32), rand_words(rng, 32, 16)):
        out = np.empty_like(inp)
        p.tfhe_external_product_to(inp, key, out, ctx)
        assert np.array_equal(out, m.schoolbook(inp, g, mb, log_n, k))
    fz = p.FullComplex64FftTable(2)
    cz = p.TfheFftContext(fz, p.ApproxSignedBasis(32, 8, 1), 1)
    z = np.full(8, 7, np.uint32)
    p.tfhe_external_product_to(np.zeros(8, np.uint32), np.ones(16, np.complex128), z, cz)
    assert not z.any()


EXACT = [  # bits, log_n, k, log_basis, ell (None = full)
    (32, 10, 1, 7, 3), (32, 11, 1, 10, 2), (32, 12, 1, 7, 3), (32, 14, 1, 10, 2),
    (64, 10, 1, 15, 2), (64, 11, 1, 15, 2), (64, 12, 1, 15, 2), (64, 14, 1, 15, 2),
    (32, 10, 2, 7, 3), (64, 9, 2, 15, 2),         # k = 2 (general form)
    (32, 10, 1, 8, None), (32, 12, 1, 8, None),   # drop_bits = 0
    (32, 10, 1, 1, 8), (64, 12, 1, 1, 10),        # log B = 1
]


@pytest.mark.parametrize("bits,log_n,k,lb,ell", EXACT)
def test_product_exact_regime(p, bits, log_n, k, lb, ell):
    """key words |g| <= 2^10 and (k+1) ell N 2^(logB-1) 2^10 <= 2^40: f64 keeps every accumulator exact"""
    n = 1 << log_n
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    L = b.decompose_length()
    assert (k + 1) * L * n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    rng = np.random.default_rng(log_n * 100 + lb)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheFftContext(fft, b, k)
    g = rng.integers(-1024, 1025, (k + 1) * L * (k + 1) * n).astype(m.UINT[bits])
    key = make_key(p, fft, g, bits)
    batch = 2
    inp = rand_words(rng, bits, batch * (k + 1) * n)
    out = run_product(p, ctx, inp, key, bits)
    W = (k + 1) * n
    for e in range(batch):
        assert np.array_equal(out[e * W:(e + 1) * W], m.schoolbook(inp[e * W:(e + 1) * W], g, mb, log_n, k)), e


REALISTIC = [(32, 10, 1, 7, 3), (32, 10, 1, 10, 2), (32, 11, 1, 7, 3), (32, 11, 1, 10, 2),
             (64, 11, 1, 23, 1), (64, 11, 1, 15, 2), (32, 12, 1, 10, 2), (64, 12, 2, 15, 2)]


def realistic_check(p, bits, log_n, k, lb, ell, key_fn):
    n = 1 << log_n
    b, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    L = b.decompose_length()
    rng = np.random.default_rng(log_n * 7 + lb + bits)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheFftContext(fft, b, k)
    g = rand_words(rng, bits, (k + 1) * L * (k + 1) * n)
    key = key_fn(rng, m.FullComplex64FftTable(log_n).forward(g.reshape(-1, n), bits)).reshape(-1)
    batch = 2
    inp = rand_words(rng, bits, batch * (k + 1) * n)
    out = run_product(p, ctx, inp, key, bits)
    W = (k + 1) * n
    for e in range(batch):
        exact = m.schoolbook(inp[e * W:(e + 1) * W], g, mb, log_n, k)
        model, _ = m.external_product(inp[e * W:(e + 1) * W], key, mb, log_n, k)
        model_err = m.centred_error(model, exact, bits).max()
        gpu_err = m.centred_error(out[e * W:(e + 1) * W], exact, bits).max()
        assert gpu_err <= 4 * model_err + 2, (e, gpu_err, model_err)


@pytest.mark.parametrize("bits,log_n,k,lb,ell", REALISTIC)
def test_product_realistic_regime(p, bits, log_n, k, lb, ell):
    realistic_check(p, bits, log_n, k, lb, ell, lambda rng, key: key)


@pytest.mark.parametrize("bits,log_n,k,lb,ell", [(32, 10, 1, 7, 3), (64, 12, 1, 15, 2)])
def test_non_hermitian_key(p, bits, log_n, k, lb, ell):
    """K + A with A[(1-j) mod N] = -conj(A[j]) has the Hermitian part of K: the product must not see A"""
    def perturb(rng, key):
        n = key.shape[-1]
        j = np.arange(n)
        a = (rng.normal(size=key.shape) + 1j * rng.normal(size=key.shape)) * np.abs(key).max()
        a = (a - np.conj(a[..., (1 - j) % n])) / 2
        return key + a
    realistic_check(p, bits, log_n, k, lb, ell, perturb)


@pytest.mark.parametrize("bits,log_n,k", [(32, 10, 1), (64, 11, 1), (32, 12, 1), (64, 10, 2)])
def test_batching_and_determinism(p, bits, log_n, k):
    n = 1 << log_n
    rng = np.random.default_rng(11)
    fft = p.FullComplex64FftTable(log_n)
    b = p.ApproxSignedBasis(bits, 7 if bits == 32 else 15, 3 if bits == 32 else 2)
    ctx = p.TfheFftContext(fft, b, k, chunk=4)
    key = m.FullComplex64FftTable(log_n).forward(
        rand_words(rng, bits, (k + 1) * b.decompose_length() * (k + 1) * n).reshape(-1, n), bits).reshape(-1)
    W = (k + 1) * n
    inp = rand_words(rng, bits, 9 * W)
    singles = np.concatenate([run_product(p, ctx, inp[e * W:(e + 1) * W], key, bits) for e in range(9)])
    for batch in (1, 7, 9):
        assert np.array_equal(run_product(p, ctx, inp[:batch * W], key, bits), singles[:batch * W]), batch
    big = p.TfheFftContext(fft, b, k)   # default chunk
    assert np.array_equal(run_product(p, big, inp, key, bits), singles)
    assert np.array_equal(run_product(p, big, inp, key, bits), singles)


@pytest.mark.parametrize("log_n", [10, 12])
def test_graph_capture_replays_the_eager_product(p, log_n):
    import torch
    n = 1 << log_n
    rng = np.random.default_rng(12)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheFftContext(fft, p.ApproxSignedBasis(32, 10, 2), 1)
    key = dev_complex(m.FullComplex64FftTable(log_n).forward(rand_words(rng, 32, 8 * n).reshape(-1, n), 32).reshape(-1))
    x = dev_words(rand_words(rng, 32, 16 * n), 32)
    eager = torch.empty_like(x)
    p.tfhe_external_product_to_dev(x, key, eager, ctx)
    torch.cuda.synchronize()
    out = torch.zeros_like(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.tfhe_external_product_to_dev(x, key, out, ctx)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_second_thread_gets_busy(p):
    n = 1 << 13
    rng = np.random.default_rng(13)
    fft = p.FullComplex64FftTable(13)
    b = p.ApproxSignedBasis(64, 15, 2)
    ctx = p.TfheFftContext(fft, b, 1)
    key = np.zeros(8 * n, np.complex128)
    inp = rand_words(rng, 64, 512 * 2 * n)
    out = np.empty_like(inp)
    seen = {}

    def worker():
        p.tfhe_external_product_to(inp, key, out, ctx)

    t = threading.Thread(target=worker)
    t.start()
    small_in, small_out = np.zeros(2 * n, np.uint64), np.zeros(2 * n, np.uint64)
    while t.is_alive() and "kind" not in seen:
        if ctx.in_use():
            try:
                p.tfhe_external_product_to(small_in, key, small_out, ctx)
                seen["kind"] = "ok"
            except p.PfheError as e:
                seen["kind"] = e.kind
    t.join()
    assert seen.get("kind") == "Busy", seen
    assert not ctx.in_use() and not out.any()


def test_device_argument_errors(p):
    import torch
    fft = p.FullComplex64FftTable(10)
    ctx = p.TfheFftContext(fft, p.ApproxSignedBasis(32, 10, 2), 1)
    x = torch.zeros(2048 + 4, dtype=torch.int32, device="cuda")
    key = torch.zeros(8 * 1024, dtype=torch.complex128, device="cuda")
    with pytest.raises(p.PfheError) as e:
        p.tfhe_external_product_to_dev(x, key, x, ctx)          # not a whole number of ciphertexts
    assert e.value.kind == "BadLength"
    with pytest.raises(p.PfheError) as e:
        p.tfhe_external_product_to_dev(x[:2048], key[:100], x[:2048], ctx)   # a key of the wrong size
    assert e.value.kind == "BadLength"
    with pytest.raises(p.PfheError) as e:
        p.tfhe_external_product_to_dev(x[1:2049], key, x[2:2050], ctx)     # misaligned
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        p.TfheFftContext(fft, p.ApproxSignedBasis(32, 10, 2), 65)
    assert e.value.kind == "Unsupported"
    out = torch.empty(1000, dtype=torch.complex128, device="cuda")
    with pytest.raises(p.PfheError) as e:
        fft.forward_torus_dev(x[:1000], out)
    assert e.value.kind == "BadLength"
