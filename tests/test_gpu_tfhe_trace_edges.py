"""GPU parity of the GLWE automorphism, the trace and their key generation (csrc/pfhe_trace.hip) against the integer model
(tests/tfhe_trace_model.py) where tests/test_gpu_tfhe_trace.py stops: there the exact regime runs at k = 1 only (the fused
kernel), the general form is compared with compositions of other device calls, and sigma_t is only ever asked for
t in {1, 3, N + 1, 2N - 1} and the trace's 2^j + 1.

  - rule 1 against tm.automorphism for EVERY odd t in 1..2N-1, so odd_inverse and sigma_word see every exponent and every
    inverse: the general form (gather, digit, multiply-accumulate, inverse and glue launches) at (32, log N 3, k 2) and
    (64, 4, 3), the fused kernel at (32, 4, 1) and (64, 5, 1); t = 5 and 2N - 3 at (32, 12, 1), the general form above the
    fused N.  The inputs hold every edge word of the digit rule, which sigma_t permutes and negates; a handle of chunk 1
    (a launch per ciphertext) and a default one;
  - the trace against tm.trace at the two small general shapes: one step and all log N, chunk 1 and the default,
    out == inp;
  - tfhe_generate_gksk_dev against tm.gksk for the full list of odd exponents at N = 8, k = 2 and 3, and its Fourier key
    bit for bit against write_fourier_form of the torus key;
  - graph capture of the general trace, u32, N = 2^5, k = 2, all steps, two chunks, replayed on two different inputs.

Every comparison is array_equal, under the exact-regime rule of tests/test_gpu_tfhe_edges.py (key words in [-2^10, 2^10],
(k+1) ell N 2^(logB-1) 2^10 <= 2^40), asserted before the device is called.

All 10 tests pass on an MI355X; no defect was found in csrc/.

What the file was seen to catch, and not to catch, on an MI355X: odd_inverse with one Newton step instead of four, built
into a copy of the library (a value only: the result stays odd and masked, so sigma_t stays a permutation of the N words).
One step leaves t^-1 right modulo 2^6, which is all that N <= 32 asks for: the nine small cases pass, and only the
N = 2^12 case fails.  The cases at every odd t pin the gather rule and the use of the inverse at every exponent; how many
bits of the inverse are right is pinned at N = 2^12 only, for t = 5 and 2N - 3 (tests/test_gpu_tfhe_trace.py sees the same
change at N >= 2^9).
Wall time on an MI355X: 3.0 s for the 10 tests of this file, 1.4 s of it the first import; the slowest case 0.45 s (N = 2^12:
the integer model), every other below 0.3 s.
"""
import numpy as np
import pytest

import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_trace_model as tm
from test_gpu_tfhe_bootstrap_edges import assert_same_rows
from test_gpu_tfhe_edges import bases, fused_shape
from test_gpu_tfhe_fft import dev_words, host_words, rand_words
from test_gpu_tfhe_lut_edges import BASES, GMAX, replays_equal_eager, shape_ids, small_words
from test_gpu_tfhe_trace import auto_run, fourier_keys, table, trace_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


GENERAL = [(32, 3, 2), (64, 4, 3)]              # bits, log_n, k
FUSED = [(32, 4, 1), (64, 5, 1)]


def exact_case(p, bits, log_n, k):
    """the handles' basis, the model's and the schoolbook product; refuses a shape outside the exact regime"""
    lb, ell = BASES[bits]
    b, mb = bases(p, bits, lb, ell, log_n, k, GMAX)
    assert (k + 1) * mb.decompose_length * (1 << log_n) * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    return b, mb, tm.exact_product(mb, log_n, k)


def edge_inputs(rng, bits, glwe, least):
    """at least `least` ciphertexts that hold every edge word of the width's basis somewhere"""
    edges = ew.edge_words(bits, *BASES[bits])
    count = max(least, -(-edges.size // glwe))
    inp = rng.permutation(np.resize(edges, count * glwe)).astype(m.UINT[bits])
    assert set(edges.tolist()) <= set(inp.tolist())
    return inp


def automorphisms_equal_the_model(p, bits, log_n, k, exponents):
    b, mb, product = exact_case(p, bits, log_n, k)
    rng = np.random.default_rng(8100 + bits + log_n + k)
    glwe = (k + 1) << log_n
    inp = edge_inputs(rng, bits, glwe, 2)
    key = small_words(rng, bits, tm.key_len(mb, log_n, k))
    fft = table(p, log_n)
    handles = [p.TfheGlweTraceContext(fft, b, k, chunk=c) for c in (1, 0)]
    assert all((ctx.scratch_bytes() == 0) == fused_shape(log_n, k) and ctx.key_len() == key.size for ctx in handles)
    d_inp, fkey = dev_words(inp, bits), fourier_keys(p, fft, dev_words(key, bits))
    for t in exponents:
        want = tm.automorphism(inp, key, t, product, mb, log_n, k)
        for ctx in handles:
            got = host_words(auto_run(p, ctx, d_inp, fkey, t, bits), bits)
            assert_same_rows(got, want, glwe, f"t {t}, t^-1 {pow(t, -1, 2 << log_n)}, scratch {ctx.scratch_bytes()}")
            assert np.array_equal(got, want)


@pytest.mark.parametrize("bits,log_n,k", GENERAL + FUSED, ids=shape_ids(GENERAL + FUSED))
def test_automorphism_equals_the_integer_model_at_every_odd_exponent(p, bits, log_n, k):
    automorphisms_equal_the_model(p, bits, log_n, k, range(1, 2 << log_n, 2))


def test_automorphism_equals_the_integer_model_above_the_fused_n(p):
    """u32, N = 2^12, k = 1: two ciphertexts hold every edge word; the host model takes most of the time"""
    automorphisms_equal_the_model(p, 32, 12, 1, (5, (2 << 12) - 3))


@pytest.mark.parametrize("bits,log_n,k", GENERAL, ids=shape_ids(GENERAL))
def test_general_trace_equals_the_integer_model(p, bits, log_n, k):
    import torch
    b, mb, product = exact_case(p, bits, log_n, k)
    batch = 3
    rng = np.random.default_rng(8200 + bits + log_n + k)
    glwe = (k + 1) << log_n
    inp = np.concatenate([edge_inputs(rng, bits, glwe, 1)[:glwe], rand_words(rng, bits, (batch - 1) * glwe)])
    keys = small_words(rng, bits, log_n * tm.key_len(mb, log_n, k))
    fft = table(p, log_n)
    one, wide = (p.TfheGlweTraceContext(fft, b, k, chunk=c) for c in (1, 0))
    assert one.scratch_bytes() > 0
    d_inp, fkeys = dev_words(inp, bits), fourier_keys(p, fft, dev_words(keys, bits))
    for steps in (1, log_n):
        ks, fks = keys[:steps * one.key_len()], fkeys[:steps * one.key_len()]
        want = tm.trace(inp, ks, steps, product, mb, log_n, k)
        for ctx in (one, wide):
            got = host_words(trace_run(p, ctx, d_inp, fks, steps, bits), bits)
            assert_same_rows(got, want, glwe, f"{steps} steps, scratch {ctx.scratch_bytes()}")
            assert np.array_equal(got, want)
        same = d_inp.clone()
        p.glwe_trace_dev(same, fks, same, one, steps)                                    # out is inp
        assert np.array_equal(host_words(same, bits), want), steps
    assert torch.equal(d_inp, dev_words(inp, bits))


@pytest.mark.parametrize("bits,log_n,k", [(32, 3, 2), (64, 3, 3)], ids=shape_ids([(32, 3, 2), (64, 3, 3)]))
def test_keys_of_every_odd_exponent_equal_the_model(p, bits, log_n, k):
    """full-range keys and randomness; the keys of all N odd exponents in one call"""
    import torch
    lb, ell = BASES[bits]
    n = 1 << log_n
    assert n == 8
    exps = list(range(1, 2 * n, 2))
    rng = np.random.default_rng(8300 + bits + k)
    fft, basis, mb = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    ctx = p.TfheGlweTraceContext(fft, basis, k)
    z_in, z_out = rand_words(rng, bits, k * n), rand_words(rng, bits, k * n)
    rand = kg.glwe_randomness(rng, bits, log_n, k, len(exps) * k * ell, 5)
    torus = dev_words(rand, bits)
    out = p.tfhe_generate_gksk_dev(dev_words(z_in, bits), dev_words(z_out, bits), fft, basis, torus, exps, k)
    assert out.numel() == len(exps) * ctx.key_len() == torus.numel()
    want = tm.gksk(rand, z_in.reshape(k, n), z_out.reshape(k, n), exps, mb, log_n, k)
    assert_same_rows(host_words(torus, bits), want, ctx.key_len(), f"row x is the key of exponent {exps}[x]")
    assert np.array_equal(host_words(torus, bits), want)
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(fourier_keys(p, fft, torus)))       # bit for bit


def test_graph_capture_of_the_general_trace(p):
    """u32, N = 2^5, k = 2, all five steps, batch 3 in chunks of 2: per chunk and step the gather, the product's chain of
    launches and the glue"""
    bits, log_n, k, batch = 32, 5, 2, 3
    rng = np.random.default_rng(8400)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, *BASES[bits])
    ctx = p.TfheGlweTraceContext(fft, basis, k, chunk=2)
    assert ctx.scratch_bytes() > 0
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, log_n * ctx.key_len()), bits))
    a, b = (dev_words(rand_words(rng, bits, batch * ctx.glwe_len()), bits) for _ in range(2))
    inp = a.clone()
    replays_equal_eager(lambda out: p.glwe_trace_dev(inp, keys, out, ctx), inp, a, b, batch * ctx.glwe_len(), bits)
