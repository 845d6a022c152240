"""GPU parity of the CMUX, the CMUX tree and the look-up handle (csrc/pfhe_cmux.hip, csrc/pfhe_lut.hip) against the integer
models (tests/tfhe_cmux_model.py, tests/tfhe_lut_model.py) where tests/test_gpu_tfhe_cmux.py and tests/test_gpu_tfhe_lut.py
compare with compositions of other device calls only, and the paths of the look-up handle that no test took:

  A. the exact regime (key or selector words in [-2^10, 2^10], (k+1) ell N 2^(logB-1) 2^10 <= 2^40, asserted before the
     device is called: the f64 product is the integer schoolbook), every comparison array_equal:
       - tfhe_cmux_dev at the general shapes (32, log N 4, k 2), (64, 3, 3) and (32, 12, 1): the chain of gather, digit,
         multiply-accumulate, inverse and glue launches, d1 - d0 walking every edge word of the digit rule;
       - tfhe_cmux_tree_dev at the two small general shapes, depth 2 and 3, a shared table (the first level's periodic
         gather) and a table per input, batch 3 on a handle of chunk 2 (a partial last chunk) and on a default one;
       - tfhe_rotate_by_bits_dev against lm.rotate_by_bits at the two general shapes (tfhe_bitrot_monomial_kernel, then the
         CMUX's general form in place, per step) and at the fused shapes (32, 5, 1) and (64, 9, 1)
         (tfhe_bitrot_loop_kernel): every r up to min(3, log N - s), s 0 and 1, o 1 and 3, r + 2 keys per input read from
         key 1 on, chunk 1 (with o = 3 a launch is one input's outputs), chunk 2 (a launch that starts at a later input),
         the default, and out == inp;
       - tfhe_lut_eval_dev against lm.lut_eval at the same four shapes: (t, r) = (0, 2) (no tree: a shared table is
         gathered by its period inside the rotation), (2, 0) (no rotation: the tree's last level writes the result),
         (1, 1), (3, 2); s = 1; o 1, 2 and 3; a shared table and a table per input; extract 0 (the result goes to the
         output) and 2 (it goes to the owned buffer, and launch_multi_extract reads it); batch 3 under chunk 2 and the
         default.
  B. what a table of tfhe_lut_table means with o = 3 outputs, two-word entries and log_stride 1, for all 2^4 patterns as
     one batch, extract 2: u32 exactly (trivial GGSWs in the basis (8, 4), which drops no bit), fused and general, a
     shared table and a table per input whose entries differ from input to input; u64 within the derived bound (noise-free
     leaves under a binary key, trivial GGSWs in the basis (4, 3), o = 2, (t, r) = (2, 1)).
  C. rot_bits = 0: rotate_accs is an asynchronous device-to-device copy per launch, skipped when out is inp; (t, r) =
     (1, 0), o = 2, batch 5 under chunk 2 (three copies, the last of one input) and the default, first_key 0 and 1.
  D. graph capture of the multi-launch general forms (k = 2), two chunks in the graph, replayed on two different inputs:
     tfhe_lut_eval_dev, tfhe_cmux_tree_dev, tfhe_extract_bits_dev with 3 bits (two per-step rotations) and
     tfhe_circuit_bootstrap_dev.  The trace's capture is in tests/test_gpu_tfhe_trace_edges.py.
  E. one look-up handle used from one stream after another (one_stream_after_another of
     tests/test_gpu_tfhe_cbs_edges.py): fused, where the calls share the owned accumulators and the tree's node buffers,
     and general, where the short call is tfhe_rotate_by_bits_dev, which writes the rotated accumulators, D and E that the
     long call's levels and steps use.

All 132 tests pass on an MI355X; no defect was found in csrc/.  The u64 case of B printed an error of 2^55.3 against an
allowance of 2^58.6 (model_err 3072; Delta/2 = 2^61).

What the file was seen to catch on an MI355X, each change built into a copy of the library (values only: no address leaves
its buffer, no length or launch bound changes):
  1. BitRot::key taking the launch's own index, b / per_input, instead of (first_acc + b) / per_input (the fused kernel
     reads the keys of input 0, 1, .. in every launch): all 8 fused rotation cases fail, at the accumulators of inputs 1 and
     2 under chunk 1; so do the 36 fused table cases with r >= 1 ((2, 0) passes) and both fused cases of B.
  2. the general form's step j reading key r - 1 - j of its input: all 8 general rotation cases fail at r = 2 (r = 1 reads the
     same key), the 24 general table cases with r = 2, and both general cases of B.
  3. rotate_accs without its copy at r = 0: both cases of C fail.  tests/test_gpu_tfhe_lut.py fails too, at its ten (2, 0)
     cases: its composition calls tfhe_rotate_by_bits_dev on the r = 0 handle, so there the change breaks the side that is
     compared with, and nothing pins the copy's words but C.
  Changes 1 to 3 were one build: 82 of 132 fail, and the CMUX, tree and graph cases, which they do not touch, pass.
  tests/test_gpu_tfhe_lut.py sees 1 and 2 as well (30 of 42 fail).
  4. ordered_on without its hipStreamWaitEvent: both stream cases fail, in 3 runs of 3, in round 0 or 1, at ciphertexts of a
     long call or at the short call's.  This is a race: a failure under the change was seen, not proven to be certain.
Wall time on an MI355X: 9.0 s for the 132 tests of this file, 1.4 s of it the first import; the slowest case 0.54 s (the
table at u64, N = 2^9, (t, r) = (3, 2), o = 3: the integer model), the N = 2^12 CMUX 0.23 s, every other below 0.4 s.
"""
import itertools

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cmux_model as xm
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_lut_model as lm
from test_gpu_tfhe_bitext import random_case as bitext_case
from test_gpu_tfhe_bootstrap_edges import assert_same_rows
from test_gpu_tfhe_cbs import product_model_error
from test_gpu_tfhe_cbs import random_case as cbs_case
from test_gpu_tfhe_cbs_edges import LONG_BATCH, SHORT_BATCH, STREAM_CHUNK, one_stream_after_another
from test_gpu_tfhe_cmux import cmux_run, empty_words, fourier_keys, table, tree_run
from test_gpu_tfhe_edges import bases, fused_shape
from test_gpu_tfhe_fft import dev_words, host_words, rand_words
from test_gpu_tfhe_lut import eval_run, rotate_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


GMAX = 1024
BASES = {32: (7, 3), 64: (15, 2)}
GENERAL = [(32, 4, 2), (64, 3, 3)]              # bits, log_n, k: the chain of launches
FUSED = [(32, 5, 1), (64, 9, 1)]                # the loop kernels
shape_ids = lambda cases: ["u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]) for c in cases]


def exact_case(p, bits, log_n, k):
    """the handles' basis, the model's, the schoolbook product and the words of one key; refuses a shape outside the exact
    regime before anything reaches the device"""
    lb, ell = BASES[bits]
    b, mb = bases(p, bits, lb, ell, log_n, k, GMAX)
    assert (k + 1) * mb.decompose_length * (1 << log_n) * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    return b, mb, memo(xm.exact_product(mb, log_n, k)), (k + 1) * mb.decompose_length * ((k + 1) << log_n)


def memo(product):
    """the same product of the same words is computed once: the model runs again for another `extract`"""
    seen = {}

    def cached(diff, key):
        at = (np.asarray(diff).tobytes(), np.asarray(key).tobytes())
        if at not in seen:
            seen[at] = product(diff, key)
        return seen[at]
    return cached


def small_words(rng, bits, size):
    return rng.integers(-GMAX, GMAX + 1, size).astype(m.UINT[bits])


# ---------------- A. the general forms against the integer model ----------------

@pytest.mark.parametrize("bits,log_n,k", GENERAL + [(32, 12, 1)], ids=shape_ids(GENERAL + [(32, 12, 1)]))
def test_general_cmux_equals_the_integer_schoolbook_over_the_edge_words(p, bits, log_n, k):
    """d1 = d0 + w with w every edge word of the basis, a key per ciphertext; a default handle (one launch sequence) and one
    of chunk 1.  At N = 2^12 two ciphertexts hold every edge word, and the host model takes most of the time"""
    b, mb, product, key_words = exact_case(p, bits, log_n, k)
    assert not fused_shape(log_n, k)
    rng = np.random.default_rng(7100 + bits + log_n + k)
    glwe = (k + 1) << log_n
    edges = ew.edge_words(bits, *BASES[bits])
    count = max(2, -(-edges.size // glwe))
    diff = rng.permutation(np.resize(edges, count * glwe)).astype(m.UINT[bits])
    assert count * glwe >= edges.size and set(edges.tolist()) <= set(diff.tolist())
    d0 = rand_words(rng, bits, count * glwe)
    with np.errstate(over="ignore"):
        d1 = (d0 + diff).astype(m.UINT[bits])
    keys = small_words(rng, bits, count * key_words)
    want = xm.cmux(d0, d1, keys, 1, product, bits, log_n, k)
    fft = table(p, log_n)
    fkeys = fourier_keys(p, fft, dev_words(keys, bits))
    for depth, chunk in ((2, 0), (1, 1)):
        ctx = p.TfheCmuxTreeContext(fft, b, k, depth, chunk=chunk)
        assert ctx.scratch_bytes() > 0 and ctx.key_len() == key_words
        got = cmux_run(p, ctx, dev_words(d0, bits), dev_words(d1, bits), fkeys, 1, bits)
        assert_same_rows(host_words(got, bits), want, glwe, f"chunk {chunk}")
        assert np.array_equal(host_words(got, bits), want)


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("bits,log_n,k", GENERAL, ids=shape_ids(GENERAL))
def test_general_tree_equals_the_integer_model(p, bits, log_n, k, depth):
    b, mb, product, key_words = exact_case(p, bits, log_n, k)
    batch = 3
    rng = np.random.default_rng(7200 + bits + log_n + depth)
    glwe = (k + 1) << log_n
    selectors = small_words(rng, bits, batch * depth * key_words)
    own = rand_words(rng, bits, batch * (glwe << depth))
    fft = table(p, log_n)
    fsel = fourier_keys(p, fft, dev_words(selectors, bits))
    handles = [p.TfheCmuxTreeContext(fft, b, k, depth, chunk=c) for c in (2, 0)]
    for what, tbl in (("a table per input", own), ("a shared table", own[:glwe << depth].copy())):
        want = xm.tree(tbl, selectors, depth, batch, product, bits, log_n, k)
        for ctx in handles:
            got = host_words(tree_run(p, ctx, dev_words(tbl, bits), fsel, batch, bits), bits)
            assert_same_rows(got, want, glwe, f"{what}, scratch {ctx.scratch_bytes()}")
            assert np.array_equal(got, want)


@pytest.mark.parametrize("o", [1, 3])
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("bits,log_n,k", GENERAL + FUSED, ids=shape_ids(GENERAL + FUSED))
def test_rotation_by_bits_equals_the_integer_model(p, bits, log_n, k, s, o):
    """One set of batch x (r_max + 2) keys; the handle of r bits gets the first r + 2 keys of every input and reads from key 1
    on, so its result is the model's accumulator after r of the r_max steps"""
    import torch
    b, mb, product, key_words = exact_case(p, bits, log_n, k)
    batch, first, r_max = 3, 1, min(3, log_n - s)
    rng = np.random.default_rng(7300 + bits + log_n + 10 * s + o)
    glwe = (k + 1) << log_n
    inp = rand_words(rng, bits, batch * o * glwe)
    master = small_words(rng, bits, batch * (r_max + 2) * key_words)
    after = {j + 1: out for j, _acc, _rot, _keys, out in
             lm.rotation_steps(inp, master, r_max, s, o, r_max + 2, first, product, bits, log_n, k)}
    fft = table(p, log_n)
    fmaster = fourier_keys(p, fft, dev_words(master, bits)).view(batch, r_max + 2, key_words)
    d_inp = dev_words(inp, bits)
    for r in range(1, r_max + 1):
        kpi = r + 2
        keys = fmaster[:, :kpi].contiguous().view(-1)
        want = lm.rotate_by_bits(inp, master.reshape(batch, r_max + 2, -1)[:, :kpi], r, s, o, kpi, first, product, bits, log_n, k)
        assert np.array_equal(want, after[r])
        for chunk in (1, 2, 0):
            ctx = p.TfheLutContext(fft, b, k, 0, r, outputs=o, log_stride=s, chunk=chunk)
            got = host_words(rotate_run(p, ctx, d_inp, keys, bits, kpi, first), bits)
            assert_same_rows(got, want, glwe, f"r {r}, chunk {chunk}")
            assert np.array_equal(got, want)
            if chunk == 2:
                acc = d_inp.clone()
                p.tfhe_rotate_by_bits_dev(acc, keys, acc, ctx, kpi, first)          # out is inp
                assert np.array_equal(host_words(acc, bits), want), r
    assert torch.equal(d_inp, dev_words(inp, bits))


LUT_TR = [(0, 2), (2, 0), (1, 1), (3, 2)]


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-input"])
@pytest.mark.parametrize("o", [1, 2, 3])
@pytest.mark.parametrize("t,r", LUT_TR)
@pytest.mark.parametrize("bits,log_n,k", GENERAL + FUSED, ids=shape_ids(GENERAL + FUSED))
def test_table_evaluation_equals_the_integer_model(p, bits, log_n, k, t, r, o, shared):
    b, mb, product, key_words = exact_case(p, bits, log_n, k)
    batch, s = 3, 1
    assert r + s <= log_n
    rng = np.random.default_rng(7400 + bits + log_n + 10 * t + r + o)
    glwe = (k + 1) << log_n
    selectors = small_words(rng, bits, batch * (t + r) * key_words)
    tbl = rand_words(rng, bits, (1 if shared else batch) * (o << t) * glwe)
    fft = table(p, log_n)
    fsel, d_tbl = fourier_keys(p, fft, dev_words(selectors, bits)), dev_words(tbl, bits)
    for extract in (0, 2):
        want = lm.lut_eval(tbl, selectors, t, r, s, o, batch, extract, product, bits, log_n, k)
        for chunk in (2, 0):
            ctx = p.TfheLutContext(fft, b, k, t, r, outputs=o, log_stride=s, chunk=chunk)
            got = host_words(eval_run(p, ctx, d_tbl, fsel, batch, extract, bits), bits)
            assert_same_rows(got, want, (k << log_n) + 1 if extract else glwe, f"extract {extract}, chunk {chunk}")
            assert np.array_equal(got, want)


# ---------------- B. what a table means with several outputs and multi-word entries ----------------

@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-input"])
@pytest.mark.parametrize("log_n,k", [(5, 1), (4, 2)], ids=["fused", "general"])
def test_every_pattern_reads_its_two_word_entry_of_every_output_u32_exactly(p, log_n, k, shared):
    """Trivial GGSWs of the bits in a basis that drops no bit and a trivial table: every product is exact, so row
    (e o + u) 2 + w IS (0, .., 0, values[u, x_e, w]) with x_e = sum_j m_{e,j} 2^j.  With a table per input the entries
    differ from input to input: input e must read its own leaves"""
    import torch
    bits, t, r, s, o, words = 32, 2, 2, 1, 3, 2
    pb, n = t + r, 1 << log_n
    assert fused_shape(log_n, k) == (k == 1)
    rng = np.random.default_rng(7500 + log_n + k)
    mb = m.ApproxSignedBasis(bits, 8, 4)
    assert mb.drop_bits == 0
    fft = table(p, log_n)
    patterns = list(itertools.product((0, 1), repeat=pb))
    batch = len(patterns)
    values = rand_words(rng, bits, (1 if shared else batch) * o * (1 << pb) * words).reshape(-1, o, 1 << pb, words)
    leaves = [p.tfhe_lut_table(dev_words(v, bits), log_n, k, t, r, s) for v in values]
    for v, leaf in zip(values, leaves):
        assert leaf.shape == (o, 1 << t, k + 1, n) and np.array_equal(host_words(leaf, bits), lm.lut_table(v, log_n, k, t, r, s))
    tbl = torch.cat([leaf.reshape(-1) for leaf in leaves])
    msgs = [bit for pat in patterns for bit in pat]
    sel = fourier_keys(p, fft, dev_words(xm.bit_ggsws(msgs, None, mb, log_n, k, rng, trivial=True), bits))
    for chunk in (3, 0):
        ctx = p.TfheLutContext(fft, p.ApproxSignedBasis(bits, 8, 4), k, t, r, outputs=o, log_stride=s, chunk=chunk)
        got = host_words(eval_run(p, ctx, tbl, sel, batch, words, bits), bits).reshape(batch, o, words, k * n + 1)
        for e, pat in enumerate(patterns):
            entry = values[0 if shared else e][:, xm.leaf_index(pat)]              # (o, words)
            assert np.array_equal(got[e, :, :, k * n], entry), (chunk, pat)
        assert not got[..., :k * n].any()


def test_every_pattern_decodes_its_entry_of_every_output_u64(p):
    """u64 gadget words do not fit f64's 53 bits, so the entry is met within the bound, as
    test_every_selector_pattern_picks_its_leaf_u64 does for the tree: o 2^t noise-free GLWE leaves of 1-bit messages under a
    binary key, trivial GGSWs of the bits in the basis (4, 3).  The result (e, u) is X^{-x_lo 2^s} leaf (u, x_hi): every
    coefficient within lut_bound with noise-free rows plus (t + r) (1 + k N) (4 model_err + 2) of it, and it decodes"""
    bits, log_n, k, t, r, s, o, pbits = 64, 6, 1, 2, 1, 1, 2, 1
    pb, n = t + r, 1 << log_n
    rng = np.random.default_rng(7600)
    mb = m.ApproxSignedBasis(bits, 4, 3)
    fft = table(p, log_n)
    z = rng.integers(0, 2, (k, n)).astype(m.UINT[bits])
    tbl, data = xm.message_table(rng, o << t, bits, log_n, k, pbits, z)
    patterns = list(itertools.product((0, 1), repeat=pb))
    batch = len(patterns)
    torus = xm.bit_ggsws([bit for pat in patterns for bit in pat], None, mb, log_n, k, rng, trivial=True)
    ctx = p.TfheLutContext(fft, p.ApproxSignedBasis(bits, 4, 3), k, t, r, outputs=o, log_stride=s)
    model_err = product_model_error(mb, torus[-ctx.key_len():], bits, log_n, k, rng)
    allowed = lm.lut_bound(t, r, bits, log_n, k, 4, 3, 0) + (t + r) * (1 + k * n) * (4 * model_err + 2)
    assert allowed < 2.0 ** (bits - pbits - 2)                       # before the device is called
    got = host_words(eval_run(p, ctx, dev_words(tbl, bits), fourier_keys(p, fft, dev_words(torus, bits)), batch, 0, bits), bits)
    got = got.reshape(batch, o, -1)
    worst = 0.0
    for e, pat in enumerate(patterns):
        x = xm.leaf_index(pat)
        lo, hi = x & ((1 << r) - 1), x >> r
        for u in range(o):
            leaf = data[(u << t) + hi]
            clear = (leaf.astype(np.uint64) << np.uint64(bits - pbits - 1)).astype(m.UINT[bits])
            want = lm.mul_monomial(clear, 2 * n - (lo << s), log_n)
            ph = bs.glwe_phase(got[e, u], z, bits, log_n, k)
            assert bs.decode(ph, pbits, bits) == bs.decode(want, pbits, bits), (pat, u)
            assert bs.decode(ph[:1], pbits, bits) == [int(leaf[lo << s])], (pat, u)
            worst = max(worst, float(m.centred_error(ph, want, bits).max()))
    print("u64 noise-free selectors (t, r) = (%d, %d), o = %d: look-up err 2^%.1f allowed 2^%.1f (model_err %g) Delta/2 2^%d"
          % (t, r, o, np.log2(max(worst, 1)), np.log2(allowed), model_err, bits - pbits - 2))
    assert worst <= allowed, (worst, allowed)


# ---------------- C. rot_bits = 0: the copy ----------------

@pytest.mark.parametrize("bits,log_n,k", [(32, 5, 1), (64, 3, 3)], ids=shape_ids([(32, 5, 1), (64, 3, 3)]))
def test_rotation_by_no_bits_is_a_copy(p, bits, log_n, k):
    import torch
    t, r, o, batch, kpi = 1, 0, 2, 5, 1
    rng = np.random.default_rng(7700 + bits)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, *BASES[bits])
    glwe = (k + 1) << log_n
    inp = rand_words(rng, bits, batch * o * glwe)
    d_inp = dev_words(inp, bits)
    assert np.array_equal(lm.rotate_by_bits(inp, inp[:0], r, 0, o, kpi, 0, None, bits, log_n, k), inp)
    for chunk in (2, 0):
        ctx = p.TfheLutContext(fft, basis, k, t, r, outputs=o, chunk=chunk)
        keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * kpi * ctx.key_len()), bits))
        for first in (0, 1):
            got = rotate_run(p, ctx, d_inp, keys, bits, kpi, first)                  # into an output of all-ones
            assert_same_rows(host_words(got, bits), inp, glwe, f"chunk {chunk}, first_key {first}")
            same = d_inp.clone()
            p.tfhe_rotate_by_bits_dev(same, keys, same, ctx, kpi, first)             # out is inp: nothing to do
            assert torch.equal(same, d_inp)
        assert torch.equal(d_inp, dev_words(inp, bits)) and not ctx.in_use()
    host = np.full(inp.size, 2 ** bits - 1, m.UINT[bits])
    p.tfhe_rotate_by_bits(inp, keys.cpu().numpy(), host, ctx, kpi, 0)
    assert np.array_equal(host, inp)


# ---------------- D. graph capture of the general forms ----------------

def replays_equal_eager(call, inputs, fresh_a, fresh_b, out_size, bits):
    """call(out) queues the handle's call on the current stream, reading `inputs`.  The eager result on each of the two fresh
    inputs first; then a linear capture on a side stream, replayed once on each: every replay equals the eager call"""
    import torch
    eager = []
    for fresh in (fresh_a, fresh_b):
        inputs.copy_(fresh)
        out = empty_words(out_size, bits)
        call(out)
        torch.cuda.synchronize()
        eager.append(out)
    assert not torch.equal(eager[0], eager[1])
    out = torch.zeros_like(eager[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(out)
    torch.cuda.current_stream().wait_stream(s)
    for fresh, want in ((fresh_a, eager[0]), (fresh_b, eager[1])):
        inputs.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_graph_capture_of_the_general_table_evaluation(p):
    """u64, N = 2^4, k = 2, (t, r) = (2, 2), o = 2, extract 1, batch 3 in chunks of 2: per chunk two tree levels, two steps of
    monomial kernel and CMUX, and the extraction, every CMUX a chain of launches"""
    bits, log_n, k, t, r, o, batch = 64, 4, 2, 2, 2, 2, 3
    rng = np.random.default_rng(7800)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, *BASES[bits])
    ctx = p.TfheLutContext(fft, basis, k, t, r, outputs=o, chunk=2)
    sel = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * (t + r) * ctx.key_len()), bits))
    a, b = (dev_words(rand_words(rng, bits, batch * (o << t) * ctx.glwe_len()), bits) for _ in range(2))
    tbl = a.clone()
    replays_equal_eager(lambda out: p.tfhe_lut_eval_dev(tbl, sel, out, ctx, 1), tbl, a, b, batch * o * ((k << log_n) + 1), bits)


def test_graph_capture_of_the_general_tree(p):
    """u64, N = 2^4, k = 2, depth 3, a shared table, batch 3 in chunks of 2"""
    bits, log_n, k, depth, batch = 64, 4, 2, 3, 3
    rng = np.random.default_rng(7801)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, *BASES[bits])
    ctx = p.TfheCmuxTreeContext(fft, basis, k, depth, chunk=2)
    sel = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * depth * ctx.key_len()), bits))
    a, b = (dev_words(rand_words(rng, bits, ctx.glwe_len() << depth), bits) for _ in range(2))
    tbl = a.clone()
    replays_equal_eager(lambda out: p.tfhe_cmux_tree_dev(tbl, sel, out, ctx), tbl, a, b, batch * ctx.glwe_len(), bits)


def test_graph_capture_of_the_general_bit_extraction(p):
    """u32, N = 2^4, k = 2, 3 bits: the per-step rotation runs twice per chunk"""
    bits, log_n, k, n, batch, delta, nbits = 32, 4, 2, 3, 3, 20, 3
    rng = np.random.default_rng(7802)
    fft, basis, ks_basis, bsk, ksk, a = bitext_case(p, rng, bits, log_n, k, n, batch)
    b = dev_words(rand_words(rng, bits, a.numel()), bits)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis, chunk=2)
    lwe = a.clone()
    replays_equal_eager(lambda out: p.tfhe_extract_bits_dev(lwe, bsk, ksk, out, ctx, delta, nbits), lwe, a, b,
                        batch * nbits * (n + 1), bits)


def test_graph_capture_of_the_general_circuit_bootstrap(p):
    """u32, N = 2^5, k = 2, 3 steps of the per-step rotation, batch 3 in chunks of 2"""
    bits, log_n, k, n, batch = 32, 5, 2, 3, 3
    rng = np.random.default_rng(7803)
    fft, basis, cbs_basis, pfks_basis, bsk, pfksk, a = cbs_case(p, rng, bits, log_n, k, n, batch)
    b = dev_words(rand_words(rng, bits, a.numel()), bits)
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, chunk=2)
    lwe = a.clone()
    replays_equal_eager(lambda out: p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx), lwe, a, b,
                        batch * ctx.ggsw_len(), bits)


# ---------------- E. one look-up handle, one stream after another ----------------

@pytest.mark.parametrize("form", ["fused", "general"])
def test_lookup_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p, form):
    """fused: u32, N = 2^8, k = 1, (t, r) = (2, 2), o = 2, extract 1, a table per input, a long call of 96 inputs: the owned
    accumulators (the rotation writes them, the extraction reads them) and both node buffers are shared by all calls.
    general: u64, N = 2^11, k = 2, (t, r) = (2, 1), o = 2, GLWE results; the short call is tfhe_rotate_by_bits_dev on the same
    handle, which writes the rotated accumulators, D and E that the long call's levels and steps use"""
    bits, log_n, k, t, r, o, extract, long_batch = (32, 8, 1, 2, 2, 2, 1, 4 * LONG_BATCH) if form == "fused" else \
        (64, 11, 2, 2, 1, 2, 0, LONG_BATCH)
    rng = np.random.default_rng(7900 + bits)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, *BASES[bits])
    make = lambda: p.TfheLutContext(fft, basis, k, t, r, outputs=o, chunk=STREAM_CHUNK)
    shape = make()
    glwe, key_len = shape.glwe_len(), shape.key_len()
    assert fused_shape(log_n, k) == (form == "fused") and shape.scratch_bytes() > STREAM_CHUNK * o * glwe * bits // 8
    row = (k << log_n) + 1 if extract else glwe

    def evaluation(batch):
        tbl = dev_words(rand_words(rng, bits, batch * (o << t) * glwe), bits)
        sel = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * (t + r) * key_len), bits))
        return (lambda ctx, out, stream: p.tfhe_lut_eval_dev(tbl, sel, out, ctx, extract, stream)), batch * o * row

    def rotation(batch):
        inp = dev_words(rand_words(rng, bits, batch * o * glwe), bits)
        keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * r * key_len), bits))
        return (lambda ctx, out, stream: p.tfhe_rotate_by_bits_dev(inp, keys, out, ctx, None, 0, stream)), batch * o * glwe

    short = evaluation(SHORT_BATCH) if form == "fused" else rotation(SHORT_BATCH)
    one_stream_after_another(make, evaluation(long_batch), short, row, bits)
