"""GPU parity of the multi-bit blind rotation (csrc/pfhe_fft_device.hpp: mb_combined_slots, MultiBitKey; csrc/pfhe_fft.hip:
tfhe_mb_blindrot_loop_kernel, tfhe_mb_mulacc_kernel, tfhe_mb_combine_key_kernel, tfhe_mbrot_impl) and of the bootstrap
handle created with a grouping factor, where tests/test_gpu_tfhe_multibit.py does not reach: bit for bit against the integer
model (tests/tfhe_multibit_model.py: exact_group, exact_rotate_loop), on the edge words of the digit rule, at every N from 2
to 512 with k up to 3 and every (k, g), with exponents whose subset sums sit on 0, N, 2N-1 and wrap 2N more than once.

Every comparison is np.array_equal / torch.equal (assert_same_rows names the first differing word).  What makes that
possible is the 2^g rule of tests/tfhe_multibit_cases.py, (k+1) ell N 2^(logB-1) gmax 2^g <= 2^40, asserted by every exact
case before the device is called (`bases` with gmax 2^g); tests/test_tfhe_multibit_model.py shows on the same inputs,
without a GPU, that the f64 model stays exact under it.  Wherever a shape has all three device forms, all three are run and
each is compared with the integer model: the default handle, the handle forced to the per-group form, and the loop composed
from tfhe_multibit_combine_key_dev and tfhe_external_product_to_dev (at k > 1 and N = 2^12 the default IS the per-group
form, and two forms are run).

  a. one group over every edge word of the basis, in both coefficient halves, under the exponent patterns of
     tfhe_multibit_cases.exponent_patterns; two ciphertexts of words that decompose to nothing, whose product is zero;
  b. three groups at log N = 1 .. 9 for each of SMALL_SHAPES, g cycling so that every (k, g) occurs, compared after one,
     two and three groups;
  c. the combined key where its arithmetic is exact: exponents in {0, N, 2N, 3N}, full-torus keys, against numpy's
     Herm(K_0) +- Herm(K_1) +- ... in f64;
  d. the bootstrap handle over the multi-bit rotation at small N, at N = 2^12 and at the accumulator init's branch points,
     against tfhe_bootstrap_model.bootstrap(rotate=exact_rotate_loop), g = 1 through the multi-bit create included;
  e. the rotation handle used from one stream after another, against a second handle that ran alone.

What the file was seen to catch on an MI355X, each change built into a copy of the library (a value or an in-bounds
index; none moves an access out of bounds or removes a barrier), this file and tests/test_gpu_tfhe_multibit.py run
against the copy:
  1. mb_combined_slots negating the root only when n >= 512 (small N loses the sign on idx & n): 64 of the 85 cases here
     fail - all 32 cases of (b) below N = 512, 18 of the 23 handle cases of (d), the 10 rows of (a) below N = 512 and the 4
     cases of (c) at N = 2 and 4; every case at N >= 512 and both stream cases pass, as they must.  Of
     test_gpu_tfhe_multibit.py 36 of 38 pass, test_forms_agree_word_for_word at N = 2 .. 256 among them (the three forms
     are wrong alike); test_multibit_bootstrap_evaluates_the_lut at N = 64 (both widths) does decode wrongly and fails, so
     that file was not blind to this change, only blind below N = 64 and to anything a decoded message absorbs.
  2. tfhe_mb_mulacc_kernel taking the key column min(c, 2): exactly the 18 cases with k = 3 fail (4 of (a), 9 of (b), 5 of
     (d); at k > 1 every handle is the per-group form), the other 67 pass; all 38 tests of test_gpu_tfhe_multibit.py pass.
     With the accumulator compared only after the last of (b)'s three groups the 9 cases of (b) had passed: they are u64,
     and a u64 accumulator is all zero after three groups whatever the keys (tfhe_multibit_cases.largest_gmax).  Hence the
     comparison after every group.
  3. tfhe_mb_blindrot_loop_kernel's sink leaving ACC[c][i] alone when to_torus(lo) is 0 and the group's exponents are all
     0: the 7 rows of (a) that have a whole-loop kernel and a basis that drops bits fail, each at exactly one word-carrying
     ciphertext (the quiet one with the all-zero exponents: got 0x1, want 0x0, in the default form only); the other 78
     cases and all of test_gpu_tfhe_multibit.py pass.  Without the quiet ciphertexts nothing here saw this change: a
     product of edge words under non-zero keys has no zero word to skip.
  4. ordered_on without its hipStreamWaitEvent: the per-group stream case fails in round 0 (5 of the long call's 24
     ciphertexts, those the short call overtook); the default one, every other case here and all of
     test_gpu_tfhe_multibit.py pass.  This is a race, run once: a failure under the change was seen, not proven certain.
Wall time on an MI355X: 10.5 s for the 85 cases, 1.7 s of it the first import; the slowest case 2.1 s (the handle at
N = 2^12: sixteen integer products of N^2 in the model), the next 0.7 s, every case of (a), (b), (c) and (e) below 0.5 s.
"""
import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_multibit_cases as cases
import tfhe_multibit_model as mbm
from test_gpu_tfhe_blind_rotate import dev_exps, whole_loop_shape
from test_gpu_tfhe_bootstrap import KS_BASIS, handle_run
from test_gpu_tfhe_bootstrap_edges import STREAM_ROUNDS, assert_same_rows
from test_gpu_tfhe_edges import bases, device_keys
from test_gpu_tfhe_fft import dev_complex, dev_words, host_words, rand_words
from test_gpu_tfhe_multibit import forced_per_group, full_torus_keys, rotate_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def rotation_handles(p, fft, b, g, k, log_n, **kw):
    """the default handle and, where that is the whole-loop kernel, the per-group form next to it"""
    ctx = p.TfheMultiBitBlindRotateContext(fft, b, g, k, **kw)
    assert (ctx.scratch_bytes() == 0) == whole_loop_shape(log_n, k)
    if not whole_loop_shape(log_n, k):
        return {"default (per-group)": ctx}
    forced = forced_per_group(lambda: p.TfheMultiBitBlindRotateContext(fft, b, g, k, **kw))
    assert forced.scratch_bytes() > 0
    return {"default (whole loop)": ctx, "per-group": forced}


def composed_loop(p, fft, pctx, acc, bsk, exps, bits, k, ell, g):
    """test_gpu_tfhe_multibit's composed_loop (per group and ciphertext tfhe_multibit_combine_key_dev, then
    tfhe_external_product_to_dev in place), each ciphertext in a tensor of its own: the product asks for 16-byte alignment,
    which ciphertext e of a batch does not have at N = 2 with three or four u32 rows"""
    import torch
    a, x = dev_words(acc, bits), dev_exps(exps)
    batch, n_mask = exps.shape
    W, klen = a.numel() // batch, pctx.key_len()
    cts = [a[e * W:(e + 1) * W].clone() for e in range(batch)]
    combined = torch.empty(klen, dtype=torch.complex128, device="cuda")
    for t in range(n_mask // g):
        group = bsk[(t << g) * klen:((t + 1) << g) * klen]
        for e in range(batch):
            p.tfhe_multibit_combine_key_dev(group, x[e, t * g:(t + 1) * g], combined, fft, ell, g, k)
            p.tfhe_external_product_to_dev(cts[e], combined, cts[e], pctx)
    return host_words(torch.cat(cts), bits)


def assert_forms_are_exact(p, fft, b, mb, c, g, k, log_n, bits):
    """every device form of the shape against exact_rotate_loop, ciphertext by ciphertext, after the first group, the first
    two, ... and all of them: a group ASSIGNS its product, so a loop's last accumulator alone can hide what the groups
    before it did (at u64 it is all zero after three groups, tfhe_multibit_cases.largest_gmax).  Returns the last one."""
    W = (k + 1) << log_n
    acc, exps, keys = c["acc"], np.ascontiguousarray(c["exps"]), c["keys"]
    batch, groups = acc.size // W, exps.shape[1] // g
    handles = rotation_handles(p, fft, b, g, k, log_n)
    pctx = p.TfheFftContext(fft, b, k)
    bsk = device_keys(p, fft, pctx, keys, bits)
    want = acc
    for done in range(1, groups + 1):
        # the model goes on from its own result of the groups before; the device runs the loop from the start
        want = np.concatenate([mbm.exact_rotate_loop(want[e * W:(e + 1) * W], keys[(done - 1) << g:done << g],
                                                     exps[e, (done - 1) * g:done * g], g, mb, log_n, k) for e in range(batch)])
        part, part_key = np.ascontiguousarray(exps[:, :done * g]), bsk[:(done << g) * pctx.key_len()]
        for form, h in handles.items():
            assert_same_rows(rotate_dev(p, h, acc, part_key, part, bits), want, W, f"{form}, {done} of {groups} groups")
        got = composed_loop(p, fft, pctx, acc, part_key, part, bits, k, mb.decompose_length, g)
        assert_same_rows(got, want, W, f"composed from the combined key and the product, {done} of {groups} groups")
    return want


# ---------------- a. one group over the edge words ----------------

@pytest.mark.parametrize("bits,log_n,k,lb,ell,g,gmax", cases.EDGE_GROUP)
def test_one_group_over_edge_words(p, bits, log_n, k, lb, ell, g, gmax):
    """The digit code is the classic product's, but its sources here are new: LdsRow (the accumulator read in place from
    LDS) and MultiBitKey in the whole loop, tfhe_mb_mulacc_kernel's per-ciphertext key in the per-group form."""
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax << g)
    c = cases.edge_group_case(bits, log_n, k, lb, ell, g, gmax)
    cases.assert_patterns_reach(c["exps"], 1 << log_n, g)
    want = assert_forms_are_exact(p, p.FullComplex64FftTable(log_n), b, mb, c, g, k, log_n, bits)
    W = (k + 1) << log_n
    for e in c["quiet"]:
        assert not want[e * W:(e + 1) * W].any()


# ---------------- b. every small N ----------------

@pytest.mark.parametrize("bits,log_n,k,lb,ell,g", cases.SMALL_CASES)
def test_rotation_at_every_small_n(p, bits, log_n, k, lb, ell, g):
    """N/2 < 256: most or all threads of a workgroup own no slot, N = 2 has a single half-spectrum slot and the twiddle
    index (r - 4 i r) mod 2N has two bits; the three forms inline the same mb_combined_slots, so only the model can tell
    whether its index, the root's sign or the mirrored key slot is right"""
    c = cases.small_n_case(bits, log_n, k, lb, ell, g)
    b, mb = bases(p, bits, lb, ell, log_n, k, c["gmax"] << g)
    cases.assert_patterns_reach(c["exps"], 1 << log_n, g)
    assert_forms_are_exact(p, p.FullComplex64FftTable(log_n), b, mb, c, g, k, log_n, bits)


# ---------------- c. the combined key where its arithmetic is exact ----------------

@pytest.mark.parametrize("bits,k,ell", [(64, 1, 2), (32, 3, 3)])
@pytest.mark.parametrize("log_n", [1, 2, 9, 11])
def test_combined_key_with_roots_of_plus_and_minus_one(p, bits, k, ell, log_n):
    """Exponents in {0, N, 2N, 3N}: every r_j is 0 or N, the twiddle index (r_j - 4 i r_j) mod 2N is r_j for every slot i,
    and the root is tw[0] = (1, 0) or its negation.  Then mb_combined_slots' two fma pairs add or subtract Herm(K_j)[2i]
    with ONE rounding per component and term (the cross terms are products with a zero), j ascending: the value numpy gives
    for Herm(K_0) +- Herm(K_1) +- ... in f64.  Equal as numbers (a zero's sign is not compared).  Full-torus keys."""
    import torch
    n = 1 << log_n
    assert m.twist(log_n)[0] == 1 + 0j
    fft = p.FullComplex64FftTable(log_n)
    polys = (k + 1) * ell * (k + 1)
    i = np.arange(n // 2)
    even, odd = 2 * i, (n + 1 - 2 * i) % n                       # slot 2i and its mirror (1 - 2i) mod N
    assert sorted(even.tolist() + odd.tolist()) == list(range(n))
    for g in (1, 2, 3, 4):
        rng = np.random.default_rng(14000 + 100 * log_n + 10 * k + g)
        keys = mbm.fourier(full_torus_keys(rng, bits, log_n, k, ell, 1 << g), log_n, bits).reshape(1 << g, polys, n)
        a, c = keys[:, :, even], keys[:, :, odd]
        herm = 0.5 * (a.real + c.real) + 1j * (0.5 * (a.imag - c.imag))
        d_keys = dev_complex(keys.reshape(-1))
        rows = [[0] * g, [n] * g, [2 * n] * g, [3 * n] * g] + [list(r) for r in rng.choice([0, n, 2 * n, 3 * n], (4, g))]
        assert {0, n, 2 * n, 3 * n} <= {int(x) for r in rows for x in r}
        for row in rows:
            r = mbm.subset_sums(row, n)
            assert set(r) <= {0, n}
            kh = herm[0].copy()
            for j in range(1, 1 << g):
                kh = kh - herm[j] if r[j] else kh + herm[j]
            want = np.empty((polys, n), np.complex128)
            want[:, even], want[:, odd] = kh, np.conj(kh)
            out = torch.full((polys * n,), float("nan"), dtype=torch.complex128, device="cuda")
            p.tfhe_multibit_combine_key_dev(d_keys, dev_exps(np.array(row, np.uint32)), out, fft, ell, g, k)
            got = out.cpu().numpy().reshape(polys, n)
            bad = np.argwhere(got != want)
            assert not bad.size, (g, row, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------- d. the bootstrap handle over the multi-bit rotation ----------------

def multibit_bootstrap_context(p, fft, basis, n, k, ks_basis, chunk, g):
    """TfheBootstrapContext(..., grouping_factor=g) takes the classic create at g = 1; this one takes
    pfhe_tfhe{,32}_bootstrap_create_multibit at every g, g = 1 included (a rotation of groups of one element, two keys
    each), through the class's own open call"""
    if g > 1:
        return p.TfheBootstrapContext(fft, basis, n, k, ks_basis, chunk=chunk, grouping_factor=g)
    ctx = object.__new__(p.TfheBootstrapContext)
    args = (n, ks_basis.log_basis() if ks_basis else 0, ks_basis.decompose_length() if ks_basis else 0, 1 if ks_basis else 0)
    ctx._open(fft, basis, k, "bootstrap", args + (g, chunk), ("_create_multibit", "_destroy", "_in_use", "_scratch_bytes"))
    ctx.grouping_factor, ctx.ks_basis, ctx.lwe_dimension, ctx.log_luts = g, ks_basis, n, 0
    return ctx


@pytest.mark.parametrize("bits,log_n,k,lb,ell,g", cases.HANDLE_CASES)
def test_multibit_handle_at_small_n_and_the_branch_points(p, bits, log_n, k, lb, ell, g):
    """test_handle_at_small_n_and_the_branch_points with a grouping factor.  Unlike a classic step, a group whose exponents
    are all 0 still multiplies by the sum of its keys, so the model runs every group of every ciphertext; with one group at
    N = 2^12 that is the time of this test.  Chunk 3 and the default, with and without the key switch, shared and
    per-ciphertext test vectors; where the shape has a whole-loop kernel, a handle forced to the per-group form as well."""
    big_n = 1 << log_n
    c = cases.handle_case(bits, log_n, k, lb, ell, g)
    b, mb = bases(p, bits, lb, ell, log_n, k, c["gmax"] << g)
    n, batch, ks_mb = c["n"], c["batch"], c["ks_mb"]
    assert n % g == 0 and 4 <= n < 4 + g
    _, neg_b = cases.assert_handle_inputs_sit_on_the_branch_points(c, bits, log_n)
    ks_basis = p.ApproxSignedBasis(bits, *KS_BASIS)
    want = {}
    for name, tv in c["tvs"].items():
        want[name, False] = bs.bootstrap(c["lwe"], c["keys"], tv, None, mb, ks_mb, log_n, k, n, rotate=cases.multibit_rotate(g))
        want[name, True] = bs.keyswitch(want[name, False], c["ksk"], k * big_n, n, ks_mb)
    assert not np.array_equal(want["shared", True], want["each", True])

    fft = p.FullComplex64FftTable(log_n)
    d_lwe, d_ksk = dev_words(c["lwe"], bits), dev_words(c["ksk"], bits)
    d_tvs = {name: dev_words(tv, bits) for name, tv in c["tvs"].items()}
    makers = {"default": lambda *a: multibit_bootstrap_context(p, fft, b, n, k, *a, g)}
    if whole_loop_shape(log_n, k):
        makers["per-group"] = lambda *a: forced_per_group(lambda: multibit_bootstrap_context(p, fft, b, n, k, *a, g))
    bsk = None
    for form, make in makers.items():
        for chunk in (3, 0):
            for with_ks in (True, False):
                ctx = make(ks_basis if with_ks else None, chunk)
                assert ctx.out_len() == (n + 1 if with_ks else k * big_n + 1)
                if bsk is None:
                    bsk = device_keys(p, fft, ctx, c["keys"], bits)
                    assert bsk.numel() == ((n // g) << g) * ctx.key_len()
                for name in d_tvs:
                    got = handle_run(p, ctx, d_lwe, bsk, d_tvs[name], d_ksk if with_ks else None, bits)
                    assert_same_rows(host_words(got, bits), want[name, with_ks], ctx.out_len(),
                                     f"{form}, chunk {chunk} key switch {with_ks} test vector {name} (neg_b {neg_b.tolist()})")


# ---------------- e. one handle, one stream after another ----------------

@pytest.mark.parametrize("form", ["default", "per_group"])
def test_multibit_rotation_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p, form):
    """test_rotation_handle_used_from_one_stream_after_another_is_ordered_by_the_library for the multi-bit handle: u32,
    N = 2^10, k = 1, g = 2, 32 mask elements (16 groups), full-torus keys.  A long call (24 ciphertexts in chunks of 2) on one
    stream, a short one (3) on ANOTHER stream queued right behind it with no events and no synchronisation by the caller,
    and the long one again; every round on a fresh pair of streams (one reused pair can be served from one hardware queue,
    which orders the two by itself).  All three results must be what a second handle gave that ran alone.
    The per-group form shares its digit spectra, accumulators and the Hermitian parts of the group's keys (spec, acc, keyh)
    between calls: it is the one that ordered_on protects.  The default form at this shape is the whole-loop kernel, which
    owns no buffer between its calls (scratch_bytes() == 0): its case pins only that the calls do not disturb each other."""
    import torch
    bits, log_n, k, g, n_mask, lb, ell = 32, 10, 1, 2, 32, 7, 3
    basis = p.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(15000)
    fft = p.FullComplex64FftTable(log_n)
    glwe = (k + 1) << log_n
    bsk = dev_complex(mbm.fourier(full_torus_keys(rng, bits, log_n, k, ell, (n_mask // g) << g), log_n, bits))
    long, short = ({"acc": dev_words(rand_words(rng, bits, batch * glwe), bits),
                    "exps": dev_exps(rng.integers(0, 2 << log_n, (batch, n_mask)))} for batch in (24, 3))
    new = lambda: p.TfheMultiBitBlindRotateContext(fft, basis, g, k, chunk=2)
    make = new if form == "default" else (lambda: forced_per_group(new))
    alone, ctx = make(), make()
    assert whole_loop_shape(log_n, k) and (ctx.scratch_bytes() == 0) == (form == "default")
    want_long, want_short = long["acc"].clone(), short["acc"].clone()
    p.tfhe_multibit_blind_rotate_dev(want_long, bsk, long["exps"], alone)
    p.tfhe_multibit_blind_rotate_dev(want_short, bsk, short["exps"], alone)
    torch.cuda.synchronize()
    assert not torch.equal(want_long, long["acc"]) and not torch.equal(want_short, short["acc"])
    for rnd in range(STREAM_ROUNDS):
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a1, a2, a3 = long["acc"].clone(), short["acc"].clone(), long["acc"].clone()      # the rotation is in place
        torch.cuda.synchronize()
        p.tfhe_multibit_blind_rotate_dev(a1, bsk, long["exps"], ctx, stream=s1.cuda_stream)
        p.tfhe_multibit_blind_rotate_dev(a2, bsk, short["exps"], ctx, stream=s2.cuda_stream)      # nothing in between
        p.tfhe_multibit_blind_rotate_dev(a3, bsk, long["exps"], ctx, stream=s1.cuda_stream)       # and back
        s1.synchronize(); s2.synchronize()
        for what, got, ref in (("long", a1, want_long), ("short", a2, want_short), ("long again", a3, want_long)):
            assert_same_rows(host_words(got, bits), host_words(ref, bits), glwe, f"round {rnd}, {what}")
    assert not ctx.in_use()
