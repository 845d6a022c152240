"""GPU parity of the bootstrap's own stages (the key switch of csrc/pfhe_bootstrap.hip; tfhe_modswitch_kernel,
tfhe_acc_init_kernel and tfhe_extract_kernel of csrc/pfhe_tfhe_stages.hip, which every handle around a blind rotation now
shares) where the random data and comfortable shapes of tests/test_gpu_tfhe_bootstrap.py do not reach:

  - the key switch at the shapes of tests/tfhe_ks_shapes.py (groups whose key rows are no multiple of four, every group
    size, a short last group, a mask shorter than a group, 128 / 129 / 256 / 257 columns, 31 / 32 / 33 ciphertexts), on
    random words and on every edge word of the digit rule;
  - the key switch's launch split at more than 65535 tiles of 32 ciphertexts;
  - the handle at N = 2 .. 512 with k up to 3, and at N = 2^12 (the per-step rotation), with inputs whose switched
    exponents sit on the branch points of the accumulator's first rotation (0, 1, N-1, N, N+1, 2N-1, a rounding tie, the
    all-ones word that wraps to 0);
  - one handle used from one stream after another with no event handling by the caller, for the bootstrap handle and the
    blind-rotation handle.

Every comparison is bit for bit.  The key switch and the handle are compared with the integer model
(tests/tfhe_bootstrap_model.py); the handle's cases assert the exact-regime rule of tests/test_gpu_tfhe_edges.py, under
which the rotation is the integer schoolbook.  The stream cases compare with a second handle that ran alone.

What the file was seen to catch on an MI355X, each change built into a copy of the library (none of them moves an access
out of bounds):
  - tfhe_keyswitch_kernel without its remainder loop: all 26 cases of the shape table fail (every entry has a group whose
    key rows are no multiple of four), while all 10 cases of test_key_switch_matches_the_integer_model still pass;
  - launch_keyswitch without the `done` offset on lwe_in: both launch-split cases fail;
  - tfhe_acc_init_kernel with `high = r > n` and the rotation still reduced for r >= n (X^N TV comes out as +TV): all 21
    handle cases fail, each at exactly the ciphertexts with neg_b = N, while every test of test_gpu_tfhe_bootstrap.py
    still passes.  (`high = r > n` ALONE changes nothing: at r = N it gives rot = N, the index (j - N) mod N = j and j < rot
    for every j, which is the same -TV[j] by the other branch; all 21 cases pass with it, as they must.)  The rule is
    MonomialShift's, one copy for this kernel and for tfhe_const_acc_init_kernel (tests/test_gpu_tfhe_cbs_edges.py).
  - ordered_on without its hipStreamWaitEvent: the bootstrap handle's case and the per-step rotation's fail in the first
    round (ciphertexts of the long call that the short one overtook); the whole-loop rotation's case passes, as it shares
    no buffer between calls.  This is a race: a failure under the change was seen, not proven to be certain.
"""
import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
from test_gpu_tfhe_blind_rotate import dev_exps, fourier_keys, per_step_context, whole_loop_shape
from test_gpu_tfhe_bootstrap import BASES, KS_BASIS, empty_words, handle_run
from test_gpu_tfhe_edges import SMALL_SHAPES, bases, device_keys, small_key
from test_gpu_tfhe_fft import dev_complex, dev_words, host_words, rand_words
from tfhe_edge_words import edge_words
from tfhe_ks_shapes import KS_EDGE_SHAPES, KS_TILE_BATCH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def assert_same_rows(got, want, row_len, what):
    """equal word for word; names the first differing (ciphertext, column) and how many ciphertexts differ"""
    got, want = np.asarray(got).reshape(-1, row_len), np.asarray(want).reshape(-1, row_len)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if bad.size:
        e, c = (int(v) for v in bad[0])
        rows = np.unique(bad[:, 0])
        pytest.fail(f"{what}: {rows.size} of {got.shape[0]} ciphertexts differ, first at ciphertext {e} column {c}: "
                    f"got {int(got[e, c]):#x}, want {int(want[e, c]):#x}; ciphertexts {rows[:8].tolist()}")


# ---------------- A / B. the key switch over the shape table ----------------

def ks_case_random(rng, bits, in_dim, out_dim, ell, batch):
    """full-range random mask and key words; the key also holds 0, 1, 2^BITS - 1 and 2^(BITS-1) at random places"""
    lwe = rand_words(rng, bits, batch * (in_dim + 1))
    ksk = rand_words(rng, bits, in_dim * ell * (out_dim + 1))
    special = np.array([0, 1, 2 ** bits - 1, 2 ** (bits - 1)], m.UINT[bits])
    at = rng.permutation(ksk.size)[:special.size]
    assert at.size == special.size
    ksk[at] = special
    return lwe, ksk


def ks_case_edge(rng, bits, in_dim, out_dim, lb, ell):
    """every edge word of the basis, laid out consecutively as mask words (the list repeated to fill the last ciphertext),
    with random b and random key words"""
    edge = edge_words(bits, lb, ell)
    batch = -(-edge.size // in_dim)
    lwe = rand_words(rng, bits, batch * (in_dim + 1)).reshape(batch, in_dim + 1)
    lwe[:, :in_dim] = np.resize(edge, batch * in_dim).reshape(batch, in_dim)
    assert set(lwe[:, :in_dim].reshape(-1).tolist()) == set(edge.tolist())      # nothing left out, nothing else in
    return lwe.reshape(-1), rand_words(rng, bits, in_dim * ell * (out_dim + 1))


def check_keyswitch(p, lwe, ksk, bits, in_dim, out_dim, lb, ell, host):
    basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    assert basis.decompose_length() == mb.decompose_length == ell and basis.drop_bits() == mb.drop_bits
    want = bs.keyswitch(lwe, ksk, in_dim, out_dim, mb)
    out = empty_words(want.size, bits)
    out.fill_(-1)                                         # the output may hold anything
    d_lwe, d_ksk = dev_words(lwe, bits), dev_words(ksk, bits)
    for run in ("first", "repeated"):
        p.lwe_keyswitch_dev(d_lwe, d_ksk, out, in_dim, out_dim, basis)
        assert_same_rows(host_words(out, bits), want, out_dim + 1, run)
    if host:
        host_out = np.full(want.size, 2 ** bits - 1, m.UINT[bits])
        p.lwe_keyswitch(lwe, ksk, host_out, in_dim, out_dim, basis)
        assert_same_rows(host_out, want, out_dim + 1, "host form")


HOST_FORM = {min(KS_EDGE_SHAPES, key=lambda s: s[4]), max(KS_EDGE_SHAPES, key=lambda s: s[4])}
assert len(HOST_FORM) == 2


@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("bits,in_dim,out_dim,lb,ell,batch", KS_EDGE_SHAPES)
def test_key_switch_over_the_shape_table(p, bits, in_dim, out_dim, lb, ell, batch, kind):
    """the device form twice into an output of all-ones; the host form at the smallest and the largest ell"""
    rng = np.random.default_rng(8000 + 100 * bits + 10 * in_dim + lb)
    if kind == "random":
        lwe, ksk = ks_case_random(rng, bits, in_dim, out_dim, ell, batch)
    else:
        lwe, ksk = ks_case_edge(rng, bits, in_dim, out_dim, lb, ell)
    host = kind == "random" and (bits, in_dim, out_dim, lb, ell, batch) in HOST_FORM
    check_keyswitch(p, lwe, ksk, bits, in_dim, out_dim, lb, ell, host)


# ---------------- C. the launch split ----------------

@pytest.mark.parametrize("bits", [32, 64])
def test_key_switch_launch_split(p, bits):
    """one ciphertext more than grid.y holds tiles of: the second launch starts at ciphertext 65535 * 32.  Every b word is
    another (the index times an odd constant, a bijection modulo 2^BITS), so input or output taken from the wrong offset
    cannot give the right words"""
    in_dim, out_dim, batch = 1, 1, 65535 * KS_TILE_BATCH + 1
    lb, ell = KS_BASIS
    rng = np.random.default_rng(8100 + bits)
    basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    lwe = np.empty((batch, 2), m.UINT[bits])
    lwe[:, 0] = rand_words(rng, bits, batch)
    odd = 0x9E3779B97F4A7C15 if bits == 64 else 0x9E3779B1
    with np.errstate(over="ignore"):
        lwe[:, 1] = (np.arange(batch, dtype=np.uint64) * np.uint64(odd) + np.uint64(12345)).astype(m.UINT[bits])
    assert np.unique(lwe[:, 1]).size == batch
    lwe = lwe.reshape(-1)
    ksk = rand_words(rng, bits, in_dim * ell * (out_dim + 1))
    want = bs.keyswitch(lwe, ksk, in_dim, out_dim, mb)
    out = empty_words(want.size, bits)
    out.fill_(-1)
    p.lwe_keyswitch_dev(dev_words(lwe, bits), dev_words(ksk, bits), out, in_dim, out_dim, basis)
    assert_same_rows(host_words(out, bits), want, out_dim + 1, "split launch")


# ---------------- D. the handle at small N and at the init's branch points ----------------

HANDLE_LOG_N = [1, 2, 3, 6, 9]
HANDLE_CASES = [(bits, log_n, k, lb, ell) for bits, k, lb, ell in SMALL_SHAPES for log_n in HANDLE_LOG_N] + [(32, 12, 1, 7, 3)]
LWE_DIM = 4


def crafted_lwe(rng, bits, log_n, n):
    """A batch whose switched exponents sit on the branch points.

    b words m 2^shift with m = (2N - r) mod 2N, shift = BITS - log_n - 1, for r in {0, 1, N-1, N, N+1, 2N-1} (fewer at N = 2,
    where some coincide): sw(b) = m exactly and neg_b = r.  Then one b on a rounding tie (1.5 * 2^shift, which rounds up to
    2) and the all-ones word (it rounds up to 2N and wraps to 0); at N = 2 a random b follows.
    Mask words: v 2^shift for v in {0, N-1, N, 2N-1} and the all-ones word at random places.  Of the other mask words,
    2^11 / N (none at N = 2^12) are full-range random; the rest are random words within half a step of 0 from either side, so that
    they switch to the exponent 0 (from above through the wrap).  A step with exponent 0 rotates by nothing, its product
    is of the zero polynomial and the integer model skips it: the model's time, which is all of this test's time at
    N >= 2^9, stays at a few products, while every ciphertext still goes through every stage on the device.  So at
    N >= 2^9 these cases add little coverage of the rotation itself, which tests/test_gpu_tfhe_edges.py pins; they are
    about the stages around it.
    Returns (lwe words, the r of the crafted b words, index of the tie, index of the all-ones b, the all-ones mask slot)."""
    big_n = 1 << log_n
    two_n, shift, ones = 2 * big_n, bits - log_n - 1, 2 ** bits - 1
    rs = sorted({0, 1, big_n - 1, big_n, big_n + 1, two_n - 1})
    b = [((two_n - r) % two_n) << shift for r in rs] + [(1 << shift) + (1 << (shift - 1)), ones]
    if len(b) % 3 == 0:                       # N = 2: one more ciphertext, so that chunks of 3 end in a partial one
        b.append(int(rng.integers(0, 2 ** bits, dtype=np.uint64)))
    batch = len(b)
    half = 1 << (shift - 1)
    near_zero = rng.integers(0, half, batch * n, dtype=np.uint64)
    from_above = rng.integers(0, 2, batch * n).astype(bool)
    a = np.where(from_above, np.uint64(ones) - near_zero, near_zero)          # all switch to 0; all-ones - x >= 2^BITS - half
    slots = rng.permutation(batch * n)
    crafted = [v << shift for v in (0, big_n - 1, big_n, two_n - 1)] + [ones]
    a[slots[:len(crafted)]] = np.array(crafted, np.uint64)
    free = slots[len(crafted):len(crafted) + (2 ** 11 >> log_n)]
    a[free] = rng.integers(0, 2 ** bits, free.size, dtype=np.uint64)
    lwe = np.concatenate([a.reshape(batch, n), np.array(b, np.uint64)[:, None]], axis=1).astype(m.UINT[bits])
    return lwe.reshape(-1), rs, len(rs), len(rs) + 1, int(slots[len(crafted) - 1])


@pytest.mark.parametrize("bits,log_n,k,lb,ell", HANDLE_CASES)
def test_handle_at_small_n_and_the_branch_points(p, bits, log_n, k, lb, ell):
    """keys |g| <= 2^10 under (k+1) ell N 2^(logB-1) 2^10 <= 2^40: the rotation is the integer schoolbook, every other stage
    is integer arithmetic, and tfhe_bootstrap_model.bootstrap is the reference word for word.  At N < 8 the key switch's
    in_dim = k N is below one group of mask words; at k = 3 extraction and init have three mask rows."""
    n, gmax, big_n = LWE_DIM, 1024, 1 << log_n
    two_n = 2 * big_n
    b, mb = bases(p, bits, lb, ell, log_n, k, gmax)
    assert (k + 1) * mb.decompose_length * big_n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    ks_basis, ks_mb = p.ApproxSignedBasis(bits, *KS_BASIS), m.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(9000 * bits + 100 * k + log_n)
    lwe, rs, tie, wrapped, ones_slot = crafted_lwe(rng, bits, log_n, n)
    batch = lwe.size // (n + 1)
    assert batch > 3 and batch % 3 != 0                      # chunk = 3: several chunks, a partial last one
    # the point of the input, from the model's modulus switch, before the device is called
    exps, neg_b = bs.modulus_switch(lwe, n, bits, log_n)
    assert neg_b[:len(rs)].tolist() == rs and set(rs) == {0, 1, big_n - 1, big_n, big_n + 1, two_n - 1}
    assert bs.sw(int(lwe.reshape(batch, n + 1)[tie, n]) - 1, bits, log_n) == 1 and neg_b[tie] == two_n - 2   # ties go up
    assert int(lwe.reshape(batch, n + 1)[wrapped, n]) == 2 ** bits - 1 and neg_b[wrapped] == 0
    assert {0, big_n - 1, big_n, two_n - 1} <= set(exps.reshape(-1).tolist())
    assert int(lwe.reshape(batch, n + 1)[:, :n].reshape(-1)[ones_slot]) == 2 ** bits - 1 and exps.reshape(-1)[ones_slot] == 0
    assert np.count_nonzero(exps) >= 3

    fft = p.FullComplex64FftTable(log_n)
    glwe = (k + 1) * big_n
    keys = [small_key(rng, bits, log_n, k, mb.decompose_length, gmax) for _ in range(n)]
    tvs = {"shared": rand_words(rng, bits, glwe), "each": rand_words(rng, bits, batch * glwe)}
    ksk = rand_words(rng, bits, k * big_n * KS_BASIS[1] * (n + 1))
    # the reference: bs.bootstrap without and with the key switch (the second is bs.keyswitch on the first, as bs.bootstrap
    # itself computes it; the rotation's model is run once per test vector)
    want = {}
    for name, tv in tvs.items():
        want[name, False] = bs.bootstrap(lwe, keys, tv, None, mb, ks_mb, log_n, k, n)
        want[name, True] = bs.keyswitch(want[name, False], ksk, k * big_n, n, ks_mb)
    assert not np.array_equal(want["shared", True], want["each", True])

    d_lwe, d_ksk = dev_words(lwe, bits), dev_words(ksk, bits)
    d_tvs = {name: dev_words(tv, bits) for name, tv in tvs.items()}
    bsk = None
    for chunk in (3, 0):
        for with_ks in (True, False):
            ctx = p.TfheBootstrapContext(fft, b, n, k, ks_basis if with_ks else None, chunk=chunk)
            assert ctx.out_len() == (n + 1 if with_ks else k * big_n + 1)
            if bsk is None:
                bsk = device_keys(p, fft, ctx, keys, bits)
            for name in tvs:
                got = handle_run(p, ctx, d_lwe, bsk, d_tvs[name], d_ksk if with_ks else None, bits)
                assert_same_rows(host_words(got, bits), want[name, with_ks], ctx.out_len(),
                                 f"chunk {chunk} key switch {with_ks} test vector {name} (neg_b {neg_b.tolist()})")


# ---------------- E. one handle, one stream after another ----------------

STREAM_ROUNDS = 5


def rand_exps(rng, log_n, batch, n):
    return dev_exps(rng.integers(0, 2 << log_n, (batch, n)))


def test_bootstrap_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p):
    """The handle's accumulator, exponents, neg_b and extracted ciphertexts are shared by all its calls.  A long call (24
    ciphertexts in chunks of 2, 32 steps) on one stream, a short one on ANOTHER stream queued right behind it with no event
    handling and no synchronisation by the caller, and the long one again: ordered_on (csrc/pfhe_plan_guard.hpp) makes each
    stream wait for the call before.  All three outputs must be what a second handle gave that ran alone."""
    import torch
    bits, log_n, k, n = 32, 10, 1, 32
    lb, ell = BASES[bits]
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(8200)
    fft = p.FullComplex64FftTable(log_n)
    glwe = (k + 1) << log_n
    bsk = dev_complex(fourier_keys([rand_words(rng, bits, (k + 1) * ell * glwe) for _ in range(n)], log_n, bits))
    ksk = dev_words(rand_words(rng, bits, (k << log_n) * KS_BASIS[1] * (n + 1)), bits)
    long, short = ({"lwe": dev_words(rand_words(rng, bits, batch * (n + 1)), bits),
                    "tv": dev_words(rand_words(rng, bits, batch * glwe), bits)} for batch in (24, 3))
    alone = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, chunk=2)
    want_long = handle_run(p, alone, long["lwe"], bsk, long["tv"], ksk, bits)
    want_short = handle_run(p, alone, short["lwe"], bsk, short["tv"], ksk, bits)
    torch.cuda.synchronize()
    assert not torch.equal(want_long[:want_short.numel()], want_short)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, chunk=2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(STREAM_ROUNDS):
        o1, o2, o3 = torch.zeros_like(want_long), torch.zeros_like(want_short), torch.zeros_like(want_long)
        torch.cuda.synchronize()
        p.tfhe_bootstrap_dev(long["lwe"], bsk, long["tv"], ksk, o1, ctx, stream=s1.cuda_stream)
        p.tfhe_bootstrap_dev(short["lwe"], bsk, short["tv"], ksk, o2, ctx, stream=s2.cuda_stream)   # nothing in between
        p.tfhe_bootstrap_dev(long["lwe"], bsk, long["tv"], ksk, o3, ctx, stream=s1.cuda_stream)     # and back
        s1.synchronize(); s2.synchronize()
        for what, got, want in (("long", o1, want_long), ("short", o2, want_short), ("long again", o3, want_long)):
            assert_same_rows(host_words(got, bits), host_words(want, bits), n + 1, f"round {rnd}, {what}")


@pytest.mark.parametrize("form", ["default", "per_step"])
def test_rotation_handle_used_from_one_stream_after_another_is_ordered_by_the_library(p, form):
    """the same for the blind-rotation handle.  At this shape the default handle is the whole-loop kernel, which owns no
    buffer between its calls (scratch_bytes() == 0): there the case pins only that the calls do not disturb each other; the
    per-step form of the same shape shares its difference, product and ping-pong buffers between calls, and is the one
    the ordering protects."""
    import torch
    bits, log_n, k, n = 32, 10, 1, 32
    lb, ell = BASES[bits]
    basis = p.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(8300)
    fft = p.FullComplex64FftTable(log_n)
    glwe = (k + 1) << log_n
    bsk = dev_complex(fourier_keys([rand_words(rng, bits, (k + 1) * ell * glwe) for _ in range(n)], log_n, bits))
    long, short = ({"acc": dev_words(rand_words(rng, bits, batch * glwe), bits), "exps": rand_exps(rng, log_n, batch, n)}
                   for batch in (24, 3))
    make = (lambda: p.TfheBlindRotateContext(fft, basis, k, chunk=2)) if form == "default" else \
        (lambda: per_step_context(p, fft, basis, k, chunk=2))
    alone, ctx = make(), make()
    assert whole_loop_shape(log_n, k) and (ctx.scratch_bytes() == 0) == (form == "default")
    want_long, want_short = long["acc"].clone(), short["acc"].clone()
    p.tfhe_blind_rotate_dev(want_long, bsk, long["exps"], alone)
    p.tfhe_blind_rotate_dev(want_short, bsk, short["exps"], alone)
    torch.cuda.synchronize()
    assert not torch.equal(want_long, long["acc"]) and not torch.equal(want_short, short["acc"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(STREAM_ROUNDS):
        a1, a2, a3 = long["acc"].clone(), short["acc"].clone(), long["acc"].clone()      # the rotation is in place
        torch.cuda.synchronize()
        p.tfhe_blind_rotate_dev(a1, bsk, long["exps"], ctx, stream=s1.cuda_stream)
        p.tfhe_blind_rotate_dev(a2, bsk, short["exps"], ctx, stream=s2.cuda_stream)      # nothing in between
        p.tfhe_blind_rotate_dev(a3, bsk, long["exps"], ctx, stream=s1.cuda_stream)       # and back
        s1.synchronize(); s2.synchronize()
        for what, got, want in (("long", a1, want_long), ("short", a2, want_short), ("long again", a3, want_long)):
            assert_same_rows(host_words(got, bits), host_words(want, bits), glwe, f"round {rnd}, {what}")
