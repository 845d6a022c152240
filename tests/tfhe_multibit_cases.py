"""Case tables and inputs of tests/test_gpu_tfhe_multibit_edges.py, in one place: the GPU file runs them on the device and
tests/test_tfhe_multibit_model.py proves, without a GPU, that the reference stays inside the condition under which "bit for
bit" can be asked (the f64 model tfhe_multibit_model.step equals the integer tfhe_multibit_model.exact_group in every word
on these very inputs).  Nothing here needs the library.

The condition.  A group's key is K = sum_j X^{r_j} K_j over 2^g keys; with key words in [-gmax, gmax] the coefficients of K
are bounded by 2^g gmax, and the exact-regime rule of tests/test_gpu_tfhe_edges.py (`bases`) carries over with gmax replaced
by 2^g gmax:
    (k+1) * ell * N * 2^(logB-1) * gmax * 2^g <= 2^40.
"""
import numpy as np

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_multibit_model as mbm
from test_gpu_tfhe_bootstrap import KS_BASIS
from test_gpu_tfhe_bootstrap_edges import crafted_lwe
from test_gpu_tfhe_edges import SMALL_LOG_N, SMALL_SHAPES, shifted_tiling, small_key
from test_gpu_tfhe_fft import rand_words
from tfhe_edge_words import edge_words


def rule_lhs(bits, log_n, k, lb, ell, g, gmax):
    """the left-hand side of the 2^g rule"""
    return (k + 1) * m.ApproxSignedBasis(bits, lb, ell).decompose_length * (1 << log_n) * 2 ** (lb - 1) * gmax * 2 ** g


def largest_gmax(bits, log_n, k, lb, ell, g):
    """The largest power of two that the 2^g rule admits as gmax.  A multi-bit group ASSIGNS the product to the accumulator
    (a classic step adds it to a full-torus accumulator), so under the rule every word that enters the second group is
    below 2^41 in magnitude, whatever entered the first.  At u32 that wraps to a full-torus word once the products reach
    2^32; at u64 with (log B, ell) = (15, 2) only the bits from 34 up are decomposed, so with keys of 2^10 a second group
    at N < 2^8 would multiply digits that are all zero and pin nothing.  Hence the keys of the cases with more than one
    group are as large as the rule lets them be: products of up to 2^40 at every N.  At u64 the second group's digits are
    then at most 2^6 (all zero at N = 512, k = 3, where 2^12 terms of random sign stay near 2^31) and its products are
    below 2^33: a THIRD group there has zero digits and checks only that zero is assigned, and the key switch of (4, 3)
    inside the u64 handle decomposes small words to zero as well.  tests/test_tfhe_multibit_model.py prints which groups
    are entered with a non-zero digit.  The u32 cases run the same templates with full-range words in every group and
    stage: what a u64 case cannot see beyond its first group, the u32 case of the same k and g does."""
    room = 2 ** 40 // rule_lhs(bits, log_n, k, lb, ell, g, 1)
    return 1 << (room.bit_length() - 1)


# ---------------- the exponent patterns ----------------

def exponent_patterns(n: int, g: int) -> np.ndarray:
    """Rows of g exponents (device-form words) whose subset sums sit where the key combination can go wrong:
      0  all 0: every r_j = 0, every root is +1;
      1  N, N, 0, N: r = N (the root's sign alone), and r_3 = 0 from two non-zero exponents;
      2  2N-1, 1, N, 2N-1: r = 2N-1, and r_3 = 0 once more, from a sum of exactly 2N;
      3  all 2N-1: every sum of two or more wraps, three terms pass 4N, four pass 6N;
      4  words of 2N and more, 0xFFFFFFFF among them: the device takes them modulo 2N;
      5  N+1, N-1, 1, N: both neighbours of N, r_3 = 0, r_7 = 1, r_15 = N+1."""
    two_n = 2 * n
    rows = [(0, 0, 0, 0), (n, n, 0, n), (two_n - 1, 1, n, two_n - 1), (two_n - 1,) * 4,
            (0xFFFFFFFF, two_n + 3, 5 * two_n + n, 0xFFFFFFFE), (n + 1, n - 1, 1, n)]
    return np.array([r[:g] for r in rows], np.uint32)


def assert_patterns_reach(exps, n: int, g: int):
    """the point of the patterns, from the model's subset sums: exps is any array of whole groups (a multiple of g words)"""
    two_n = 2 * n
    rows = [[int(x) for x in r] for r in np.asarray(exps).reshape(-1, g)]
    sums = [mbm.subset_sums(r, n) for r in rows]
    assert any(not any(r) and set(s) == {0} for r, s in zip(rows, sums))                    # every r_j = 0, all exponents 0
    assert any(n in s for s in sums) and any(two_n - 1 in s for s in sums)                  # r_j = N, r_j = 2N-1
    assert any(all(x >= two_n for x in r) and 0xFFFFFFFF in r for r in rows)                # device-form words
    if g >= 2:                                                                              # r_j = 0 from non-zero exponents
        assert any(r[:2] == [n, n] and s[3] == 0 for r, s in zip(rows, sums))
        assert any(r[:2] == [two_n - 1, 1] and s[3] == 0 for r, s in zip(rows, sums))
    if g >= 3:                                                                              # wraps 2N more than once
        assert any(sum(x % two_n for x in r[:3]) >= 2 * two_n for r in rows)
    if g >= 4:
        assert any(sum(x % two_n for x in r) >= 3 * two_n for r in rows)


# ---------------- a. one group over the edge words ----------------

EDGE_GROUP = [  # bits, log_n, k, log_basis, ell (None = full), g, gmax: tests/test_gpu_tfhe_edges.py's EDGE_PRODUCT with g
    (32, 10, 1, 7, 3, 2, 1024), (64, 11, 1, 15, 2, 3, 1024), (32, 9, 1, 10, 2, 4, 1024), (64, 5, 1, 23, 1, 1, 1024),
    (64, 6, 1, 23, 1, 2, 64), (32, 5, 1, 16, None, 3, 16), (64, 8, 1, 1, 10, 4, 1024), (64, 10, 1, 7, 3, 1, 1024),
    (64, 2, 2, 21, 3, 2, 64), (32, 6, 2, 7, 3, 1, 1024), (32, 7, 2, 10, 2, 4, 1024),          # k = 2
    (32, 4, 3, 7, 3, 3, 1024), (64, 3, 3, 15, 2, 4, 1024), (64, 9, 3, 15, 2, 1, 64), (32, 8, 3, 7, 3, 2, 1024),   # k = 3
    (32, 12, 1, 10, 2, 2, 64),     # the general form at k = 1
]
# gmax below 1024 is what EDGE_PRODUCT has for the same basis (16 at log B 16 full length, 64 at log B 21 and at the general
# form) or what the issue's CPU check of the reference ran (64 at log B 23 with g = 2 and at u64, N = 512, k = 3): none was
# lowered after a device run.


def quiet_words(words, mb):
    """the edge words every digit of which is 0 (0 itself, words below half a unit of the lowest kept level, and the words
    that round up to 2^BITS): a ciphertext of them has the zero product under any key"""
    digits = np.stack(mb.digits(words))
    return words[~digits.any(axis=0)]


def edge_group_case(bits, log_n, k, lb, ell, g, gmax):
    """ONE group.  Accumulators: every edge word of the basis through shifted_tiling, then the same ciphertexts with the
    halves of every polynomial exchanged (each word in both coefficient halves), ciphertext e with exponent pattern e mod 6;
    then two ciphertexts of quiet words, with the all-zero pattern and with the all-(2N-1) one: their product is zero, and
    a form that did not ASSIGN it would leave the words standing."""
    n = 1 << log_n
    mb = m.ApproxSignedBasis(bits, lb, ell)
    words = edge_words(bits, lb, ell)
    pats = exponent_patterns(n, g)
    W = (k + 1) * n
    batch = max(-(-len(words) // W) + 1, -(-len(pats) // 2))
    tiled = shifted_tiling(words, batch * (k + 1), n)
    acc = np.concatenate([tiled, np.roll(tiled.reshape(-1, n), n // 2, axis=1).reshape(-1)])
    halves = acc.reshape(-1, 2, n // 2)
    assert set(words.tolist()) <= set(halves[:, 0].reshape(-1).tolist())
    assert set(words.tolist()) <= set(halves[:, 1].reshape(-1).tolist())
    exps = pats[np.arange(2 * batch) % len(pats)]
    quiet = np.resize(quiet_words(words, mb), W)
    assert quiet.any() or mb.drop_bits == 0
    acc = np.concatenate([acc, quiet, quiet])
    exps = np.concatenate([exps, pats[[0, 3]]])
    rng = np.random.default_rng(11000 * bits + 100 * log_n + 10 * lb + g)
    keys = [small_key(rng, bits, log_n, k, mb.decompose_length, gmax) for _ in range(1 << g)]
    return dict(mb=mb, acc=acc, exps=exps, keys=keys, quiet=(2 * batch, 2 * batch + 1))


# ---------------- b. every small N ----------------

SMALL_GROUPS, SMALL_BATCH = 3, 5
SMALL_CASES = [(bits, log_n, k, lb, ell, 1 + (log_n - 1 + i) % 4)            # bits, log_n, k, log_basis, ell, g
               for i, (bits, k, lb, ell) in enumerate(SMALL_SHAPES) for log_n in SMALL_LOG_N]
assert {(c[2], c[5]) for c in SMALL_CASES} == {(k, g) for k in (1, 2, 3) for g in (1, 2, 3, 4)}


def small_n_case(bits, log_n, k, lb, ell, g):
    """three groups, batch 5: ciphertext e < 4 takes pattern (3 e + t) mod 6 in group t (every pattern twice, in different
    groups), the last one random exponents below 2N; random accumulators; keys of largest_gmax"""
    n, groups, batch = 1 << log_n, SMALL_GROUPS, SMALL_BATCH
    gmax = largest_gmax(bits, log_n, k, lb, ell, g)
    mb = m.ApproxSignedBasis(bits, lb, ell)
    pats = exponent_patterns(n, g)
    rng = np.random.default_rng(12000 * bits + 100 * k + 10 * log_n + g)
    exps = rng.integers(0, 2 * n, (batch, groups, g)).astype(np.uint32)
    for e in range(batch - 1):
        for t in range(groups):
            exps[e, t] = pats[(3 * e + t) % len(pats)]
    keys = [small_key(rng, bits, log_n, k, ell, gmax) for _ in range(groups << g)]
    acc = rand_words(rng, bits, batch * (k + 1) * n)
    return dict(mb=mb, acc=acc, exps=exps.reshape(batch, groups * g), keys=keys, gmax=gmax)


# ---------------- d. the bootstrap handle over the multi-bit rotation ----------------

HANDLE_LOG_N = [1, 2, 3, 6, 9]
# g cycles through 2, 3, 4 along each shape's log N, from another start per shape: every (k, g) occurs, and the u64 shapes
# take g = 4, ONE group, at N = 512, where a second group would see zero digits only (largest_gmax: products of 2^12 random
# signs stay near 2^31); N = 2^12 takes g = 4 for the model's time (one product of 0.3 s per ciphertext and test vector)
_G_START = (0, 1, 2, 1)
HANDLE_CASES = [(bits, log_n, k, lb, ell, (2, 3, 4)[(j + _G_START[s]) % 3])                 # bits, log_n, k, log_basis, ell, g
                for s, (bits, k, lb, ell) in enumerate(SMALL_SHAPES) for j, log_n in enumerate(HANDLE_LOG_N)] + [
    (32, 12, 1, 7, 3, 4),                                                                   # the per-group form at k = 1
    (32, 2, 1, 7, 3, 1), (32, 6, 2, 7, 3, 1)]     # g = 1 through the multi-bit create (four groups: u32, see largest_gmax)
assert {(c[2], c[5]) for c in HANDLE_CASES} >= {(k, g) for k in (1, 2, 3) for g in (2, 3, 4)}
assert all(c[5] == 4 for c in HANDLE_CASES if c[0] == 64 and c[1] == 9)


def lwe_dimension(g):
    """the smallest multiple of g that is at least 4"""
    return g * -(-4 // g)


def handle_case(bits, log_n, k, lb, ell, g):
    """tests/test_gpu_tfhe_bootstrap_edges.py's crafted_lwe (neg_b on 0, 1, N-1, N, N+1, 2N-1, a rounding tie, the all-ones
    word) with lwe_dimension(g) mask words, (n / g) 2^g keys of largest_gmax, a shared and a per-ciphertext test vector and a
    key-switch key"""
    n, big_n = lwe_dimension(g), 1 << log_n
    gmax = largest_gmax(bits, log_n, k, lb, ell, g)
    mb, ks_mb = m.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, *KS_BASIS)
    rng = np.random.default_rng(13000 * bits + 100 * k + 10 * log_n + g)
    lwe, rs, tie, wrapped, ones_slot = crafted_lwe(rng, bits, log_n, n)
    batch = lwe.size // (n + 1)
    glwe = (k + 1) * big_n
    keys = [small_key(rng, bits, log_n, k, mb.decompose_length, gmax) for _ in range((n // g) << g)]
    tvs = {"shared": rand_words(rng, bits, glwe), "each": rand_words(rng, bits, batch * glwe)}
    ksk = rand_words(rng, bits, k * big_n * KS_BASIS[1] * (n + 1))
    return dict(mb=mb, ks_mb=ks_mb, n=n, batch=batch, lwe=lwe, rs=rs, tie=tie, wrapped=wrapped, ones_slot=ones_slot,
                keys=keys, tvs=tvs, ksk=ksk, gmax=gmax)


def assert_handle_inputs_sit_on_the_branch_points(c, bits, log_n):
    """what test_handle_at_small_n_and_the_branch_points asserts of its input, from the model's modulus switch"""
    n, batch, big_n = c["n"], c["batch"], 1 << log_n
    two_n = 2 * big_n
    rows = c["lwe"].reshape(batch, n + 1)
    exps, neg_b = bs.modulus_switch(c["lwe"], n, bits, log_n)
    assert batch > 3 and batch % 3 != 0                      # chunk = 3: several chunks, a partial last one
    assert neg_b[:len(c["rs"])].tolist() == c["rs"] and set(c["rs"]) == {0, 1, big_n - 1, big_n, big_n + 1, two_n - 1}
    assert bs.sw(int(rows[c["tie"], n]) - 1, bits, log_n) == 1 and neg_b[c["tie"]] == two_n - 2       # ties go up
    assert int(rows[c["wrapped"], n]) == 2 ** bits - 1 and neg_b[c["wrapped"]] == 0
    assert {0, big_n - 1, big_n, two_n - 1} <= set(exps.reshape(-1).tolist())
    assert int(rows[:, :n].reshape(-1)[c["ones_slot"]]) == 2 ** bits - 1 and exps.reshape(-1)[c["ones_slot"]] == 0
    assert np.count_nonzero(exps) >= 3
    return exps, neg_b


def multibit_rotate(g):
    """tfhe_bootstrap_model.bootstrap's `rotate` for a handle created with the grouping factor g"""
    return lambda acc_e, keys, exps_e, basis, log_n, k: mbm.exact_rotate_loop(acc_e, keys, exps_e, g, basis, log_n, k)
