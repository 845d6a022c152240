"""The numpy model of the multi-bit blind rotation (tests/tfhe_multibit_model.py) against what it has to mean: M(r) is the
transform of the monomial, indicator keys rotate a message by X^{sum a_i s_i}, the combined key of g = 1 is
K_0 + X^a K_1, and on full-torus keys the model's own error against the exact integer step is printed per shape (the
quantity the GPU tests' error rule is relative to).  Then the exact regime: for every exact case of
tests/test_gpu_tfhe_multibit_edges.py (the tables of tests/tfhe_multibit_cases.py) the 2^g rule holds and the f64 model
equals the integer model word for word on that file's own inputs."""
import itertools

import numpy as np
import pytest

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_multibit_cases as cases
import tfhe_multibit_model as mbm


@pytest.mark.parametrize("log_n", [1, 2, 6])
def test_monomial_spectrum_is_the_forward_transform_of_the_monomial(log_n):
    n = 1 << log_n
    fft = m.FullComplex64FftTable(log_n)
    worst = 0.0
    for r in range(2 * n):
        want = fft.forward(mbm.monomial(r, log_n, 32), 32)
        got = mbm.monomial_spectrum(r, log_n)
        worst = max(worst, float(np.abs(got - want).max()))
        # Hermitian symmetry in the full layout: M[(1 - k) mod N] = conj(M[k])
        k = np.arange(n)
        assert np.abs(got[(1 - k) % n] - np.conj(got)).max() < 1e-15
    print(f"N {n}: max |M(r) - forward(X^r)| = {worst:.3g}")
    assert worst < 1e-13
    assert np.array_equal(mbm.monomial_spectrum(2 * n + 3, log_n), mbm.monomial_spectrum(3, log_n))


@pytest.mark.parametrize("bits,log_n,lb,ell", [(32, 6, 10, 2), (64, 6, 15, 2)])
@pytest.mark.parametrize("g", [1, 2, 3])
def test_indicator_keys_rotate_the_message_for_every_key_pattern(bits, log_n, lb, ell, g):
    n, k = 1 << log_n, 1
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + g)
    for pattern in itertools.product((0, 1), repeat=2 * g):       # two groups: every pattern of each
        exps = np.array([0, n, 2 * n - 1, n + 1, 5, 2 * n - 3][:2 * g], np.uint32)
        exps[-1] = rng.integers(0, 2 * n)
        bsk = mbm.fourier(mbm.multibit_indicator_bsk(basis, log_n, k, pattern, g), log_n, bits)
        msg = rng.integers(0, 1 << bm.PLAINTEXT_BITS, n)
        acc = bm.encode([msg], bits, log_n, k)
        out = mbm.rotate_loop(acc, bsk, exps, g, basis, log_n, k)
        mask_err, got = bm.decode(out, bits, log_n, k)
        total = sum(int(a) * s for a, s in zip(exps, pattern))
        assert mask_err == 0.0, pattern
        assert got == bm.expected_decode(msg, total, n), (pattern, total)


@pytest.mark.parametrize("bits,log_n", [(32, 5), (64, 7)])
def test_combined_key_of_one_element_is_k0_plus_the_rotated_k1(bits, log_n):
    n = 1 << log_n
    rng = np.random.default_rng(bits)
    k0, k1 = (rng.integers(-1024, 1025, 8 * n).astype(m.UINT[bits]) for _ in range(2))
    for a in (0, 1, n - 1, n, 2 * n - 1, 3 * n + 2):
        got = mbm.combine_key(mbm.fourier([k0, k1], log_n, bits), [a], log_n)
        want = mbm.fourier([bm.add(k0, bm.rotate(k1, a, n))], log_n, bits)
        assert np.abs(got - want).max() < 1e-7, a                 # entries up to N 2^11: f64 keeps them to ~1e-10
        assert np.array_equal(mbm.exact_key([k0, k1], [a], log_n), bm.add(k0, bm.rotate(k1, a, n)))


MODEL_SHAPES = [(32, 6, 1, 7, 3, 2), (32, 8, 1, 7, 3, 3), (32, 10, 1, 10, 2, 4), (64, 6, 1, 15, 2, 2), (64, 10, 1, 15, 2, 2),
                (32, 6, 2, 7, 3, 2)]


@pytest.mark.parametrize("bits,log_n,k,lb,ell,g", MODEL_SHAPES)
def test_model_error_against_the_exact_group_on_full_torus_keys(bits, log_n, k, lb, ell, g):
    """the model's own error: zero where f64 holds every accumulator (u32), a few times the single product's at u64 (the
    combined key is a sum of 2^g full-torus keys).  The bound is the f64 budget of the sum: 2^g keys of N (k+1) ell terms of
    magnitude 2^(BITS-1) 2^(logB-1) each, relative 2^-53 per operation of a log2(N)-deep transform."""
    n = 1 << log_n
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + log_n + g)
    keys = [rng.integers(0, 2 ** bits, (k + 1) * ell * (k + 1) * n, dtype=np.uint64).astype(m.UINT[bits]) for _ in range(1 << g)]
    exps = [int(x) for x in rng.integers(0, 2 * n, g)]
    acc = rng.integers(0, 2 ** bits, (k + 1) * n, dtype=np.uint64).astype(m.UINT[bits])
    model = mbm.step(acc, mbm.fourier(keys, log_n, bits), exps, basis, log_n, k)
    exact = mbm.exact_group(acc, keys, exps, basis, log_n, k)
    err = float(m.centred_error(model, exact, bits).max())
    single, _ = m.external_product(acc, mbm.fourier(keys[:1], log_n, bits), basis, log_n, k)
    single_err = float(m.centred_error(single, m.schoolbook(acc, keys[0], basis, log_n, k), bits).max())
    print(f"bits {bits} N 2^{log_n} k {k} logB {lb} ell {ell} g {g}: model_err {err:.3g} (single product {single_err:.3g})")
    budget = (1 << g) * n * (k + 1) * ell * 2.0 ** (bits - 1) * 2.0 ** (lb - 1) * 2.0 ** -53 * 4 * log_n
    assert err <= max(1.0, budget)


# ---------------- the exact regime of tests/test_gpu_tfhe_multibit_edges.py ----------------
#
# The GPU file asks for every word of the integer model.  That can only be asked where f64 holds every accumulator: under
# the 2^g rule of tests/tfhe_multibit_cases.py.  Here the rule is asserted for every exact case of that file, and the f64
# model (the key combined in the Fourier domain, as the device combines it) is shown to give the integer model's words on
# that file's own inputs.  Necessary, not sufficient: the device rounds in another order.

def assert_step_is_exact(acc, keys, exps, g, mb, log_n, k):
    """every ciphertext of acc through every group: step (f64) == exact_group (integers), the integer result carried on;
    returns the integer result and, per group, whether any ciphertext entered it with a non-zero digit"""
    W = (k + 1) << log_n
    exps = np.asarray(exps).reshape(acc.size // W, -1)
    groups = exps.shape[1] // g
    fourier = [mbm.fourier(keys[t << g:(t + 1) << g], log_n, mb.bits) for t in range(groups)]
    out, live = [], [False] * groups
    for e in range(acc.size // W):
        a = acc[e * W:(e + 1) * W]
        for t in range(groups):
            live[t] = live[t] or bool(np.stack(mb.digits(a)).any())
            x = exps[e, t * g:(t + 1) * g]
            exact = mbm.exact_group(a, keys[t << g:(t + 1) << g], x, mb, log_n, k)
            assert np.array_equal(mbm.step(a, fourier[t], x, mb, log_n, k), exact), (e, t, x.tolist())
            a = exact
        out.append(a)
    return np.concatenate(out), live


def test_exact_rotate_loop_is_exact_group_over_the_groups_with_exponents_modulo_2n():
    bits, log_n, k, g = 32, 3, 1, 2
    n = 1 << log_n
    mb = m.ApproxSignedBasis(bits, 7, 3)
    rng = np.random.default_rng(5)
    keys = [rng.integers(-1024, 1025, 2 * 3 * 2 * n).astype(np.uint32) for _ in range(3 << g)]
    acc = rng.integers(0, 2 ** bits, 2 * n, dtype=np.uint64).astype(np.uint32)
    exps = rng.integers(0, 2 * n, 3 * g).astype(np.uint32)
    want = acc
    for t in range(3):
        want = mbm.exact_group(want, keys[t << g:(t + 1) << g], exps[t * g:(t + 1) * g], mb, log_n, k)
    assert np.array_equal(mbm.exact_rotate_loop(acc, keys, exps, g, mb, log_n, k), want)
    big = (exps.astype(np.uint64) + 2 * n * np.array([1, 3, 5, 2 ** 27 - 1, 7, 2], np.uint64)).astype(np.uint32)
    assert big.min() >= 2 * n
    assert np.array_equal(mbm.exact_rotate_loop(acc, keys, big, g, mb, log_n, k), want)
    assert not np.array_equal(want, acc)


@pytest.mark.parametrize("bits,log_n,k,lb,ell,g,gmax", cases.EDGE_GROUP)
def test_edge_group_cases_stay_in_the_exact_regime(bits, log_n, k, lb, ell, g, gmax):
    assert cases.rule_lhs(bits, log_n, k, lb, ell, g, gmax) <= 2 ** 40
    c = cases.edge_group_case(bits, log_n, k, lb, ell, g, gmax)
    cases.assert_patterns_reach(c["exps"], 1 << log_n, g)
    assert all(np.abs(key.view(m.SINT[bits]).astype(np.int64)).max() <= gmax for key in c["keys"])
    assert gmax <= cases.largest_gmax(bits, log_n, k, lb, ell, g)
    out, _ = assert_step_is_exact(c["acc"], c["keys"], c["exps"], g, c["mb"], log_n, k)
    W = (k + 1) << log_n
    for e in c["quiet"]:                                   # the product of the quiet ciphertexts is zero
        assert not out[e * W:(e + 1) * W].any()
        assert c["acc"][e * W:(e + 1) * W].any() or c["mb"].drop_bits == 0


@pytest.mark.parametrize("bits,log_n,k,lb,ell,g", cases.SMALL_CASES)
def test_small_n_cases_stay_in_the_exact_regime(bits, log_n, k, lb, ell, g):
    c = cases.small_n_case(bits, log_n, k, lb, ell, g)
    assert 2 ** 39 < cases.rule_lhs(bits, log_n, k, lb, ell, g, c["gmax"]) <= 2 ** 40
    cases.assert_patterns_reach(c["exps"], 1 << log_n, g)
    out, live = assert_step_is_exact(c["acc"], c["keys"], c["exps"], g, c["mb"], log_n, k)
    print(f"groups entered with a non-zero digit: {live}")
    assert live[0] and (all(live) or bits == 64)           # u64 beyond the first group: tfhe_multibit_cases.largest_gmax
    W = (k + 1) << log_n
    want = np.concatenate([mbm.exact_rotate_loop(c["acc"][e * W:(e + 1) * W], c["keys"], c["exps"][e], g, c["mb"], log_n, k)
                           for e in range(cases.SMALL_BATCH)])
    assert np.array_equal(out, want)


@pytest.mark.parametrize("bits,log_n,k,lb,ell,g", cases.HANDLE_CASES)
def test_handle_cases_stay_in_the_exact_regime(bits, log_n, k, lb, ell, g):
    """the rotation's inputs as the handle forms them (ACC = X^{neg_b} TV, the switched mask), with the shared test vector;
    and bootstrap(rotate=...) is sample extraction of exactly these accumulators"""
    c = cases.handle_case(bits, log_n, k, lb, ell, g)
    assert 2 ** 39 < cases.rule_lhs(bits, log_n, k, lb, ell, g, c["gmax"]) <= 2 ** 40
    assert c["n"] % g == 0 and 4 <= c["n"] < 4 + g
    exps, neg_b = cases.assert_handle_inputs_sit_on_the_branch_points(c, bits, log_n)
    tv = c["tvs"]["shared"]
    acc = np.concatenate([bm.rotate(tv, int(r), 1 << log_n) for r in neg_b])
    out, live = assert_step_is_exact(acc, c["keys"], exps, g, c["mb"], log_n, k)
    assert all(live) and out.any()                         # every group multiplies something: tfhe_multibit_cases.HANDLE_CASES
    if log_n <= 6:
        want = bs.bootstrap(c["lwe"], c["keys"], tv, None, c["mb"], c["ks_mb"], log_n, k, c["n"], rotate=cases.multibit_rotate(g))
        assert np.array_equal(want, bs.sample_extract(out, log_n, k, 0))


def test_bootstrap_model_default_rotation_is_unchanged():
    bits, log_n, k, n = 32, 3, 1, 4
    mb, ks_mb = m.ApproxSignedBasis(bits, 7, 3), m.ApproxSignedBasis(bits, 4, 3)
    rng = np.random.default_rng(6)
    keys = [rng.integers(-1024, 1025, 2 * 3 * 2 << log_n).astype(np.uint32) for _ in range(n)]
    lwe = rng.integers(0, 2 ** bits, 3 * (n + 1), dtype=np.uint64).astype(np.uint32)
    tv = rng.integers(0, 2 ** bits, 2 << log_n, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(bs.bootstrap(lwe, keys, tv, None, mb, ks_mb, log_n, k, n),
                          bs.bootstrap(lwe, keys, tv, None, mb, ks_mb, log_n, k, n, rotate=bm.exact_rotate))
