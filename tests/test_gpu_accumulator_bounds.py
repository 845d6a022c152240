"""The u64 RNS side's lazily reduced sums at their worst-case operands (the twin of test_gpu_rns32.py::
test_u32_product_accumulators_at_their_bound).  Uniformly random residues put a sum of L products near HALF its maximum,
so a random-data test cannot tell a right overflow bound from a wrong one; every case here is constructed to sit ON the
bound.  Each bound comment of the device code and the case that pins it:

  csrc/pfhe_convert.hip, dot_mod: "16 of them stay below 2^128 and 17 need not"
      test_converter_at_the_accumulator_bound: 62-bit bases of 16 / 17 / 24 / 31 / 32 moduli, scaled residues t_i = q_i - 1.
      The cases "31->9", "32->2" (the pair kernel) and "32->8" assert on Python integers that the true sum is >= 2^128 for
      some output modulus and that the wrapped sum reduces to another residue; every case asserts that no 16-term chunk
      reaches 2^128.  test_conv32_words_share_the_fold: the same kernels on 32-bit words.
  csrc/pfhe_rns.hip, gadget_mulacc_kernel: "8 products of residues < 2^62 stay below 2^127: fold before the next 8"
      test_product_at_the_accumulator_bound[mulacc-*]: N = 2^6 and N = 2^12 with the separate kernels, 61- and 62-bit primes,
      14 / 16 / 28 terms (product) and 7 / 8 / 14 terms (row) — on a fold, 4 / 6 pending and the maximal 7 pending, the last
      with a canonical maximum added on top.
  csrc/pfhe_extprod.hip, mac(PmArith): "can take FOUR terms before it must be folded again" and, in the epilogue of
  gadget_block_mulacc_kernel, "pending terms < 5.5 * 2^K, old < 2^K"
      test_product_at_the_accumulator_bound[block-pm*], [block15-pm*]: 16 terms end on a fold, 14 and 10 leave two pending,
      the row call of 5 terms leaves one and the row call of 7 terms the maximal three, each added to q - 1 (the
      5.5 * 2^K + old case); Q61 and a base that holds the pseudo-Mersenne prime with the largest admissible c next to the
      two of the multi-pass plans.
      [small-pm*]: extprod_small_kernel, whose accumulating form STARTS from the old word (old + four terms).
  csrc/pfhe_extprod.hip, the inv_tail epilogue: "Its butterflies take any representative below 3 * 2^K, so the fold alone is
  enough"
      [block15-*]: only a two-pass ring runs the kernel's inverse tail (N = 2^15, coefficient-form product).  The lazily
      accumulated words go into the inverse block pass folded but not canonical, with 0 and 2 terms pending (PmArith), and
      as Barrett-reduced words (Mont, Shoup).  At N = 2^12 (block-*) coefficient form is the NTT-form kernel followed by the
      table's inverse transform, so those cases pin the accumulators and the canonical store, not the tail.
  csrc/pfhe_extprod.hip, mac(BarrettMac): "the lazy transform leaves digit_hat in [0,4q): Barrett takes any product"
      [block-mont], [block-shoup62], [block15-mont], [block15-shoup62], [small-mont*], [small-shoup62*]: RAW transform outputs of all-(q - 1) digit polynomials
      times q - 1 plus a canonical accumulator; tests/test_modmath_host.py pins the reduction itself for any 64-bit factor.

Inputs of the product cases (pyref.Gadget checks the construction): v = -sum_j 2^(drop + j log B) mod Q has the signed digit
-1 at every level, whose lift is q_i - 1, the largest canonical residue.  Family (a): only coefficient 0 of every polynomial is
v — every digit transform is the constant q - 1, every term is 1 (mod q) against a key of q - 1 everywhere, and the result is
the number of terms at every position (asserted as a closed form AND against the oracle).  Family (b): every coefficient is v
— digit polynomials of q - 1 throughout, the highest the forward butterflies and the raw outputs get from canonical input;
against the all-(q - 1) key and against a random one.  Expected words come from the oracle alone.

Which arithmetic a table takes (PmArith, MontArith, ShoupArith) is decided by its primes and by the switches read when it
is created; the plan report (transform_form) names kernels and launches, not the arithmetic, so the test asserts the plan
and the shape but NOT the policy.  Today: every prime of Q61 and of the largest-c bases is 2^61 - c with c < 2^28
(PmArith); the 60-bit generic primes, and Q61 under PFHE_DISABLE_PM, are below 2^61 (MontArith); the 62-bit primes are
above it (ShoupArith).
"""
import numpy as np
import pytest

import pyref
from gpu_util import rand_rns, to_dev, to_host
from primes import ntt_primes_below
from pyref import Q61
from test_gpu_fuzz import pm_prime
from test_gpu_ntt import MULTIPASS_PRIMES
from test_gpu_u32 import to_dev32, to_host32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pf():
    import primus_fhe_amd as p
    return p


# ---------------------------------------------------------------------------------------------------------------------
# 1. base conversion
# ---------------------------------------------------------------------------------------------------------------------
P62 = ntt_primes_below(40, 62, 4)
# (inputs, outputs, the true sum must reach 2^128 for some output modulus)
CONV_CASES = {
    "16->2": (P62[:16], P62[16:18], False),     # exactly one chunk; the pair kernel on ConvWide<16>
    "17->3": (P62[:17], P62[17:20], False),     # one term past the chunk
    "24->2": (P62[:24], P62[24:26], False),     # ConvWide<24> filled; the pair kernel
    "31->9": (P62[:31], P62[31:40], True),
    "32->2": (P62[:32], P62[32:34], True),      # the pair kernel on ConvWide<32>
    "32->8": (P62[:32], P62[32:40], True),
}


def product(moduli):
    Q = 1
    for q in moduli:
        Q *= q
    return Q


def bound_columns(rng, moduli, n):
    """n >= 5 columns of residues, modulus-major: column 0 makes every scaled residue q_i - 1, column 1 is q_i - 1,
    column 2 is zero, the rest are uniformly random."""
    Q = product(moduli)
    x = rand_rns(rng, moduli, n)
    for i, q in enumerate(moduli):
        x[i * n + 0] = (-(Q // q)) % q
        x[i * n + 1] = q - 1
        x[i * n + 2] = 0
    return x


def scaled(moduli, x, n):
    """The scaled residues t_i = x_i (Q/q_i)^-1 mod q_i of every column, on Python integers: [column][i]."""
    Q = product(moduli)
    inv = [pow(Q // q, -1, q) for q in moduli]
    return [[int(x[i * n + c]) * inv[i] % q for i, q in enumerate(moduli)] for c in range(n)]


@pytest.mark.parametrize("case", list(CONV_CASES))
@pytest.mark.parametrize("n", [5, 777])
def test_converter_at_the_accumulator_bound(pf, orc, case, n):
    mod_in, mod_out, wraps = CONV_CASES[case]
    lin, lout = len(mod_in), len(mod_out)
    assert not set(mod_in) & set(mod_out)
    rng = np.random.default_rng(lin * 100 + lout)
    Q = product(mod_in)
    x = bound_columns(rng, mod_in, n)
    # the test's own condition, on Python integers
    t = scaled(mod_in, x, n)
    t0 = t[0]
    assert t0 == [q - 1 for q in mod_in]
    sums = [sum(ti * ((Q // q) % p) for ti, q in zip(t0, mod_in)) for p in mod_out]
    if wraps:   # a single 128-bit accumulator wraps, and the wrapped value is another residue
        assert any(s >= 1 << 128 for s in sums)
        assert any(s >= 1 << 128 and (s % (1 << 128)) % p != s % p for s, p in zip(sums, mod_out))
    for p in mod_out:   # the reference's order (chunks of 16) is itself exact: no chunk reaches 2^128, even at t_i = q_i - 1
        terms = [(q - 1) * ((Q // q) % p) for q in mod_in]
        assert all(sum(terms[a:a + 16]) < 1 << 128 for a in range(0, lin, 16))
    conv = pf.BaseConverter(pf.RNSBase(mod_in), pf.RNSBase(mod_out))
    oin = orc.RNSBase(mod_in)
    oconv = orc.BaseConverter(oin, orc.RNSBase(mod_out))
    assert np.array_equal(conv.base_change_matrix(), oconv.base_change_matrix)
    exp = oconv.fast_convert_array(x, n)
    # the oracle against sum_i t_i (Q/q_i) mod p_j on Python integers, every column
    punct = [Q // q for q in mod_in]
    for c in range(n):
        s = sum(ti * m for ti, m in zip(t[c], punct))
        assert [int(exp[j * n + c]) for j in range(lout)] == [s % p for p in mod_out], c
    out = np.zeros(lout * n, np.uint64)
    conv.fast_convert_array(x, out, n)
    bad = np.nonzero(out != exp)[0]
    print(f"{case} n={n}: fast_convert_array differs from the oracle in {bad.size} of {out.size} words"
          + (f", first at output modulus {bad[0] // n}, column {bad[0] % n}" if bad.size else ""))
    assert np.array_equal(out, exp)
    dout = to_dev(np.zeros(lout * n, np.uint64))
    conv.fast_convert_array_dev(to_dev(x), dout, n)
    assert np.array_equal(to_host(dout), exp)
    if lout == 2:
        pairs = to_dev(np.zeros(2 * n, np.uint64))
        conv.fast_convert_array_to_pairs_dev(to_dev(x), pairs, n)
        got = to_host(pairs)
        assert np.array_equal(got[0::2], exp[:n]) and np.array_equal(got[1::2], exp[n:])
    # exact conversion to the first output modulus: the same dot product, minus round(sum t_i / q_i) * Q
    e = pf.BaseConverter(pf.RNSBase(mod_in), pf.RNSBase(mod_out[:1]))
    eexp = orc.BaseConverter(oin, orc.RNSBase(mod_out[:1])).exact_convert_array(x, n)
    eo = np.zeros(n, np.uint64)
    e.exact_convert_array(x, eo, n)
    assert np.array_equal(eo, eexp)
    deo = to_dev(np.zeros(n, np.uint64))
    e.exact_convert_array_dev(to_dev(x), deo, n)
    assert np.array_equal(to_host(deo), eexp)


def test_conv32_words_share_the_fold(pf, orc):
    """BaseConverter32 runs the same kernels on 32-bit words: 32 moduli below 2^30 take ConvWide<32> and its fold."""
    P30 = ntt_primes_below(34, 30, 4)
    mod_in, mod_out, n = P30[:32], P30[32:], 261
    rng = np.random.default_rng(3230)
    Q = product(mod_in)
    x = bound_columns(rng, mod_in, n).astype(np.uint32)
    t = scaled(mod_in, x, n)
    assert t[0] == [q - 1 for q in mod_in]
    conv = pf.BaseConverter32(pf.RNSBase32(mod_in), pf.RNSBase32(mod_out))
    oin = orc.RNSBase32(mod_in)
    exp = orc.BaseConverter32(oin, orc.RNSBase32(mod_out)).fast_convert_array(x, n)
    for c in range(n):
        s = sum(ti * (Q // q) for ti, q in zip(t[c], mod_in))
        assert [int(exp[j * n + c]) for j in range(2)] == [s % p for p in mod_out], c
    out = np.zeros(2 * n, np.uint32)
    conv.fast_convert_array(x, out, n)
    assert np.array_equal(out, exp)
    pairs = to_dev32(np.zeros(2 * n, np.uint32))
    conv.fast_convert_array_to_pairs_dev(to_dev32(x), pairs, n)
    got = to_host32(pairs)
    assert np.array_equal(got[0::2], exp[:n]) and np.array_equal(got[1::2], exp[n:])
    e = pf.BaseConverter32(pf.RNSBase32(mod_in), pf.RNSBase32(mod_out[:1]))
    eo = np.zeros(n, np.uint32)
    e.exact_convert_array(x, eo, n)
    assert np.array_equal(eo, orc.BaseConverter32(oin, orc.RNSBase32(mod_out[:1])).exact_convert_array(x, n))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the external product
# ---------------------------------------------------------------------------------------------------------------------
LOG_B = 13                                             # Q61: 14 levels, 28 terms
PM_EDGE_PRIME = pm_prime(61, 12, True)                 # 2^61 - c with the largest admissible c: the tightest term bound
PM_EDGE = [PM_EDGE_PRIME] + list(MULTIPASS_PRIMES["pm"])
S62 = ntt_primes_below(3, 62, 12)                      # above Montgomery's 2^61: the Shoup transforms
MONT = list(MULTIPASS_PRIMES["mont"])                  # generic 60-bit primes: the Montgomery transforms
# the same kinds of prime for a ring of 2^15 (2^16 | q - 1)
PM_EDGE15 = [pm_prime(61, 15, True)] + list(MULTIPASS_PRIMES["pm"])
S62_15 = ntt_primes_below(3, 62, 15)
# id: (log_n, moduli, switches, batch, level counts).  Terms: (k + 1) ell in the product, ell in the row call.
#   fold every 8 (gadget_mulacc_kernel): 16 on a fold, 7 the most pending, 14 / 28 in between
#   fold every 4 (PmArith): 16 and 8 on a fold, 7 the most pending (3), 14 and 10 leave two, 5 leaves one
FORMS = {
    # gadget_mulacc_kernel: tiny rings, and any ring with the separate kernels
    "mulacc-n6-q61": (6, Q61, (), 2, (7, 8, None)),
    "mulacc-n6-s62": (6, S62, (), 2, (7, 8, None)),
    "mulacc-n12-q61-unfused": (12, Q61, ("PFHE_DISABLE_FUSED_EXTPROD",), 2, (7, 8, None)),
    # gadget_block_mulacc_kernel<., 2, .>: 54 ciphertexts x 3 limbs x 1 block = 162 workgroups >= fused_min_wgs = 160.
    # N = 2^12 is a single-pass ring: coefficient-form output is the kernel's canonical NTT-form words followed by the
    # table's inverse transform, NOT the kernel's inverse tail
    "block-pm-q61": (12, Q61, (), 54, (5, 7, 8)),
    "block-pm-largest-c": (12, PM_EDGE, (), 54, (5, 7, 8)),
    "block-mont": (12, Q61, ("PFHE_DISABLE_PM",), 54, (7, 8)),
    "block-shoup62": (12, S62, (), 54, (7, 8)),
    # the same kernel on the smallest two-pass ring, N = 2^15 (rings up to 2^14 are one block pass): 7 ciphertexts x 3
    # limbs x 8 blocks = 168 workgroups.  Here the coefficient-form product takes the kernel's inverse tail (inv_tail:
    # passes == 2, not accumulating): the accumulators go into the inverse block pass after the fold alone, with 0 (16
    # terms) or 2 (14, 10 terms) products pending.  The digits come from the lifting strided pass (int32 digits).
    "block15-pm-q61": (15, Q61, (), 7, (5, 7, 8)),
    "block15-pm-largest-c": (15, PM_EDGE15, (), 7, (5, 7, 8)),
    "block15-mont": (15, Q61, ("PFHE_DISABLE_PM",), 7, (7, 8)),
    "block15-shoup62": (15, S62_15, (), 7, (7, 8)),
    # extprod_small_kernel: N = 2^10 / 2^11, k = 1, log B <= 31, batch * L >= 1024
    "small-pm-n10": (10, [PM_EDGE_PRIME, Q61[0]], (), 512, (5, 7, 8)),
    "small-pm-n11": (11, [PM_EDGE_PRIME, Q61[0]], (), 512, (5, 7, 8)),
    "small-mont-n10": (10, MONT, (), 512, (7, 8)),
    "small-shoup62-n10": (10, S62[:2], (), 512, (7, 8)),
    "small-shoup62-n11": (11, S62[:2], (), 512, (7, 8)),
}


def polys_at_the_bound(moduli, n, g):
    """(family a, family b): one RNS polynomial each, modulus-major."""
    v = (-sum(1 << (g.drop + j * g.log_basis) for j in range(g.ell))) % g.Q
    assert g.signed_digits(v) == [-1] * g.ell
    a = np.zeros(len(moduli) * n, np.uint64)
    for i, q in enumerate(moduli):
        a[i * n] = v % q
    b = np.concatenate([np.full(n, v % q, np.uint64) for q in moduli])
    return a, b


def full_of_q_minus_one(moduli, n, polys):
    return np.tile(np.concatenate([np.full(n, q - 1, np.uint64) for q in moduli]), polys)


@pytest.mark.parametrize("form", list(FORMS))
def test_product_at_the_accumulator_bound(pf, orc, form, monkeypatch):
    log_n, moduli, switches, batch, levels = FORMS[form]
    k, n, L = 1, 1 << log_n, len(moduli)
    W = L * n
    G = (k + 1) * W
    rng = np.random.default_rng(len(form) * 1000 + log_n)
    for s in switches:      # read when the table / the plan is created
        monkeypatch.setenv(s, "1")
    table, base = pf.U64DcrtTable(log_n, moduli), pf.RNSBase(moduli)
    otable, obase = orc.U64DcrtTable(log_n, moduli), orc.RNSBase(moduli)
    if form.startswith("block"):      # the shape that takes the fused kernel, and the passes of its transform plan
        assert (batch * L) << (log_n - 12) >= 160
        assert table.transform_form(W) == (("ntt_block_kernel<12,fwd>", 1) if log_n == 12 else
                                           ("ntt_strided_kernel<K=3,fwd> + ntt_block_kernel<12,fwd>", 2))
    if form.startswith("small"):
        assert batch * L >= 1024 and LOG_B <= 31 and base.big_uint_value_len() <= 4
    for rev in levels:
        basis = pf.BigUintApproxSignedBasis(base, LOG_B, rev)
        obasis = orc.BigUintApproxSignedBasis(obase, LOG_B, rev)
        g = pyref.Gadget(moduli, LOG_B, rev)
        ell = g.ell
        assert ell == basis.decompose_length() == obasis.decompose_length == (rev or ell)
        ctx = pf.DcrtGlevContext(table, base, basis, k, batch)
        terms = (k + 1) * ell
        # the plan's scratch tells which digit buffers it holds: the small-ring kernel needs the compact int32 digits next
        # to the digit polynomials and so does the lifting strided pass of the two-pass ring; the single-pass 2^12 ring and
        # the tiny ring have the digit polynomials only
        digit_polys, compact = batch * (k + 1) * ell * W * 8, form.startswith("small") or log_n == 15
        assert ctx.scratch_bytes() == digit_polys + (batch * (k + 1) * ell * n * 4 if compact else 0)
        pa, pb = polys_at_the_bound(moduli, n, g)
        key_max = full_of_q_minus_one(moduli, n, (k + 1) * ell * (k + 1))
        key_rnd = rand_rns(rng, moduli, n, (k + 1) * ell * (k + 1))
        acc_max = full_of_q_minus_one(moduli, n, k + 1)
        for family, poly, ggsw in (("a", pa, key_max), ("b", pb, key_max), ("b-random-key", pb, key_rnd)):
            tag = (form, ell, family)
            glwe1 = np.tile(poly, k + 1)
            exp = orc.mul_dcrt_ggsw_to(otable, obase, obasis, k, glwe1.copy(), ggsw)
            exp_coeff = exp.copy()
            otable.inverse_transform_slice(exp_coeff)
            glev = ggsw[:ell * (k + 1) * W].copy()
            exp_row = acc_max.copy()
            orc.add_dcrt_glev_mul_crt_poly_assign(otable, obase, obasis, k, exp_row, glev, poly.copy())
            if family == "a":   # closed forms: every term is (q - 1)^2 = 1 (mod q) at every position
                assert (exp == terms).all(), tag
                assert (exp_coeff.reshape(-1, n)[:, 0] == terms).all() and not exp_coeff.reshape(-1, n)[:, 1:].any(), tag
                assert (exp_row == ell - 1).all(), tag
            glwe = np.tile(glwe1, batch)
            out = np.zeros_like(glwe)
            pf.mul_dcrt_ggsw_to(glwe, ggsw, out, ctx)                              # NTT-form output
            assert np.array_equal(out, np.tile(exp, batch)), tag
            pf.mul_dcrt_ggsw_to(glwe, ggsw, out, ctx, into_coeff_form=True)        # coefficient form (block15-*: the inverse tail)
            assert np.array_equal(out, np.tile(exp_coeff, batch)), tag
            dacc = to_dev(np.tile(acc_max, batch))                                 # the accumulating row call on q - 1
            pf.add_dcrt_glev_mul_crt_poly_assign_dev(dacc, to_dev(glev), to_dev(np.tile(poly, batch)), ctx)
            assert np.array_equal(to_host(dacc), np.tile(exp_row, batch)), tag
