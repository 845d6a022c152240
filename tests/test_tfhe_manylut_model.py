"""CPU checks of the many-LUT model (tests/tfhe_manylut_model.py): (a) the strided modulus switch against its statement on big
integers at every stride and at the edge words; (b) with trivial bootstrapping keys in the exact regime the model's SHARED
circuit bootstrap of both bits has the row phases f_r(m g_l) exactly, as tests/test_tfhe_cbs_model.py (b) holds for the
existing path; (c) the many-LUT bootstrap returns each of 2^v step functions of the stride-rounded phase exactly; (d) the
worst-case margin of the strided switch holds at the three noisy shapes of the GPU file.  Nothing here imports the library,
and nothing needs a GPU."""
import numpy as np
import pytest

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_fft_model as m
import tfhe_manylut_model as ml


# ---------------- (a) the strided switch ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n", [1, 4, 10])
def test_strided_switch_is_round_half_up_times_the_stride(bits, log_n):
    rng = np.random.default_rng(bits + log_n)
    for v in range(log_n + 1):
        words = ml.strided_edge_words(bits, log_n, v) + [int(x) for x in rng.integers(0, 2 ** bits, 64, dtype=np.uint64)]
        got = [ml.sw_strided(w, bits, log_n, v) for w in words]
        assert got == [ml.sw_statement(w, bits, log_n, v) for w in words], (bits, log_n, v)
        assert all(g % (1 << v) == 0 and 0 <= g < (2 << log_n) for g in got)
        # the edge list holds what it claims: exact ties of the dropped bits, words that round up to 2N and wrap to 0 ...
        drop = bits - log_n - 1 + v
        assert any(w % (1 << drop) == 1 << (drop - 1) for w in words)
        top = [w for w in words if (2 * w * (2 << log_n) + ((1 << v) << bits)) // (2 * ((1 << v) << bits)) == (2 << log_n) >> v]
        assert top and all(ml.sw_strided(w, bits, log_n, v) == 0 for w in top)
        # ... and body words that wrap when the offset is added; the vector form agrees with the scalar one on both
        offset = 1 << (bits - 2)
        assert any(w + offset >= 1 << bits for w in words)
        n = len(words) - 1
        lwe = np.array(words, np.uint64).astype(m.UINT[bits])
        exps, neg_b = ml.modulus_switch_strided(cm.offset_inputs(lwe, n, bits), n, bits, log_n, v)
        assert [int(x) for x in exps[0]] == got[:n]
        assert int(neg_b[0]) == (-ml.sw_strided((words[n] + offset) % (1 << bits), bits, log_n, v)) % (2 << log_n)
        if v == 0:
            assert got == [bs.sw(w, bits, log_n) for w in words]
            e0, b0 = bs.modulus_switch(lwe, n, bits, log_n)
            e1, b1 = ml.modulus_switch_strided(lwe, n, bits, log_n, 0)
            assert np.array_equal(e0, e1) and np.array_equal(b0, b1)


# ---------------- (b) the shared circuit bootstrap in the exact regime ----------------

# bits, log_n, k, n, rotation basis (drop 0), pfks basis, cbs basis: 2^drop_pf divides every g_l / 2
EXACT_CASES = [(32, 4, 1, 3, (8, 4), (4, 5), (5, 1)), (32, 4, 1, 3, (8, 4), (4, 5), (5, 2)), (32, 5, 2, 2, (8, 4), (6, 3), (4, 3)),
               (32, 5, 1, 3, (8, 4), (4, 6), (4, 4)), (64, 4, 1, 3, (16, 4), (8, 6), (9, 2)), (64, 5, 2, 2, (16, 4), (7, 5), (6, 4)),
               (64, 5, 1, 3, (16, 4), (8, 6), (9, 3)), (64, 4, 2, 1, (16, 4), (8, 6), (9, 1)),
               (32, 1, 1, 1, (8, 4), (4, 5), (5, 2)), (64, 2, 2, 1, (16, 4), (7, 5), (6, 4))]     # 2^v = N


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "u%d-N%d-k%d-l%d" % (c[0], 1 << c[1], c[2], c[6][1]))
def test_shared_circuit_bootstrap_of_a_bit_is_a_ggsw_of_the_bit(case):
    bits, log_n, k, n, rot, pf, cb = case
    big_n = 1 << log_n
    basis, pfks_basis, cbs_basis = (m.ApproxSignedBasis(bits, *b) for b in (rot, pf, cb))
    levels = cbs_basis.decompose_length
    v = ml.log_stride(levels)
    assert basis.drop_bits == 0 and 1 <= pfks_basis.drop_bits <= cbs_basis.drop_bits - 1 and (1 << v) <= big_n
    rng = np.random.default_rng(bits + log_n + k + levels)
    s = rng.integers(0, 2, n)
    s[0] = 1
    z = rng.integers(0, 2, (k, big_n)).astype(m.UINT[bits])
    keys = [bm.trivial_ggsw(basis, log_n, k, int(si)) for si in s]
    pfksk = cm.noise_free_pfksk(bs.flatten_key(z), z, pfks_basis, log_n, k, rng)
    msgs = np.array([0, 1, 1, 0])
    if (1 << v) == big_n:
        # every word switches to 0 or N, so the masks sit on multiples of the half turn, where the switch is exact; the
        # offset phase m/2 + 1/4 would be an exact tie of the switch (rounded up, to the wrong side for both bits), so the
        # inputs carry an error of -1: the only room the margin leaves at this stride
        a = rng.integers(0, 2, (len(msgs), n)).astype(np.uint64) << np.uint64(bits - 1)
        with np.errstate(over="ignore"):
            b = a @ s.astype(np.uint64) + (msgs.astype(np.uint64) << np.uint64(bits - 1)) - np.uint64(1)
        lwe = np.concatenate([a, b[:, None]], axis=1).astype(m.UINT[bits]).reshape(-1)
    else:
        drift, room = ml.switch_margin(n, log_n, v)
        assert drift < room               # the switched phase stays a quarter turn's worth away from the sign changes
        lwe = bs.lwe_encrypt(msgs.astype(np.uint64) << np.uint64(bits - 1), s, bits, rng)
    ext = ml.shared_extracted(lwe, keys, basis, cbs_basis, log_n, k, n).reshape(len(msgs), levels, -1)
    for e, msg in enumerate(msgs):            # trivial keys: the masks stay zero and the body is m g_l exactly
        assert not ext[e, :, :k * big_n].any()
        assert [int(x) for x in ext[e, :, k * big_n]] == [int(msg) * int(g) for g in cm.gadget(cbs_basis)]
    ggsw = ml.shared_circuit_bootstrap(lwe, keys, pfksk, basis, cbs_basis, pfks_basis, log_n, k, n)
    assert ggsw.size == len(msgs) * (k + 1) * levels * (k + 1) * big_n
    got = cm.ggsw_row_phases(ggsw, z, bits, log_n, k)
    assert np.array_equal(got, cm.expected_row_phases(msgs, z, cbs_basis, log_n, k))
    if levels == 1:                           # one level: the existing path, word for word
        assert np.array_equal(ggsw, cm.circuit_bootstrap(lwe, keys, pfksk, basis, cbs_basis, pfks_basis, log_n, k, n))


def test_exact_cases_cover_what_they_must():
    assert {(c[0], c[2]) for c in EXACT_CASES} >= {(32, 1), (32, 2), (64, 1), (64, 2)}
    assert {c[6][1] for c in EXACT_CASES} >= {1, 2, 3, 4}
    assert any(1 << ml.log_stride(c[6][1]) == 1 << c[1] for c in EXACT_CASES)
    tv = ml.shared_test_vector(m.ApproxSignedBasis(32, 4, 3), 3, 1).reshape(2, 8)
    half = [(-(1 << (32 - 12 + 4 * l - 1))) % 2 ** 32 for l in range(3)]
    assert not tv[0].any() and [int(x) for x in tv[1]] == (half + [0]) * 2          # one unused slot


# ---------------- (c) the many-LUT bootstrap ----------------

@pytest.mark.parametrize("bits, log_n, k, n, v", [(32, 5, 1, 3, 1), (32, 5, 2, 2, 2), (64, 6, 1, 3, 2), (64, 4, 1, 1, 3),
                                                  (32, 3, 1, 1, 0)])
def test_many_lut_bootstrap_returns_every_function_of_the_rounded_phase(bits, log_n, k, n, v):
    """2^v different step functions, every one constant on boxes of N/4 exponents (wider than the stride): output (e, i) is
    +-f_i at the stride-rounded phase, one sign for all i, and with v = 0 the ordinary bootstrap"""
    big_n, luts = 1 << log_n, 1 << v
    basis = m.ApproxSignedBasis(bits, bits // 4, 4)
    rng = np.random.default_rng(bits + log_n + v)
    s = rng.integers(0, 2, n)
    s[0] = 1
    keys = [bm.trivial_ggsw(basis, log_n, k, int(si)) for si in s]
    box = max(big_n // 4, 1)
    values = rng.integers(1, 2 ** (bits - 4), (luts, big_n // box), dtype=np.uint64)        # f_i on box q
    tvs = np.zeros((luts, k + 1, big_n), m.UINT[bits])
    tvs[:, k] = np.repeat(values, box, axis=1).astype(m.UINT[bits])
    tv = ml.many_lut_test_vector(tvs)
    for c in range(big_n):
        assert np.array_equal(tv[:, c], tvs[c % luts, :, c - c % luts])
    lwe = rng.integers(0, 2 ** bits, (9, n + 1), dtype=np.uint64).astype(m.UINT[bits]).reshape(-1)
    out = ml.many_lut_bootstrap(lwe, keys, tv.reshape(-1), None, basis, None, log_n, k, n, v).reshape(9, luts, -1)
    exps, neg_b = ml.modulus_switch_strided(lwe, n, bits, log_n, v)
    for e in range(9):
        p = (-int(neg_b[e]) - sum(int(x) * int(si) for x, si in zip(exps[e], s))) % (2 * big_n)    # the rotated phase
        assert p % luts == 0
        for i in range(luts):
            want = int(values[i, (p % big_n) // box]) * (1 if p < big_n else -1)
            assert int(out[e, i, k * big_n]) == want % (1 << bits), (e, i, p)
            assert not out[e, i, :k * big_n].any()
    if v == 0:
        assert np.array_equal(out.reshape(-1), bs.bootstrap(lwe, keys, tv.reshape(-1), None, basis, None, log_n, k, n))


# ---------------- (d) the margin ----------------

def test_the_switch_margin_holds_at_every_noisy_shape():
    seen = []
    for bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, p in cm.NOISY_CASES:
        v = ml.log_stride(cb_ell)
        drift, room = ml.switch_margin(n, log_n, v)
        assert drift < room, (bits, log_n, n, v)
        seen.append((v, drift, room))
    assert seen == [(1, 5, 8), (2, 18, 32), (2, 14, 16)]
    assert [ml.log_stride(l) for l in (1, 2, 3, 4, 5, 8, 9)] == [0, 1, 2, 2, 3, 3, 4]
