"""The model of the bootstrap steps (tests/tfhe_bootstrap_model.py) against what each step MEANS, on the CPU: the modulus
switch rounds to nearest, the extracted sample carries the chosen coefficient's phase, the key switch keeps the phase up
to the gadget's rounding, and the whole bootstrap evaluates its look-up table on every message."""
import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m


# ---------------- modulus switch ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n", [1, 2, 9, 10, 14])
def test_modulus_switch_rounds_to_nearest_ties_up(bits, log_n):
    two_n = 2 << log_n
    rng = np.random.default_rng(bits + log_n)
    words = bs.boundary_words(bits, log_n) + [int(w) for w in rng.integers(0, 2 ** bits, 200, dtype=np.uint64)]
    for w in words:
        want = ((2 * w * two_n + (1 << bits)) >> (bits + 1)) % two_n      # floor(w 2N / 2^BITS + 1/2) mod 2N
        assert bs.sw(w, bits, log_n) == want, hex(w)
    # the array form is the same rule, and neg_b is the negated b
    n = len(words) - 1
    exps, neg_b = bs.modulus_switch(np.array(words, m.UINT[bits]), n, bits, log_n)
    assert exps.shape == (1, n) and [int(v) for v in exps[0]] == [bs.sw(w, bits, log_n) for w in words[:n]]
    assert int(neg_b[0]) == (two_n - bs.sw(words[n], bits, log_n)) % two_n


# ---------------- extraction ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_extracted_phase_is_the_coefficient_of_the_glwe_phase(bits, k):
    log_n, n = 4, 16
    rng = np.random.default_rng(bits * 10 + k)
    batch = 3
    glwe = rng.integers(0, 2 ** bits, batch * (k + 1) * n, dtype=np.uint64).astype(m.UINT[bits])
    z = rng.integers(0, 2, (k, n))
    for h in (0, 1, n - 1):
        lwe = bs.sample_extract(glwe, log_n, k, h)
        assert lwe.size == batch * (k * n + 1)
        got = bs.lwe_phase(lwe, bs.flatten_key(z), bits)
        for e in range(batch):
            want = bs.glwe_phase(glwe[e * (k + 1) * n:(e + 1) * (k + 1) * n], z, bits, log_n, k)[h]
            assert got[e] == want, (h, e)


# ---------------- key switch ----------------

@pytest.mark.parametrize("bits,in_dim,out_dim,lb,ell", [(32, 16, 5, 4, 3), (32, 8, 3, 8, None), (64, 16, 5, 7, 4),
                                                        (64, 8, 4, 1, 20), (32, 32, 7, 2, 8)])
def test_key_switch_moves_the_phase_by_the_gadget_rounding_at_most(bits, in_dim, out_dim, lb, ell):
    """with a noise-free key, phase_out = b - sum_i s_i (a_i rounded to its kept digits), so the phase moves by at most
    in_dimension * 2^(drop_bits - 1) (s_i in {0, 1}); with drop_bits = 0 it does not move"""
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + in_dim + lb)
    s_in, s_out = rng.integers(0, 2, in_dim), rng.integers(0, 2, out_dim)
    ksk = bs.noise_free_ksk(s_in, s_out, basis, rng)
    batch = 9
    lwe = rng.integers(0, 2 ** bits, batch * (in_dim + 1), dtype=np.uint64).astype(m.UINT[bits])
    out = bs.keyswitch(lwe, ksk, in_dim, out_dim, basis)
    assert out.size == batch * (out_dim + 1)
    moved = m.centred_error(bs.lwe_phase(out, s_out, bits), bs.lwe_phase(lwe, s_in, bits), bits)
    bound = in_dim * 2 ** (basis.drop_bits - 1) if basis.drop_bits else 0
    assert moved.max() <= bound, (moved.max(), bound)


# ---------------- the whole bootstrap ----------------

@pytest.mark.parametrize("bits,lb,ell,ks_lb,ks_ell", [(32, 7, 3, 4, 3), (64, 15, 2, 4, 3)])
@pytest.mark.parametrize("with_ks", [False, True])
def test_bootstrap_evaluates_the_lut_on_every_message(bits, lb, ell, ks_lb, ks_ell, with_ks):
    log_n, p, n, k = 6, 2, 7, 1
    c = bs.meaning_case(bits, log_n, p, n, k, lb, ell, ks_lb, ks_ell, seed=bits + with_ks, repeats=6)
    out = bs.bootstrap(c["lwe"], c["keys"], c["tv"], c["ksk"] if with_ks else None, c["basis"], c["ks_basis"], log_n, k, n)
    key = c["s"] if with_ks else bs.flatten_key(c["z"])
    got = bs.decode(bs.lwe_phase(out, key, bits), p, bits)
    assert got == [bs.lut(p)(int(v)) for v in c["msgs"]]
    # the wrapping box was reached: some message 0 switched to a negative phase
    exps, neg_b = bs.modulus_switch(c["lwe"], n, bits, log_n)
    phase = [(-int(nb) - int(np.dot(e.astype(np.int64), c["s"]))) % (2 << log_n) for e, nb in zip(exps, neg_b)]
    assert any(ph >= (1 << log_n) for ph, v in zip(phase, c["msgs"]) if v == 0)


def test_per_ciphertext_test_vectors():
    """a test vector per ciphertext: each ciphertext goes through its own table"""
    bits, log_n, p, n, k = 32, 6, 2, 7, 1
    c = bs.meaning_case(bits, log_n, p, n, k, 7, 3, 4, 3, seed=5, repeats=1)
    tables = [lambda v, j=j: (v + j) % (1 << p) for j in range(len(c["msgs"]))]
    tvs = np.concatenate([bs.lut_test_vector(f, p, bits, log_n, k) for f in tables])
    out = bs.bootstrap(c["lwe"], c["keys"], tvs, None, c["basis"], None, log_n, k, n)
    got = bs.decode(bs.lwe_phase(out, bs.flatten_key(c["z"]), bits), p, bits)
    assert got == [f(int(v)) for f, v in zip(tables, c["msgs"])]
