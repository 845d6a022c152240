"""The integer model of key generation, encryption and phase (tests/tfhe_keygen_model.py) against the models it has to agree
with, and the whole bootstrap on noisy generated keys in exact integers: the conventions a user would otherwise have to
rebuild by hand (row order (r, level), levels least significant first, drop_bits + l log_basis, the phase b - <a,s>)."""
import itertools

import numpy as np
import pytest

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg


@pytest.mark.parametrize("bits", [32, 64])
def test_encrypt_then_phase_returns_noise_plus_message_exactly(bits):
    rng = np.random.default_rng(bits)
    for dim, batch in ((1, 1), (63, 3), (130, 5)):
        for key in (rng.integers(0, 2, dim).astype(m.UINT[bits]), kg.uniform_words(rng, bits, dim)):
            rand = kg.lwe_randomness(rng, bits, dim, batch, 1 << 10)
            rand.reshape(batch, dim + 1)[:, dim] += m.UINT[bits](5 << (bits - 4))
            ct = kg.lwe_body_mac(rand, key, bits)
            assert not np.array_equal(ct, rand)
            assert np.array_equal(kg.lwe_body_mac(ct, key, bits, subtract=True), rand)
            assert np.array_equal(bs.lwe_phase(ct, key, bits), rand.reshape(batch, dim + 1)[:, dim])
    for log_n, k in ((1, 1), (4, 2), (6, 3)):
        n = 1 << log_n
        for z in (rng.integers(0, 2, (k, n)).astype(m.UINT[bits]), kg.uniform_words(rng, bits, k * n).reshape(k, n)):
            rand = kg.glwe_randomness(rng, bits, log_n, k, 3, 1 << 10)
            ct = kg.glwe_body_mac(rand, z, bits, log_n, k)
            assert np.array_equal(kg.glwe_body_mac(ct, z, bits, log_n, k, subtract=True), rand)
            for e in range(3):
                one = ct.reshape(3, -1)[e]
                assert np.array_equal(bs.glwe_phase(one, z, bits, log_n, k), rand.reshape(3, k + 1, n)[e, k])


@pytest.mark.parametrize("bits,lb,ell", [(32, 7, 3), (32, 8, 4), (32, 1, 5), (64, 15, 2), (64, 16, 4)])
def test_ggsw_with_zero_masks_and_zero_noise_is_the_trivial_ggsw(bits, lb, ell):
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(lb)
    for log_n, k in ((1, 1), (3, 2)):
        z = rng.integers(0, 2, (k, 1 << log_n)).astype(m.UINT[bits])
        msgs = [0, 1, (1 << bits) - 1, 12345]
        zero = np.zeros(len(msgs) * (k + 1) * ell * (k + 1) << log_n, m.UINT[bits])
        got = kg.ggsw_encrypt(zero, msgs, z, basis, log_n, k).reshape(len(msgs), -1)
        for q, msg in enumerate(msgs):
            want = bm.trivial_ggsw(basis, log_n, k, 1).astype(np.uint64) * np.uint64(msg)
            assert np.array_equal(got[q], want.astype(m.UINT[bits])), (log_n, k, msg)
        assert np.array_equal(got[1], bm.trivial_ggsw(basis, log_n, k, 1))


@pytest.mark.parametrize("bits,lb,ell,noise", [(32, 7, 3, 64), (64, 15, 2, 2 ** 20)])
@pytest.mark.parametrize("k", [1, 2])
def test_the_product_with_an_encrypted_ggsw_multiplies_the_phase(bits, lb, ell, noise, k):
    """phase(schoolbook(ct, GGSW(m))) = m phase(ct) within the per-step term of the bound, for m = 0 and 1"""
    log_n = 5
    n = 1 << log_n
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + k)
    z = rng.integers(0, 2, (k, n)).astype(m.UINT[bits])
    rand_ct = kg.glwe_randomness(rng, bits, log_n, k, 1, noise)
    rand_ct.reshape(k + 1, n)[k] += kg.uniform_words(rng, bits, n)            # any message
    ct = kg.glwe_body_mac(rand_ct, z, bits, log_n, k)
    phase = bs.glwe_phase(ct, z, bits, log_n, k)
    for msg in (0, 1):
        ggsw = kg.ggsw_encrypt(kg.glwe_randomness(rng, bits, log_n, k, (k + 1) * ell, noise), [msg], z, basis, log_n, k)
        out = m.schoolbook(ct, ggsw, basis, log_n, k)
        got = bs.glwe_phase(out, z, bits, log_n, k)
        want = phase if msg else np.zeros_like(phase)
        err = m.centred_error(got, want, bits).max()
        assert 0 < err <= kg.step_bound(bits, log_n, k, lb, ell, noise), (msg, err)


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_exactly_one_indicator_per_group_is_one(g):
    for bits in (32, 64):
        for key in itertools.product((0, 1), repeat=2 * g):             # every binary key of two groups
            msgs = kg.indicator_messages(key, g, bits)
            assert len(msgs) == 2 << g
            for t in range(2):
                group = msgs[t << g:(t + 1) << g]
                pattern = sum(key[t * g + b] << b for b in range(g))
                assert group == [int(j == pattern) for j in range(1 << g)]
    assert kg.bsk_messages([1, 0, (1 << 32) - 1], 0, 32) == [1, 0, (1 << 32) - 1]


@pytest.mark.parametrize("bits", [32, 64])
def test_the_noise_free_key_switch_key_is_the_model_with_zero_noise(bits):
    rng = np.random.default_rng(bits + 3)
    for in_dim, out_dim, lb, ell in ((4, 1, 8, None), (64, 7, 4, 3), (16, 33, 4, 6)):
        basis = m.ApproxSignedBasis(bits, lb, ell)
        s_in, s_out = rng.integers(0, 2, in_dim), rng.integers(0, 2, out_dim)
        want = bs.noise_free_ksk(s_in, s_out, basis, rng)
        rand = want.reshape(-1, out_dim + 1).copy()
        rand[:, out_dim] = 0                                              # its masks, zero noise
        assert np.array_equal(kg.ksk(rand.reshape(-1), s_in, s_out, basis), want)


@pytest.mark.parametrize("case", kg.NOISY_CASES, ids=lambda c: "u%d-N%d-k%d-n%d-g%d" % (c[0], 1 << c[1], c[2], c[3], c[6]))
def test_the_noisy_bootstrap_decodes_in_exact_integers(case):
    """keys generated by the model from noisy randomness, the rotation as the exact schoolbook: (a) the switched phase stays
    in its box, (b) the bound is below Delta/2, (c) every output decodes to f(m), (d) the error is within the bound"""
    bits, log_n, k, n, lb, ell, g, p, noise = case
    big_n = 1 << log_n
    c = kg.noisy_case(*case, seed=1000 + bits + log_n + k + g)
    basis, ks_basis = c["basis"], c["ks_basis"]
    bound = kg.noise_bound(bits, log_n, k, n, lb, ell, g, *kg.KS_BASIS, noise)
    assert (n + 1) / 2 < big_n / 2 ** (p + 1)
    assert bound < 2.0 ** (bits - p - 2)
    lwe = kg.lwe_body_mac(c["lwe_rand"], c["s"], bits)
    keys = kg.bsk(c["rand_bsk"], c["s"], c["z"], basis, log_n, k, g).reshape(c["keys"], -1)
    ksk = kg.ksk(c["rand_ksk"], bs.flatten_key(c["z"]), c["s"], ks_basis)
    out = kg.exact_bootstrap(lwe, list(keys), c["tv"], ksk, basis, ks_basis, log_n, k, n, g)
    phases = bs.lwe_phase(out, c["s"], bits)
    want = [bs.lut(p)(int(v)) for v in c["msgs"]]
    assert bs.decode(phases, p, bits) == want
    err = kg.phase_error(phases, c["msgs"], p, bits)
    print("bits %d log_n %d k %d g %d: err 2^%.1f bound 2^%.1f" % (bits, log_n, k, g, np.log2(max(err, 1)), np.log2(bound)))
    assert 0 < err <= bound
