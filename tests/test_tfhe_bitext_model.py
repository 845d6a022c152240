"""The bit-extraction model (tests/tfhe_bitext_model.py) against what it means, on the CPU: on noise-free keys every message
of `bits` bits at delta gives outputs whose phases decode to the bits of m, least significant first, and message bits at
or above delta + bits do not matter; and the derived bound tfhe_bitext_model.bit_bound is under the margin for every
noisy shape the GPU tests run."""
import numpy as np
import pytest

import tfhe_bitext_model as bx
import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_lut_model as lm

# the rotation's basis drops no bit, so that on trivial keys the rotation is exact; the key switch's basis does
ROT_BASIS = {32: (8, 4), 64: (16, 4)}
KS_BASIS = {32: (4, 6), 64: (8, 6)}


def cases():
    """u32 and u64, log N 4 to 6, k = 1 and 2, bits 1 to 5, delta from 1 up to BITS - bits: every value of each parameter,
    not their whole product (the rotation is a schoolbook product per step)"""
    out = []
    for bits in (32, 64):
        for nbits in (1, 2, 3, 4, 5):
            deltas = sorted({1, bits // 2, bits - nbits - 1, bits - nbits})
            for j, delta in enumerate(deltas):
                log_n = 4 + (nbits + j) % 3
                k = 1 + (nbits + j) % 2 if log_n < 6 else 1
                out.append((bits, log_n, k, nbits, delta))
    return out


def test_cases_cover_the_ranges():
    cs = cases()
    assert {c[0] for c in cs} == {32, 64} and {c[1] for c in cs} == {4, 5, 6} and {c[2] for c in cs} == {1, 2}
    assert {c[3] for c in cs} == {1, 2, 3, 4, 5}
    for bits in (32, 64):
        for nbits in range(1, 6):
            assert {1, bits - nbits} <= {c[4] for c in cs if c[0] == bits and c[3] == nbits}


@pytest.mark.parametrize("bits,log_n,k,nbits,delta", cases(), ids=lambda v: str(v))
def test_every_message_decodes_to_its_bits_on_noise_free_keys(bits, log_n, k, nbits, delta):
    n, big_n = 3, 1 << log_n
    basis, ks_basis = m.ApproxSignedBasis(bits, *ROT_BASIS[bits]), m.ApproxSignedBasis(bits, *KS_BASIS[bits])
    assert basis.drop_bits == 0 and ks_basis.drop_bits >= 1
    # the only errors: the key switch drops k N words' low bits, and the modulus switch rounds n + 1 words
    ks_round = k * big_n * 2.0 ** (ks_basis.drop_bits - 1)
    assert ks_round * (2 * big_n) / 2.0 ** bits + (n + 1) / 2 < big_n / 2
    rng = np.random.default_rng(bits + 10 * log_n + 100 * k + nbits + delta)
    s = rng.integers(0, 2, n)
    s[0] = 1
    z = rng.integers(0, 2, (k, big_n))
    keys = [bm.trivial_ggsw(basis, log_n, k, int(si)) for si in s]
    ksk = bs.noise_free_ksk(bs.flatten_key(z), s, ks_basis, rng)
    msgs = list(range(1 << nbits))
    # the same messages again under random bits at and above delta + bits (shifted out), where there is room for any
    top = bits - delta - nbits
    high = [int(rng.integers(0, 1 << min(top, 16))) << nbits for _ in msgs] if top else []
    values = [((v + h) << delta) % (1 << bits) for v, h in zip(msgs + msgs[:len(high)], [0] * len(msgs) + high)]
    lwe = bs.lwe_encrypt(np.array(values, np.uint64), bs.flatten_key(z), bits, rng)
    out = bx.extract_bits(lwe, keys, ksk, basis, ks_basis, log_n, k, n, delta, nbits)
    got = bx.decode_bits(bs.lwe_phase(out, s, bits), bits)
    want = [(v >> i) & 1 for v in (msgs + msgs[:len(high)]) for i in range(nbits)]
    assert got == want
    # and the phases are close: only the key switch's rounding is between them and m_i 2^(BITS-1)
    err = m.centred_error(bs.lwe_phase(out, s, bits), (np.array(want, np.uint64) << np.uint64(bits - 1)).astype(m.UINT[bits]),
                          bits).max()
    assert err <= ks_round


def test_hand_check_of_the_bound_at_the_first_noisy_shape():
    """u32, log N 6, n 8, log B 7, ell 3, E 64, key switch (4, 6): the margin is 2^29.8, and six bits at delta = 26 reach
    2^27.6 at i = 1"""
    bits, log_n, k, n, lb, ell, _g, _p, noise = kg.NOISY_CASES[0]
    assert (bits, log_n, k, n, lb, ell, noise) == (32, 6, 1, 8, 7, 3, 64) and kg.KS_BASIS == (4, 6)
    big_n = 1 << log_n
    margin = (big_n / 2 - (n + 1) / 2) * 2.0 ** bits / (2 * big_n)
    assert abs(np.log2(margin) - 29.8) < 0.05
    b1 = bx.bit_bound(bits, log_n, k, n, lb, ell, *kg.KS_BASIS, noise, noise, 26, 1)
    assert abs(np.log2(b1) - 27.6) < 0.1
    assert bx.all_bits_fit(bits, log_n, k, n, lb, ell, *kg.KS_BASIS, noise, noise, 26, 6)


def test_bound_is_under_the_margin_for_every_noisy_shape_of_the_gpu_tests():
    for bits, log_n, k, n, lb, ell, noise, nbits, delta in bx.meaning_shapes():
        assert delta + nbits <= bits
        assert bx.all_bits_fit(bits, log_n, k, n, lb, ell, *kg.KS_BASIS, noise, noise, delta, nbits), (bits, log_n, k, nbits)
    for idx, (case, t, r) in enumerate(lm.NOISY_LUTS):
        bits, log_n, k, n, lb, ell, noise = case[:7]
        noise = bx.CHAIN_NOISE.get(idx, noise)
        p = t + r
        assert p == (3 if bits == 32 else 5)
        # fresh encryptions with |e_in| <= E at delta = BITS - p; the bit ciphertext's own error must also leave the circuit
        # bootstrap its quarter turn, which is the same condition
        assert bx.all_bits_fit(bits, log_n, k, n, lb, ell, *kg.KS_BASIS, noise, noise, bits - p, p), (bits, log_n, k)
