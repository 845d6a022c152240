"""The numpy model of packing (tests/tfhe_pack_model.py) against the project's other models, on the CPU: the identities
that tie the packing key switch to the LWE key switch and the multi-message extraction to sample extraction, the meaning
of the packed phase with a noise-free key, and the derived noise bound on its four shapes."""
import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_pack_model as pm


def test_the_convolution_form_of_the_negacyclic_product_is_the_schoolbook():
    rng = np.random.default_rng(11)
    for n in (2, 4, 16, 64):
        a, b = (rng.integers(0, 2 ** 64, n, dtype=np.uint64) for _ in range(2))
        assert np.array_equal(pm.negacyclic(a, b), m.negacyclic_u64(a, b))


@pytest.mark.parametrize("bits, log_n, k, n, lb, ell", [(32, 3, 1, 5, 4, 6), (32, 4, 2, 7, 7, 3), (64, 3, 1, 6, 15, 3),
                                                        (64, 2, 2, 5, 1, 9), (32, 1, 1, 3, 8, 4)])
def test_count_one_is_the_lwe_key_switch_through_extraction_at_index_0(bits, log_n, k, n, lb, ell):
    """extraction is linear, so index 0 of the pack equals keyswitch against the rows' index-0 extractions, word for word"""
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + log_n)
    big_n = 1 << log_n
    pksk = kg.uniform_words(rng, bits, n * ell * (k + 1) * big_n)
    lwe = kg.uniform_words(rng, bits, 3 * (n + 1))
    edges = ew.edge_words(bits, lb, ell)
    lwe[:min(len(edges), n)] = edges[:n]
    packed = pm.pack_keyswitch(lwe, pksk, n, 1, basis, log_n, k)
    ksk = pm.extracted_key_rows(pksk, log_n, k)
    want = bs.keyswitch(lwe, ksk, n, k * big_n, basis)
    assert np.array_equal(bs.sample_extract(packed, log_n, k, 0), want)


@pytest.mark.parametrize("bits, log_n, k", [(32, 1, 1), (32, 3, 2), (64, 4, 1), (64, 2, 3)])
def test_the_expansion_of_the_first_few_is_sample_extraction_at_every_index(bits, log_n, k):
    rng = np.random.default_rng(3 * bits + log_n)
    n = 1 << log_n
    g = kg.uniform_words(rng, bits, 3 * (k + 1) * n)
    for count in sorted({1, 2, n - 1, n} - {0}):
        multi = pm.extract_first_few(g, log_n, k, count)
        assert multi.size == 3 * (k * n + count)
        lwe = pm.multimsg_extract(multi, log_n, k, count).reshape(3, count, k * n + 1)
        for h in range(count):
            assert np.array_equal(lwe[:, h].reshape(-1), bs.sample_extract(g, log_n, k, h)), (count, h)
    # the layout itself: a_0, -a_{N-1}, ..., -a_1 per mask polynomial, then the bodies
    one = pm.extract_first_few(g, log_n, k, n).reshape(3, -1)[0]
    a = g.reshape(3, k + 1, n)[0]
    with np.errstate(over="ignore"):
        assert one[0] == a[0, 0] and one[1] == (0 - a[0, n - 1]).astype(a.dtype) and one[n - 1] == (0 - a[0, 1]).astype(a.dtype)
    assert np.array_equal(one[k * n:], a[k])


@pytest.mark.parametrize("bits, log_n, k, n, lb, ell, count", [(32, 3, 1, 5, 4, 6, 8), (32, 4, 2, 6, 7, 3, 5),
                                                               (64, 3, 1, 4, 15, 3, 7), (64, 2, 1, 5, 16, 4, 4)])
def test_a_noise_free_key_gives_the_switched_phase_exactly(bits, log_n, k, n, lb, ell, count):
    """phase coefficient i < count of the pack = b_i - sum_j a~_{i,j} s_j, a~ the value the kept digits recompose to"""
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(7 * bits + count)
    big_n = 1 << log_n
    s = rng.integers(0, 2 ** bits, n, dtype=np.uint64).astype(m.UINT[bits])     # any words, not only bits
    z = rng.integers(0, 2, (k, big_n)).astype(m.UINT[bits])
    rand = kg.glwe_randomness(rng, bits, log_n, k, n * ell, 0)
    pksk = pm.generate_pksk(rand, s, z, basis, log_n, k)
    lwe = kg.uniform_words(rng, bits, 2 * count * (n + 1))
    packed = pm.pack_keyswitch(lwe, pksk, n, count, basis, log_n, k).reshape(2, -1)
    x = lwe.reshape(2, count, n + 1).astype(np.uint64)
    digits = basis.digits(x[:, :, :n])
    with np.errstate(over="ignore"):
        approx = sum(d.astype(np.int64).view(np.uint64) << np.uint64(basis.drop_bits + l * lb) for l, d in enumerate(digits))
        want = (x[:, :, n] - approx @ s.astype(np.uint64)).astype(m.UINT[bits])
    for e in range(2):
        phase = bs.glwe_phase(packed[e], z, bits, log_n, k)
        assert np.array_equal(phase[:count], want[e])


@pytest.mark.parametrize("case", pm.NOISY_CASES, ids=lambda c: "u%d-logn%d-k%d-n%d-lb%d-ell%d-count%d" % c[:7])
def test_noisy_keys_stay_within_the_derived_bound(case):
    bits, log_n, k, n, lb, ell, count, noise, p = case
    bound = pm.noise_bound(bits, n, lb, ell, count, noise)
    assert bound < 2.0 ** (bits - p - 2)
    c = pm.noisy_case(*case, seed=5)
    pksk = pm.generate_pksk(c["rand_pksk"], c["s"], c["z"], c["basis"], log_n, k)
    packed = pm.pack_keyswitch(c["lwe"], pksk, n, count, c["basis"], log_n, k).reshape(c["batch"], -1)
    phases = np.concatenate([bs.glwe_phase(packed[e], c["z"], bits, log_n, k)[:count] for e in range(c["batch"])])
    assert bs.decode(phases, p, bits) == list(c["msgs"])
    err = pm.message_error(phases, c["msgs"], c["delta"], bits)
    lwe = pm.multimsg_extract(pm.extract_first_few(packed.reshape(-1), log_n, k, count), log_n, k, count)
    lwe_phases = bs.lwe_phase(lwe, bs.flatten_key(c["z"]), bits)
    assert np.array_equal(lwe_phases, phases)                                 # extraction moves the phase, nothing else
    print(f"err 2^{np.log2(max(err, 1)):.1f} bound 2^{np.log2(bound):.1f}")
    assert err <= bound
