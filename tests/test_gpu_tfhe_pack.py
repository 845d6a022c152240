"""GPU parity of packing (include/pfhe.h, pfhe_tfhe{,32}_pack_keyswitch*, _pksk_generate_dev, _sample_extract_first_few*,
_multimsg_extract*): every call bit for bit against the integer model (tests/tfhe_pack_model.py), then the round trip on
noisy keys, all on the device, decoded within the derived bound.

The packing key switch's kernel (csrc/pfhe_pack.hip) has these edges, and PACK_CASES names the case that takes each:
  - U = 2 at N = 2 and U = 4 from N = 4 on; a tile of T = min(N, 256) coefficients: N = 4 and 64 leave lanes of every wave
    without coefficients, N = 256 is exactly one tile, N = 1024 is four tiles per component;
  - the ciphertexts of a group are walked in blocks of J = min(count rounded up to U, 1024, 4096 / ell rounded down to U):
    one block (most cases), several whole blocks ("blocks"), a partial last block ("partial block"); count no multiple of U
    pads the last U-step with zero digits (count 1, 2, 5, N - 1);
  - a window of T + J <= 320 words is staged four key rows side by side, one row per wave, a longer one a row at a time
    with the block's ciphertexts split over the four waves: 320 ("window320") and 324 ("window324") are the two sides,
    "partial block" takes both in one call (blocks of 204 and 52 ciphertexts), and the rows of a group are no multiple of
    four in "n2-count1" (15) and "n4-count3" (99); split over the waves, fewer than 4 U ciphertexts would leave waves idle
    and 1024 give every wave 256;
  - the mask words are decomposed in groups of ki = 4096 / (ell J): one group (count and in_dimension small), a partial
    last group ("partial group": ki = 21, in_dimension 33), one mask word per group (count = N = 1024);
  - grid.y holds 65535 groups: "grid" runs 65538.
"""
import zlib

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_keygen_model as kg
import tfhe_pack_model as pm
from test_gpu_tfhe_fft import dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


_TABLES = {}


def table(p, log_n):
    if log_n not in _TABLES:
        _TABLES[log_n] = p.FullComplex64FftTable(log_n)
    return _TABLES[log_n]


def pack_inputs(rng, bits, log_n, k, n, lb, ell, count, batch):
    """full-range random key words; random ciphertexts with the basis's digit edge words spread over the masks"""
    big_n = 1 << log_n
    basis = m.ApproxSignedBasis(bits, lb, ell)
    pksk = rand_words(rng, bits, n * basis.decompose_length * (k + 1) * big_n)
    lwe = rand_words(rng, bits, batch * count * (n + 1)).reshape(batch * count, n + 1)
    edges = ew.edge_words(bits, lb, ell)
    at = rng.permutation(batch * count * n)[:min(batch * count * n, 2 * edges.size)]
    lwe[at // n, at % n] = rng.permutation(np.tile(edges, 2))[:at.size]
    return basis, pksk, lwe.reshape(-1)


def device_pack(p, lwe, pksk, bits, log_n, k, n, count, batch, basis, stream=None):
    import torch
    d_out = torch.full((batch * (k + 1) << log_n,), -1, dtype=getattr(torch, "int%d" % bits), device="cuda")  # uninitialised
    p.lwe_pack_keyswitch_dev(dev_words(lwe, bits), dev_words(pksk, bits), d_out, n, count, table(p, log_n),
                             p.ApproxSignedBasis(bits, basis.log_basis, basis.decompose_length), k, stream=stream)
    return d_out


# (id, bits, log_n, k, in_dimension, log_basis, ell (None: the full length), count, batch)
PACK_CASES = [
    ("n2-count1", 32, 1, 1, 5, 4, 3, 1, 3),
    ("n2-count2", 64, 1, 2, 5, 15, None, 2, 3),
    ("n4-count3", 32, 2, 1, 33, 7, 3, 3, 1),
    ("n4-count4-logb1", 64, 2, 2, 5, 1, 9, 4, 3),
    ("n64-count5", 32, 6, 2, 33, 4, None, 5, 3),
    ("n64-count63", 64, 6, 1, 5, 8, 8, 63, 1),
    ("n64-count64-partial-group", 32, 6, 1, 33, 4, 3, 64, 3),
    ("partial-group", 64, 6, 1, 33, 8, 6, 32, 1),
    ("n256-one-tile", 32, 8, 1, 5, 7, 3, 256, 1),
    ("blocks", 32, 8, 1, 3, 1, 32, 256, 1),
    ("partial-block", 32, 8, 2, 3, 1, 20, 255, 1),
    ("n1024-count1", 32, 10, 1, 33, 4, 3, 1, 3),
    ("n1024-count2", 64, 10, 1, 33, 15, 3, 2, 1),
    ("n1024-count64-window320", 32, 10, 1, 5, 4, 3, 64, 1),
    ("n1024-count65-window324", 64, 10, 1, 5, 15, 3, 65, 1),
    ("n1024-count1023", 32, 10, 1, 5, 7, 3, 1023, 1),
    ("n1024-count1024", 64, 10, 1, 5, 15, 2, 1024, 1),
    ("n1024-k2-count37", 32, 10, 2, 5, 4, None, 37, 3),
    ("n2048-two-blocks", 64, 11, 1, 2, 16, 2, 2048, 1),
]


@pytest.mark.parametrize("case", PACK_CASES, ids=[c[0] for c in PACK_CASES])
def test_pack_keyswitch_matches_the_model(p, case):
    """both widths, k = 1 and 2, N = 2, 4, 64, 256, 1024 (2048 for the second block of 1024 ciphertexts), count 1, 2, N - 1, N
    and values that are no multiple of 4, in_dimension 5 and 33, drop_bits 0 (ell None, or ell log_basis = BITS) and above,
    log_basis 1, batch 1 and 3: see the module docstring for the kernel edge each case takes"""
    _, bits, log_n, k, n, lb, ell, count, batch = case
    rng = np.random.default_rng(zlib.crc32(case[0].encode()))
    basis, pksk, lwe = pack_inputs(rng, bits, log_n, k, n, lb, ell, count, batch)
    want = pm.pack_keyswitch(lwe, pksk, n, count, basis, log_n, k)
    got = host_words(device_pack(p, lwe, pksk, bits, log_n, k, n, count, batch, basis), bits)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


@pytest.mark.parametrize("bits", [32, 64])
def test_pack_keyswitch_across_the_grid_boundary_and_repeated(p, bits):
    """"grid": 65538 groups at N = 2 are two launches (grid.y holds 65535); the groups repeat three distinct ones, so the
    result is the model's three, tiled: the batch size changes nothing.  A second call into the same output repeats it."""
    log_n, k, n, lb, ell, count, distinct = 1, 1, 3, 8, 2, 2, 3
    reps = 21846
    rng = np.random.default_rng(bits)
    basis, pksk, lwe = pack_inputs(rng, bits, log_n, k, n, lb, ell, count, distinct)
    want = np.tile(pm.pack_keyswitch(lwe, pksk, n, count, basis, log_n, k), reps)
    d_in, d_key = dev_words(np.tile(lwe, reps), bits), dev_words(pksk, bits)
    import torch
    d_out = torch.empty(want.size, dtype=d_in.dtype, device="cuda")
    for _ in range(2):
        p.lwe_pack_keyswitch_dev(d_in, d_key, d_out, n, count, table(p, log_n), p.ApproxSignedBasis(bits, lb, ell), k)
        assert np.array_equal(host_words(d_out, bits), want)


@pytest.mark.parametrize("bits", [32, 64])
def test_pack_host_form_and_a_call_queued_behind_its_producer(p, bits):
    """the host form at one shape; and on a non-default stream, the encryption that produces the input and the pack right
    behind it with no synchronisation in between"""
    import torch
    log_n, k, n, lb, ell, count, batch = 6, 1, 9, 4, 3, 7, 3
    rng = np.random.default_rng(bits + 1)
    basis, pksk, lwe = pack_inputs(rng, bits, log_n, k, n, lb, ell, count, batch)
    want = pm.pack_keyswitch(lwe, pksk, n, count, basis, log_n, k)
    fft, dev_basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    out = np.zeros(want.size, m.UINT[bits])
    p.lwe_pack_keyswitch(lwe, pksk, out, n, count, fft, dev_basis, k)
    assert np.array_equal(out, want)
    s = rand_words(rng, bits, n)
    encrypted = kg.lwe_body_mac(lwe, s, bits)
    want = pm.pack_keyswitch(encrypted, pksk, n, count, basis, log_n, k)
    d_in, d_s, d_key = dev_words(lwe, bits), dev_words(s, bits), dev_words(pksk, bits)
    d_out = torch.zeros(want.size, dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    p.lwe_encrypt_dev(d_in, d_s, stream=stream.cuda_stream)
    p.lwe_pack_keyswitch_dev(d_in, d_key, d_out, n, count, fft, dev_basis, k, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(host_words(d_out, bits), want)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("k", [1, 2])
def test_generate_pksk_matches_the_model_and_accumulates(p, bits, k):
    """word for word; a second call adds the body (and the message term) a second time, as the body calls document"""
    log_n, n, lb, ell = 5, 7, 6, 3
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rng = np.random.default_rng(bits + k)
    key_in = rand_words(rng, bits, n)                                          # any words, not only bits
    z = rand_words(rng, bits, k << log_n)
    rand = kg.glwe_randomness(rng, bits, log_n, k, n * ell, 1 << 10)
    want = pm.generate_pksk(rand, key_in, z.reshape(k, -1), basis, log_n, k)
    d = dev_words(rand, bits)
    args = (dev_words(key_in, bits), dev_words(z, bits), table(p, log_n), p.ApproxSignedBasis(bits, lb, ell), d, k)
    p.tfhe_generate_pksk_dev(*args)
    assert np.array_equal(host_words(d, bits), want)
    p.tfhe_generate_pksk_dev(*args)
    assert np.array_equal(host_words(d, bits), pm.generate_pksk(want, key_in, z.reshape(k, -1), basis, log_n, k))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n", [1, 10])
def test_multi_message_extraction_matches_the_model_and_sample_extraction(p, bits, log_n):
    """count 1 and N, k = 1 and 2, batch 3: the layout and its expansion against the model, and every expanded ciphertext
    against glwe_sample_extract_dev at its index"""
    import torch
    n = 1 << log_n
    rng = np.random.default_rng(bits + log_n)
    fft = table(p, log_n)
    for k, batch in ((1, 3), (2, 3)):
        glwe = rand_words(rng, bits, batch * (k + 1) * n)
        d_glwe = dev_words(glwe, bits)
        singles = {}
        d_one = torch.empty(batch * (k * n + 1), dtype=d_glwe.dtype, device="cuda")
        for h in sorted({0, 1, n // 2, n - 1}):
            p.glwe_sample_extract_dev(d_glwe, d_one, fft, k, h)
            singles[h] = host_words(d_one, bits).copy()
            assert np.array_equal(singles[h], bs.sample_extract(glwe, log_n, k, h))
        for count in (1, n):
            d_multi = torch.empty(batch * (k * n + count), dtype=d_glwe.dtype, device="cuda")
            p.glwe_sample_extract_first_few_dev(d_glwe, d_multi, fft, count, k)
            multi = host_words(d_multi, bits)
            assert np.array_equal(multi, pm.extract_first_few(glwe, log_n, k, count)), (k, count)
            d_lwe = torch.empty(batch * count * (k * n + 1), dtype=d_glwe.dtype, device="cuda")
            p.multimsg_lwe_extract_dev(d_multi, d_lwe, fft, count, k)
            lwe = host_words(d_lwe, bits)
            assert np.array_equal(lwe, pm.multimsg_extract(multi, log_n, k, count)), (k, count)
            rows = lwe.reshape(batch, count, k * n + 1)
            for h in range(count):                                             # the model's sample extraction at every index
                assert np.array_equal(rows[:, h].reshape(-1), bs.sample_extract(glwe, log_n, k, h)), (k, count, h)
            for h in (h for h in singles if h < count):                        # and the device's own
                assert np.array_equal(rows[:, h].reshape(-1), singles[h]), (k, count, h)


@pytest.mark.parametrize("bits", [32, 64])
def test_multi_message_host_forms(p, bits):
    log_n, k, count, batch = 4, 2, 5, 3
    n = 1 << log_n
    rng = np.random.default_rng(bits + 3)
    glwe = rand_words(rng, bits, batch * (k + 1) * n)
    multi = np.zeros(batch * (k * n + count), m.UINT[bits])
    p.glwe_sample_extract_first_few(glwe, multi, table(p, log_n), count, k)
    assert np.array_equal(multi, pm.extract_first_few(glwe, log_n, k, count))
    lwe = np.zeros(batch * count * (k * n + 1), m.UINT[bits])
    p.multimsg_lwe_extract(multi, lwe, table(p, log_n), count, k)
    assert np.array_equal(lwe, pm.multimsg_extract(multi, log_n, k, count))


@pytest.mark.parametrize("case", pm.NOISY_CASES, ids=lambda c: "u%d-logn%d-k%d-n%d-lb%d-ell%d-count%d" % c[:7])
def test_round_trip_on_noisy_keys(p, case):
    """All on the device: binary keys, torus_noise(bound=E) on every row of the packing key, noise-free inputs of p-bit
    messages; the key is generated, the inputs packed, the GLWE phase taken; then the first few extracted, expanded and their
    LWE phases taken under the flattened GLWE key.
      (1) bound = count n ell (B/2) E + n 2^(drop_bits-1) < Delta/2 = 2^(BITS-p-2);
      (2) every coefficient below count and every extracted phase decodes to its message;
      (3) the largest centred distance from Delta m is at most the bound.
    The arithmetic is exact, so the bound is derived, not measured."""
    import torch
    bits, log_n, k, n, lb, ell, count, noise, prec = case
    big_n = 1 << log_n
    bound = pm.noise_bound(bits, n, lb, ell, count, noise)
    assert bound < 2.0 ** (bits - prec - 2)
    c = pm.noisy_case(*case, seed=9, batch=3)
    batch, basis = c["batch"], p.ApproxSignedBasis(bits, lb, ell)
    fft = table(p, log_n)
    # the key's randomness: masks from the case, bodies from the device's own bounded noise
    rand = dev_words(c["rand_pksk"], bits).reshape(n * ell, k + 1, big_n)
    rand[:, k] = p.torus_noise(n * ell * big_n, bits, bound=noise).reshape(n * ell, big_n)
    assert int(rand[:, k].abs().max()) <= noise
    pksk = rand.reshape(-1).contiguous()
    d_z = dev_words(c["z"].reshape(-1), bits)
    p.tfhe_generate_pksk_dev(dev_words(c["s"], bits), d_z, fft, basis, pksk, k)
    packed = torch.empty(batch * (k + 1) * big_n, dtype=pksk.dtype, device="cuda")
    p.lwe_pack_keyswitch_dev(dev_words(c["lwe"], bits), pksk, packed, n, count, fft, basis, k)
    multi = torch.empty(batch * (k * big_n + count), dtype=pksk.dtype, device="cuda")
    p.glwe_sample_extract_first_few_dev(packed, multi, fft, count, k)
    lwe = torch.empty(batch * count * (k * big_n + 1), dtype=pksk.dtype, device="cuda")
    p.multimsg_lwe_extract_dev(multi, lwe, fft, count, k)
    p.lwe_phase_dev(lwe, d_z)
    lwe_phases = host_words(lwe, bits).reshape(batch * count, k * big_n + 1)[:, k * big_n]
    p.glwe_phase_dev(packed, d_z, fft, k)
    glwe_phases = host_words(packed, bits).reshape(batch, k + 1, big_n)[:, k, :count].reshape(-1)
    assert np.array_equal(lwe_phases, glwe_phases)
    assert bs.decode(glwe_phases, prec, bits) == list(c["msgs"]) and bs.decode(lwe_phases, prec, bits) == list(c["msgs"])
    err = pm.message_error(glwe_phases, c["msgs"], c["delta"], bits)
    print(f"{case}: err 2^{np.log2(max(err, 1)):.1f} bound 2^{np.log2(bound):.1f}")
    assert err <= bound
