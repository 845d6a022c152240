"""GPU parity of the random layer (pfhe_csprng_keystream_dev, pfhe_rand{,32}_*): every word the device writes against the
integer model (tests/csprng_model.py) bit for bit, the fused seeded encryption against the composition of public calls word
for word, the seeded key-switch key against the unseeded call on the same randomness, and a bootstrap under keys and inputs
drawn through this layer alone, decoded within the worst-case bound with |e| <= 2^b."""
import numpy as np
import pytest

import csprng_model as cm
import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg
from test_gpu_tfhe_fft import dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

KEY_A = bytes(range(32))
KEY_B = bytes((7 * i + 3) % 256 for i in range(32))
NONCE_HIGH = 0xfedcba9876543210          # bits set in both nonce words
CARRY = ((1 << 32) - 1) * 16 + 5         # a word offset inside block 2^32 - 1: the next block carries into state word 13


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


def empty(bits, n, fill=None):
    import torch
    dtype = torch.int32 if bits == 32 else torch.int64
    return torch.empty(n, dtype=dtype, device="cuda") if fill is None else torch.full((n,), fill, dtype=dtype, device="cuda")


# ---------------- the stream ----------------

@pytest.mark.parametrize("offset", [0, 5, CARRY])
def test_keystream_matches_the_model(p, offset):
    """a range that starts and ends inside a block, one block, two, and more than a workgroup's; past the output nothing is
    written"""
    for key, nonce in ((KEY_A, 0), (KEY_B, NONCE_HIGH), (KEY_A, 1 << 63)):
        seed = p.RandSeed(key, nonce)
        for n in (1, 15, 16, 17, 1000):
            out = empty(32, n + 8, fill=-2)
            p.csprng_keystream_dev(seed, offset, out[:n])
            got = host_words(out, 32)
            assert np.array_equal(got[:n], cm.keystream(key, nonce, offset, n)), (nonce, n)
            assert np.all(got[n:] == np.uint32(0xfffffffe)), (nonce, n)


def test_keystream_is_rfc_8439s_block(p):
    """RFC 8439 §2.3.2 through the device: its 32-bit counter 1 and 96-bit nonce are counter 1 | 0x09000000 << 32, nonce
    0x4a000000 here"""
    out = empty(32, 16)
    p.csprng_keystream_dev(p.RandSeed(KEY_A, 0x4a000000), (1 | 0x09000000 << 32) * 16, out)
    assert host_words(out, 32).tobytes()[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4"
    assert host_words(out, 32).tobytes()[-4:].hex() == "a2503c4e"


# ---------------- the samplers ----------------

def sample_model(name, key, nonce, offset, n, bits, b):
    if name == "tuniform":
        return cm.tuniform(key, nonce, offset, b, n, bits)
    return getattr(cm, name)(key, nonce, offset, n, bits)


def sample_device(p, name, seed, offset, out, b):
    if name == "tuniform":
        p.torus_tuniform_dev(seed, offset, b, out)
    else:
        getattr(p, "torus_%s_dev" % name)(seed, offset, out)


SAMPLER_CASES = [("uniform", None), ("binary", None), ("ternary", None), ("tuniform", 0), ("tuniform", 17), ("tuniform", "max")]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name, b", SAMPLER_CASES)
def test_samplers_match_the_model(p, bits, name, b):
    """offsets that are no multiple of 16 or 32 and lengths on both sides of a word of bits and of a block; the carry
    offset for the samplers that read whole words"""
    b = bits - 2 if b == "max" else b
    seed = p.RandSeed(KEY_B, NONCE_HIGH)
    for offset in (0, 5, 37, 1003, CARRY):
        for n in (1, 31, 33, 1000):
            out = empty(bits, n + 4, fill=-2)
            sample_device(p, name, seed, offset, out[:n], b)
            got = host_words(out, bits)
            assert np.array_equal(got[:n], sample_model(name, KEY_B, NONCE_HIGH, offset, n, bits, b)), (offset, n)
            assert np.all(got[n:] == m.UINT[bits](-2 % (1 << bits))), (offset, n)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name, b", [("uniform", None), ("binary", None), ("ternary", None), ("tuniform", 17)])
def test_samplers_beyond_one_workgroup(p, bits, name, b):
    """2^21 + 3 outputs from an odd offset: many workgroups.  Compared on a fixed 1 in 997 of the indices and on the first and
    last 64 outputs, so what is left out is stated here and not chosen by the code under test; the range written alone in two
    halves is the same words (launch independence)."""
    n, offset = (1 << 21) + 3, 12345
    seed = p.RandSeed(KEY_A, 3)
    out = empty(bits, n)
    sample_device(p, name, seed, offset, out, b)
    got = host_words(out, bits)
    want = sample_model(name, KEY_A, 3, offset, n, bits, b)
    at = np.concatenate([np.arange(64), np.arange(0, n, 997), np.arange(n - 64, n)])
    assert np.array_equal(got[at], want[at])
    halves = empty(bits, n)
    cut = 1000003
    sample_device(p, name, seed, offset + cut, halves[cut:], b)
    sample_device(p, name, seed, offset, halves[:cut], b)
    import torch
    assert torch.equal(halves, out)


# ---------------- rows ----------------

ROW_SHAPES = [(1, 1), (7, 1), (630, 1), (16, 8), (24, 8)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("mask_len, body_len", ROW_SHAPES)
def test_fill_rows_matches_the_model(p, bits, mask_len, body_len):
    """rows 1, 5 and 257 from a first row that puts both streams inside a block, stored and added; rows [a, a + b) written
    alone are that slice of rows [0, R)"""
    mask, noise = p.RandSeed(KEY_A, NONCE_HIGH), p.RandSeed(KEY_B, 5)
    b = 17
    pitch = mask_len + body_len
    rng = np.random.default_rng(bits + pitch)
    for rows in (1, 5, 257):
        for first in (0, 3):
            want = cm.fill_rows(KEY_A, NONCE_HIGH, KEY_B, 5, first, mask_len, body_len, b, rows, bits)
            out = empty(bits, rows * pitch + 3, fill=-2)
            p.tfhe_fill_rows_dev(mask, noise, first, mask_len, body_len, b, out[:rows * pitch])
            got = host_words(out, bits)
            assert np.array_equal(got[:rows * pitch], want.reshape(-1)), (rows, first)
            assert np.all(got[rows * pitch:] == m.UINT[bits](-2 % (1 << bits)))
            base = rand_words(rng, bits, rows * pitch)
            d = dev_words(base, bits)
            p.tfhe_fill_rows_dev(mask, noise, first, mask_len, body_len, b, d, add=True)
            added = cm.fill_rows(KEY_A, NONCE_HIGH, KEY_B, 5, first, mask_len, body_len, b, rows, bits, into=base)
            assert np.array_equal(host_words(d, bits), added.reshape(-1)), (rows, first)
    whole = empty(bits, 257 * pitch)
    p.tfhe_fill_rows_dev(mask, noise, 0, mask_len, body_len, b, whole)
    for a, count in ((0, 1), (100, 57), (256, 1)):
        part = empty(bits, count * pitch)
        p.tfhe_fill_rows_dev(mask, noise, a, mask_len, body_len, b, part)
        assert np.array_equal(host_words(part, bits), host_words(whole, bits)[a * pitch:(a + count) * pitch]), (a, count)


@pytest.mark.parametrize("bits", [32, 64])
def test_fill_rows_at_the_largest_bound_and_refusals(p, bits):
    mask, noise = p.RandSeed(KEY_A, 1), p.RandSeed(KEY_A, 2)       # one key, two nonces: two streams
    out = empty(bits, 5 * 9)
    p.tfhe_fill_rows_dev(mask, noise, 2, 8, 1, bits - 2, out)
    assert np.array_equal(host_words(out, bits), cm.fill_rows(KEY_A, 1, KEY_A, 2, 2, 8, 1, bits - 2, 5, bits).reshape(-1))
    with pytest.raises(p.PfheError) as e:
        p.tfhe_fill_rows_dev(mask, p.RandSeed(KEY_A, 1), 0, 8, 1, 3, out)
    assert e.value.kind == "BadArgument" and "differ" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.tfhe_fill_rows_dev(mask, noise, 0, 8, 1, bits - 1, out)
    assert e.value.kind == "BadArgument"
    with pytest.raises(p.PfheError) as e:
        p.tfhe_fill_rows_dev(mask, noise, 0, 7, 1, 3, out)           # 45 words are not rows of 8
    assert e.value.kind == "BadLength"


# ---------------- seeded ciphertexts ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("dim", [1, 17, 63, 64, 65, 630, 1025])
def test_seeded_encryption_is_fill_rows_then_encrypt(p, bits, dim):
    """bodies[r] += <mask(R), key> + noise(R) equals the body slot of tfhe_fill_rows_dev(add) + lwe_encrypt_dev word for word:
    one block per row, a row inside one block, rows that straddle blocks, more blocks than lanes (1025); keys are random
    words; the host form equals the device form"""
    mask, noise = p.RandSeed(KEY_B, NONCE_HIGH), p.RandSeed(KEY_A, 9)
    rng = np.random.default_rng(bits + dim)
    key = rand_words(rng, bits, dim)
    d_key = dev_words(key, bits)
    for rows, first, b in ((1, 0, 0), (5, 3, 17), (257, 1000, bits - 2)):
        msgs = rand_words(rng, bits, rows)
        full = np.zeros((rows, dim + 1), m.UINT[bits])
        full[:, dim] = msgs
        d_full = dev_words(full.reshape(-1), bits)
        p.tfhe_fill_rows_dev(mask, noise, first, dim, 1, b, d_full, add=True)
        p.lwe_encrypt_dev(d_full, d_key)
        want = host_words(d_full, bits).reshape(rows, dim + 1)
        bodies = dev_words(msgs, bits)
        p.lwe_encrypt_seeded_dev(mask, noise, first, d_key, b, bodies)
        assert np.array_equal(host_words(bodies, bits), want[:, dim]), (rows, first)
        host = msgs.copy()
        p.lwe_encrypt_seeded(mask, noise, first, key, b, host)
        assert np.array_equal(host, want[:, dim]), (rows, first)
        # the receiving side: the full ciphertexts from the mask seed and the bodies
        out = empty(bits, rows * (dim + 1), fill=-2)
        p.seeded_expand_dev(mask, first, dim, 1, bodies, out)
        assert np.array_equal(host_words(out, bits).reshape(rows, dim + 1), want), (rows, first)


@pytest.mark.parametrize("bits", [32, 64])
def test_seeded_encryption_against_the_model(p, bits):
    """the composition above is device against device; here the fused call against plain integers"""
    dim, rows, first, b = 37, 9, 11, 6
    mask, noise = p.RandSeed(KEY_A, 4), p.RandSeed(KEY_B, 4)
    rng = np.random.default_rng(bits)
    key, msgs = rand_words(rng, bits, dim), rand_words(rng, bits, rows)
    rand = cm.fill_rows(KEY_A, 4, KEY_B, 4, first, dim, 1, b, rows, bits)
    want = [(int(msgs[r]) + int(rand[r, dim]) + sum(int(a) * int(s) for a, s in zip(rand[r, :dim], key))) % (1 << bits)
            for r in range(rows)]
    bodies = dev_words(msgs, bits)
    p.lwe_encrypt_seeded_dev(mask, noise, first, dev_words(key, bits), b, bodies)
    assert [int(v) for v in host_words(bodies, bits)] == want


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("mask_len, body_len", ROW_SHAPES)
def test_seeded_expand_is_fill_rows_masks_with_the_bodies_in_place(p, bits, mask_len, body_len):
    mask, noise = p.RandSeed(KEY_A, 7), p.RandSeed(KEY_B, 7)
    pitch = mask_len + body_len
    rng = np.random.default_rng(bits + pitch)
    for rows, first in ((1, 0), (5, 2), (257, 40)):
        filled = empty(bits, rows * pitch)
        p.tfhe_fill_rows_dev(mask, noise, first, mask_len, body_len, 3, filled)
        want = host_words(filled, bits).reshape(rows, pitch).copy()
        bodies = rand_words(rng, bits, rows * body_len)
        want[:, mask_len:] = bodies.reshape(rows, body_len)
        out = empty(bits, rows * pitch + 2, fill=-2)
        p.seeded_expand_dev(mask, first, mask_len, body_len, dev_words(bodies, bits), out[:rows * pitch])
        got = host_words(out, bits)
        assert np.array_equal(got[:rows * pitch], want.reshape(-1)), (rows, first)
        assert np.all(got[rows * pitch:] == m.UINT[bits](-2 % (1 << bits)))
        host = np.zeros(rows * pitch, m.UINT[bits])
        p.seeded_expand(mask, first, mask_len, body_len, bodies, host)
        assert np.array_equal(host, want.reshape(-1)), (rows, first)
    buf = empty(bits, 4 * pitch)
    with pytest.raises(p.PfheError) as e:                              # the bodies inside the output
        p.seeded_expand_dev(mask, 0, mask_len, body_len, buf[pitch:pitch + 4 * body_len], buf)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)


# ---------------- keys ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("in_dim, out_dim", [(64, 7), (130, 33)])
def test_seeded_key_switch_key_expands_to_the_unseeded_key(p, bits, in_dim, out_dim):
    """tfhe_generate_ksk_seeded_dev + seeded_expand_dev equals tfhe_generate_ksk_dev on tfhe_fill_rows_dev's buffer bit for
    bit, at (in_dim * ell) words instead of in_dim * ell * (out_dim + 1); and the model's key on the model's randomness"""
    mask, noise = p.RandSeed(KEY_A, 21), p.RandSeed(KEY_B, 22)
    rng = np.random.default_rng(bits + in_dim)
    b = bits // 2
    for lb, ell in ((4, 6), (8, None)):
        basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
        rows = in_dim * mb.decompose_length
        s_in = rng.integers(0, 2, in_dim).astype(m.UINT[bits])
        s_out = rand_words(rng, bits, out_dim) if lb == 8 else rng.integers(0, 2, out_dim).astype(m.UINT[bits])
        d_in, d_out = dev_words(s_in, bits), dev_words(s_out, bits)
        unseeded = empty(bits, rows * (out_dim + 1))
        p.tfhe_fill_rows_dev(mask, noise, 5, out_dim, 1, b, unseeded)
        rand = host_words(unseeded, bits).copy()
        assert np.array_equal(rand, cm.fill_rows(KEY_A, 21, KEY_B, 22, 5, out_dim, 1, b, rows, bits).reshape(-1))
        p.tfhe_generate_ksk_dev(d_in, d_out, basis, unseeded)
        assert np.array_equal(host_words(unseeded, bits), kg.ksk(rand, s_in, s_out, mb))
        seeded = p.tfhe_generate_ksk_seeded_dev(mask, noise, d_in, d_out, basis, b, first_row=5)
        assert seeded.numel() == rows
        expanded = empty(bits, rows * (out_dim + 1))
        p.seeded_expand_dev(mask, 5, out_dim, 1, seeded, expanded)
        import torch
        assert torch.equal(expanded, unseeded), (lb, ell)


@pytest.mark.parametrize("bits", [32, 64])
def test_bootstrapping_key_from_fill_rows_matches_the_model(p, bits):
    """the `rand` argument of tfhe_generate_bsk_dev is GLWE rows (k*N, N): filled by one call, the generated key is the
    model's on the model's randomness, at the smallest shape of tests/test_gpu_tfhe_keygen.py"""
    log_n, n, k = 6, 12, 1
    lb, ell = {32: (7, 3), 64: (15, 2)}[bits]
    basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    fft = p.FullComplex64FftTable(log_n)
    shape = p.TfheKeyShape(fft, basis, n, k)
    rng = np.random.default_rng(bits)
    s = rng.integers(0, 2, n).astype(m.UINT[bits])
    z = rng.integers(0, 2, (k, 1 << log_n)).astype(m.UINT[bits])
    big_n, rows = 1 << log_n, n * (k + 1) * ell
    torus = empty(bits, shape.bsk_len())
    p.tfhe_fill_rows_dev(p.RandSeed(KEY_A, 1), p.RandSeed(KEY_B, 1), 0, k * big_n, big_n, bits // 2, torus)
    rand = cm.fill_rows(KEY_A, 1, KEY_B, 1, 0, k * big_n, big_n, bits // 2, rows, bits).reshape(-1)
    assert np.array_equal(host_words(torus, bits), rand)
    p.tfhe_generate_bsk_dev(shape, dev_words(s, bits), dev_words(z.reshape(-1), bits), torus)
    assert np.array_equal(host_words(torus, bits), kg.bsk(rand, s, z, mb, log_n, k, 0))


# ---------------- end to end ----------------

@pytest.mark.parametrize("case", kg.NOISY_CASES[:2], ids=lambda c: "u%d-N%d-k%d-n%d" % (c[0], 1 << c[1], c[2], c[3]))
def test_bootstrap_under_keys_and_inputs_drawn_through_this_layer(p, case):
    """The first two shapes of test_noisy_bootstrap_decodes_on_the_device with nothing from numpy's or torch's generators:
    binary keys from torus_binary_dev, the bootstrapping key from tfhe_fill_rows_dev + tfhe_generate_bsk_dev, the key-switch
    key seeded and expanded, the inputs seeded ciphertexts, expanded.  TUniform(b) with 2^b that test's noise makes
    |e| <= 2^b hard, so tfhe_keygen_model.noise_bound(..., 2^b) is a worst case and not a statistical one.  Asserted: the
    phase errors of the fresh ciphertexts lie in [-2^b, 2^b] and take both signs; conditions (a) to (d) of that test."""
    import torch
    from test_gpu_tfhe_keygen import product_model_error
    bits, log_n, k, n, lb, ell, g, pbits, noise = case
    assert g == 0
    b = noise.bit_length() - 1
    assert 1 << b == noise
    big_n = 1 << log_n
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *kg.KS_BASIS)
    mb, mks = m.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, *kg.KS_BASIS)
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis)
    secret, public = p.RandSeed(KEY_A, 100), p.RandSeed(KEY_B, 200)      # the keys and all noise; the masks
    s, z = empty(bits, n), empty(bits, k * big_n)
    p.torus_binary_dev(secret.with_nonce(101), 0, s)
    p.torus_binary_dev(secret.with_nonce(102), 0, z)
    s_host, z_host = host_words(s, bits), host_words(z, bits).reshape(k, big_n)
    assert set(np.unique(s_host)) <= {0, 1} and set(np.unique(z_host)) == {0, 1}
    # the bootstrapping key: rows of (k N, N)
    torus = empty(bits, ctx.bsk_len())
    p.tfhe_fill_rows_dev(public.with_nonce(201), secret.with_nonce(103), 0, k * big_n, big_n, b, torus)
    rand_bsk = host_words(torus, bits).copy()
    bsk = p.tfhe_generate_bsk_dev(ctx, s, z, torus)
    keys_torus = host_words(torus, bits).reshape(n, -1)
    assert np.array_equal(keys_torus.reshape(-1), kg.bsk(rand_bsk, s_host, z_host, mb, log_n, k, 0))
    # the key-switch key: seeded, then expanded as the receiving side would
    seeded = p.tfhe_generate_ksk_seeded_dev(public.with_nonce(202), secret.with_nonce(104), z, s, ks_basis, b)
    ksk = empty(bits, ctx.ksk_len())
    p.seeded_expand_dev(public.with_nonce(202), 0, n, 1, seeded, ksk)
    assert seeded.numel() * (n + 1) == ksk.numel()
    # fresh ciphertexts: every p-bit message 16 times; the first two rounds are bootstrapped
    msgs = np.tile(np.arange(1 << pbits), 16)
    delta = 1 << (bits - pbits - 1)
    encoded = (msgs.astype(np.uint64) * np.uint64(delta)).astype(m.UINT[bits])
    bodies = dev_words(encoded, bits)
    p.lwe_encrypt_seeded_dev(public.with_nonce(203), secret.with_nonce(105), 0, s, b, bodies)
    lwe = empty(bits, len(msgs) * (n + 1))
    p.seeded_expand_dev(public.with_nonce(203), 0, n, 1, bodies, lwe)
    fresh = lwe.clone()
    p.lwe_phase_dev(fresh, s)
    diff = host_words(fresh, bits).reshape(-1, n + 1)[:, n] - encoded          # unsigned words: the difference wraps
    e = [int(v) - (1 << bits) if int(v) >> (bits - 1) else int(v) for v in diff]
    assert all(-(1 << b) <= int(v) <= (1 << b) for v in e), "a fresh phase error outside [-2^b, 2^b]"
    assert any(int(v) < 0 for v in e) and any(int(v) > 0 for v in e)
    count = 2 << pbits
    bound = kg.noise_bound(bits, log_n, k, n, lb, ell, 0, *kg.KS_BASIS, 1 << b)
    assert (n + 1) / 2 < big_n / 2 ** (pbits + 1)                                            # (a)
    assert bound < 2.0 ** (bits - pbits - 2)                                                 # (b)
    tv = bs.lut_test_vector(bs.lut(pbits), pbits, bits, log_n, k)
    out = empty(bits, count * (n + 1), fill=0)
    p.tfhe_bootstrap_dev(lwe[:count * (n + 1)], bsk, dev_words(tv, bits), ksk, out, ctx)
    p.lwe_phase_dev(out, s)
    phases = host_words(out, bits).reshape(-1, n + 1)[:, n]
    err = kg.phase_error(phases, msgs[:count], pbits, bits)
    model_err = product_model_error({"basis": mb}, keys_torus, bits, log_n, k, 0, np.random.default_rng(bits))
    allowed = bound + n * (1 + k * big_n) * (4 * model_err + 2)
    print("bits %d: fresh |e| max %d of 2^%d, err 2^%.1f bound 2^%.1f allowed 2^%.1f Delta/2 2^%d"
          % (bits, max(abs(int(v)) for v in e), b, np.log2(max(err, 1)), np.log2(bound), np.log2(allowed), bits - pbits - 2))
    assert bs.decode(phases, pbits, bits) == [bs.lut(pbits)(int(v)) for v in msgs[:count]]   # (c)
    assert err <= allowed                                                                    # (d)
    assert mks.decompose_length * k * big_n == seeded.numel()
