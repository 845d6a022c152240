"""The random layer at far positions and launch edges, every word against the integer model
(tests/csprng_model.py) bit for bit.  tests/test_gpu_csprng.py stays at the bottom of the stream; here every sampler crosses
the carry of its OWN block counter into state word 13, runs at a block counter with high bits in both words and ends at the
cap 2^64 - 2^20; rows and seeded ciphertexts start at first rows whose 64-bit index arithmetic passes 2^32 (the mask
stream's carry, the noise stream's carry, a row above 2^40, the cap), with body rows that straddle TUniform blocks, mask rows
as long as a wave's and a workgroup's span, and two body workgroups; and the calls are captured in a graph whose replays
outlive their RandSeed objects, and issued on two streams.  tests/test_csprng_model.py anchors the model at these indices."""
import gc

import numpy as np
import pytest

import csprng_model as cm
import tfhe_fft_model as m
from test_gpu_tfhe_fft import dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

KEY_A = bytes(range(32))
KEY_B = bytes((7 * i + 3) % 256 for i in range(32))
KEY_C = bytes((11 * i + 5) % 256 for i in range(32))
NONCE_HIGH = 0xfedcba9876543210
CAP = (1 << 64) - (1 << 20)                      # pfhe_csprng_device.hpp: kRandMaxIndex
BOTH = 0x89abcdef01234567                        # a block counter with high bits in both of its words
THREADS = 256                                    # a workgroup computes one block per thread, a wave 64 blocks


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


def guard_word(bits):
    return m.UINT[bits](-2 % (1 << bits))


def per_block(name, bits):
    """outputs one ChaCha block yields (§26): a stream word of the output's width, a u64 word, a bit, two bits"""
    return {"keystream": 16, "uniform": 64 // (bits // 8), "tuniform": 8, "binary": 512, "ternary": 256}[name]


def flat_model(name, key, nonce, offset, n, bits, b):
    if name == "keystream":
        return cm.keystream(key, nonce, offset, n)
    if name == "tuniform":
        return cm.tuniform(key, nonce, offset, b, n, bits)
    return getattr(cm, name)(key, nonce, offset, n, bits)


def flat_device(p, name, seed, offset, out, b, stream=None):
    if name == "keystream":
        p.csprng_keystream_dev(seed, offset, out, stream=stream)
    elif name == "tuniform":
        p.torus_tuniform_dev(seed, offset, b, out, stream=stream)
    else:
        getattr(p, "torus_%s_dev" % name)(seed, offset, out, stream=stream)


# the four flat samplers of each width and the keystream under its own name; TUniform at both ends of its bound
FLAT_CASES = [(32, "keystream", None)] + [(bits, name, b) for bits in (32, 64) for name, b in
                                          (("uniform", None), ("binary", None), ("ternary", None), ("tuniform", 0),
                                           ("tuniform", "max"))]
flat_cases = pytest.mark.parametrize("bits, name, b", FLAT_CASES, ids=lambda v: str(v))


def flat_against_the_model(p, name, bits, b, seed, key, nonce, offset, n):
    """outputs [offset, offset + n) into a buffer with guard words behind them; returns the device's tensor of n + 8 words"""
    out = empty(bits, n + 8, fill=-2)
    flat_device(p, name, seed, offset, out[:n], b)
    got = host_words(out, bits)
    assert np.array_equal(got[:n], flat_model(name, key, nonce, offset, n, bits, b)), (name, bits, offset, n)
    assert np.all(got[n:] == guard_word(bits)), (name, bits, offset, n)
    return out


# ---------------- the flat samplers ----------------

@flat_cases
def test_flat_samplers_cross_the_carry_of_their_own_block_counter(p, bits, name, b):
    """offset (2^32 - 1) per + per - 3: the last three outputs of block 2^32 - 1, then block 2^32, whose counter has state
    word 12 = 0 and word 13 = 1; the longest range is more than a workgroup's blocks, all but the first past the carry"""
    b = bits - 2 if b == "max" else b
    per = per_block(name, bits)
    offset = ((1 << 32) - 1) * per + per - 3
    seed = p.RandSeed(KEY_B, NONCE_HIGH)
    for n in (1, 7, 40, 3 * 256 * per + 5):
        first_block, last_block = offset // per, (offset + n - 1) // per
        assert first_block == (1 << 32) - 1
        if n == 1:
            assert last_block == first_block                       # the one output below the carry
        else:
            assert first_block < 2 ** 32 <= last_block
        if n > 40:
            assert last_block - first_block + 1 > 3 * THREADS
        flat_against_the_model(p, name, bits, b, seed, KEY_B, NONCE_HIGH, offset, n)


@flat_cases
def test_flat_samplers_at_a_counter_with_high_bits_in_both_words(p, bits, name, b):
    b = bits - 2 if b == "max" else b
    per, n = per_block(name, bits), 1000
    block = BOTH % ((CAP - n - 5) // per)                          # reduced so that the range ends below the cap
    offset = block * per + 5
    assert offset + n <= CAP and offset // per == block
    assert block >> 32 >= 1 << 16 and (block & 0xffffffff) >= 1 << 16
    flat_against_the_model(p, name, bits, b, p.RandSeed(KEY_A, NONCE_HIGH), KEY_A, NONCE_HIGH, offset, n)


@flat_cases
def test_flat_samplers_end_at_the_cap_and_one_more_is_refused(p, bits, name, b):
    """the last output index of a call may be 2^64 - 2^20 - 1, at lengths of one output, a few blocks and many workgroups;
    the same range from an offset one higher is refused; the longest range written in two calls cut at an odd index is the
    same words (launch independence at the cap)"""
    import torch
    b = bits - 2 if b == "max" else b
    per = per_block(name, bits)
    seed = p.RandSeed(KEY_B, 3)
    for n in (1, 1000, (1 << 19) + 3):
        offset = CAP - n
        assert offset + n == CAP and (offset + n - 1) // per == (CAP - 1) // per == CAP // per - 1
        whole = flat_against_the_model(p, name, bits, b, seed, KEY_B, 3, offset, n)
        refused = empty(bits, n, fill=-2)
        with pytest.raises(p.PfheError) as e:
            flat_device(p, name, seed, offset + 1, refused, b)
        assert e.value.kind == "BadLength" and "2^64 - 2^20" in str(e.value)
        assert bool((refused == -2).all())
    cut = 262145 + 1000
    assert cut % 2 == 1 and 0 < cut < n and (offset + cut) % per != 0     # an odd index, inside a block
    halves = empty(bits, n + 8, fill=-2)
    flat_device(p, name, seed, offset + cut, halves[cut:n], b)
    flat_device(p, name, seed, offset, halves[:cut], b)
    assert torch.equal(halves, whole)


# ---------------- rows ----------------

def rows_against_the_model(p, bits, mask_len, body_len, first, rows, b, rng, expand_on_host=False):
    """tfhe_fill_rows_dev stored and added and seeded_expand_dev at one shape against cm.fill_rows, each into a buffer with
    guard words behind it; returns the stored rows as the device wrote them"""
    mask, noise = p.RandSeed(KEY_A, NONCE_HIGH), p.RandSeed(KEY_B, 5)
    pitch = mask_len + body_len
    tag = (bits, mask_len, body_len, first, rows)
    want = cm.fill_rows(KEY_A, NONCE_HIGH, KEY_B, 5, first, mask_len, body_len, b, rows, bits)
    out = empty(bits, rows * pitch + 3, fill=-2)
    p.tfhe_fill_rows_dev(mask, noise, first, mask_len, body_len, b, out[:rows * pitch])
    got = host_words(out, bits)
    assert np.array_equal(got[:rows * pitch], want.reshape(-1)), tag
    assert np.all(got[rows * pitch:] == guard_word(bits)), tag
    base = rand_words(rng, bits, rows * pitch)
    d = dev_words(np.concatenate([base, np.full(3, guard_word(bits))]), bits)
    p.tfhe_fill_rows_dev(mask, noise, first, mask_len, body_len, b, d[:rows * pitch], add=True)
    added = cm.fill_rows(KEY_A, NONCE_HIGH, KEY_B, 5, first, mask_len, body_len, b, rows, bits, into=base)
    assert np.array_equal(host_words(d, bits)[:rows * pitch], added.reshape(-1)), tag
    assert np.all(host_words(d, bits)[rows * pitch:] == guard_word(bits)), tag
    bodies = rand_words(rng, bits, rows * body_len)
    expanded = want.copy()
    expanded[:, mask_len:] = bodies.reshape(rows, body_len)
    out = empty(bits, rows * pitch + 3, fill=-2)
    p.seeded_expand_dev(mask, first, mask_len, body_len, dev_words(bodies, bits), out[:rows * pitch])
    assert np.array_equal(host_words(out, bits)[:rows * pitch], expanded.reshape(-1)), tag
    assert np.all(host_words(out, bits)[rows * pitch:] == guard_word(bits)), tag
    if expand_on_host:
        host = np.zeros(rows * pitch, m.UINT[bits])
        p.seeded_expand(mask, first, mask_len, body_len, bodies, host)
        assert np.array_equal(host, expanded.reshape(-1)), tag
    return got[:rows * pitch].reshape(rows, pitch)


@pytest.mark.parametrize("bits", [32, 64])
def test_rows_at_shapes_that_straddle_blocks_waves_and_workgroups(p, bits):
    """body_len in {3, 9, 13}: body rows straddle the 8 outputs of a TUniform block; mask_len at a wave's span (64 blocks of
    uniform outputs) and one to each side of it, and above a workgroup's span; a GLWE-shaped row (128, 64) at 40 rows, whose
    bodies take two workgroups; rows in {1, 5, 41}"""
    uniform = per_block("uniform", bits)
    span, group = 64 * uniform, THREADS * uniform
    assert (span, group) == {32: (1024, 4096), 64: (512, 2048)}[bits]
    shapes = [(7, 3), (16, 9), (24, 13), (span - 1, 1), (span, 3), (span + 1, 1), (group + 1, 9)]
    assert {s[1] % 8 for s in shapes} >= {3, 1, 5}
    rng = np.random.default_rng(500 + bits)
    for mask_len, body_len in shapes:
        for rows in (1, 5, 41):
            rows_against_the_model(p, bits, mask_len, body_len, 3, rows, 17, rng)
    rows = 40
    assert (rows * 64 + 7) // 8 > THREADS                             # more body blocks than one workgroup computes
    for first in (0, 3):
        rows_against_the_model(p, bits, 128, 64, first, rows, bits - 2, rng, expand_on_host=first == 3)


FAR_SHAPES = [(630, 1), (7, 3), (128, 64)]
FAR_ROWS = 5


def far_first_rows(bits, mask_len, body_len, rows):
    """the first rows at which the 64-bit index arithmetic of the row kernels passes 2^32, each with what it is chosen for
    asserted: {name: first_row}"""
    uniform, noise, longest = per_block("uniform", bits), per_block("tuniform", bits), max(mask_len, body_len)
    blocks = lambda first, length, per: (first * length // per, ((first + rows) * length - 1) // per)
    far = {}
    far["mask carry"] = (2 ** 32 * uniform) // mask_len - 2
    lo, hi = blocks(far["mask carry"], mask_len, uniform)
    assert lo < 2 ** 32 <= hi
    far["noise carry"] = (2 ** 32 * noise) // body_len - 2
    lo, hi = blocks(far["noise carry"], body_len, noise)
    assert lo < 2 ** 32 <= hi and (body_len > 1 or far["noise carry"] == 2 ** 35 - 2)
    far["above 2^40"] = (1 << 40) + 12345
    assert far["above 2^40"] > 2 ** 40 and blocks(far["above 2^40"], body_len, noise)[0] > 2 ** 32
    far["cap"] = CAP // longest - rows
    assert (far["cap"] + rows) * longest <= CAP < (far["cap"] + rows + 1) * longest
    return far


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("mask_len, body_len", FAR_SHAPES)
def test_rows_at_far_first_rows(p, bits, mask_len, body_len):
    """five rows straddling the mask stream's counter carry, the noise stream's, from a row above 2^40 and ending at the cap
    (one row further is refused); rows [a, a + c) written alone at the far first row are that slice of the whole"""
    rng = np.random.default_rng(600 + bits + mask_len)
    mask, noise = p.RandSeed(KEY_A, NONCE_HIGH), p.RandSeed(KEY_B, 5)
    pitch = mask_len + body_len
    for name, first in far_first_rows(bits, mask_len, body_len, FAR_ROWS).items():
        b = bits - 2 if name == "cap" else 17
        whole = rows_against_the_model(p, bits, mask_len, body_len, first, FAR_ROWS, b, rng,
                                       expand_on_host=(mask_len, name) == (7, "mask carry"))
        for a, count in ((0, 1), (1, 3), (4, 1)):
            part = empty(bits, count * pitch)
            p.tfhe_fill_rows_dev(mask, noise, first + a, mask_len, body_len, b, part)
            assert np.array_equal(host_words(part, bits).reshape(count, pitch), whole[a:a + count]), (name, a, count)
    first = CAP // max(mask_len, body_len) - FAR_ROWS + 1
    out = empty(bits, FAR_ROWS * pitch, fill=-2)
    with pytest.raises(p.PfheError) as e:
        p.tfhe_fill_rows_dev(mask, noise, first, mask_len, body_len, 3, out)
    assert e.value.kind == "BadLength" and "2^64 - 2^20" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.seeded_expand_dev(mask, CAP // mask_len - FAR_ROWS + 1, mask_len, body_len, empty(bits, FAR_ROWS * body_len), out)
    assert e.value.kind == "BadLength"
    assert bool((out == -2).all())


# ---------------- seeded encryption ----------------

def seeded_bodies(mask_key, mask_nonce, noise_key, noise_nonce, first, key, b, msgs, bits):
    """bodies[r] = msgs[r] + <mask(R), key> + noise(R) modulo 2^bits in Python integers, the randomness from cm.fill_rows"""
    dim, rows = len(key), len(msgs)
    rand = cm.fill_rows(mask_key, mask_nonce, noise_key, noise_nonce, first, dim, 1, b, rows, bits)
    secret = [int(s) for s in key]
    return [(int(msgs[r]) + int(rand[r, dim]) + sum(int(a) * s for a, s in zip(rand[r, :dim], secret))) % (1 << bits)
            for r in range(rows)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("dim", [1, 17, 630, 1025])
def test_seeded_encryption_at_far_first_rows(p, bits, dim):
    """the fused call against plain integers and against tfhe_fill_rows_dev(add) + lwe_encrypt_dev, at first rows where
    row / 8 crosses 2^32 (the noise block), row n / per crosses 2^32 (the mask blocks), row > 2^40 and (first_row + rows) n
    is the cap; rows 5 and 9 leave a last workgroup of four waves partial; b at both ends; the key is random words"""
    rng = np.random.default_rng(700 + bits + dim)
    mask, noise = p.RandSeed(KEY_B, NONCE_HIGH), p.RandSeed(KEY_A, 9)
    key = rand_words(rng, bits, dim)
    d_key = dev_words(key, bits)
    for rows, b in ((5, 0), (9, bits - 2)):
        assert rows % 4 == 1
        for name, first in far_first_rows(bits, dim, 1, rows).items():
            if name == "noise carry":
                assert first // 8 < 2 ** 32 <= (first + rows - 1) // 8
            msgs = rand_words(rng, bits, rows)
            want = seeded_bodies(KEY_B, NONCE_HIGH, KEY_A, 9, first, key, b, msgs, bits)
            bodies = dev_words(np.concatenate([msgs, np.full(3, guard_word(bits))]), bits)
            p.lwe_encrypt_seeded_dev(mask, noise, first, d_key, b, bodies[:rows])
            got = host_words(bodies, bits)
            assert [int(v) for v in got[:rows]] == want, (name, rows, first)
            assert np.all(got[rows:] == guard_word(bits)), (name, rows)
            full = np.zeros((rows, dim + 1), m.UINT[bits])
            full[:, dim] = msgs
            d_full = dev_words(full.reshape(-1), bits)
            p.tfhe_fill_rows_dev(mask, noise, first, dim, 1, b, d_full, add=True)
            p.lwe_encrypt_dev(d_full, d_key)
            assert np.array_equal(host_words(d_full, bits).reshape(rows, dim + 1)[:, dim], got[:rows]), (name, rows)
            if (name, rows) == ("cap", 9):
                host = msgs.copy()
                p.lwe_encrypt_seeded(mask, noise, first, key, b, host)
                assert [int(v) for v in host] == want
                with pytest.raises(p.PfheError) as e:
                    p.lwe_encrypt_seeded_dev(mask, noise, first + 1, d_key, b, bodies[:rows])
                assert e.value.kind == "BadLength"
                assert np.array_equal(host_words(bodies, bits), got)


def test_seeded_bodies_helper_on_a_case_by_hand():
    """the helper the device is held against, on one row written out"""
    first, b, bits = 11, 6, 32
    key, msgs = np.array([3, 0xfffffffe], np.uint32), np.array([5], np.uint32)
    a = cm.keystream(KEY_A, 4, first * 2, 2)
    e = cm.tuniform(KEY_B, 4, first, b, 1, bits)
    assert seeded_bodies(KEY_A, 4, KEY_B, 4, first, key, b, msgs, bits) == \
        [(5 + int(e[0]) + 3 * int(a[0]) + 0xfffffffe * int(a[1])) % 2 ** 32]


# ---------------- capture and streams ----------------

def issue_all(p, bits, seeds, bufs, first, stream=None):
    """the four calls of the capture test, on `stream`"""
    mask, noise = seeds
    rows_out, bodies, key, expanded, flat = bufs
    p.tfhe_fill_rows_dev(mask, noise, first, 7, 3, 17, rows_out, stream=stream)
    p.lwe_encrypt_seeded_dev(mask, noise, first, key, 17, bodies, stream=stream)
    p.seeded_expand_dev(mask, first, 7, 3, rows_out[:15], expanded, stream=stream)
    p.torus_ternary_dev(noise, first * 256 + 5, flat, stream=stream)


def all_from_the_model(bits, first, key):
    rows = cm.fill_rows(KEY_A, NONCE_HIGH, KEY_B, 5, first, 7, 3, 17, 5, bits)
    bodies = seeded_bodies(KEY_A, NONCE_HIGH, KEY_B, 5, first, key, 17, np.zeros(9, m.UINT[bits]), bits)
    expanded = rows.copy()
    expanded[:, 7:] = rows.reshape(-1)[:15].reshape(5, 3)
    return rows.reshape(-1), np.array(bodies, dtype=np.uint64).astype(m.UINT[bits]), expanded.reshape(-1), \
        cm.ternary(KEY_B, 5, first * 256 + 5, 1000, bits)


def buffers(bits, key):
    return (empty(bits, 50, fill=0), empty(bits, 9, fill=0), dev_words(key, bits), empty(bits, 50, fill=0),
            empty(bits, 1000, fill=0))


@pytest.mark.parametrize("bits", [32, 64])
def test_a_captured_graph_replays_the_eager_words_after_its_seeds_are_gone(p, bits):
    """tfhe_fill_rows_dev, lwe_encrypt_seeded_dev, seeded_expand_dev and a flat sampler captured in one graph on a side
    stream at a first row past the counter carry.  A seed is read at the call and lives in the kernel arguments: the RandSeed
    objects are deleted and collected and fresh ones of other keys allocated, and each of two replays on zeroed outputs
    still equals the eager words, which equal the model's"""
    import torch
    first = (1 << 35) + 3
    key = rand_words(np.random.default_rng(800 + bits), bits, 37)
    want = all_from_the_model(bits, first, key)
    seeds = [p.RandSeed(KEY_A, NONCE_HIGH), p.RandSeed(KEY_B, 5)]
    eager = buffers(bits, key)
    issue_all(p, bits, seeds, eager, first)
    torch.cuda.synchronize()
    outputs = lambda bufs: (bufs[0], bufs[1], bufs[3], bufs[4])
    for got, words in zip(outputs(eager), want):
        assert np.array_equal(host_words(got, bits), words)
    bufs = buffers(bits, key)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            issue_all(p, bits, seeds, bufs, first, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    del seeds[:]
    gc.collect()
    others = [p.RandSeed(KEY_C, 1 + i) for i in range(8)]              # fresh seeds where the old ones may have been
    for _ in range(2):
        for out in outputs(bufs):
            out.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, ref in zip(outputs(bufs), outputs(eager)):
            assert torch.equal(got, ref)
    assert len(others) == 8


@pytest.mark.parametrize("bits", [32, 64])
def test_the_calls_give_the_same_words_on_two_streams_in_turn(p, bits):
    import torch
    first = (1 << 40) + 7
    key = rand_words(np.random.default_rng(900 + bits), bits, 37)
    want = all_from_the_model(bits, first, key)
    seeds = [p.RandSeed(KEY_A, NONCE_HIGH), p.RandSeed(KEY_B, 5)]
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            bufs = buffers(bits, key)
            issue_all(p, bits, seeds, bufs, first, stream=s)
        s.synchronize()
        for got, words in zip((bufs[0], bufs[1], bufs[3], bufs[4]), want):
            assert np.array_equal(host_words(got, bits), words)
