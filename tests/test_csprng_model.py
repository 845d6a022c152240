"""The model of the random layer (tests/csprng_model.py) held against what it restates: the RFC 8439 §2.3.2 block, a keystream
written by openssl (tests/golden/chacha20_keystream.json, one case crossing block counter 2^32), the reference's binary and
ternary loops restated literally over the model's next_u32, the stated probabilities of TUniform by exhaustive
enumeration, and the array forms at far positions (a sampler's own counter carry, a counter with bits in both words, the last
legal index) against the block function and the sampler's rule on single outputs.  No GPU, no library."""
import json
import os
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import csprng_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32))

# RFC 8439 §2.3.2: key 00..1f, block counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00: the state after the block function
RFC_STATE = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574, 0x03020100, 0x07060504, 0x0b0a0908, 0x0f0e0d0c,
             0x13121110, 0x17161514, 0x1b1a1918, 0x1f1e1d1c, 0x00000001, 0x09000000, 0x4a000000, 0x00000000]
RFC_BLOCK = [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
             0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]


def test_block_function_is_rfc_8439s():
    assert cm.block_from_state(RFC_STATE) == RFC_BLOCK
    # the same block through the stream's layout: the RFC's 32-bit counter and 96-bit nonce are state words 12 and 13..15,
    # here the low and high halves of the 64-bit counter and the 64-bit nonce
    assert cm.block(KEY, 0x4a000000, 1 | 0x09000000 << 32) == RFC_BLOCK
    serial = b"".join(w.to_bytes(4, "little") for w in RFC_BLOCK)
    assert serial[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4"


def test_stream_is_openssls_keystream():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "chacha20_keystream.json")))
    assert len(doc["cases"]) >= 3
    crossed = False
    for case in doc["cases"]:
        want = np.frombuffer(bytes.fromhex(case["keystream"]), dtype="<u4")
        key, counter, nonce = bytes.fromhex(case["key"]), case["counter"], case["nonce"]
        assert case["iv"] == (counter.to_bytes(8, "little") + nonce.to_bytes(8, "little")).hex()
        got = cm.keystream(key, nonce, counter * 16, want.size)
        assert np.array_equal(got, want), case["name"]
        # any sub-range is the same words: the stream is addressed by position
        assert np.array_equal(cm.keystream(key, nonce, counter * 16 + 5, want.size - 7), want[5:-2])
        blocks = want.size // 16
        crossed |= (counter & cm.MASK32) + blocks - 1 > cm.MASK32
    assert crossed, "no case carries the block counter into state word 13"


def test_array_forms_are_the_scalar_rules():
    """blocks() is block() on many counters, across the carry into state word 13 and at the top of the counter; tuniform() is
    tuniform_value() on every word"""
    for first in (0, (1 << 32) - 2, (1 << 64) - 2, 0x123456789abcdef):
        got = cm.blocks(KEY, 0xfedcba9876543210, first, 4)
        for i in range(4):
            assert [int(w) for w in got[i]] == cm.block(KEY, 0xfedcba9876543210, first + i), (first, i)
    for bits in (32, 64):
        for b in (0, 17, bits - 2):
            words = cm.stream_u64(KEY, 9, 3, 50)
            want = [cm.tuniform_value(int(w), b, bits) for w in words]
            assert [int(v) for v in cm.tuniform(KEY, 9, 3, b, 50, bits)] == want


def test_generator_view_is_the_same_words():
    s = cm.Stream(KEY, 7, word_pos=13)
    words = cm.keystream(KEY, 7, 13, 8)
    assert [s.next_u32() for _ in range(4)] == [int(w) for w in words[:4]]
    assert s.next_u64() == int(words[4]) | int(words[5]) << 32
    assert int(cm.stream_u64(KEY, 7, 9, 1)[0]) == int(words[5]) | int(words[6]) << 32   # u64 word 9 = u32 words 18, 19


def reference_binary(length, rng, one=1):
    """sample_binary_values_to (primus_distr/src/common.rs:22-42), restated: chunks of 32 values per next_u32, low bit first,
    and one more word for the remainder (drawn even when the remainder is empty)"""
    s = [0, one]
    result = []
    for _ in range(length // 32):
        r = rng.next_u32()
        for _ in range(32):
            result.append(s[r & 1])
            r >>= 1
    r = rng.next_u32()
    for _ in range(length % 32):
        result.append(s[r & 1])
        r >>= 1
    return result


def reference_ternary(length, minus_one, rng):
    """sample_ternary_values_to (common.rs:56-76), restated: chunks of 16 values per next_u32, two bits each, low pair first"""
    s = [0, 0, 1, minus_one]
    result = []
    for _ in range(length // 16):
        r = rng.next_u32()
        for _ in range(16):
            result.append(s[r & 3])
            r >>= 2
    r = rng.next_u32()
    for _ in range(length % 16):
        result.append(s[r & 3])
        r >>= 2
    return result


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("length", [1, 31, 32, 33, 100, 515])
def test_binary_and_ternary_are_the_references_loops(bits, length):
    """on the same word stream from word 0 on; and from a later word, which is an offset that is a multiple of 32 / 16"""
    for start in (0, 3):
        got = cm.binary(KEY, 1, 32 * start, length, bits)
        assert got.dtype == (np.uint32 if bits == 32 else np.uint64)
        assert [int(v) for v in got] == reference_binary(length, cm.Stream(KEY, 1, start))
        got = cm.ternary(KEY, 1, 16 * start, length, bits)
        assert [int(v) for v in got] == reference_ternary(length, (1 << bits) - 1, cm.Stream(KEY, 1, start))
    # an offset inside a word continues that word: outputs [5, 5 + length) are that slice of outputs [0, 5 + length)
    assert np.array_equal(cm.binary(KEY, 1, 5, length, bits), cm.binary(KEY, 1, 0, 5 + length, bits)[5:])
    assert np.array_equal(cm.ternary(KEY, 1, 5, length, bits), cm.ternary(KEY, 1, 0, 5 + length, bits)[5:])


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("b", [0, 1, 2])
def test_tuniform_by_exhaustive_enumeration(bits, b):
    """every value of the b + 2 bits the rule reads, each equally likely: the support is [-2^b, 2^b], the two ends have
    probability 2^-(b+2), every other value 2^-(b+1), the mean is 0 and the variance (2^(2b+1) + 1) / 6; higher bits of the
    stream word change nothing"""
    total = 1 << (b + 2)
    signed = lambda v: v - (1 << bits) if v >> (bits - 1) else v
    counts = Counter(signed(cm.tuniform_value(r, b, bits)) for r in range(total))
    assert sorted(counts) == list(range(-(1 << b), (1 << b) + 1))
    for v, c in counts.items():
        want = Fraction(1, 1 << (b + 2)) if abs(v) == 1 << b else Fraction(1, 1 << (b + 1))
        assert Fraction(c, total) == want, (v, c)
    assert sum(v * c for v, c in counts.items()) == 0
    assert Fraction(sum(v * v * c for v, c in counts.items()), total) == Fraction((1 << (2 * b + 1)) + 1, 6)
    for r in range(total):
        assert cm.tuniform_value(r | 0xdeadbeef << (b + 2), b, bits) == cm.tuniform_value(r, b, bits)


@pytest.mark.parametrize("bits", [32, 64])
def test_tuniform_at_the_largest_bound(bits):
    """b = BITS - 2: r of all ones gives +2^b, r = 0 gives -2^b (r + 1 would not fit the word at 64 bits)"""
    b = bits - 2
    ones = (1 << (b + 2)) - 1
    assert cm.tuniform_value(ones, b, bits) == 1 << b
    assert cm.tuniform_value((1 << 64) - 1, b, bits) == 1 << b
    assert cm.tuniform_value(0, b, bits) == (1 << bits) - (1 << b)
    assert cm.tuniform_value(1, b, bits) == (1 << bits) - (1 << b) + 1
    with pytest.raises(AssertionError):
        cm.tuniform_value(0, b + 1, bits)


# ---- far positions: what tests/test_gpu_csprng_edges.py trusts the model at ----

NONCE = 0xfedcba9876543210
CAP = (1 << 64) - (1 << 20)                      # the largest output index a call may end at
BOTH = 0x89abcdef01234567                        # a block counter with bits set in both state words
PER = {("uniform", 32): 16, ("uniform", 64): 8, ("tuniform", 32): 8, ("tuniform", 64): 8, ("binary", 32): 512,
       ("binary", 64): 512, ("ternary", 32): 256, ("ternary", 64): 256}


def u32_word(j):
    """u32 stream word j from block() alone"""
    return cm.block(KEY, NONCE, j // 16)[j % 16]


def output_by_the_rule(name, i, bits, b):
    """output i of a sampler from block() and §26's rule, in Python integers; no array code of the model is used"""
    if name == "binary":
        return (u32_word(i // 32) >> (i % 32)) & 1
    if name == "ternary":
        return [0, 0, 1, (1 << bits) - 1][(u32_word(i // 16) >> (2 * (i % 16))) & 3]
    if name == "uniform" and bits == 32:
        return u32_word(i)
    word = u32_word(2 * i) | u32_word(2 * i + 1) << 32
    if name == "uniform":
        return word
    r = word & ((1 << (b + 2)) - 1)
    return ((r >> 1) + (r & 1) - (1 << b)) % (1 << bits)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["uniform", "binary", "ternary", "tuniform"])
def test_single_outputs_at_far_positions_follow_from_the_block_function(bits, name):
    """the array forms at the sampler's own counter carry, at a counter with bits in both words and at the last legal index
    are block() and the sampler's rule on one output each; Python integers carry the offsets and blocks() wraps the counter"""
    per = PER[name, bits]
    carry = ((1 << 32) - 1) * per + per - 3
    both = (BOTH % ((CAP - 8) // per)) * per + 5
    assert (both // per) >> 32 > 1 << 16 and ((both // per) & cm.MASK32) > 1 << 16
    for b in ((0, bits - 2) if name == "tuniform" else (None,)):
        sample = (lambda off, n: cm.tuniform(KEY, NONCE, off, b, n, bits)) if name == "tuniform" else \
                 (lambda off, n: getattr(cm, name)(KEY, NONCE, off, n, bits))
        for offset, n in ((carry, 7), (both, 3), (CAP - 3, 3)):
            got = sample(offset, n)
            assert got.dtype == (np.uint32 if bits == 32 else np.uint64) and got.size == n
            assert [int(v) for v in got] == [output_by_the_rule(name, offset + j, bits, b) for j in range(n)], (offset, b)
        assert carry // per == (1 << 32) - 1 and (carry + 6) // per == 1 << 32          # the seven outputs cross the carry
        # the last legal index, written out: output 2^64 - 2^20 - 1 sits in block (2^64 - 2^20 - 1) div per
        last = (1 << 64) - (1 << 20) - 1
        assert int(sample(last, 1)[0]) == output_by_the_rule(name, last, bits, b)
    if name == "uniform" and bits == 32:
        blk = cm.block(KEY, NONCE, (1 << 60) - (1 << 16) - 1)
        assert int(cm.uniform(KEY, NONCE, (1 << 64) - (1 << 20) - 1, 1, 32)[0]) == blk[15]
        assert u32_word(carry + 3) == cm.block(KEY, NONCE, 1 << 32)[0] != cm.block(KEY, NONCE, 0)[0]


@pytest.mark.parametrize("bits", [32, 64])
def test_fill_rows_at_a_far_first_row_is_two_flat_ranges(bits):
    mk, nk = KEY, bytes(range(1, 33))
    for mask_len, body_len, first in ((7, 3, (1 << 40) + 12345), (630, 1, (1 << 35) - 2), (128, 64, CAP // 128 - 5)):
        rows = 5
        got = cm.fill_rows(mk, 3, nk, 4, first, mask_len, body_len, bits - 2, rows, bits)
        assert got.shape == (rows, mask_len + body_len)
        assert np.array_equal(got[:, :mask_len].reshape(-1), cm.uniform(mk, 3, first * mask_len, rows * mask_len, bits))
        assert np.array_equal(got[:, mask_len:].reshape(-1),
                              cm.tuniform(nk, 4, first * body_len, bits - 2, rows * body_len, bits))
        assert np.array_equal(cm.fill_rows(mk, 3, nk, 4, first + 1, mask_len, body_len, bits - 2, 3, bits), got[1:4])


def test_fill_rows_is_two_flat_ranges():
    mk, nk = KEY, bytes(range(1, 33))
    whole = cm.fill_rows(mk, 3, nk, 4, 0, 7, 2, 5, 9, 32)
    part = cm.fill_rows(mk, 3, nk, 4, 2, 7, 2, 5, 4, 32)
    assert np.array_equal(part, whole[2:6])
    assert np.array_equal(whole[:, :7].reshape(-1), cm.uniform(mk, 3, 0, 63, 32))
    assert np.array_equal(whole[:, 7:].reshape(-1), cm.tuniform(nk, 4, 0, 5, 18, 32))
    base = np.arange(36, dtype=np.uint32) * np.uint32(0x9e3779b9)
    added = cm.fill_rows(mk, 3, nk, 4, 2, 7, 2, 5, 4, 32, into=base)
    assert np.array_equal(added[:, :7], part[:, :7])
    assert np.array_equal(added[:, 7:], base.reshape(4, 9)[:, 7:] + part[:, 7:])
