"""The Python model of the random layer: the ChaCha20 block function of RFC 8439 with a 64-bit block counter
(state words 12, 13) and a 64-bit nonce (words 14, 15), the position-addressed stream over it, and the four samplers, all in
plain integers.  Every word the device writes is held against this file bit for bit; this file is held against the RFC's test
vector, against a keystream written by openssl, and against restatements of the reference's sampler loops
(tests/test_csprng_model.py)."""
import numpy as np

MASK32 = 0xffffffff
CONSTANTS = (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)   # "expand 32-byte k"


def key_words(key: bytes):
    assert len(key) == 32
    return [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]


def _rotl(v, c):
    return ((v << c) & MASK32) | (v >> (32 - c))


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & MASK32
    x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & MASK32
    x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & MASK32
    x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & MASK32
    x[b] = _rotl(x[b] ^ x[c], 7)


def block_from_state(state):
    """the 20-round block function on 16 state words: 16 output words"""
    x = list(state)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12)
        _quarter(x, 1, 5, 9, 13)
        _quarter(x, 2, 6, 10, 14)
        _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15)
        _quarter(x, 1, 6, 11, 12)
        _quarter(x, 2, 7, 8, 13)
        _quarter(x, 3, 4, 9, 14)
    return [(a + b) & MASK32 for a, b in zip(x, state)]


def block(key: bytes, nonce: int, counter: int):
    """block `counter` (64 bits) of the stream of (key, nonce): u32 stream words 16*counter .. 16*counter + 15"""
    counter &= (1 << 64) - 1
    return block_from_state(list(CONSTANTS) + key_words(key) +
                            [counter & MASK32, counter >> 32, nonce & MASK32, (nonce >> 32) & MASK32])


def blocks(key: bytes, nonce: int, first: int, count: int) -> np.ndarray:
    """blocks [first, first + count) as a count x 16 array: block() on all of them at once, the same rounds on numpy columns
    (uint32 arrays wrap on their own); tests/test_csprng_model.py holds it against block() word for word"""
    counters = (np.arange(count, dtype=np.uint64) + np.uint64(first % (1 << 64)))   # wraps like the 64-bit counter
    state = [np.full(count, w, np.uint32) for w in list(CONSTANTS) + key_words(key)]
    state += [(counters & np.uint64(MASK32)).astype(np.uint32), (counters >> np.uint64(32)).astype(np.uint32),
              np.full(count, nonce & MASK32, np.uint32), np.full(count, (nonce >> 32) & MASK32, np.uint32)]
    x = [s.copy() for s in state]

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def quarter(a, b, c, d):
        x[a] += x[b]
        x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]
        x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]
        x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]
        x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        quarter(0, 4, 8, 12)
        quarter(1, 5, 9, 13)
        quarter(2, 6, 10, 14)
        quarter(3, 7, 11, 15)
        quarter(0, 5, 10, 15)
        quarter(1, 6, 11, 12)
        quarter(2, 7, 8, 13)
        quarter(3, 4, 9, 14)
    return np.stack([a + b for a, b in zip(x, state)], axis=1)


def keystream(key: bytes, nonce: int, word_offset: int, n_words: int) -> np.ndarray:
    """u32 stream words [word_offset, word_offset + n_words)"""
    if n_words == 0:
        return np.empty(0, np.uint32)
    first, last = word_offset // 16, (word_offset + n_words - 1) // 16
    words = blocks(key, nonce, first, last - first + 1).reshape(-1)
    skip = word_offset - 16 * first
    return words[skip:skip + n_words].copy()


class Stream:
    """The stream as a stateful generator from a u32 word position on: next_u32 / next_u64 (low word first), what a
    rand::RngCore over the same block layout yields.  The samplers below never use it: they address positions."""

    def __init__(self, key: bytes, nonce: int = 0, word_pos: int = 0):
        self.key, self.nonce, self.pos = key, nonce, word_pos

    def next_u32(self) -> int:
        w = block(self.key, self.nonce, self.pos // 16)[self.pos % 16]
        self.pos += 1
        return w

    def next_u64(self) -> int:
        lo = self.next_u32()
        return lo | self.next_u32() << 32


def stream_u64(key: bytes, nonce: int, offset: int, n: int) -> np.ndarray:
    """u64 stream words [offset, offset + n): word j is u32 words 2j (low half) and 2j + 1"""
    w = keystream(key, nonce, 2 * offset, 2 * n).astype(np.uint64)
    return w[0::2] | (w[1::2] << np.uint64(32))


def uniform(key: bytes, nonce: int, offset: int, n: int, bits: int) -> np.ndarray:
    return keystream(key, nonce, offset, n) if bits == 32 else stream_u64(key, nonce, offset, n)


def _dtype(bits):
    return np.uint32 if bits == 32 else np.uint64


def binary(key: bytes, nonce: int, offset: int, n: int, bits: int) -> np.ndarray:
    """output i = bit i mod 32 of u32 stream word i div 32"""
    first = offset // 32
    words = keystream(key, nonce, first, (offset + n + 31) // 32 - first) if n else np.empty(0, np.uint32)
    i = np.arange(offset, offset + n, dtype=np.uint64)
    w = words[(i // np.uint64(32) - np.uint64(first)).astype(np.int64)].astype(np.uint64)
    return ((w >> (i % np.uint64(32))) & np.uint64(1)).astype(_dtype(bits))


def ternary(key: bytes, nonce: int, offset: int, n: int, bits: int) -> np.ndarray:
    """output i = [0, 0, 1, -1][(w >> 2 (i mod 16)) & 3], w = u32 stream word i div 16"""
    first = offset // 16
    words = keystream(key, nonce, first, (offset + n + 15) // 16 - first) if n else np.empty(0, np.uint32)
    i = np.arange(offset, offset + n, dtype=np.uint64)
    w = words[(i // np.uint64(16) - np.uint64(first)).astype(np.int64)].astype(np.uint64)
    two = ((w >> (np.uint64(2) * (i % np.uint64(16)))) & np.uint64(3)).astype(np.int64)
    table = np.array([0, 0, 1, (1 << bits) - 1], dtype=_dtype(bits))
    return table[two]


def tuniform_value(word: int, b: int, bits: int) -> int:
    """TUniform(b) of one u64 stream word: r its low b + 2 bits, (r >> 1) + (r & 1) - 2^b modulo 2^bits"""
    assert 0 <= b <= bits - 2
    r = word & ((1 << (b + 2)) - 1)
    return ((r >> 1) + (r & 1) - (1 << b)) % (1 << bits)


def tuniform(key: bytes, nonce: int, offset: int, b: int, n: int, bits: int) -> np.ndarray:
    """output i takes u64 stream word i, at both widths"""
    assert 0 <= b <= bits - 2
    r = stream_u64(key, nonce, offset, n) & np.uint64((1 << (b + 2)) - 1)
    # tuniform_value on a whole array: uint64 arithmetic wraps modulo 2^64, and truncation to 32 bits is modulo 2^32
    return ((r >> np.uint64(1)) + (r & np.uint64(1)) - np.uint64(1 << b)).astype(_dtype(bits))


def fill_rows(mask_key, mask_nonce, noise_key, noise_nonce, first_row, mask_len, body_len, b, rows, bits, into=None):
    """rows x (mask_len + body_len) words: mask word j of absolute row R is uniform output R*mask_len + j of the mask stream,
    body word j TUniform output R*body_len + j of the noise stream, stored, or added to `into`'s bodies when given"""
    out = np.zeros((rows, mask_len + body_len), _dtype(bits)) if into is None else into.reshape(rows, mask_len + body_len).copy()
    out[:, :mask_len] = uniform(mask_key, mask_nonce, first_row * mask_len, rows * mask_len, bits).reshape(rows, mask_len)
    noise = tuniform(noise_key, noise_nonce, first_row * body_len, b, rows * body_len, bits).reshape(rows, body_len)
    out[:, mask_len:] = noise if into is None else out[:, mask_len:] + noise      # numpy's unsigned sums wrap
    return out
