"""Edge words of the power-of-two signed decomposition (tests/tfhe_fft_model.py, ApproxSignedBasis): the torus words whose
per-level fields and dropped bits sit where digit_step and init_carry branch.  A uniformly random word reaches any of
these with probability about 2^-log_basis per digit, so the tests that must see them take them from here.

Per level the field (the log_basis bits of that level) is one of
    0, 1, B/2 - 1, B/2, B/2 + 1, B - 2, B - 1        (reduced mod B, duplicates removed)
 - B/2 - 1 / B/2 / B/2 + 1: the largest positive digit, the digit -B/2 with a carry, and its neighbour;
 - B - 1 with an incoming carry: the field sum B, digit 0 with a carry; B - 2 with a carry: digit -1;
and the dropped part (the low drop_bits bits) one of 0, 2^(drop-1) - 1, 2^(drop-1), 2^drop - 1: the rounding boundary of
init_carry from both sides.  Up to three levels every combination is listed.  Above that, one level takes each field value
in turn while every other level holds a background of 0, B - 1, B/2 - 1 or B/2: the long carry chains (0x7FFF..., 0xFFFF...)
and the carry discarded at the top.
"""
import itertools

import numpy as np

UINT = {32: np.uint32, 64: np.uint64}


def shape(bits: int, log_basis: int, reverse_length=None):
    """(decompose_length, drop_bits) as ApproxSignedBasis::new derives them"""
    ell = bits // log_basis if reverse_length is None else reverse_length
    return ell, bits - ell * log_basis


def field_values(log_basis: int):
    B = 1 << log_basis
    return sorted({v % B for v in (0, 1, B // 2 - 1, B // 2, B // 2 + 1, B - 2, B - 1)})


def dropped_values(drop_bits: int):
    if drop_bits == 0:
        return [0]
    return sorted({0, (1 << (drop_bits - 1)) - 1, 1 << (drop_bits - 1), (1 << drop_bits) - 1})


def edge_words(bits: int, log_basis: int, reverse_length=None) -> np.ndarray:
    """the sorted edge words of ApproxSignedBasis(bits, log_basis, reverse_length), uint32 / uint64"""
    ell, drop = shape(bits, log_basis, reverse_length)
    B = 1 << log_basis
    fields = field_values(log_basis)
    if ell <= 3:
        levels = itertools.product(fields, repeat=ell)
    else:
        backgrounds = sorted({0, B - 1, (B // 2 - 1) % B, B // 2})
        levels = (tuple(f if i == lvl else bg for i in range(ell))
                  for bg in backgrounds for lvl in range(ell) for f in fields)
    words = {0, 1, (1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1}
    for combo in levels:
        kept = sum(f << (drop + i * log_basis) for i, f in enumerate(combo))
        words.update(kept | d for d in dropped_values(drop))
    return np.array(sorted(words), dtype=UINT[bits])
