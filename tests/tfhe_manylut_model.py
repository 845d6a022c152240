"""Reference model of the many-LUT steps around the blind rotation (include/pfhe.h, pfhe_tfhe{,32}_modswitch_stride_dev,
_bootstrap_create_many_lut, _cbs_create_with), shared by the CPU model test and the GPU parity tests.  Exact,
wrapping numpy; built on tests/tfhe_bootstrap_model.py, tests/tfhe_blindrot_model.py and tests/tfhe_cbs_model.py.

Conventions are theirs: the phase is b - <a,s>, levels least significant first, g_l = 2^(drop_bits + l log_basis); v is a
number of stride bits, 0 <= v <= log N.

  - sw_v(w) = ((((w >> (BITS - log N - 2 + v)) + 1) >> 1) << v) mod 2N: w 2N / 2^v / 2^BITS rounded half up, times 2^v;
  - many_lut_bootstrap: the strided switch, ACC = X^{neg_b} TV, exact_rotate, extraction at every index i < 2^v (output
    (e, i) at e 2^v + i) and, with a key, the key switch of every row;
  - shared_extracted / shared_circuit_bootstrap: the strided switch of (a, b + 2^(BITS-2)) with v = ceil(log2 ell_cb), the
    patterned test vector (body coefficient c is -g_{c mod 2^v}/2, 0 where the basis has no such level), ONE exact_rotate per
    input, extraction at index l with g_l/2 added to the body, and the private key switch.
"""
import numpy as np

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_fft_model as m


def sw_strided(w: int, bits: int, log_n: int, v: int) -> int:
    """one word, in Python integers"""
    return ((((int(w) >> (bits - log_n - 2 + v)) + 1) >> 1) << v) % (2 << log_n)


def sw_statement(w: int, bits: int, log_n: int, v: int) -> int:
    """the rule as a statement on big integers: round w 2N / 2^v / 2^BITS half up, times 2^v, modulo 2N"""
    num, den = int(w) * (2 << log_n), (1 << v) << bits
    return ((2 * num + den) // (2 * den) << v) % (2 << log_n)


def strided_edge_words(bits: int, log_n: int, v: int):
    """0, 1, all ones, the half turn, and for several multiples m of the stride the exact tie below m's cell with both of
    its neighbours: the words that round up to 2N are among them (m = 2N / 2^v), and so are the words that wrap when
    2^(BITS-2) is added (the ties around three quarters of a turn)"""
    cell = bits - log_n - 1 + v                 # a word's cell is 2^cell wide
    cells = (2 << log_n) >> v
    words = {0, 1, (1 << bits) - 1, 1 << (bits - 1), (3 << (bits - 2)) - 1, 3 << (bits - 2)}
    for mm in sorted({0, 1, 2, cells // 4, cells // 2 - 1, cells // 2, 3 * cells // 4, cells - 1, cells}):
        for d in (-2, -1, 0, 1, 2):
            words.add((mm * (1 << cell) - (1 << (cell - 1)) + d) % (1 << bits))
    return sorted(words)


def modulus_switch_strided(lwe, n: int, bits: int, log_n: int, v: int):
    """(exps: batch x n, neg_b: batch) as uint32"""
    x = np.asarray(lwe).astype(np.uint64).reshape(-1, n + 1)
    mask = np.uint64((2 << log_n) - 1)
    val = ((((x >> np.uint64(bits - log_n - 2 + v)) + np.uint64(1)) >> np.uint64(1)) << np.uint64(v)) & mask
    neg_b = (np.uint64(2 << log_n) - val[:, n]) & mask
    return val[:, :n].astype(np.uint32), neg_b.astype(np.uint32)


def log_stride(levels: int) -> int:
    """ceil(log2 levels)"""
    return (levels - 1).bit_length()


def many_lut_test_vector(tvs) -> np.ndarray:
    """TV[c] = tvs[c mod 2^v][c - (c mod 2^v)] on the last axis; tvs: 2^v x ... x N"""
    t = np.asarray(tvs)
    luts, n = t.shape[0], t.shape[-1]
    c = np.arange(n)
    low = c % luts
    return np.moveaxis(t[low, ..., c - low], 0, -1).copy()


def multi_extract(glwe, log_n: int, k: int, count: int) -> np.ndarray:
    """batch accumulators -> batch x count LWE ciphertexts, row e count + h the extraction of accumulator e at index h"""
    rows = [bs.sample_extract(glwe, log_n, k, h).reshape(-1, (k << log_n) + 1) for h in range(count)]
    return np.stack(rows, axis=1).reshape(-1)


def many_lut_bootstrap(lwe_in, keys_coeff, tv, ksk, basis, ks_basis, log_n: int, k: int, n: int, v: int) -> np.ndarray:
    bits, big_n = basis.bits, 1 << log_n
    glwe = (k + 1) * big_n
    exps, neg_b = modulus_switch_strided(lwe_in, n, bits, log_n, v)
    tv = np.asarray(tv).astype(m.UINT[bits])
    accs = []
    for e in range(exps.shape[0]):
        t = tv if tv.size == glwe else tv[e * glwe:(e + 1) * glwe]
        accs.append(bm.exact_rotate(bm.rotate(t, int(neg_b[e]), big_n), keys_coeff, exps[e], basis, log_n, k))
    lwe = multi_extract(np.concatenate(accs), log_n, k, 1 << v)
    return lwe if ksk is None else bs.keyswitch(lwe, ksk, k * big_n, n, ks_basis)


def shared_test_vector(cbs_basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """the trivial GLWE whose body coefficient c is -g_{c mod 2^v}/2 for c mod 2^v < ell_cb and 0 otherwise"""
    bits, levels = cbs_basis.bits, cbs_basis.decompose_length
    stride = 1 << log_stride(levels)
    tv = np.zeros((k + 1, 1 << log_n), m.UINT[bits])
    for c in range(1 << log_n):
        if c % stride < levels:
            tv[k, c] = (-cm.half_gadget(cbs_basis, c % stride)) % (1 << bits)
    return tv.reshape(-1)


def add_half_gadgets(lwe, cbs_basis: m.ApproxSignedBasis, words: int) -> np.ndarray:
    """body of row (e, l) += g_l/2; lwe: batch x ell_cb x words"""
    levels = cbs_basis.decompose_length
    out = np.asarray(lwe).reshape(-1, levels, words).copy()
    with np.errstate(over="ignore"):
        for l in range(levels):
            out[:, l, words - 1] += m.UINT[cbs_basis.bits](cm.half_gadget(cbs_basis, l))
    return out.reshape(-1)


def shared_extracted(lwe_in, keys_coeff, basis, cbs_basis, log_n: int, k: int, n: int, rotate=None) -> np.ndarray:
    """stages 1-4 of the shared circuit bootstrap: batch x ell_cb LWE ciphertexts of k N + 1 words.  rotate(acc, exps_e):
    another rotation than exact_rotate over keys_coeff (the multi-bit one)"""
    bits, big_n, levels = basis.bits, 1 << log_n, cbs_basis.decompose_length
    v = log_stride(levels)
    exps, neg_b = modulus_switch_strided(cm.offset_inputs(lwe_in, n, bits), n, bits, log_n, v)
    tv = shared_test_vector(cbs_basis, log_n, k)
    accs = []
    for e in range(exps.shape[0]):
        acc = bm.rotate(tv, int(neg_b[e]), big_n)
        accs.append(rotate(acc, exps[e]) if rotate else bm.exact_rotate(acc, keys_coeff, exps[e], basis, log_n, k))
    return add_half_gadgets(multi_extract(np.concatenate(accs), log_n, k, levels), cbs_basis, k * big_n + 1)


def shared_circuit_bootstrap(lwe_in, keys_coeff, pfksk, basis, cbs_basis, pfks_basis, log_n: int, k: int, n: int,
                             rotate=None) -> np.ndarray:
    lwe = shared_extracted(lwe_in, keys_coeff, basis, cbs_basis, log_n, k, n, rotate)
    return cm.private_keyswitch(lwe, pfksk, k << log_n, cbs_basis.decompose_length, pfks_basis, log_n, k)


def switch_margin(n: int, log_n: int, v: int):
    """(worst-case drift, what it must stay below): n + 1 roundings, each off by at most 2^(v-1) exponents (half an exponent
    at v = 0) against key words of magnitude at most 1, and the quarter turn N / 2 between the offset phase and a sign change"""
    return 2.0 ** (v - 1) * (n + 1), (1 << log_n) / 2
