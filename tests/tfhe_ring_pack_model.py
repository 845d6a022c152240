"""Reference model of ring packing by automorphisms (include/pfhe.h, pfhe_ringpack{,32}_*), shared by the CPU model test and the GPU tests.  Wrapping numpy, built on
tests/tfhe_trace_model.py: a `product(ct, key)` argument is the f64 Fourier model on Fourier keys or the exact integer
schoolbook on torus-form keys, as there.

  rule A   level l in 1..log N, s = N / 2^l, t = 2^l + 1:
           D = even - X^s odd, S = even + X^s odd, out = S + rule 1(D, key, t)                          modulo 2^BITS
  rule B   m = ceil(log2 count); node_0[i] = embed(lwe[i]) for i < count, all zero for count <= i < 2^m;
           node_l[r] = rule A(node_{l-1}[r], node_{l-1}[r + 2^(m-l)], keys[log N - l], level l), l = 1..m, r < 2^(m-l);
           out = trace(node_m[0], keys[0 .. log N - m), log N - m steps)            (node_m[0] itself when m = log N)
  keys     the full trace's: keys[s - 1] is the key of t_s = 2^(log N - s + 1) + 1, so level l takes keys[log N - l]

Why it packs.  sigma_t with t = 2^l + 1 fixes X^j for j a multiple of 2s = N / 2^(l-1) and negates X^j for j an odd
multiple of s.  S + sigma_t(D) = (even + sigma_t(even)) + X^s (odd + sigma_t(odd)) as words, so in either child a
coefficient at an odd multiple of s is cancelled exactly, whatever it holds, and one at a multiple of 2s is doubled.  By
induction the multiples of s of a level-l node hold 2^l times the coefficient 0 of its 2^l leaves, leaf i of the node at
the sum of s_l' over the levels l' at which it was on the odd side: coefficient i N / 2^m of the root.  The m merges use
t = 3, 5, .., 2^m + 1; the trailing trace steps use t = N + 1, .., 2^(m+1) + 1, which fix every multiple of N / 2^m, double
it log N - m more times and clear every other coefficient.  Total factor N.
"""
import numpy as np

import tfhe_fft_model as m
import tfhe_trace_model as tm


def ceil_log2(count: int) -> int:
    return (count - 1).bit_length()


def slot(i: int, count: int, log_n: int) -> int:
    """the coefficient that holds N times the phase of input i of `count`"""
    return i * ((1 << log_n) >> ceil_log2(count))


def mul_monomial(ct, r: int, bits: int, log_n: int, k: int) -> np.ndarray:
    """X^r times every polynomial of a batch of GLWE ciphertexts, 0 <= r < 2N"""
    n = 1 << log_n
    x = np.asarray(ct).astype(m.UINT[bits]).reshape(-1, n)
    j = np.arange(n)
    src = (j - r) % (2 * n)
    with np.errstate(over="ignore"):
        out = np.where(src < n, x[:, src % n], (0 - x[:, src % n]).astype(m.UINT[bits])).astype(m.UINT[bits])
    return out.reshape(-1)


def merge_parts(even, odd, level: int, bits: int, log_n: int, k: int):
    """(D, S) of rule A"""
    assert 1 <= level <= log_n
    ev = np.asarray(even).astype(m.UINT[bits]).reshape(-1)
    shifted = mul_monomial(odd, (1 << log_n) >> level, bits, log_n, k)
    with np.errstate(over="ignore"):
        return (ev - shifted).astype(m.UINT[bits]), (ev + shifted).astype(m.UINT[bits])


def merge(even, odd, key, level: int, product, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """rule A on a batch of pairs against one key"""
    d, s = merge_parts(even, odd, level, basis.bits, log_n, k)
    with np.errstate(over="ignore"):
        return (s + tm.automorphism(d, key, (1 << level) + 1, product, basis, log_n, k)).astype(m.UINT[basis.bits])


def pack_levels(lwe, keys, count: int, product, basis: m.ApproxSignedBasis, log_n: int, k: int):
    """rule B on ONE group of `count` LWE ciphertexts as its calls of rule A: yields (level, nodes of the level, node-major)
    for level 0..m, then ("out", result)"""
    bits, n = basis.bits, 1 << log_n
    glwe = (k + 1) * n
    mm = ceil_log2(count)
    assert 1 <= count <= n
    keys = np.asarray(keys).reshape(log_n, -1)
    nodes = np.zeros((1 << mm, glwe), m.UINT[bits])
    nodes[:count] = tm.embed(np.asarray(lwe).reshape(count, k * n + 1), bits, log_n, k).reshape(count, glwe)
    yield 0, nodes
    for level in range(1, mm + 1):
        half = 1 << (mm - level)
        nodes = merge(nodes[:half].reshape(-1), nodes[half:2 * half].reshape(-1), keys[log_n - level], level, product, basis,
                      log_n, k).reshape(half, glwe)
        yield level, nodes
    root = nodes[0]
    if mm < log_n:
        root = tm.trace(root, keys[:log_n - mm].reshape(-1), log_n - mm, product, basis, log_n, k)
    yield "out", root


def pack(lwe, keys, count: int, product, basis: m.ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """rule B on a batch of groups"""
    n = 1 << log_n
    groups = np.asarray(lwe).reshape(-1, count * (k * n + 1))
    out = []
    for g in groups:
        for _, res in pack_levels(g, keys, count, product, basis, log_n, k):
            pass
        out.append(res)
    return np.concatenate(out)


def expected_phase(lwe_phases, count: int, bits: int, log_n: int) -> np.ndarray:
    """the noise-free phase of a pack: N phi_i at slot(i, count), 0 elsewhere"""
    want = np.zeros(1 << log_n, np.uint64)
    for i, phi in enumerate(lwe_phases):
        want[slot(i, count, log_n)] = (int(phi) << log_n) % (1 << bits)
    return want.astype(m.UINT[bits])


def ring_pack_bound(e0: float, bits, log_n, k, lb, ell, noise) -> float:
    """|coefficient of the phase of the pack's output - its noise-free value| for inputs whose phases are off by at most e0,
    for every count: ring_pack_bound = trace_bound(log N, e0) = N e0 + (N - 1) ks_bound.
    A coefficient of a level-l node at a multiple of s is (child + sigma_t(child)) at a multiple of 2s of ONE child (the
    other child's term there sits at an odd multiple of s and cancels as an identity of words, its error with it) plus the
    key switch of D: e <- 2 e + ks_bound, and only errors at such slots ever reach such a slot.  The trailing trace steps
    fix the multiples of N / 2^m: e <- 2 e + ks_bound again, log N steps in all, which is the full trace's recurrence.  A
    coefficient j that is no multiple of N / 2^m, 2^v || j, may carry a larger error out of the merges (both children meet
    there), but trace step v + 1 cancels it as words and leaves that step's key-switch error alone, which the remaining
    steps at most double: at most (2^(log N - m - v) - 1) ks_bound, below the bound."""
    return tm.trace_bound(log_n, e0, bits, log_n, k, lb, ell, noise)
