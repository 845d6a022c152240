"""Reference model of the look-up table on encrypted bits (include/pfhe.h, pfhe_tfhe{,32}_lut_*, _rotate_by_bits*,
_lut_eval*), shared by the CPU model test and the GPU tests.  Wrapping numpy, built on
tests/tfhe_cmux_model.py: a `product(diff, key)` argument is the f64 Fourier model or the exact integer schoolbook.

  rule 1   acc_0 = inp[a], acc_{j+1} = acc_j + product(X^{2N - 2^(j+s)} acc_j - acc_j, keys[(a // o) kpi + first_key + j]),
           j = 0..r-1, out[a] = acc_r: per step the monomial multiplication, then the CMUX with per_key = o
  rule 2   stage A, the tree on the nodes (input, output, leaf) with bit r + j at level j (t CMUX calls with per_key =
           o 2^(t-1-j) and a key stride of p = t + r); stage B, rule 1 with kpi = p, first_key = 0; stage C, sample extraction
           at the indices below `extract`, row (e o + u) extract + i
"""
import numpy as np

import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_cmux_model as xm
import tfhe_fft_model as m


def mul_monomial(glwe, e: int, log_n: int) -> np.ndarray:
    """X^e p on every polynomial of N words, e modulo 2N: coefficient j is +-p[(j - e) mod N], the wrapped part negated"""
    n = 1 << log_n
    p = np.asarray(glwe).reshape(-1, n)
    e %= 2 * n
    j = np.arange(n)
    src = (j - e) % n
    negate = ((j - e) // n) % 2 == 1            # floor division: how many times the index wrapped
    with np.errstate(over="ignore"):
        return np.where(negate, (0 - p[:, src]).astype(p.dtype), p[:, src]).reshape(-1)


def exponent(j: int, log_stride: int, log_n: int) -> int:
    return (2 << log_n) - (1 << (j + log_stride))


def rotation_steps(inp, keys, r: int, log_stride: int, outputs: int, keys_per_input: int, first_key: int, product, bits: int,
                   log_n: int, k: int):
    """rule 1 as its r pairs of calls: yields (j, acc, the rotated acc, keys of step j, acc after the step)"""
    glwe = (k + 1) << log_n
    acc = np.asarray(inp).reshape(-1, glwe).copy()
    assert acc.shape[0] % outputs == 0 and first_key + r <= keys_per_input
    if r == 0:
        return
    keys =np.asarray(keys).reshape(acc.shape[0] // outputs, keys_per_input, -1)
    for j in range(r):
        rot = mul_monomial(acc, exponent(j, log_stride, log_n), log_n)
        step_keys = keys[:, first_key + j]
        out = xm.cmux(acc.reshape(-1), rot, step_keys, outputs, product, bits, log_n, k)
        yield j, acc.reshape(-1), rot, step_keys.reshape(-1), out
        acc = out.reshape(-1, glwe)


def rotate_by_bits(inp, keys, r: int, log_stride: int, outputs: int, keys_per_input: int, first_key: int, product, bits: int,
                   log_n: int, k: int) -> np.ndarray:
    out = np.asarray(inp).reshape(-1).copy()
    for *_, out in rotation_steps(inp, keys, r, log_stride, outputs, keys_per_input, first_key, product, bits, log_n, k):
        pass
    return out


def tree_stage(table, selectors, t: int, r: int, outputs: int, batch: int, product, bits: int, log_n: int, k: int):
    """stage A as its t CMUX calls: the batch * o results (t = 0: the table, tiled over the batch when it is shared)"""
    glwe = (k + 1) << log_n
    table = np.asarray(table).reshape(-1, glwe)
    leaves = outputs << t
    assert table.shape[0] in (leaves, batch * leaves)
    nodes = np.tile(table, (batch, 1)) if table.shape[0] == leaves and batch > 1 else table
    sel = np.asarray(selectors).reshape(batch, t + r, -1)
    for j in range(t):
        pair = nodes.reshape(-1, 2, glwe)
        nodes = xm.cmux(pair[:, 0], pair[:, 1], sel[:, r + j], outputs << (t - 1 - j), product, bits, log_n, k).reshape(-1, glwe)
    return nodes.reshape(-1)


def lut_eval(table, selectors, t: int, r: int, log_stride: int, outputs: int, batch: int, extract: int, product, bits: int,
             log_n: int, k: int) -> np.ndarray:
    """rule 2: batch * o GLWE ciphertexts, or with extract batch * o * extract LWE ciphertexts"""
    acc = tree_stage(table, selectors, t, r, outputs, batch, product, bits, log_n, k)
    acc = rotate_by_bits(acc, selectors, r, log_stride, outputs, t + r, 0, product, bits, log_n, k)
    if not extract:
        return acc
    rows = [bs.sample_extract(acc, log_n, k, i).reshape(batch * outputs, -1) for i in range(extract)]
    return np.stack(rows, axis=1).reshape(-1)


def lut_table(values, log_n: int, k: int, t: int, r: int, log_stride: int = 0) -> np.ndarray:
    """tfhe_lut_table: (outputs, 2^p[, words]) entries as trivial GLWE leaves (outputs, 2^t, k+1, N)"""
    values = np.asarray(values)
    if values.ndim == 2:
        values = values[:, :, None]
    outputs, entries, words = values.shape
    assert entries == 1 << (t + r) and words <= 1 << log_stride and r + log_stride <= log_n
    leaves = np.zeros((outputs, 1 << t, k + 1, 1 << log_n), values.dtype)
    for x in range(entries):
        c = (x & ((1 << r) - 1)) << log_stride
        leaves[:, x >> r, k, c:c + words] = values[:, x]
    return leaves


# ---------------- the bound on noisy selectors ----------------

def lut_bound(t: int, r: int, bits, log_n, k, cb_lb, cb_ell, row_noise) -> float:
    """|coefficient of the phase of the result - the chosen entry's| for a noise-free table and selectors whose rows are off
    by at most row_noise: (t + r) times tfhe_cbs_model.product_bound.  A rotation step has the CMUX's shape,
    phi + m (X^e phi - phi) + eps with m exactly 0 or 1, so like a tree level it adds one product step to its input's error
    (X^e permutes the coefficients of that error and changes signs only)."""
    return (t + r) * cm.product_bound(bits, log_n, k, cb_lb, cb_ell, row_noise)


# (case of tfhe_cmux_model.NOISY_TREES, tree depth t, rotation bits r): the u32 shape leaves room for three steps
# (2^26.87 each under 2^29), the u64 shapes for five and more
NOISY_LUTS = [(xm.NOISY_TREES[0][0], 1, 2), (xm.NOISY_TREES[1][0], 2, 3), (xm.NOISY_TREES[2][0], 2, 3)]


def noisy_lut_bound(case, t: int, r: int) -> float:
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, _p = case
    return lut_bound(t, r, bits, log_n, k, cb_lb, cb_ell, cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell))
