"""Reference model of the batched CMUX and of the CMUX tree (include/pfhe.h, pfhe_tfhe{,32}_cmux_tree_*, _cmux*), shared by
the CPU model test and the GPU tests.  Wrapping numpy, built on tests/tfhe_fft_model.py: a `product(diff, key)` argument is
either the f64 Fourier model (fourier_product: tfhe_fft_model.external_product on a Fourier key) or the exact integer
schoolbook (exact_product: tfhe_fft_model.schoolbook on a torus-form key).

  rule 1   out[i] = d0[i] + product(d1[i] - d0[i], keys[i // per_key])                                    modulo 2^BITS
  rule 2   node_{j+1}[e][i] = node_j[e][2i] + product(node_j[e][2i+1] - node_j[e][2i], selectors[e d + j]), j = 0..d-1,
           node_0[e] the table (shared, or input e's), out[e] = node_d[e][0]: leaf sum_j m_{e,j} 2^j, bit 0 the least
           significant bit of the leaf index; it is d calls of rule 1 with per_key = 2^(d-1-j) and a key stride of d.
"""
import numpy as np

import tfhe_cbs_model as cm
import tfhe_fft_model as m
import tfhe_keygen_model as kg


def fourier_product(basis: m.ApproxSignedBasis, log_n: int, k: int):
    return lambda diff, key: m.external_product(diff, key, basis, log_n, k)[0]


def exact_product(basis: m.ApproxSignedBasis, log_n: int, k: int):
    return lambda diff, key: m.schoolbook(diff, key, basis, log_n, k)


def cmux(d0, d1, keys, per_key: int, product, bits: int, log_n: int, k: int) -> np.ndarray:
    """rule 1 on count ciphertexts; keys: count / per_key keys, one per row"""
    glwe = (k + 1) << log_n
    a, b = np.asarray(d0).reshape(-1, glwe), np.asarray(d1).reshape(-1, glwe)
    keys = np.asarray(keys).reshape(a.shape[0] // per_key, -1)
    assert a.shape == b.shape and a.shape[0] % per_key == 0
    out = np.empty_like(a)
    with np.errstate(over="ignore"):
        for i in range(a.shape[0]):
            out[i] = a[i] + product((b[i] - a[i]).astype(m.UINT[bits]), keys[i // per_key]).astype(m.UINT[bits])
    return out.reshape(-1)


def tree_levels(table, selectors, depth: int, batch: int, product, bits: int, log_n: int, k: int):
    """rule 2 as its d calls of rule 1: yields (j, d0, d1, keys of level j, per_key, nodes of level j + 1)"""
    glwe = (k + 1) << log_n
    table = np.asarray(table).reshape(-1, glwe)
    assert table.shape[0] in (1 << depth, batch << depth)
    nodes = (np.tile(table, (batch, 1)) if table.shape[0] == 1 << depth and batch > 1 else table).reshape(-1, 2, glwe)
    sel = np.asarray(selectors).reshape(batch, depth, -1)
    for j in range(depth):
        per_key = 1 << (depth - 1 - j)
        out = cmux(nodes[:, 0], nodes[:, 1], sel[:, j], per_key, product, bits, log_n, k)
        yield j, nodes[:, 0].reshape(-1), nodes[:, 1].reshape(-1), sel[:, j].reshape(-1), per_key, out
        nodes = out.reshape(-1, 2, glwe) if j + 1 < depth else out


def tree(table, selectors, depth: int, batch: int, product, bits: int, log_n: int, k: int) -> np.ndarray:
    out = None
    for *_, out in tree_levels(table, selectors, depth, batch, product, bits, log_n, k):
        pass
    return out


def leaf_index(bits_of_input) -> int:
    """sum_j m_j 2^j"""
    return sum(int(b) << j for j, b in enumerate(bits_of_input))


def bit_ggsws(msgs, z, basis: m.ApproxSignedBasis, log_n: int, k: int, rng, trivial: bool = False) -> np.ndarray:
    """noise-free torus-form GGSWs of the bits in msgs under z: uniform masks, or none at all (trivial)"""
    rows = len(msgs) * (k + 1) * basis.decompose_length
    if trivial:
        return kg.ggsw_add_gadget(np.zeros(rows * ((k + 1) << log_n), m.UINT[basis.bits]), msgs, basis, log_n, k)
    return kg.ggsw_encrypt(kg.glwe_randomness(rng, basis.bits, log_n, k, rows, 0), msgs, z, basis, log_n, k)


def to_fourier(torus, bits: int, log_n: int) -> np.ndarray:
    """write_fourier_form: polynomial after polynomial"""
    return m.FullComplex64FftTable(log_n).forward(np.asarray(torus).reshape(-1, 1 << log_n), bits).reshape(-1)


def message_table(rng, leaves: int, bits: int, log_n: int, k: int, p: int, z, trivial: bool = False):
    """`leaves` noise-free GLWE ciphertexts of p-bit messages under one padding bit: (words, messages leaves x N)"""
    n = 1 << log_n
    data = rng.integers(0, 1 << p, (leaves, n))
    rand = np.zeros((leaves, k + 1, n), m.UINT[bits]) if trivial else \
        kg.glwe_randomness(rng, bits, log_n, k, leaves, 0).reshape(leaves, k + 1, n)
    with np.errstate(over="ignore"):
        rand[:, k] += (data.astype(np.uint64) << np.uint64(bits - p - 1)).astype(m.UINT[bits])
    words = rand.reshape(-1) if trivial else kg.glwe_body_mac(rand.reshape(-1), z, bits, log_n, k)
    return words, data


# ---------------- the bound on noisy selectors ----------------

def tree_bound(depth: int, bits, log_n, k, cb_lb, cb_ell, row_noise) -> float:
    """|coefficient of the phase of out[e] - the chosen leaf's| for a noise-free table and selectors whose rows are off by at
    most row_noise: depth times tfhe_cbs_model.product_bound.  With m exactly 0 or 1 the phase of a node is
    phi_0 + m (phi_1 - phi_0) + eps, eps one product step (the digits of d1 - d0 against the rows' errors, and the rounding of
    the decomposition), so a level adds one step to the larger of its two inputs' errors, whatever they are."""
    return depth * cm.product_bound(bits, log_n, k, cb_lb, cb_ell, row_noise)


# (bits, log_n, k, n, rotation lb, ell, noise E, pfks lb, ell, cbs lb, ell, p), depth: the u64 shapes of the circuit
# bootstrap's noisy test, and a u32 shape of the tree's own (that file's u32 shape leaves no room for a second level)
NOISY_TREES = [
    ((32, 4, 1, 4, 8, 4, 2, 4, 8, 3, 3, 1), 3),
    (cm.NOISY_CASES[1], 3),
    (cm.NOISY_CASES[2], 3),
]


def noisy_tree_bound(case, depth: int) -> float:
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, _p = case
    return tree_bound(depth, bits, log_n, k, cb_lb, cb_ell, cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell))
