"""The integer model of the linear layer with clear weights on LWE ciphertexts (include/pfhe.h, pfhe_lwe{,32}_linear*;
DESIGN.md §25): a wrapping uint64 matrix product cast to the word, the worst-case growth of the noise, and the small
two-layer network the GPU test runs through tfhe_dense_layer_dev."""
import numpy as np

import tfhe_bootstrap_model as bs
import tfhe_fft_model as m
import tfhe_keygen_model as kg


def signed_weights(weights) -> np.ndarray:
    """the weights as Python-sized signed integers (int64): int8 weights as they are, word weights in two's complement"""
    w = np.ascontiguousarray(weights)
    if w.dtype.kind == "u":
        w = w.view(np.dtype("i%d" % w.dtype.itemsize))
    return w.astype(np.int64)


def linear(lwe_in, weights, bias, dimension: int, in_features: int, out_features: int, bits: int) -> np.ndarray:
    """out[e][o][c] = sum_i W[o][i] in[e][i][c] + [c = dimension] bias[o] modulo 2^bits: the product of the sign-extended
    weights and the words in wrapping uint64 arithmetic, cast to the word (2^bits divides 2^64).  Flat, as the call writes it."""
    row = dimension + 1
    x = np.asarray(lwe_in).astype(np.uint64).reshape(-1, in_features, row)
    w = signed_weights(weights).reshape(out_features, in_features).view(np.uint64)
    with np.errstate(over="ignore"):
        out = np.matmul(w, x)                                   # batch x out_features x row, wrapping
        if bias is not None:
            out[:, :, dimension] += np.asarray(bias).astype(np.uint64).reshape(1, out_features)
    return out.astype(m.UINT[bits]).reshape(-1)


def linear_bound(weights, e_in: float) -> float:
    """the worst case of the output's noise when every input's is at most e_in: max_o sum_i |W[o][i]| e_in"""
    w = signed_weights(weights)
    return float(np.abs(w.astype(object)).sum(axis=-1).max()) * e_in


# ---------------- the two-layer network of the GPU test ----------------
#
# Three encrypted bits x at Delta = 2^(BITS-3) (p = 2 message bits under one padding bit).
#   layer 1, 3 -> 2:  s0 = x0 + x1 + x2,  s1 = x0 - x1 + x2 + 1 (the bias makes the negative weight's sum non-negative),
#                     both in 0..3; h = [s >= 2], the threshold table
#   layer 2, 2 -> 1:  t = h0 + 2 h1 in 0..3; y = tfhe_bootstrap_model.lut(2)(t)
NET_P = 2
W1 = np.array([[1, 1, 1], [1, -1, 1]], np.int8)
B1 = np.array([0, 1])
W2 = np.array([[1, 2]], np.int8)
DENSE_CASES = [kg.NOISY_CASES[0], kg.NOISY_CASES[1]]           # the first shape and its u64 shape


def threshold(v: int) -> int:
    return 1 if v >= 2 else 0


def clear_network(x):
    """the clear network on three bits: (layer-1 sums, hidden bits, layer-2 sum, output)"""
    s = [int(W1[o].astype(int) @ np.asarray(x)) + int(B1[o]) for o in range(2)]
    h = [threshold(v) for v in s]
    t = int(W2[0].astype(int) @ np.asarray(h))
    return s, h, t, bs.lut(NET_P)(t)


def dense_margin(case, weights):
    """(left, right) of the layer's condition linear_bound(W, E) 2N / 2^BITS + (n+1)/2 < N / 2^(p+1): the sums of inputs whose
    noise is at most E = max(fresh noise, tfhe_keygen_model.noise_bound) switch into their message's box"""
    bits, log_n, k, n, lb, ell, g, p, noise = case
    big_n = 1 << log_n
    e_in = max(float(noise), kg.noise_bound(bits, log_n, k, n, lb, ell, g, *kg.KS_BASIS, noise))
    return linear_bound(weights, e_in) * 2 * big_n / 2.0 ** bits + (n + 1) / 2, big_n / 2 ** (p + 1)
