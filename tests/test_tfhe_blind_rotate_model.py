"""CPU test of the model the GPU blind rotation over the TFHE product is pinned to (tests/tfhe_blindrot_model.py): with
trivially encrypted key bits s_i the loop takes (0, Delta * m) to (0, Delta * X^{sum a_i s_i} * m), u32 and u64."""
import numpy as np
import pytest

import blindrot_model
import tfhe_blindrot_model as bm
import tfhe_fft_model as m


def test_rotate_is_the_negacyclic_monomial_product():
    rng = np.random.default_rng(1)
    n = 16
    for bits in (32, 64):
        x = rng.integers(0, 2 ** bits, 2 * n, dtype=np.uint64).astype(m.UINT[bits])
        for r in (0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n + 3):
            want = np.zeros_like(x)
            for p in range(2):
                for j in range(n):
                    d = j + r
                    v = int(x[p * n + j]) * (-1 if (d // n) % 2 else 1)
                    want[p * n + d % n] = v % (1 << bits)
            assert np.array_equal(bm.rotate(x, r, n), want), (bits, r)
        assert np.array_equal(bm.add(bm.sub(x, x[::-1].copy()), x[::-1].copy()), x)


@pytest.mark.parametrize("bits,log_n,k,lb,ell", [(32, 5, 1, 7, 3), (64, 5, 1, 15, 2), (32, 4, 2, 8, None), (64, 4, 1, 1, 10)])
def test_trivial_keys_rotate_the_message(bits, log_n, k, lb, ell):
    n = 1 << log_n
    rng = np.random.default_rng(bits + log_n)
    basis = m.ApproxSignedBasis(bits, lb, ell)
    assert basis.drop_bits <= bits - bm.PLAINTEXT_BITS      # Delta * m survives the approximate decomposition exactly
    n_steps, batch = 8, 3
    secret = [1, 0, 1, 1, 0, 1, 1, 1]
    keys = [bm.trivial_ggsw(basis, log_n, k, s) for s in secret]
    msgs = rng.integers(0, 1 << bm.PLAINTEXT_BITS, (batch, n))
    acc = bm.encode(msgs, bits, log_n, k)
    W = (k + 1) * n
    for e in range(batch):
        exps = blindrot_model.special_exponents(np.random.default_rng(e), n, n_steps)
        if e:
            exps = np.roll(exps, e)
        out = bm.exact_rotate(acc[e * W:(e + 1) * W], keys, exps, basis, log_n, k)
        mask_err, got = bm.decode(out, bits, log_n, k)
        total = sum(int(a) * s for a, s in zip(exps, secret))
        assert mask_err == 0 and got == bm.expected_decode(msgs[e], total, n), (e, total)


def test_zero_key_bits_leave_the_accumulator():
    bits, log_n, k = 32, 4, 1
    basis = m.ApproxSignedBasis(bits, 8, None)
    rng = np.random.default_rng(3)
    acc = rng.integers(0, 2 ** 32, 2 << log_n, dtype=np.uint64).astype(np.uint32)
    keys = [bm.trivial_ggsw(basis, log_n, k, 0)] * 3
    assert np.array_equal(bm.exact_rotate(acc, keys, [1, 17, 31], basis, log_n, k), acc)
    # a one-bit with drop_bits = 0 is the exact rotation of a full-torus accumulator
    keys = [bm.trivial_ggsw(basis, log_n, k, 1)]
    assert np.array_equal(bm.exact_rotate(acc, keys, [19], basis, log_n, k), bm.rotate(acc, 19, 16))
