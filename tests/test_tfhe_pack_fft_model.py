"""The numpy model of the Fourier packing key switch (tests/tfhe_pack_fft_model.py) against the exact integer model
(tests/tfhe_pack_model.py): bit for bit in the exact regime whatever the slice width, within the f64 transform's error on
full-torus keys, and the half-spectrum key against the Hermitian part of the full transform.  No GPU."""
import numpy as np
import pytest

import tfhe_fft_model as m
import tfhe_pack_fft_model as fm
import tfhe_pack_model as pm

CASE_ID = lambda c: "u%d-logn%d-k%d-n%d-lb%d-ell%d-count%d" % c


@pytest.mark.parametrize("case", fm.EXACT_CASES, ids=CASE_ID)
def test_exact_regime_equals_the_integer_route(case):
    """keys in [-2^10, 2^10] and n ell N 2^(logB-1) 2^10 <= 2^40 (test_gpu_tfhe_fft.py::test_product_exact_regime's
    condition): every f64 sum is far below 2^53, so the rounding of the inverse recovers the integers, with slices of 3, of
    the build's 4 and of 8 mask words"""
    bits, log_n, k, n, lb, ell, count = case
    assert fm.exact_regime_holds(case)
    basis, pksk, lwe = fm.case_inputs(case, small_keys=True, batch=2)
    want = pm.pack_keyswitch(lwe, pksk, n, count, basis, log_n, k)
    fkey = fm.half_spectrum_key(pksk, bits, log_n)
    for width in (3, fm.SLICE, 8):
        got = fm.pack_keyswitch_fft(lwe, fkey, n, count, basis, log_n, k, slice_width=width)
        assert np.array_equal(got, want), (width, np.nonzero(got != want)[0][:8])


# the round trip's precision p of the shape (tfhe_pack_model.NOISY_CASES); 3, the tighter bound, for a shape it has not
P_OF = {c[:7]: c[8] for c in pm.NOISY_CASES}


@pytest.mark.parametrize("case", fm.FULL_TORUS_CASES, ids=CASE_ID)
def test_full_torus_keys_stay_within_the_transforms_error(case):
    """u32: the products stay below 2^53 and the route is still exact; u64: the error is the f64 transform's, asserted
    2^16 below half the message spacing Delta/2 = 2^(BITS-p-2).  The figure printed here is the yardstick of
    test_gpu_tfhe_pack_fft.py (4 x the model's error + 2)."""
    bits = case[0]
    err = fm.full_torus_model_error(case)
    print(f"{CASE_ID(case)}: model error 2^{np.log2(max(err, 1)):.1f}")
    if bits == 32:
        assert err == 0
    else:
        assert err < 2.0 ** (bits - P_OF.get(case, 3) - 2) / 2.0 ** 16


@pytest.mark.parametrize("bits,log_n", [(32, 1), (32, 5), (64, 4), (64, 11)])
def test_half_spectrum_key_is_the_hermitian_part_of_the_full_transform(bits, log_n):
    n = 1 << log_n
    rng = np.random.default_rng(bits + log_n)
    x = rng.integers(0, 2 ** bits, 3 * n, dtype=np.uint64).astype(m.UINT[bits]).reshape(3, n)
    full = m.FullComplex64FftTable(log_n).forward(x, bits)
    half = fm.half_spectrum_key(x, bits, log_n)
    herm = m.hermitian_even(full)
    scale = np.abs(full).max()
    assert half.shape == (3, n // 2)
    assert np.abs(half - herm).max() <= 1e-13 * n * scale
    assert np.abs(half - full[:, ::2]).max() <= 1e-13 * n * scale     # for a real polynomial the even entries already
