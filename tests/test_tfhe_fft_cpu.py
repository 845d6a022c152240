"""CPU-side checks of the torus FFT / TFHE product boundary: the kernels of csrc/pfhe_fft.hip use no scratch memory
(tools/kernel_resources.py reads the compiler's remarks), and argument errors are reported before the device is touched."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_fft_kernels_use_no_scratch():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_fft.hip"))
    names = {r["pretty"] for r in rows}
    for must in ("fft_forward_kernel<unsigned int>", "fft_forward_kernel<unsigned long long>",
                 "fft_inverse_kernel<unsigned int, true>", "fft_inverse_kernel<unsigned long long, false>",
                 "tfhe_fused_kernel<unsigned int>", "tfhe_fused_kernel<unsigned long long>",
                 "tfhe_digit_fwd_kernel<unsigned long long>", "tfhe_mulacc_kernel", "tfhe_key_herm_kernel"):
        assert must in names, (must, sorted(names))
    bad = [(r["pretty"], r.get("ScratchSize", 0)) for r in rows if r.get("ScratchSize", 0) > 0]
    assert not bad, bad


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


def test_argument_errors_before_the_device(pfhe):
    import torch
    for log_n in (0, 15, 40):
        with pytest.raises(pfhe.PfheError) as e:
            pfhe.FullComplex64FftTable(log_n)
        assert e.value.kind == "Unsupported"
    h = C.c_void_p()
    lib = pfhe.lib()
    # ApproxSignedBasis::new's assert!s, checked before the table is looked at
    for fn, lb, length in (("pfhe_tfhe32_plan_create", 0, 0), ("pfhe_tfhe32_plan_create", 32, 0),
                           ("pfhe_tfhe32_plan_create", 10, 4), ("pfhe_tfhe_plan_create", 64, 0),
                           ("pfhe_tfhe_plan_create", 15, 5), ("pfhe_tfhe_plan_create", 15, 2)):
        assert getattr(lib, fn)(None, 1, lb, length, 0, C.byref(h)) == 33, (fn, lb, length)  # PFHE_ERR_BAD_ARGUMENT
    for args in ((32, 0), (32, 32), (64, 64)):
        with pytest.raises(pfhe.PfheError) as e:
            pfhe.ApproxSignedBasis(*args)
        assert e.value.kind == "BadArgument"
    with pytest.raises(pfhe.PfheError):
        pfhe.ApproxSignedBasis(32, 10, 4)
    b = pfhe.ApproxSignedBasis(64, 15, 2)
    assert (b.decompose_length(), b.drop_bits()) == (2, 34)
    assert (pfhe.ApproxSignedBasis(32, 7).decompose_length(), pfhe.ApproxSignedBasis(32, 7).drop_bits()) == (4, 4)
    if not torch.cuda.is_available():
        with pytest.raises(pfhe.PfheError) as e:
            pfhe.FullComplex64FftTable(10)
        assert e.value.kind == "NoDevice"
