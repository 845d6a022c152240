"""CPU-side checks of key generation, encryption and phase (pfhe_tfhe{,32}_lwe_body_mac*, _glwe_body_mac*,
_ggsw_add_gadget_dev, _bsk_generate_dev, _ksk_generate_dev): the entry points are in the ctypes table and the package's
__all__, every refusal arrives before the device is touched and in the stated order, nothing is computed without a device,
and the compiler's resource report shows no scratch memory and no spilled register for the new kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("lwe_body_mac_dev", "lwe_body_mac", "glwe_body_mac_dev", "glwe_body_mac", "ggsw_add_gadget_dev", "bsk_generate_dev",
         "ksk_generate_dev")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("lwe_encrypt", "lwe_encrypt_dev", "lwe_phase", "lwe_phase_dev", "glwe_encrypt", "glwe_encrypt_dev", "glwe_phase",
          "glwe_phase_dev", "ggsw_add_gadget_dev", "TfheKeyShape", "tfhe_generate_bsk_dev", "tfhe_generate_ksk_dev",
          "torus_uniform", "torus_noise")

BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36


def test_keygen_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_keygen.hip"))
    by_name = {r["pretty"]: r for r in rows}
    want = ["tfhe_lwe_body_mac_kernel<%s>" % w for w in ("unsigned int", "unsigned long long")]
    want += ["tfhe_ggsw_add_gadget_kernel<%s>" % w for w in ("unsigned int", "unsigned long long")]
    want += ["tfhe_glwe_body_mac_kernel<%s, %d>" % (w, u) for w in ("unsigned int", "unsigned long long") for u in (1, 2, 4, 8)]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    for name in want:
        assert by_name[name].get("ScratchSize", 0) == 0 and by_name[name].get("VGPRs Spill", 0) == 0, by_name[name]


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


@pytest.fixture(scope="module")
def table_stand_in():
    """A non-null table pointer for calls that must be refused before the table is read: zeroed host memory, which none of
    the checks below dereferences.  Every call that gets it is one the library has to refuse on its arguments alone."""
    buf = C.create_string_buffer(4096)
    return buf, C.cast(buf, C.c_void_p)


def last_error(lib):
    return lib.pfhe_last_error().decode(errors="replace")


def test_symbols_are_in_the_ctypes_table_and_the_package(pfhe):
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.pfhe_tfhe_bsk_generate_dev.argtypes[11] == C.POINTER(C.c_double)
    assert len(lib.pfhe_tfhe_lwe_body_mac_dev.argtypes) == len(lib.pfhe_tfhe_lwe_body_mac.argtypes) + 1
    assert len(lib.pfhe_tfhe32_glwe_body_mac_dev.argtypes) == len(lib.pfhe_tfhe32_glwe_body_mac.argtypes) + 1
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    for fn in (pfhe.torus_uniform, pfhe.torus_noise):
        assert "NOT CRYPTOGRAPHIC" in fn.__doc__ and "generator" in fn.__doc__


@pytest.mark.parametrize("w", ["", "32"])
def test_the_lwe_body_call_refuses_its_arguments_in_order(pfhe, w):
    """dimension, then the lengths, then zero ciphertexts as a no-op, then null pointers, then the device"""
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    for form, tail in (("lwe_body_mac_dev", (None,)), ("lwe_body_mac", ())):
        call = getattr(lib, f"pfhe_tfhe{w}_{form}")
        for sub in (0, 1):
            for dim in (0, 2 ** 31 - 1, 2 ** 40):
                assert call(-1, None, 7, dim, None, 3, sub, *tail) == BAD_ARGUMENT
                assert "dimension must be in 1..2^31-2" in last_error(lib)
            assert call(-1, ptr, 12, 3, ptr, 4, sub, *tail) == BAD_LENGTH         # the key is not `dimension` words
            assert call(-1, ptr, 13, 3, ptr, 3, sub, *tail) == BAD_LENGTH         # 13 is no multiple of 4
            assert "batch*(dimension+1)" in last_error(lib)
            assert call(-1, None, 0, 3, None, 3, sub, *tail) == 0                 # zero ciphertexts: nothing is looked at
            assert call(-1, None, 8, 3, ptr, 3, sub, *tail) == BAD_ARGUMENT
            assert call(-1, ptr, 8, 3, None, 3, sub, *tail) == BAD_ARGUMENT
            assert call(-1, C.c_void_p(ptr.value + 256), 8, 3, ptr, 3, sub, *tail) == NO_DEVICE   # device -1, the last check
    dev = getattr(lib, f"pfhe_tfhe{w}_lwe_body_mac_dev")
    assert dev(0, ptr, 8, 3, ptr, 3, 0, None) == BAD_ARGUMENT and "overlap" in last_error(lib)


@pytest.mark.parametrize("w", ["", "32"])
def test_the_glwe_body_call_refuses_the_table_and_the_dimension_first(pfhe, table_stand_in, w):
    lib = pfhe.lib()
    _, fft = table_stand_in
    for form, tail in (("glwe_body_mac_dev", (None,)), ("glwe_body_mac", ())):
        call = getattr(lib, f"pfhe_tfhe{w}_{form}")
        assert call(None, 0, None, 5, None, 3, 0, *tail) == BAD_ARGUMENT          # the table before anything else
        for k in (0, 65, 2 ** 40):
            assert call(fft, k, None, 5, None, 3, 1, *tail) == BAD_ARGUMENT
            assert "glwe_dimension must be in 1..64" in last_error(lib)


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_ggsw_calls_run_the_plans_checks_first_and_in_its_order(pfhe, table_stand_in, w, bits):
    """the basis's assert!s, k > 64 and the table with pfhe_tfhe_plan_create's status and message; then what is the calls'
    own: k = 0, the grouping factor, lwe_dimension and its divisibility, all before the table is read"""
    lib = pfhe.lib()
    _, fft = table_stand_in
    h = C.c_void_p()
    gadget = getattr(lib, f"pfhe_tfhe{w}_ggsw_add_gadget_dev")
    bsk = getattr(lib, f"pfhe_tfhe{w}_bsk_generate_dev")
    lb = 7 if bits == 32 else 15
    for table, k, log_basis, length in ((fft, 1, 0, 0), (fft, 1, bits, 0), (fft, 65, lb, bits), (None, 65, lb, bits),
                                        (fft, 65, lb, 2), (None, 65, lb, 2), (None, 1, lb, 2), (None, 0, lb, 2)):
        plan = getattr(lib, f"pfhe_tfhe{w}_plan_create")(table, k, log_basis, length, 0, C.byref(h))
        message = last_error(lib)
        assert plan in (BAD_ARGUMENT, UNSUPPORTED) and not h.value
        assert gadget(table, k, log_basis, length, None, 5, None, 3, None) == plan
        assert plan != UNSUPPORTED or last_error(lib) == message
        for g in (0, 2, 5):
            assert bsk(table, k, log_basis, length, g, None, 7, None, 3, None, 5, None, 9, None) == plan
            assert plan != UNSUPPORTED or last_error(lib) == message
    assert gadget(fft, 0, lb, 2, None, 5, None, 3, None) == BAD_ARGUMENT
    assert "glwe_dimension must be at least 1" in last_error(lib)
    for g in (5, 6, 2 ** 40):                                                    # judged before n and n % g
        for n in (0, 7, 630):
            assert bsk(fft, 1, lb, 2, g, None, n, None, 3, None, 5, None, 9, None) == BAD_ARGUMENT
            assert "grouping_factor must be 0 (the classic layout) or in 1..4" in last_error(lib)
    for g in (0, 1, 4):
        for n in (0, 2 ** 31 - 1):
            assert bsk(fft, 1, lb, 2, g, None, n, None, 3, None, 5, None, 9, None) == BAD_ARGUMENT
            assert "lwe_dimension must be in 1..2^31-2" in last_error(lib)
    for g, n in ((2, 7), (3, 7), (4, 630), (3, 1)):
        assert bsk(fft, 1, lb, 2, g, None, n, None, 3, None, 5, None, 9, None) == BAD_ARGUMENT
        assert "lwe_dimension must be a multiple of grouping_factor" in last_error(lib)


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_key_switch_key_call_refuses_its_arguments_in_order(pfhe, w, bits):
    """ApproxSignedBasis::new's assert!s, the dimensions, the length, null pointers, the device: the key switch's order"""
    lib = pfhe.lib()
    call = getattr(lib, f"pfhe_tfhe{w}_ksk_generate_dev")
    buf = (C.c_uint64 * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    far = C.c_void_p(ptr.value + 16384)
    for lb, length in ((0, 0), (bits, 0), (4, bits // 4 + 1)):
        assert call(-1, None, 0, None, 0, lb, length, None, 5, None) == BAD_ARGUMENT
    for din, dout in ((0, 3), (3, 0), (2 ** 31 - 1, 3), (3, 2 ** 31 - 1)):
        assert call(-1, None, din, None, dout, 4, 3, None, 5, None) == BAD_ARGUMENT
        assert "both dimensions must be in 1..2^31-2" in last_error(lib)
    assert call(-1, ptr, 8, ptr, 3, 4, 3, far, 8 * 3 * 4 + 1, None) == BAD_LENGTH
    assert call(-1, ptr, 8, ptr, 3, 4, 0, far, 8 * 3 * 4, None) == BAD_LENGTH       # length 0: the full BITS / 4 levels
    assert "in_dimension*ell*(out_dimension+1)" in last_error(lib)
    for args in ((None, ptr, far), (ptr, None, far), (ptr, ptr, None)):
        assert call(-1, args[0], 8, args[1], 3, 4, 3, args[2], 96, None) == BAD_ARGUMENT
    assert call(-1, ptr, 8, ptr, 3, 4, 3, ptr, 96, None) == BAD_ARGUMENT and "overlap" in last_error(lib)
    assert call(-1, ptr, 8, ptr, 3, 4, 3, far, 96, None) == NO_DEVICE               # device -1, the last check


def test_no_fallback_without_a_device(pfhe):
    """without a GPU the host forms report NoDevice and leave the buffers as they were: nothing is computed on the CPU"""
    import torch
    lwe = np.arange(1, 9, dtype=np.uint64)
    key = np.array([1, 0, 1], np.uint64)
    if torch.cuda.is_available():
        pfhe.lwe_encrypt(lwe, key)
        assert list(lwe) == [1, 2, 3, 4 + 1 + 3, 5, 6, 7, 8 + 5 + 7]
        pfhe.lwe_phase(lwe, key)
        assert list(lwe) == list(range(1, 9))
        return
    for call in (pfhe.lwe_encrypt, pfhe.lwe_phase):
        with pytest.raises(pfhe.PfheError) as e:
            call(lwe, key)
        assert e.value.kind == "NoDevice" and list(lwe) == list(range(1, 9))
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.glwe_encrypt(lwe, key, pfhe.FullComplex64FftTable(1))
    assert e.value.kind == "NoDevice"
