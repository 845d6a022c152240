"""CPU-side checks of the many-LUT entries (pfhe_tfhe{,32}_modswitch_stride_dev, _bootstrap_create_many_lut,
_cbs_create_with): the entry points are in the ctypes table, declared in include/pfhe.h and mirrored in include/pfhe.hpp, the
Python names are exported, every refusal of the two creates and of the strided switch arrives before the device is touched
and in the stated order, and the compiler's resource report shows the stage kernels that do the many-LUT steps
(csrc/pfhe_tfhe_stages.hip: one kernel per stage for every form) for both word types with no scratch memory, no spilled
register and no LDS, as profiles/tfhe_stages_a_kernel_resources.txt records them."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("modswitch_stride_dev", "bootstrap_create_many_lut", "cbs_create_with")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("lwe_modulus_switch_strided_dev", "tfhe_many_lut_test_vector")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36
# the strided switch, the patterned accumulator and the multi-index extraction are arguments of these; with them in the file,
# the caller's-test-vector accumulator and the subtracting form of the extraction
KERNELS = ("tfhe_modswitch_kernel<%s>", "tfhe_const_acc_init_kernel<%s>", "tfhe_extract_kernel<%s, false>",
           "tfhe_acc_init_kernel<%s>", "tfhe_extract_kernel<%s, true>")


def test_many_lut_kernels_use_no_scratch_no_lds_and_spill_nothing():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_tfhe_stages.hip"))
    by_name = {r["pretty"]: r for r in rows}
    want = [kern % w for kern in KERNELS for w in ("unsigned int", "unsigned long long")]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    recorded = open(os.path.join(ROOT, "profiles", "tfhe_stages_a_kernel_resources.txt")).read()
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        assert r.get("LDS Size", 0) == 0, r
        line = next(l for l in recorded.splitlines() if l.startswith(name + " "))
        assert "spill   0 scratch    0" in line and line.rstrip().endswith("lds 0"), line


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


class TableStandIn(C.Structure):
    """What the library's table starts with: the device, log N and N.  With device -1 every call that passes its argument
    checks ends in NoDevice, the last check, so the order of the refusals before it can be seen without a GPU; nothing
    here owns device memory (the twiddle pointer stays null) and the library never frees a table it did not make."""
    _fields_ = [("device", C.c_int), ("log_n", C.c_uint32), ("n", C.c_size_t), ("tw", C.c_void_p)]


@pytest.fixture(scope="module")
def table():
    t = TableStandIn(-1, 3, 8, None)     # N = 8
    return t, C.cast(C.pointer(t), C.c_void_p)


def last_error(lib):
    return lib.pfhe_last_error().decode(errors="replace")


def test_symbols_are_in_the_ctypes_table_the_headers_and_the_package(pfhe):
    lib = pfhe.lib()
    header = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    import cpp_mirror
    mirror = cpp_mirror.mirror_symbols()       # tied to the compiled include/pfhe.hpp by test_cpp_header.py
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
        assert "int %s(" % name in header and name in mirror, name
    for w in ("", "32"):
        plain, strided = getattr(lib, f"pfhe_tfhe{w}_modswitch_dev"), getattr(lib, f"pfhe_tfhe{w}_modswitch_stride_dev")
        assert len(strided.argtypes) == len(plain.argtypes) + 1 and strided.argtypes[5] == C.c_uint32
        multibit, many = (getattr(lib, f"pfhe_tfhe{w}_bootstrap_create_{g}") for g in ("multibit", "many_lut"))
        assert len(many.argtypes) == len(multibit.argtypes) + 1 and many.argtypes[9] == C.c_uint32
        create, with_ = getattr(lib, f"pfhe_tfhe{w}_cbs_create"), getattr(lib, f"pfhe_tfhe{w}_cbs_create_with")
        assert len(with_.argtypes) == len(create.argtypes) + 2 and with_.argtypes[10] == C.c_int
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    import inspect
    assert inspect.signature(pfhe.TfheBootstrapContext.__init__).parameters["log_luts"].default == 0
    params = inspect.signature(pfhe.TfheCircuitBootstrapContext.__init__).parameters
    assert params["grouping_factor"].default == 1 and params["shared_rotation"].default is False


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_strided_switch_refuses_its_arguments_in_order(pfhe, w, bits):
    """log_n, log_stride above log_n, lwe_dimension, the lengths, the empty batch, null pointers, and only then the device"""
    lib = pfhe.lib()
    call = getattr(lib, f"pfhe_tfhe{w}_modswitch_stride_dev")
    buf = (C.c_uint64 * 256)()
    ptr = C.cast(buf, C.c_void_p)
    exps, neg_b = C.c_void_p(ptr.value + 512), C.c_void_p(ptr.value + 1024)
    n, batch = 5, 3
    for log_n in (0, 15):
        assert call(-1, None, 7, 0, log_n, 99, None, 1, None, 1, None) == BAD_ARGUMENT          # whatever else is wrong
        assert "log_n must be in 1..14" in last_error(lib)
    for log_n, stride in ((1, 2), (10, 11), (14, 2 ** 31)):
        assert call(-1, None, 7, 0, log_n, stride, None, 1, None, 1, None) == BAD_ARGUMENT      # before lwe_dimension
        assert "log_stride must be at most log_n" in last_error(lib)
    for dim in (0, 2 ** 32 - 1):
        assert call(-1, ptr, 7, dim, 10, 10, exps, 1, neg_b, 1, None) == BAD_ARGUMENT
        assert "lwe_dimension" in last_error(lib)
    good = (batch * (n + 1), n, 10, 3)
    assert call(-1, ptr, good[0] + 1, *good[1:], exps, batch * n, neg_b, batch, None) == BAD_LENGTH
    assert call(-1, ptr, *good, exps, batch * n + 1, neg_b, batch, None) == BAD_LENGTH
    assert call(-1, ptr, *good, exps, batch * n, neg_b, batch + 1, None) == BAD_LENGTH
    assert call(-1, None, 0, n, 10, 3, None, 0, None, 0, None) == 0                              # an empty batch is a no-op
    for args in ((None, exps, neg_b), (ptr, None, neg_b), (ptr, exps, None)):
        assert call(-1, args[0], *good, args[1], batch * n, args[2], batch, None) == BAD_ARGUMENT
    for stride in (0, 3, 10):
        assert call(-1, ptr, good[0], n, 10, stride, exps, batch * n, neg_b, batch, None) == NO_DEVICE   # the last check


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_bootstrap_create_many_lut_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """a null out pointer; the rotation's checks in their order (the basis's assert!s, Unsupported above 64, the table, g
    outside the multi-bit range), the divisibility, log_luts above log N; a refusal leaves the handle null.  What follows
    (the dimensions, the key switch's basis) is decided by the rotation's create on the device, as in the existing creates."""
    lib = pfhe.lib()
    _, fft = table
    create = getattr(lib, f"pfhe_tfhe{w}_bootstrap_create_many_lut")
    h = C.c_void_p(1)
    n, k, lb, ell = 6, 1, 7, 3
    assert create(fft, k, lb, ell, n, 4, 2, 1, 0, 1, 0, None) == BAD_ARGUMENT                       # nowhere to put the handle
    for g in (0, 1, 2):
        for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
            h.value = 1
            assert create(None, 65, bad_lb, bad_len, 0, 0, 0, 0, g, 99, 0, C.byref(h)) == BAD_ARGUMENT   # whatever else is wrong
            assert not h.value
        assert create(None, 65, lb, ell, 0, 0, 0, 0, g, 99, 0, C.byref(h)) == UNSUPPORTED             # before the table
        assert create(None, k, lb, ell, n, 4, 2, 1, g, 1, 0, C.byref(h)) == BAD_ARGUMENT              # no table
    for g in (5, 2 ** 40):
        assert create(fft, k, lb, ell, n, 4, 2, 1, g, 99, 0, C.byref(h)) == BAD_ARGUMENT              # before log_luts
        assert "grouping_factor must be in 1..4" in last_error(lib)
    assert create(fft, k, lb, ell, 7, 4, 2, 1, 2, 99, 0, C.byref(h)) == BAD_ARGUMENT                  # before log_luts
    assert "multiple of grouping_factor" in last_error(lib)
    for g in (0, 1, 2):
        for luts in (4, 15, 2 ** 31):                                                                 # log N = 3
            h.value = 1
            assert create(fft, k, lb, ell, n, 4, 2, 1, g, luts, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
            assert "log_luts must be at most log N" in last_error(lib)
        for luts in (0, 1, 3):
            h.value = 1
            assert create(fft, k, lb, ell, n, 4, 2, 1, g, luts, 0, C.byref(h)) == NO_DEVICE and not h.value   # the last check


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_cbs_create_with_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the existing create's order with the options' refusals in their places: a null out pointer; the rotation's checks (the
    basis's assert!s, Unsupported above 64, the table, g outside the multi-bit range); lwe_dimension no multiple of g; the
    dimensions; the two other bases' assert!s; drop_bits of the output basis; ell_cb above N with a shared rotation; and only
    then the device"""
    lib = pfhe.lib()
    _, fft = table
    create = getattr(lib, f"pfhe_tfhe{w}_cbs_create_with")
    h = C.c_void_p(1)
    n, k, lb, ell = 6, 1, 7, 3
    good = (4, 3, 4, 2)                  # the output basis (3 levels, drop_bits BITS - 12) and the key switch's
    assert create(fft, k, lb, ell, n, *good, 2, 1, 0, None) == BAD_ARGUMENT                          # nowhere to put the handle
    for g, shared in ((0, 0), (1, 1), (2, 0), (2, 1)):
        for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
            h.value = 1
            assert create(None, 65, bad_lb, bad_len, 0, 0, 0, 0, 0, g, shared, 0, C.byref(h)) == BAD_ARGUMENT
            assert not h.value
        assert create(None, 65, lb, ell, 0, 0, 0, 0, 0, g, shared, 0, C.byref(h)) == UNSUPPORTED     # before the table
        assert create(None, k, lb, ell, n, *good, g, shared, 0, C.byref(h)) == BAD_ARGUMENT          # no table
    for g in (5, 2 ** 40):
        assert create(fft, 0, lb, ell, 0, 0, 0, 0, 0, g, 1, 0, C.byref(h)) == BAD_ARGUMENT           # before the dimensions
        assert "grouping_factor must be in 1..4" in last_error(lib)
    for g, dim in ((2, 7), (3, 4), (4, 6)):
        assert create(fft, 0, lb, ell, dim, 0, 0, 0, 0, g, 1, 0, C.byref(h)) == BAD_ARGUMENT         # before the dimensions
        assert "multiple of grouping_factor" in last_error(lib)
    for g, shared in ((1, 1), (2, 0), (2, 1)):
        for kk, dim in ((0, n), (k, 0), (k, 2 ** 31)):                                                # multiples of g
            assert create(fft, kk, lb, ell, dim, 0, 0, 0, 0, g, shared, 0, C.byref(h)) == BAD_ARGUMENT   # before the other bases
            assert "glwe_dimension must be at least 1 and lwe_dimension in 1..2^31-2" in last_error(lib)
        for cb in ((0, 1), (bits, 1), (4, bits // 4 + 1)):
            assert create(fft, k, lb, ell, n, *cb, 0, 0, g, shared, 0, C.byref(h)) == BAD_ARGUMENT   # before the key switch's
        for pf in ((0, 1), (bits, 1), (4, bits // 4 + 1)):
            assert create(fft, k, lb, ell, n, 4, 0, *pf, g, shared, 0, C.byref(h)) == BAD_ARGUMENT   # before drop_bits
            assert "drop" not in last_error(lib)
        for cb in ((4, 0), (4, bits // 4), (1, bits)):
            assert create(fft, k, lb, ell, n, *cb, 4, 2, g, shared, 0, C.byref(h)) == BAD_ARGUMENT   # before ell_cb > N
            assert "must drop at least one bit" in last_error(lib)
    # ell_cb above N = 8: refused with a shared rotation only, last before the device
    for g in (1, 2):
        h.value = 1
        assert create(fft, k, lb, ell, n, 3, 9, 4, 2, g, 1, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
        assert "at most N levels" in last_error(lib)
        assert create(fft, k, lb, ell, n, 3, 9, 4, 2, g, 0, 0, C.byref(h)) == NO_DEVICE
        assert create(fft, k, lb, ell, n, 3, 8, 4, 2, g, 1, 0, C.byref(h)) == NO_DEVICE              # ell_cb = N
    for g, shared in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (4, 1)):
        h.value = 1
        dim = 8 if g == 4 else n
        assert create(fft, k, lb, ell, dim, *good, g, shared, 3, C.byref(h)) == NO_DEVICE and not h.value   # the last check


@pytest.mark.parametrize("w", ["", "32"])
def test_calls_on_no_handle_are_refused(pfhe, w):
    """the handles of the new creates are the existing ones: their calls refuse a null handle as before"""
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    bsk = C.cast(buf, C.POINTER(C.c_double))
    assert getattr(lib, f"pfhe_tfhe{w}_cbs_dev")(None, ptr, 8, bsk, 8, ptr, 8, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_cbs")(None, ptr, 8, bsk, 8, ptr, 8, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_bootstrap_dev")(None, ptr, 8, bsk, 8, ptr, 8, ptr, 8, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_bootstrap")(None, ptr, 8, bsk, 8, ptr, 8, ptr, 8, ptr, 8) == BAD_ARGUMENT
    for pre in ("cbs", "bootstrap"):
        assert getattr(lib, f"pfhe_tfhe{w}_{pre}_in_use")(None) == 0
        assert getattr(lib, f"pfhe_tfhe{w}_{pre}_scratch_bytes")(None) == 0
        getattr(lib, f"pfhe_tfhe{w}_{pre}_destroy")(None)


def test_python_contexts_check_the_widths_before_the_library(pfhe):
    b32, b64 = pfhe.ApproxSignedBasis(32, 4, 3), pfhe.ApproxSignedBasis(64, 4, 3)
    with pytest.raises(TypeError):
        pfhe.TfheCircuitBootstrapContext(None, b32, 4, 1, b64, b32, grouping_factor=2, shared_rotation=True)
    with pytest.raises(TypeError):
        pfhe.TfheBootstrapContext(None, b32, 4, 1, b64, log_luts=1)
    with pytest.raises(ValueError):
        import torch
        pfhe.tfhe_many_lut_test_vector(torch.zeros((3, 2, 8), dtype=torch.int64))
