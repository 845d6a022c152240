"""CPU-side checks of the circuit bootstrap (pfhe_tfhe{,32}_private_keyswitch*, _pfksk_generate_dev, _cbs_*): the entry points
are in the ctypes table and the Python names exported, every refusal arrives before the device is touched and in the stated
order, and the compiler's resource report shows the new kernels for both word types with no scratch memory, no spilled
register and the stated LDS size."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("private_keyswitch_dev", "private_keyswitch", "pfksk_generate_dev", "cbs_create", "cbs_destroy", "cbs_in_use",
         "cbs_scratch_bytes", "cbs_dev", "cbs")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("lwe_private_keyswitch", "lwe_private_keyswitch_dev", "tfhe_generate_pfksk_dev", "TfheCircuitBootstrapContext",
          "tfhe_circuit_bootstrap", "tfhe_circuit_bootstrap_dev")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36


def test_cbs_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources
    csrc = os.path.join(ROOT, "primus-fhe_amd", "csrc")
    by_name = {r["pretty"]: r for r in kernel_resources.report(os.path.join(csrc, "pfhe_cbs.hip"))}
    words = ("unsigned int", "unsigned long long")
    want = [kern % w for kern in ("tfhe_pfks_kernel<%s>", "tfhe_pfksk_add_message_kernel<%s>") for w in words]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    # the switch, the accumulator from constants and the extraction are the stage kernels of csrc/pfhe_tfhe_stages.hip
    stages = {r["pretty"]: r for r in kernel_resources.report(os.path.join(csrc, "pfhe_tfhe_stages.hip"))}
    staged = [kern % w for kern in ("tfhe_modswitch_kernel<%s>", "tfhe_const_acc_init_kernel<%s>",
                                    "tfhe_extract_kernel<%s, false>") for w in words]
    by_name.update({name: stages[name] for name in staged})
    want += staged
    for name in want:
        assert by_name[name].get("ScratchSize", 0) == 0 and by_name[name].get("VGPRs Spill", 0) == 0, by_name[name]
        assert by_name[name].get("SGPRs Spill", 0) == 0, by_name[name]
    # the key switch: the digits of 64 key rows x 32 ciphertexts, whatever the shape; the other kernels use no LDS
    for w, size in (("unsigned int", 4), ("unsigned long long", 8)):
        assert by_name["tfhe_pfks_kernel<%s>" % w].get("LDS Size", 0) == 64 * 32 * size
    for name in want[2:]:
        assert by_name[name].get("LDS Size", 0) == 0, name


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


def test_symbols_are_in_the_ctypes_table_and_the_package(pfhe):
    assert len(NAMES) == 18
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    for w in ("", "32"):
        for form in ("private_keyswitch", "cbs"):
            dev, host = getattr(lib, f"pfhe_tfhe{w}_{form}_dev"), getattr(lib, f"pfhe_tfhe{w}_{form}")
            assert len(dev.argtypes) == len(host.argtypes) + 1
        assert getattr(lib, f"pfhe_tfhe{w}_private_keyswitch_dev").argtypes[8] == C.c_uint32
        assert [getattr(lib, f"pfhe_tfhe{w}_cbs_create").argtypes[i] for i in (2, 5, 7)] == [C.c_uint32] * 3
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_private_key_switch_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the basis's assert!s, the dimensions, the table, levels, the lengths, the empty batch, null pointers, overlap (device
    form only), and only then the device"""
    lib = pfhe.lib()
    _, fft = table
    buf = (C.c_uint64 * 16384)()
    ptr = C.cast(buf, C.c_void_p)
    key = C.c_void_p(ptr.value + 8192)
    out = C.c_void_p(ptr.value + 65536)
    n, k, in_dim, ell, levels = 8, 1, 4, 2, 3
    len_in, len_key = 2 * levels * (in_dim + 1), (k + 1) * (in_dim + 1) * ell * (k + 1) * n
    len_out = 2 * (k + 1) * levels * (k + 1) * n
    for form, tail in (("private_keyswitch_dev", (None,)), ("private_keyswitch", ())):
        call = getattr(lib, f"pfhe_tfhe{w}_{form}")
        # ApproxSignedBasis::new's assert!s first, whatever else is wrong
        for lb, length in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
            assert call(None, 0, None, 7, 0, 0, None, 1, lb, length, None, 3, *tail) == BAD_ARGUMENT, (w, lb, length)
        for kk, dim in ((0, in_dim), (65, in_dim), (k, 0), (k, 2 ** 31 - 1)):
            assert call(None, kk, None, 7, dim, 0, None, 1, 4, ell, None, 3, *tail) == BAD_ARGUMENT
            assert "glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2" in last_error(lib)
        assert call(None, k, ptr, len_in, in_dim, levels, key, len_key, 4, ell, out, len_out, *tail) == BAD_ARGUMENT   # no table
        for lv in (0, 65, 2 ** 40):
            assert call(fft, k, None, 7, in_dim, lv, None, 1, 4, ell, None, 3, *tail) == BAD_ARGUMENT
            assert "levels must be in 1..64" in last_error(lib)
        assert call(fft, k, ptr, len_in + 1, in_dim, levels, key, len_key, 4, ell, out, len_out, *tail) == BAD_LENGTH
        assert call(fft, k, ptr, len_in, in_dim, levels, key, len_key - 1, 4, ell, out, len_out, *tail) == BAD_LENGTH
        assert call(fft, k, ptr, len_in, in_dim, levels, key, len_key, 4, ell, out, len_out - 1, *tail) == BAD_LENGTH
        assert call(fft, k, ptr, len_in, in_dim, levels, key, len_key, 4, 0, out, len_out, *tail) == BAD_LENGTH  # the full length
        assert "batch*levels*(in_dimension+1)" in last_error(lib)
        # one ciphertext of the group missing: the batch is counted in groups of `levels`
        assert call(fft, k, ptr, len_in - (in_dim + 1), in_dim, levels, key, len_key, 4, ell, out, len_out, *tail) == BAD_LENGTH
        assert call(fft, k, None, 0, in_dim, levels, None, len_key, 4, ell, None, 0, *tail) == 0    # an empty batch is a no-op
        for args in ((None, key, out), (ptr, None, out), (ptr, key, None)):
            assert call(fft, k, args[0], len_in, in_dim, levels, args[1], len_key, 4, ell, args[2], len_out, *tail) == BAD_ARGUMENT
        assert call(fft, k, ptr, len_in, in_dim, levels, key, len_key, 4, ell, out, len_out, *tail) == NO_DEVICE   # the last check
    dev, host = getattr(lib, f"pfhe_tfhe{w}_private_keyswitch_dev"), getattr(lib, f"pfhe_tfhe{w}_private_keyswitch")
    for a, b in ((ptr, key), (key, ptr)):
        assert dev(fft, k, a, len_in, in_dim, levels, b, len_key, 4, ell, ptr, len_out, None) == BAD_ARGUMENT
        assert last_error(lib) == "private key switch: the output must not overlap an input"
        assert host(fft, k, a, len_in, in_dim, levels, b, len_key, 4, ell, ptr, len_out) == NO_DEVICE   # it stages
    assert dev(fft, k, ptr, len_in, in_dim, levels, ptr, len_key, 4, ell, out, len_out, None) == NO_DEVICE  # inputs may overlap


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_key_call_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the packing key's order: the basis's assert!s, the dimensions (and the table), the lengths, null pointers, overlap,
    the size of the launch, the device"""
    lib = pfhe.lib()
    _, fft = table
    call = getattr(lib, f"pfhe_tfhe{w}_pfksk_generate_dev")
    buf = (C.c_uint64 * 16384)()
    ptr = C.cast(buf, C.c_void_p)
    z = C.c_void_p(ptr.value + 1024)
    far = C.c_void_p(ptr.value + 8192)
    n, k, in_dim, ell = 8, 1, 4, 3
    length = (k + 1) * (in_dim + 1) * ell * (k + 1) * n
    for lb, levels in ((0, 0), (bits, 0), (4, bits // 4 + 1)):
        assert call(None, 0, None, 0, None, 0, lb, levels, None, 5, None) == BAD_ARGUMENT
    for kk, dim in ((0, in_dim), (65, in_dim), (k, 0), (k, 2 ** 31 - 1)):
        assert call(None, kk, None, dim, None, 3, 4, ell, None, 5, None) == BAD_ARGUMENT
        assert "glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2" in last_error(lib)
    assert call(None, k, ptr, in_dim, z, k * n, 4, ell, far, length, None) == BAD_ARGUMENT       # no table
    assert call(fft, k, ptr, in_dim, z, k * n + 1, 4, ell, far, length, None) == BAD_LENGTH
    assert call(fft, k, ptr, in_dim, z, k * n, 4, ell, far, length + 1, None) == BAD_LENGTH
    assert call(fft, k, ptr, in_dim, z, k * n, 4, ell, far, in_dim * ell * (k + 1) * n, None) == BAD_LENGTH   # a packing key
    assert call(fft, k, ptr, in_dim, z, k * n, 4, 0, far, length, None) == BAD_LENGTH            # length 0: the full BITS / 4
    assert "(k+1)*(in_dimension+1)*ell*(k+1)*N" in last_error(lib)
    for args in ((None, z, far), (ptr, None, far), (ptr, z, None)):
        assert call(fft, k, args[0], in_dim, args[1], k * n, 4, ell, args[2], length, None) == BAD_ARGUMENT
    for key_in, glwe_key in ((far, z), (ptr, far)):
        assert call(fft, k, key_in, in_dim, glwe_key, k * n, 4, ell, far, length, None) == BAD_ARGUMENT
        assert last_error(lib) == "private key-switch key: the keys must not overlap pfksk"
    assert call(fft, k, ptr, in_dim, ptr, k * n, 4, ell, far, length, None) == NO_DEVICE        # the last check
    # 2^30 * 3 * 2 rows are more than a launch takes: judged after the overlap and before the device; pointers never followed
    at = lambda a: C.c_void_p(a)
    big = (k + 1) * (2 ** 30 + 1) * ell * (k + 1) * n
    assert call(fft, k, at(2 ** 40), 2 ** 30, at(2 ** 41), k * n, 4, ell, at(2 ** 44), big, None) == BAD_LENGTH
    assert call(fft, k, at(2 ** 44), 2 ** 30, at(2 ** 41), k * n, 4, ell, at(2 ** 44), big, None) == BAD_ARGUMENT


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_cbs_create_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the rotation's checks in their order (the basis's assert!s, Unsupported above 64, the table), then the dimensions, the
    two other bases' assert!s and the output basis's drop_bits, and only then the device; a refusal leaves the handle null"""
    lib = pfhe.lib()
    _, fft = table
    create = getattr(lib, f"pfhe_tfhe{w}_cbs_create")
    h = C.c_void_p(1)
    n, k, lb, ell = 5, 1, 7, 3
    good = (4, 3, 4, 2)                  # the output basis (drop_bits BITS - 12) and the key switch's
    assert create(fft, k, lb, ell, n, *good, 0, None) == BAD_ARGUMENT                              # nowhere to put the handle
    for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        h.value = 1
        assert create(None, 65, bad_lb, bad_len, 0, 0, 0, 0, 0, 0, C.byref(h)) == BAD_ARGUMENT   # whatever else is wrong
        assert not h.value
    assert create(None, 65, lb, ell, 0, 0, 0, 0, 0, 0, C.byref(h)) == UNSUPPORTED                 # before the table
    assert create(None, k, lb, ell, n, *good, 0, C.byref(h)) == BAD_ARGUMENT                      # no table
    for kk, dim in ((0, n), (k, 0), (k, 2 ** 31 - 1)):
        assert create(fft, kk, lb, ell, dim, 0, 0, 0, 0, 0, C.byref(h)) == BAD_ARGUMENT            # before the other bases
        assert "glwe_dimension must be at least 1 and lwe_dimension in 1..2^31-2" in last_error(lib)
    for cb in ((0, 1), (bits, 1), (4, bits // 4 + 1)):
        assert create(fft, k, lb, ell, n, *cb, 0, 0, 0, C.byref(h)) == BAD_ARGUMENT                # before the key switch's basis
    for pf in ((0, 1), (bits, 1), (4, bits // 4 + 1)):
        assert create(fft, k, lb, ell, n, 4, 0, *pf, 0, C.byref(h)) == BAD_ARGUMENT                # before drop_bits
        assert "drop" not in last_error(lib)
    for cb in ((4, 0), (4, bits // 4), (1, bits)):
        assert create(fft, k, lb, ell, n, *cb, 4, 2, 0, C.byref(h)) == BAD_ARGUMENT
        assert "must drop at least one bit" in last_error(lib)
    h.value = 1
    assert create(fft, k, lb, ell, n, *good, 0, C.byref(h)) == NO_DEVICE and not h.value          # the last check
    assert create(fft, k, lb, ell, n, *good, 3, C.byref(h)) == NO_DEVICE


@pytest.mark.parametrize("w", ["", "32"])
def test_calls_on_no_handle_are_refused(pfhe, w):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    bsk = C.cast(buf, C.POINTER(C.c_double))
    assert getattr(lib, f"pfhe_tfhe{w}_cbs_dev")(None, ptr, 8, bsk, 8, ptr, 8, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_cbs")(None, ptr, 8, bsk, 8, ptr, 8, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_cbs_in_use")(None) == 0
    assert getattr(lib, f"pfhe_tfhe{w}_cbs_scratch_bytes")(None) == 0
    getattr(lib, f"pfhe_tfhe{w}_cbs_destroy")(None)


def test_python_context_checks_the_widths_before_the_library(pfhe):
    b32, b64 = pfhe.ApproxSignedBasis(32, 4, 3), pfhe.ApproxSignedBasis(64, 4, 3)
    with pytest.raises(TypeError):
        pfhe.TfheCircuitBootstrapContext(None, b32, 4, 1, b64, b32)
    with pytest.raises(TypeError):
        pfhe.TfheCircuitBootstrapContext(None, b64, 4, 1, b64, b32)


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.FullComplex64FftTable(3)
    assert e.value.kind == "NoDevice"
