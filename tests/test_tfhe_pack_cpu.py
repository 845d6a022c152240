"""CPU-side checks of packing (pfhe_tfhe{,32}_pack_keyswitch*, _pksk_generate_dev, _sample_extract_first_few*,
_multimsg_extract*): the entry points are in the ctypes table and the Python names exported, every refusal arrives before
the device is touched and in the stated order, and the compiler's resource report shows the new kernels for both word
types with no scratch memory and no spilled register."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("pack_keyswitch_dev", "pack_keyswitch", "pksk_generate_dev", "sample_extract_first_few_dev",
         "sample_extract_first_few", "multimsg_extract_dev", "multimsg_extract")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("lwe_pack_keyswitch", "lwe_pack_keyswitch_dev", "tfhe_generate_pksk_dev", "glwe_sample_extract_first_few",
          "glwe_sample_extract_first_few_dev", "multimsg_lwe_extract", "multimsg_lwe_extract_dev")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE = 32, 33, 34


def test_pack_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_pack.hip"))
    by_name = {r["pretty"]: r for r in rows}
    words = ("unsigned int", "unsigned long long")
    want = ["tfhe_pack_keyswitch_kernel<%s, %d>" % (w, u) for w in words for u in (2, 4)]
    want += ["%s<%s>" % (kern, w) for kern in ("tfhe_pksk_add_message_kernel", "tfhe_extract_first_few_kernel",
                                               "tfhe_multimsg_extract_kernel") for w in words]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    for name in want:
        assert by_name[name].get("ScratchSize", 0) == 0 and by_name[name].get("VGPRs Spill", 0) == 0, by_name[name]
    # the packing key switch: a window of 256 + 1024 words and 4096 digit words, whatever the shape
    for w, size in (("unsigned int", 4), ("unsigned long long", 8)):
        for u in (2, 4):
            assert by_name["tfhe_pack_keyswitch_kernel<%s, %d>" % (w, u)].get("LDS Size", 0) == (256 + 1024 + 4096) * size


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
    assert len(NAMES) == 14
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    for form in ("pack_keyswitch", "sample_extract_first_few", "multimsg_extract"):
        for w in ("", "32"):
            dev, host = getattr(lib, f"pfhe_tfhe{w}_{form}_dev"), getattr(lib, f"pfhe_tfhe{w}_{form}")
            assert len(dev.argtypes) == len(host.argtypes) + 1
    assert lib.pfhe_tfhe32_pack_keyswitch_dev.argtypes[8] == C.c_uint32
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_packing_key_switch_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the basis's assert!s, the dimensions, the table, count, the lengths, the empty batch, null pointers and overlap,
    and only then the device"""
    lib = pfhe.lib()
    _, fft = table
    buf = (C.c_uint64 * 8192)()
    ptr = C.cast(buf, C.c_void_p)
    key = C.c_void_p(ptr.value + 8192)
    out = C.c_void_p(ptr.value + 40960)
    n, k, in_dim, ell, count = 8, 1, 4, 2, 3
    len_in, len_key, len_out = 2 * count * (in_dim + 1), in_dim * ell * (k + 1) * n, 2 * (k + 1) * n
    for form, tail in (("pack_keyswitch_dev", (None,)), ("pack_keyswitch", ())):
        call = getattr(lib, f"pfhe_tfhe{w}_{form}")
        # ApproxSignedBasis::new's assert!s first, whatever else is wrong
        for lb, length in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
            assert call(None, 0, None, 7, 0, 0, None, 1, lb, length, None, 3, *tail) == BAD_ARGUMENT, (w, lb, length)
        for kk, dim in ((0, in_dim), (65, in_dim), (k, 0), (k, 2 ** 31 - 1)):
            assert call(None, kk, None, 7, dim, 0, None, 1, 4, ell, None, 3, *tail) == BAD_ARGUMENT
            assert "glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2" in last_error(lib)
        assert call(None, k, ptr, len_in, in_dim, count, key, len_key, 4, ell, out, len_out, *tail) == BAD_ARGUMENT   # no table
        for c in (0, n + 1, 2 ** 40):
            assert call(fft, k, None, 7, in_dim, c, None, 1, 4, ell, None, 3, *tail) == BAD_ARGUMENT
            assert "count must be in 1..N" in last_error(lib)
        assert call(fft, k, ptr, len_in + 1, in_dim, count, key, len_key, 4, ell, out, len_out, *tail) == BAD_LENGTH
        assert call(fft, k, ptr, len_in, in_dim, count, key, len_key - 1, 4, ell, out, len_out, *tail) == BAD_LENGTH
        assert call(fft, k, ptr, len_in, in_dim, count, key, len_key, 4, ell, out, len_out - 1, *tail) == BAD_LENGTH
        assert call(fft, k, ptr, len_in, in_dim, count, key, len_key, 4, 0, out, len_out, *tail) == BAD_LENGTH  # the full length
        assert "batch*count*(in_dimension+1)" in last_error(lib)
        assert call(fft, k, None, 0, in_dim, count, None, len_key, 4, ell, None, 0, *tail) == 0      # an empty batch is a no-op
        for args in ((None, key, out), (ptr, None, out), (ptr, key, None)):
            assert call(fft, k, args[0], len_in, in_dim, count, args[1], len_key, 4, ell, args[2], len_out, *tail) == BAD_ARGUMENT
        assert call(fft, k, ptr, len_in, in_dim, count, key, len_key, 4, ell, out, len_out, *tail) == NO_DEVICE   # the last check
    dev = getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_dev")
    assert dev(fft, k, ptr, len_in, in_dim, count, key, len_key, 4, ell, ptr, len_out, None) == BAD_ARGUMENT
    assert "overlap" in last_error(lib)
    assert dev(fft, k, ptr, len_in, in_dim, count, key, len_key, 4, ell, key, len_out, None) == BAD_ARGUMENT
    assert "overlap" in last_error(lib)


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_the_packing_key_call_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the key-switch key's order: the basis's assert!s, the dimensions (and the table), the lengths, null pointers, overlap,
    the device"""
    lib = pfhe.lib()
    _, fft = table
    call = getattr(lib, f"pfhe_tfhe{w}_pksk_generate_dev")
    buf = (C.c_uint64 * 8192)()
    ptr = C.cast(buf, C.c_void_p)
    z = C.c_void_p(ptr.value + 1024)
    far = C.c_void_p(ptr.value + 8192)
    n, k, in_dim, ell = 8, 1, 4, 3
    length = in_dim * ell * (k + 1) * n
    for lb, levels in ((0, 0), (bits, 0), (4, bits // 4 + 1)):
        assert call(None, 0, None, 0, None, 0, lb, levels, None, 5, None) == BAD_ARGUMENT
    for kk, dim in ((0, in_dim), (65, in_dim), (k, 0), (k, 2 ** 31 - 1)):
        assert call(None, kk, None, dim, None, 3, 4, ell, None, 5, None) == BAD_ARGUMENT
        assert "glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2" in last_error(lib)
    assert call(None, k, ptr, in_dim, z, k * n, 4, ell, far, length, None) == BAD_ARGUMENT       # no table
    assert call(fft, k, ptr, in_dim, z, k * n + 1, 4, ell, far, length, None) == BAD_LENGTH
    assert call(fft, k, ptr, in_dim, z, k * n, 4, ell, far, length + 1, None) == BAD_LENGTH
    assert call(fft, k, ptr, in_dim, z, k * n, 4, 0, far, length, None) == BAD_LENGTH            # length 0: the full BITS / 4
    assert "in_dimension*ell*(k+1)*N" in last_error(lib)
    for args in ((None, z, far), (ptr, None, far), (ptr, z, None)):
        assert call(fft, k, args[0], in_dim, args[1], k * n, 4, ell, args[2], length, None) == BAD_ARGUMENT
    assert call(fft, k, ptr, in_dim, z, k * n, 4, ell, ptr, length, None) == BAD_ARGUMENT and "overlap" in last_error(lib)
    assert call(fft, k, ptr, in_dim, z, k * n, 4, ell, far, length, None) == NO_DEVICE          # the last check


@pytest.mark.parametrize("w", ["", "32"])
def test_the_packing_calls_test_every_written_buffer_and_no_other(pfhe, table, w):
    """the packing key against either key, one at a time, and the size of its launch after the overlap; the host forms
    refuse no overlap, and inputs may overlap each other"""
    lib = pfhe.lib()
    _, fft = table
    gen = getattr(lib, f"pfhe_tfhe{w}_pksk_generate_dev")
    buf = (C.c_uint64 * 8192)()
    ptr = C.cast(buf, C.c_void_p)
    z, far = C.c_void_p(ptr.value + 1024), C.c_void_p(ptr.value + 8192)
    n, k, in_dim, ell, count = 8, 1, 4, 3, 3
    length = in_dim * ell * (k + 1) * n
    for key_in, glwe_key in ((far, z), (ptr, far)):
        assert gen(fft, k, key_in, in_dim, glwe_key, k * n, 4, ell, far, length, None) == BAD_ARGUMENT
        assert last_error(lib) == "packing key: the keys must not overlap pksk"
    assert gen(fft, k, ptr, in_dim, ptr, k * n, 4, ell, far, length, None) == NO_DEVICE
    # 2^30 * 3 rows are more than a launch takes: judged after the overlap and before the device; pointers never followed
    at = lambda a: C.c_void_p(a)
    big = 2 ** 30 * ell * (k + 1) * n
    assert gen(fft, k, at(2 ** 40), 2 ** 30, at(2 ** 41), k * n, 4, ell, at(2 ** 44), big, None) == BAD_LENGTH
    assert gen(fft, k, at(2 ** 44), 2 ** 30, at(2 ** 41), k * n, 4, ell, at(2 ** 44), big, None) == BAD_ARGUMENT
    len_in, len_key, len_out = 2 * count * (in_dim + 1), in_dim * ell * (k + 1) * n, 2 * (k + 1) * n
    dev, host = getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_dev"), getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch")
    assert dev(fft, k, ptr, len_in, in_dim, count, ptr, len_key, 4, ell, far, len_out, None) == NO_DEVICE
    for a, b in ((ptr, far), (far, ptr)):
        assert dev(fft, k, a, len_in, in_dim, count, b, len_key, 4, ell, ptr, len_out, None) == BAD_ARGUMENT
        assert last_error(lib) == "packing key switch: the output must not overlap an input"
        assert host(fft, k, a, len_in, in_dim, count, b, len_key, 4, ell, ptr, len_out) == NO_DEVICE
    glwe, multi, lwe = 2 * (k + 1) * n, 2 * (k * n + count), 2 * count * (k * n + 1)
    for name, len_a, len_b, text in (("sample_extract_first_few", glwe, multi, "multi-message extraction: the output must not overlap the input"),
                                     ("multimsg_extract", multi, lwe, "multi-message expansion: the output must not overlap the input")):
        assert getattr(lib, f"pfhe_tfhe{w}_{name}_dev")(fft, k, ptr, len_a, count, ptr, len_b, None) == BAD_ARGUMENT
        assert last_error(lib) == text
        assert getattr(lib, f"pfhe_tfhe{w}_{name}")(fft, k, ptr, len_a, count, ptr, len_b) == NO_DEVICE


@pytest.mark.parametrize("w", ["", "32"])
def test_the_multi_message_calls_refuse_their_arguments_in_order(pfhe, table, w):
    """the table, the dimension, count, the lengths, the empty batch, null pointers, overlap (device forms), the device"""
    lib = pfhe.lib()
    _, fft = table
    buf = (C.c_uint64 * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    far = C.c_void_p(ptr.value + 16384)
    n, k, count = 8, 2, 3
    glwe, multi, lwe = 2 * (k + 1) * n, 2 * (k * n + count), 2 * count * (k * n + 1)
    for name, len_a, len_b in (("sample_extract_first_few", glwe, multi), ("multimsg_extract", multi, lwe)):
        for form, tail in ((name + "_dev", (None,)), (name, ())):
            call = getattr(lib, f"pfhe_tfhe{w}_{form}")
            assert call(None, k, ptr, len_a, count, far, len_b, *tail) == BAD_ARGUMENT            # the table before anything
            for kk in (0, 65):
                assert call(fft, kk, None, 5, count, None, 3, *tail) == BAD_ARGUMENT
                assert "glwe_dimension must be in 1..64" in last_error(lib)
            for c in (0, n + 1):
                assert call(fft, k, None, 5, c, None, 3, *tail) == BAD_ARGUMENT
                assert "count must be in 1..N" in last_error(lib)
            assert call(fft, k, ptr, len_a + 1, count, far, len_b, *tail) == BAD_LENGTH
            assert call(fft, k, ptr, len_a, count, far, len_b + 1, *tail) == BAD_LENGTH
            assert call(fft, k, None, 0, count, None, 0, *tail) == 0                              # an empty batch is a no-op
            assert call(fft, k, None, len_a, count, far, len_b, *tail) == BAD_ARGUMENT
            assert call(fft, k, ptr, len_a, count, None, len_b, *tail) == BAD_ARGUMENT
            assert call(fft, k, ptr, len_a, count, far, len_b, *tail) == NO_DEVICE                # the last check
        dev = getattr(lib, f"pfhe_tfhe{w}_{name}_dev")
        assert dev(fft, k, ptr, len_a, count, ptr, len_b, None) == BAD_ARGUMENT and "overlap" in last_error(lib)


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.FullComplex64FftTable(3)
    assert e.value.kind == "NoDevice"
