"""CPU-side checks of the GLWE automorphism, the trace, their keys and the LWE embedding (pfhe_tfhe{,32}_glwe_trace_*,
_glwe_automorphism*, _gksk_generate_dev, _lwe_embed*): the 22 entry points are in the ctypes table and the Python names
exported, every refusal that precedes the device arrives in the stated order, and the compiler's resource report shows the
loop kernel for both word types with no scratch memory, no spilled register, no static LDS and at most 128 registers."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("glwe_trace_create", "glwe_trace_destroy", "glwe_trace_in_use", "glwe_trace_scratch_bytes", "glwe_automorphism",
         "glwe_automorphism_dev", "glwe_trace", "glwe_trace_dev", "gksk_generate_dev", "lwe_embed", "lwe_embed_dev")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("TfheGlweTraceContext", "glwe_automorphism", "glwe_automorphism_dev", "glwe_keyswitch", "glwe_keyswitch_dev",
          "glwe_trace", "glwe_trace_dev", "tfhe_generate_gksk_dev", "lwe_embed_glwe", "lwe_embed_glwe_dev")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36


def test_trace_kernels_use_no_scratch_spill_nothing_and_stay_within_128_registers():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_trace.hip"))
    by_name = {r["pretty"]: r for r in rows}
    words = ("unsigned int", "unsigned long long")
    per_word = ("tfhe_trace_loop_kernel", "tfhe_trace_gather_kernel", "tfhe_trace_sub_kernel", "tfhe_gksk_message_kernel",
                "tfhe_lwe_embed_kernel")
    want = ["%s<%s>" % (kern, w) for kern in per_word for w in words]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    # the general form's multiply-accumulate is the product's own kernel (pfhe_fft.hip), called with the k mask rows
    product = {r["pretty"]: r for r in kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_fft.hip"))}
    by_name["tfhe_mulacc_kernel"] = product["tfhe_mulacc_kernel"]
    want.append("tfhe_mulacc_kernel")
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        assert r.get("LDS Size", 0) == 0, r       # the digit spectrum and ACC are dynamic LDS sized by the launch
    for w in words:
        # four waves per SIMD, the rotation loop's class
        assert by_name["tfhe_trace_loop_kernel<%s>" % w].get("VGPRs", 999) <= 128
        assert by_name["tfhe_trace_loop_kernel<%s>" % w].get("Occupancy", 0) >= 4
    recorded = open(os.path.join(ROOT, "profiles", "tfhe_trace_a_kernel_resources.txt")).read()
    recorded += open(os.path.join(ROOT, "profiles", "tfhe_stages_a_kernel_resources.txt")).read()       # tfhe_mulacc_kernel
    for name in want:
        assert name in recorded, name


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


class TableStandIn(C.Structure):
    """What the library's table starts with: the device, log N and N.  With device -1 a create that passes its argument
    checks ends in NoDevice, the last check, so the order of the refusals before it can be seen without a GPU; nothing
    here owns device memory and the library never frees a table it did not make."""
    _fields_ = [("device", C.c_int), ("log_n", C.c_uint32), ("n", C.c_size_t), ("tw", C.c_void_p)]


@pytest.fixture(scope="module")
def table():
    t = TableStandIn(-1, 3, 8, None)     # N = 8
    return t, C.cast(C.pointer(t), C.c_void_p)


def last_error(lib):
    return lib.pfhe_last_error().decode(errors="replace")


def test_symbols_are_in_the_ctypes_table_and_the_package(pfhe):
    assert len(NAMES) == 22
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    for w in ("", "32"):
        for form in ("glwe_automorphism", "glwe_trace", "lwe_embed"):
            dev, host = getattr(lib, f"pfhe_tfhe{w}_{form}_dev"), getattr(lib, f"pfhe_tfhe{w}_{form}")
            assert len(dev.argtypes) == len(host.argtypes) + 1
        assert getattr(lib, f"pfhe_tfhe{w}_glwe_trace_create").argtypes[2] == C.c_uint32
        assert getattr(lib, f"pfhe_tfhe{w}_glwe_automorphism_dev").argtypes[5] == C.c_uint32       # t
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_create_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the product plan's checks in their order (the basis's assert!s, Unsupported above 64, the table), then dimension 0, and
    only then the device; a refusal leaves the handle null"""
    lib = pfhe.lib()
    _, fft = table
    create = getattr(lib, f"pfhe_tfhe{w}_glwe_trace_create")
    h = C.c_void_p(1)
    k, lb, ell = 1, 7, 3
    assert create(fft, k, lb, ell, 0, None) == BAD_ARGUMENT                          # nowhere to put the handle
    for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        h.value = 1
        assert create(None, 65, bad_lb, bad_len, 0, C.byref(h)) == BAD_ARGUMENT      # whatever else is wrong
        assert not h.value
    assert create(None, 65, lb, ell, 0, C.byref(h)) == UNSUPPORTED                   # before the table
    assert "glwe_dimension above 64" in last_error(lib)
    assert create(None, k, lb, ell, 0, C.byref(h)) == BAD_ARGUMENT                   # no table
    h.value = 1
    assert create(fft, 0, lb, ell, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
    assert "glwe_dimension must be at least 1" in last_error(lib)
    for chunk in (0, 1, 5):
        h.value = 1
        assert create(fft, k, lb, ell, chunk, C.byref(h)) == NO_DEVICE and not h.value   # the last check
    assert create(fft, 2, lb, 0, 5, C.byref(h)) == NO_DEVICE                         # the general form, the full length


@pytest.mark.parametrize("w", ["", "32"])
def test_calls_on_no_handle_are_refused(pfhe, w):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    keys = C.cast(buf, C.POINTER(C.c_double))
    assert getattr(lib, f"pfhe_tfhe{w}_glwe_automorphism_dev")(None, ptr, 8, keys, 8, 3, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_glwe_automorphism")(None, ptr, 8, keys, 8, 3, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_glwe_trace_dev")(None, ptr, 8, keys, 8, 1, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_glwe_trace")(None, ptr, 8, keys, 8, 1, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_glwe_trace_in_use")(None) == 0
    assert getattr(lib, f"pfhe_tfhe{w}_glwe_trace_scratch_bytes")(None) == 0
    getattr(lib, f"pfhe_tfhe{w}_glwe_trace_destroy")(None)


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_stateless_calls_refuse_their_values_before_the_device(pfhe, table, w, bits):
    lib = pfhe.lib()
    _, fft = table
    buf = (C.c_uint64 * 512)()
    ptr = C.cast(buf, C.c_void_p)
    out = C.cast(buf, C.POINTER(C.c_double))
    gen = getattr(lib, f"pfhe_tfhe{w}_gksk_generate_dev")
    ex = (C.c_uint32 * 2)(9, 5)
    k, lb, ell, n = 1, 7, 3, 8
    one = k * ell * (k + 1) * n
    assert gen(None, k, lb, ell, ptr, n, ptr, n, ex, 2, ptr, 2 * one, out, 2 * one, None) == BAD_ARGUMENT       # no table
    assert gen(fft, 0, lb, ell, ptr, 0, ptr, 0, ex, 2, ptr, 0, out, 0, None) == BAD_ARGUMENT
    assert "at least 1" in last_error(lib)
    for bad in ((C.c_uint32 * 2)(9, 4), (C.c_uint32 * 2)(17, 3), (C.c_uint32 * 2)(0, 3)):
        assert gen(fft, k, lb, ell, ptr, n, ptr, n, bad, 2, ptr, 2 * one, out, 2 * one, None) == BAD_ARGUMENT
        assert "odd and in 1..2N-1" in last_error(lib)
    assert gen(fft, k, lb, ell, ptr, n, ptr, n, ex, 2, ptr, 2 * one - 1, out, 2 * one - 1, None) == BAD_LENGTH
    assert gen(fft, k, lb, ell, ptr, n, ptr, n + 1, ex, 2, ptr, 2 * one, out, 2 * one, None) == BAD_LENGTH
    assert gen(fft, k, lb, ell, ptr, n, ptr, n, ex, 2, None, 2 * one, out, 2 * one, None) == BAD_ARGUMENT      # a null buffer
    embed_dev, embed = getattr(lib, f"pfhe_tfhe{w}_lwe_embed_dev"), getattr(lib, f"pfhe_tfhe{w}_lwe_embed")
    assert embed_dev(None, 1, ptr, n + 1, ptr, 2 * n, None) == BAD_ARGUMENT
    assert embed(fft, 0, ptr, n + 1, ptr, 2 * n) == BAD_ARGUMENT and embed(fft, 65, ptr, n + 1, ptr, 2 * n) == BAD_ARGUMENT
    assert embed(fft, 1, ptr, n + 2, ptr, 2 * n) == BAD_LENGTH and embed(fft, 1, ptr, n + 1, ptr, 2 * n + 1) == BAD_LENGTH
    assert embed(fft, 1, ptr, 0, ptr, 0) == 0                                                                 # nothing to do
    assert embed(fft, 1, None, n + 1, ptr, 2 * n) == BAD_ARGUMENT
    assert embed(fft, 1, ptr, n + 1, ptr, 2 * n) == NO_DEVICE                                                 # the last check


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.FullComplex64FftTable(3)
    assert e.value.kind == "NoDevice"
