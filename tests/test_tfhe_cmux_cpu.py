"""CPU-side checks of the CMUX and the CMUX tree (pfhe_tfhe{,32}_cmux_tree_*, _cmux, _cmux_dev): the entry points are in the
ctypes table and the Python names exported, every refusal that precedes the device arrives in the stated order, and the
compiler's resource report shows the new kernels for both word types with no scratch memory, no spilled register and the
fused product's LDS."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("cmux_tree_create", "cmux_tree_destroy", "cmux_tree_in_use", "cmux_tree_scratch_bytes", "cmux_dev", "cmux",
         "cmux_tree_dev", "cmux_tree")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("TfheCmuxTreeContext", "tfhe_cmux", "tfhe_cmux_dev", "tfhe_cmux_tree", "tfhe_cmux_tree_dev")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36


def test_cmux_kernels_use_no_scratch_spill_nothing_and_keep_the_products_lds():
    import kernel_resources
    csrc = os.path.join(ROOT, "primus-fhe_amd", "csrc")
    with ThreadPoolExecutor(2) as ex:
        rows, fft_rows = ex.map(kernel_resources.report, [os.path.join(csrc, f) for f in ("pfhe_cmux.hip", "pfhe_fft.hip")])
    by_name = {r["pretty"]: r for r in rows}
    product = {r["pretty"]: r for r in fft_rows}
    words = ("unsigned int", "unsigned long long")
    want = ["tfhe_cmux_kernel<%s>" % w for w in words] + \
           ["tfhe_cmux_glue_kernel<%s, %s>" % (w, b) for w in words for b in ("false", "true")]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
    for w in words:
        # the digit spectrum is dynamic LDS sized by the launch (lds_bytes(log N), 17 KiB at N = 2^11), as the fused
        # product's: neither kernel declares any of its own
        fused = product["tfhe_fused_kernel<%s>" % w]
        assert by_name["tfhe_cmux_kernel<%s>" % w].get("LDS Size", 0) == fused.get("LDS Size", 0) == 0
        # four waves per SIMD, the rotation loop's figure: at most 128 registers
        assert by_name["tfhe_cmux_kernel<%s>" % w].get("VGPRs", 999) <= 128
        assert by_name["tfhe_cmux_kernel<%s>" % w].get("Occupancy", 0) >= 4
    recorded = open(os.path.join(ROOT, "profiles", "tfhe_cmux_a_kernel_resources.txt")).read()
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
    assert len(NAMES) == 16
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    for w in ("", "32"):
        for form in ("cmux", "cmux_tree"):
            dev, host = getattr(lib, f"pfhe_tfhe{w}_{form}_dev"), getattr(lib, f"pfhe_tfhe{w}_{form}")
            assert len(dev.argtypes) == len(host.argtypes) + 1
        assert getattr(lib, f"pfhe_tfhe{w}_cmux_tree_create").argtypes[2] == C.c_uint32
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_create_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the product plan's checks in their order (the basis's assert!s, Unsupported above 64, the table), then the depth, and
    only then the device; a refusal leaves the handle null"""
    lib = pfhe.lib()
    _, fft = table
    create = getattr(lib, f"pfhe_tfhe{w}_cmux_tree_create")
    h = C.c_void_p(1)
    k, lb, ell = 1, 7, 3
    assert create(fft, k, lb, ell, 3, 0, None) == BAD_ARGUMENT                       # nowhere to put the handle
    for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        h.value = 1
        assert create(None, 65, bad_lb, bad_len, 0, 0, C.byref(h)) == BAD_ARGUMENT   # whatever else is wrong
        assert not h.value
    assert create(None, 65, lb, ell, 0, 0, C.byref(h)) == UNSUPPORTED                # before the table and the depth
    assert "glwe_dimension above 64" in last_error(lib)
    assert create(None, k, lb, ell, 0, 0, C.byref(h)) == BAD_ARGUMENT                # no table, before the depth
    assert "depth" not in last_error(lib)
    for depth in (0, 17, 2 ** 40):
        h.value = 1
        assert create(fft, k, lb, ell, depth, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
        assert "depth must be in 1..16" in last_error(lib)
    for depth in (1, 16):
        h.value = 1
        assert create(fft, k, lb, ell, depth, 0, C.byref(h)) == NO_DEVICE and not h.value   # the last check
    assert create(fft, 2, lb, 0, 3, 5, C.byref(h)) == NO_DEVICE                      # the general form, the full length


@pytest.mark.parametrize("w", ["", "32"])
def test_calls_on_no_handle_are_refused(pfhe, w):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    keys = C.cast(buf, C.POINTER(C.c_double))
    assert getattr(lib, f"pfhe_tfhe{w}_cmux_dev")(None, ptr, 8, ptr, 8, keys, 8, 1, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_cmux")(None, ptr, 8, ptr, 8, keys, 8, 1, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_cmux_tree_dev")(None, ptr, 8, keys, 8, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_cmux_tree")(None, ptr, 8, keys, 8, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_cmux_tree_in_use")(None) == 0
    assert getattr(lib, f"pfhe_tfhe{w}_cmux_tree_scratch_bytes")(None) == 0
    getattr(lib, f"pfhe_tfhe{w}_cmux_tree_destroy")(None)


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.FullComplex64FftTable(3)
    assert e.value.kind == "NoDevice"
