"""CPU-side checks of ring packing (pfhe_ringpack{,32}_*): the 16 entry points are
in the ctypes table and the Python names exported, every refusal that precedes the device arrives in the stated order, calls
on no handle are refused, the C++ mirror class leaves exactly its own symbols undefined, and the compiler's resource report
shows the merge kernel for both word types with no scratch memory, no spilled register, no static LDS, at most 128
registers and four waves per SIMD."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("create", "destroy", "in_use", "scratch_bytes", "merge", "merge_dev", "pack", "pack_dev")
NAMES = [pre + g for pre in ("pfhe_ringpack_", "pfhe_ringpack32_") for g in CALLS]
PUBLIC = ("TfheRingPackContext", "glwe_ring_merge", "glwe_ring_merge_dev", "lwe_ring_pack", "lwe_ring_pack_dev")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36


def test_ring_pack_kernels_use_no_scratch_spill_nothing_and_stay_within_128_registers():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_ring_pack.hip"))
    by_name = {r["pretty"]: r for r in rows}
    words = ("unsigned int", "unsigned long long")
    # the merge kernel reads its children as GLWE nodes or, <W, true>, as LWE leaves through the embedding's index rule
    merge = ["tfhe_ring_merge_kernel<%s, %s>" % (w, leaf) for w in words for leaf in ("true", "false")]
    want = merge + ["tfhe_ring_prepare_kernel<%s>" % w for w in words]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        assert r.get("LDS Size", 0) == 0, r       # the digit spectrum and ACC are dynamic LDS sized by the launch
    for name in merge:
        # four waves per SIMD, the trace loop's class
        assert by_name[name].get("VGPRs", 999) <= 128
        assert by_name[name].get("Occupancy", 0) >= 4
    recorded = open(os.path.join(ROOT, "profiles", "tfhe_ring_pack_a_kernel_resources.txt")).read()
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
        for form in ("merge", "pack"):
            dev, host = getattr(lib, f"pfhe_ringpack{w}_{form}_dev"), getattr(lib, f"pfhe_ringpack{w}_{form}")
            assert len(dev.argtypes) == len(host.argtypes) + 1
        assert getattr(lib, f"pfhe_ringpack{w}_create").argtypes[2] == C.c_uint32
        assert len(getattr(lib, f"pfhe_ringpack{w}_create").argtypes) == 7
        assert getattr(lib, f"pfhe_ringpack{w}_merge_dev").argtypes[7] == C.c_uint32       # level
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    header = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "primus_ntt_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert name + "(" in header and "pub fn " + name + "(" in ffi, name


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_create_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """the product plan's checks in their order (the basis's assert!s, Unsupported above 64, the table), then dimension 0,
    then max_count 0 or above N, and only then the device; a refusal leaves the handle null"""
    lib = pfhe.lib()
    _, fft = table
    create = getattr(lib, f"pfhe_ringpack{w}_create")
    h = C.c_void_p(1)
    k, lb, ell, n = 1, 7, 3, 8
    assert create(fft, k, lb, ell, n, 0, None) == BAD_ARGUMENT                          # nowhere to put the handle
    for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        h.value = 1
        assert create(None, 65, bad_lb, bad_len, 0, 0, C.byref(h)) == BAD_ARGUMENT      # whatever else is wrong
        assert not h.value
    assert create(None, 65, lb, ell, 0, 0, C.byref(h)) == UNSUPPORTED                   # before the table
    assert "glwe_dimension above 64" in last_error(lib)
    assert create(None, k, lb, ell, n, 0, C.byref(h)) == BAD_ARGUMENT                   # no table
    h.value = 1
    assert create(fft, 0, lb, ell, 0, 0, C.byref(h)) == BAD_ARGUMENT and not h.value    # the dimension before max_count
    assert "glwe_dimension must be at least 1" in last_error(lib)
    for bad in (0, n + 1, 2 ** 40):
        h.value = 1
        assert create(fft, k, lb, ell, bad, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
        assert "max_count must be in 1..N" in last_error(lib)
    for max_count in (1, 3, n):
        for chunk in (0, 1, 5):
            h.value = 1
            assert create(fft, k, lb, ell, max_count, chunk, C.byref(h)) == NO_DEVICE and not h.value   # the last check
    assert create(fft, 2, lb, 0, n, 5, C.byref(h)) == NO_DEVICE                         # the general form, the full length


@pytest.mark.parametrize("w", ["", "32"])
def test_calls_on_no_handle_are_refused(pfhe, w):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    keys = C.cast(buf, C.POINTER(C.c_double))
    assert getattr(lib, f"pfhe_ringpack{w}_merge_dev")(None, ptr, 8, ptr, 8, keys, 8, 1, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_ringpack{w}_merge")(None, ptr, 8, ptr, 8, keys, 8, 1, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_ringpack{w}_pack_dev")(None, ptr, 8, keys, 8, 1, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_ringpack{w}_pack")(None, ptr, 8, keys, 8, 1, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_ringpack{w}_in_use")(None) == 0
    assert getattr(lib, f"pfhe_ringpack{w}_scratch_bytes")(None) == 0
    getattr(lib, f"pfhe_ringpack{w}_destroy")(None)


def test_mirror_class_leaves_exactly_its_own_symbols_undefined():
    """TfheRingPackT is a template only: the unit that instantiates it leaves undefined what a unit that only includes the
    header does (a subset of the 306 pinned by tests/test_cpp_header.py) plus the 16 of its own list"""
    import cpp_mirror
    support = os.path.join(ROOT, "tests", "support")
    own = set(open(os.path.join(support, "cpp_mirror_ringpack_symbols.txt")).read().split())
    assert own == set(NAMES)
    undefined = cpp_mirror.undefined_pfhe_symbols(os.path.join(support, "cpp_mirror_ringpack_instantiate.cpp"))
    old = cpp_mirror.mirror_symbols()
    assert len(old) == 306 and not own & old
    assert undefined - old == own, sorted((undefined - old) ^ own)
    text = open(os.path.join(ROOT, "include", "pfhe.hpp")).read()
    assert "class TfheRingPackT : public detail::Fns<W>::TfheRingPack" in text
    assert "using TfheRingPack = TfheRingPackT<uint64_t>;" in text and "using TfheRingPack32 = TfheRingPackT<uint32_t>;" in text


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.FullComplex64FftTable(3)
    assert e.value.kind == "NoDevice"
