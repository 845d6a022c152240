"""CPU-side checks of the packing key switch in the Fourier domain (pfhe_tfhe{,32}_packfft_plan_*, _packfft_key_dev,
_pack_keyswitch_fft*): the 14 entry points are in the ctypes table and the Python names exported, plan creation refuses its
arguments in the stated order before the device is touched, the calls refuse a missing plan, and the compiler's resource
report shows the new kernels with no scratch memory and no spilled register, as the committed report lists them.

A plan owns device memory, so none can be made here: what the packing calls refuse BEHIND a plan (count, the lengths, the
empty batch, null pointers, overlap) is checked where there is a device, in tests/test_gpu_tfhe_pack_fft.py."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("packfft_plan_create", "packfft_plan_destroy", "packfft_plan_in_use", "packfft_plan_scratch_bytes", "packfft_key_dev",
         "pack_keyswitch_fft_dev", "pack_keyswitch_fft")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("TfhePackFftContext", "tfhe_pack_key_fourier_dev", "lwe_pack_keyswitch_fft", "lwe_pack_keyswitch_fft_dev")
BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 33, 34, 36
SOURCE = os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_pack_fft.hip")
REPORT = os.path.join(ROOT, "profiles", "tfhe_pack_fft_a_kernel_resources.txt")
WORDS = ("unsigned int", "unsigned long long")


def test_packfft_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources
    rows = kernel_resources.report(SOURCE)
    by_name = {r["pretty"]: r for r in rows}
    want = ["tfhe_pack_key_fwd_kernel<%s>" % w for w in WORDS]
    want += ["tfhe_packfft_accumulate_kernel<%s, %d>" % (w, k1) for w in WORDS for k1 in (2, 3, 4)]
    want += ["tfhe_packfft_finish_kernel<%s>" % w for w in WORDS]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        assert r.get("LDS Size", 0) == 0, r       # all LDS is dynamic: the transform buffer and the staged words
    # the committed report names the same kernels and says the same of each (register counts may move with the compiler)
    committed = {l[:70].strip(): l for l in open(REPORT) if l.startswith("tfhe_")}
    assert sorted(committed) == sorted(want)
    for name in want:
        assert " spill   0 scratch    0 " in committed[name], committed[name]
        assert committed[name].rstrip().endswith("lds 0"), committed[name]


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


def stand_in(log_n):
    t = TableStandIn(-1, log_n, 1 << log_n, None)
    return t, C.cast(C.pointer(t), C.c_void_p)


def last_error(lib):
    return lib.pfhe_last_error().decode(errors="replace")


def test_symbols_are_in_the_ctypes_table_and_the_package(pfhe):
    assert len(NAMES) == 14
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    for w in ("", "32"):
        dev, host = getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_fft_dev"), getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_fft")
        assert len(dev.argtypes) == len(host.argtypes) + 1
        assert dev.argtypes[4] == C.POINTER(C.c_double)
        assert len(getattr(lib, f"pfhe_tfhe{w}_packfft_plan_create").argtypes) == \
            len(getattr(lib, f"pfhe_tfhe{w}_plan_create").argtypes) + 1
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_plan_creation_refuses_its_arguments_in_order(pfhe, w, bits):
    """the basis's assert!s; Unsupported for k > 3, the null table, Unsupported for log N > 11; k = 0 and the range of
    in_dimension; and only then the device"""
    lib = pfhe.lib()
    create = getattr(lib, f"pfhe_tfhe{w}_packfft_plan_create")
    h = C.c_void_p()
    keep11, t11 = stand_in(11)
    keep12, t12 = stand_in(12)
    assert create(t11, 1, 630, 4, 3, 0, None) == BAD_ARGUMENT                     # nowhere to put the plan
    # ApproxSignedBasis::new's assert!s first, whatever else is wrong
    for lb, length in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        assert create(None, 4, 0, lb, length, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
        assert create(t12, 65, 2 ** 31, lb, length, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
    # k > 3 before the table is looked at, the null table before log N
    for k in (4, 5, 64, 65, 2 ** 40):
        assert create(None, k, 0, 4, 3, 0, C.byref(h)) == UNSUPPORTED and not h.value
        assert "glwe_dimension above 3" in last_error(lib)
        assert create(t12, k, 630, 4, 3, 0, C.byref(h)) == UNSUPPORTED and "glwe_dimension above 3" in last_error(lib)
    assert create(None, 0, 0, 4, 3, 0, C.byref(h)) == BAD_ARGUMENT and not h.value   # no table
    assert create(None, 1, 630, 4, 3, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
    for k, dim in ((1, 630), (0, 630), (3, 0)):
        assert create(t12, k, dim, 4, 3, 0, C.byref(h)) == UNSUPPORTED and not h.value
        assert "log N above 11" in last_error(lib)
    for k, dim in ((0, 630), (1, 0), (2, 2 ** 31 - 1), (3, 2 ** 40)):
        assert create(t11, k, dim, 4, 3, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
        assert "glwe_dimension must be in 1..3 and in_dimension in 1..2^31-2" in last_error(lib)
    for k, dim, length in ((1, 630, 3), (2, 1, 0), (3, 2 ** 31 - 2, 1)):
        assert create(t11, k, dim, 4, length, 0, C.byref(h)) == NO_DEVICE and not h.value     # the last check
    del keep11, keep12


def test_the_calls_refuse_a_missing_plan(pfhe):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    f64 = C.cast(buf, C.POINTER(C.c_double))
    for w in ("", "32"):
        assert getattr(lib, f"pfhe_tfhe{w}_packfft_plan_in_use")(None) == 0
        assert getattr(lib, f"pfhe_tfhe{w}_packfft_plan_scratch_bytes")(None) == 0
        getattr(lib, f"pfhe_tfhe{w}_packfft_plan_destroy")(None)
        assert getattr(lib, f"pfhe_tfhe{w}_packfft_key_dev")(None, ptr, 16, f64, 8, None) == BAD_ARGUMENT
        assert getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_fft_dev")(None, ptr, 8, 1, f64, 8, ptr, 8, None) == BAD_ARGUMENT
        assert getattr(lib, f"pfhe_tfhe{w}_pack_keyswitch_fft")(None, ptr, 8, 1, f64, 8, ptr, 8) == BAD_ARGUMENT


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.TfhePackFftContext(pfhe.FullComplex64FftTable(10), pfhe.ApproxSignedBasis(32, 4, 3), 630)
    assert e.value.kind == "NoDevice"
