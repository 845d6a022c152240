"""CPU-side checks of the multi-bit blind rotation (pfhe_tfhe{,32}_mbrot_*, pfhe_tfhe_mb_combine_key_dev,
pfhe_tfhe{,32}_bootstrap_create_multibit): the entry points are in the ctypes table, argument errors come with the product
plan's statuses in its order before the device is touched, and the compiler's resource report shows no scratch memory and
no spilled register for the new kernels, with room for three workgroups per CU in both loop instantiations."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_")
         for g in ("mbrot_create", "mbrot_destroy", "mbrot_in_use", "mbrot_scratch_bytes", "mbrot_rotate_dev", "mbrot_rotate",
                   "bootstrap_create_multibit")] + ["pfhe_tfhe_mb_combine_key_dev"]

BAD_ARGUMENT, UNSUPPORTED = 33, 36


def test_multibit_kernels_use_no_scratch_and_leave_three_workgroups_per_cu():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_fft.hip"))
    by_name = {r["pretty"]: r for r in rows}
    loops = ["tfhe_mb_blindrot_loop_kernel<unsigned int>", "tfhe_mb_blindrot_loop_kernel<unsigned long long>"]
    for name in loops + ["tfhe_mb_mulacc_kernel", "tfhe_mb_combine_key_kernel"]:
        assert name in by_name, (name, sorted(by_name))
        assert by_name[name].get("ScratchSize", 0) == 0 and by_name[name].get("VGPRs Spill", 0) == 0, by_name[name]
    # the LDS of the u64 / 2^11 loop (17,424 + 32,768 B) leaves three workgroups per CU: the registers must allow as many
    for name in loops:
        assert by_name[name].get("Occupancy", 0) >= 3, by_name[name]


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


def test_symbols_are_in_the_ctypes_table(pfhe):
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.pfhe_tfhe_mbrot_rotate_dev.argtypes[3] == C.POINTER(C.c_double)
    assert len(lib.pfhe_tfhe_mbrot_create.argtypes) == len(lib.pfhe_tfhe_blindrot_create.argtypes) + 1
    assert len(lib.pfhe_tfhe32_bootstrap_create_multibit.argtypes) == len(lib.pfhe_tfhe32_bootstrap_create.argtypes) + 1
    for name in ("TfheMultiBitBlindRotateContext", "tfhe_multibit_blind_rotate", "tfhe_multibit_blind_rotate_dev",
                 "tfhe_multibit_combine_key_dev"):
        assert hasattr(pfhe, name) and name in pfhe.__all__, name


@pytest.mark.parametrize("grouping", [0, 1, 2, 4, 5])
def test_create_reports_the_plans_statuses_in_the_plans_order(pfhe, grouping):
    """whatever the grouping factor, the plan's checks come first and in pfhe_tfhe_plan_create's order: the basis's
    assert!s, then the GLWE dimension, then the table"""
    lib = pfhe.lib()
    h = C.c_void_p()
    for w, lb, length in (("32", 0, 0), ("32", 32, 0), ("32", 10, 4), ("", 64, 0), ("", 15, 5)):
        plan = getattr(lib, f"pfhe_tfhe{w}_plan_create")(None, 65, lb, length, 0, C.byref(h))
        assert plan == BAD_ARGUMENT
        assert getattr(lib, f"pfhe_tfhe{w}_mbrot_create")(None, 65, lb, length, grouping, 0, C.byref(h)) == plan
        assert getattr(lib, f"pfhe_tfhe{w}_bootstrap_create_multibit")(None, 65, lb, length, 7, 4, 3, 1, grouping, 0,
                                                                     C.byref(h)) == plan
        assert not h.value
    for w, lb in (("32", 10), ("", 15)):
        assert getattr(lib, f"pfhe_tfhe{w}_mbrot_create")(None, 65, lb, 2, grouping, 0, C.byref(h)) == UNSUPPORTED
        assert getattr(lib, f"pfhe_tfhe{w}_bootstrap_create_multibit")(None, 65, lb, 2, 6, 4, 3, 1, grouping, 0,
                                                                     C.byref(h)) == UNSUPPORTED
        assert getattr(lib, f"pfhe_tfhe{w}_mbrot_create")(None, 1, lb, 2, grouping, 0, C.byref(h)) == BAD_ARGUMENT   # no table
        assert getattr(lib, f"pfhe_tfhe{w}_mbrot_create")(None, 1, lb, 2, grouping, 0, None) == BAD_ARGUMENT
        assert getattr(lib, f"pfhe_tfhe{w}_bootstrap_create_multibit")(None, 1, lb, 2, 7, 4, 3, 1, grouping, 0,
                                                                     C.byref(h)) == BAD_ARGUMENT
        assert not h.value


@pytest.fixture(scope="module")
def table_stand_in():
    """A non-null table pointer for calls that must be refused before the table is read: zeroed host memory, which none of
    the checks below dereferences.  Every call that gets it is one the library has to refuse on its arguments alone."""
    buf = C.create_string_buffer(4096)
    return buf, C.cast(buf, C.c_void_p)


def last_error(lib):
    return lib.pfhe_last_error().decode(errors="replace")


@pytest.mark.parametrize("w, lb", [("32", 10), ("", 15)])
def test_grouping_and_divisibility_are_refused_before_the_device(pfhe, table_stand_in, w, lb):
    """with a table and a plan that passes, grouping 0 and 5 (and a size_t's worth of others) are BAD_ARGUMENT with the
    message of the grouping check from both creates, and lwe_dimension % g != 0 is BAD_ARGUMENT with the bootstrap's own
    message; no device is needed for either, and the table is not read"""
    lib = pfhe.lib()
    _, fft = table_stand_in
    h = C.c_void_p()
    mbrot = getattr(lib, f"pfhe_tfhe{w}_mbrot_create")
    boot = getattr(lib, f"pfhe_tfhe{w}_bootstrap_create_multibit")
    for g in (0, 5, 6, 2**32, 2**64 - 1):
        assert mbrot(fft, 1, lb, 2, g, 0, C.byref(h)) == BAD_ARGUMENT
        assert last_error(lib) == "grouping_factor must be in 1..4" and not h.value
        # the grouping factor is judged before the divisibility: 630 is a multiple of 5 and of 6, 7 of neither
        for n in (630, 7):
            for ks in (0, 1):
                assert boot(fft, 1, lb, 2, n, 4, 3, ks, g, 0, C.byref(h)) == BAD_ARGUMENT
                assert last_error(lib) == "grouping_factor must be in 1..4" and not h.value
    for g, n in ((2, 7), (3, 7), (4, 7), (4, 630), (3, 1), (2, 2**31 + 1)):
        assert boot(fft, 1, lb, 2, n, 4, 3, 1, g, 0, C.byref(h)) == BAD_ARGUMENT
        assert last_error(lib) == "TFHE multi-bit bootstrap: lwe_dimension must be a multiple of grouping_factor"
        assert not h.value
    assert mbrot(fft, 1, lb, 2, 2, 0, None) == BAD_ARGUMENT and boot(fft, 1, lb, 2, 8, 4, 3, 1, 2, 0, None) == BAD_ARGUMENT


@pytest.mark.parametrize("grouping", [0, 1, 2, 3, 4, 5])
def test_the_plans_status_comes_before_the_grouping_and_the_divisibility(pfhe, table_stand_in, grouping):
    """a bad basis or k > 64 is reported with the plan's status and message whatever the grouping factor and
    lwe_dimension % g are, the table being there"""
    lib = pfhe.lib()
    _, fft = table_stand_in
    h = C.c_void_p()
    for w, k, lb, length in (("32", 1, 0, 0), ("32", 1, 32, 0), ("32", 65, 10, 4), ("", 1, 64, 0), ("", 65, 15, 5),
                             ("32", 65, 10, 2), ("", 65, 15, 2)):
        plan = getattr(lib, f"pfhe_tfhe{w}_plan_create")(fft, k, lb, length, 0, C.byref(h))
        message = last_error(lib)
        assert plan == (UNSUPPORTED if length == 2 else BAD_ARGUMENT) and not h.value
        assert getattr(lib, f"pfhe_tfhe{w}_mbrot_create")(fft, k, lb, length, grouping, 0, C.byref(h)) == plan
        assert last_error(lib) == message and not h.value
        assert getattr(lib, f"pfhe_tfhe{w}_bootstrap_create_multibit")(fft, k, lb, length, 7, 4, 3, 1, grouping, 0,
                                                                     C.byref(h)) == plan
        assert last_error(lib) == message and not h.value


def test_the_combined_key_call_refuses_its_arguments_in_order(pfhe, table_stand_in):
    lib = pfhe.lib()
    _, fft = table_stand_in
    call = lib.pfhe_tfhe_mb_combine_key_dev
    assert call(None, 65, 0, 0, None, 0, None, 0, None, 0, None) == BAD_ARGUMENT      # the table first
    assert call(fft, 65, 0, 0, None, 0, None, 0, None, 0, None) == UNSUPPORTED        # then k > 64
    for ell, g in ((0, 2), (65, 2), (2, 0), (2, 5)):
        assert call(fft, 1, ell, g, None, 0, None, 0, None, 0, None) == BAD_ARGUMENT
        assert "decompose_length must be in 1..64 and grouping_factor in 1..4" in last_error(lib)


def test_null_handles_and_the_combined_key_call(pfhe):
    lib = pfhe.lib()
    assert lib.pfhe_tfhe_mbrot_in_use(None) == 0 and lib.pfhe_tfhe32_mbrot_scratch_bytes(None) == 0
    assert lib.pfhe_tfhe_mbrot_rotate_dev(None, None, 0, None, 0, None, 0, None) == BAD_ARGUMENT
    assert lib.pfhe_tfhe32_mbrot_rotate(None, None, 0, None, 0, None, 0) == BAD_ARGUMENT
    assert lib.pfhe_tfhe_mb_combine_key_dev(None, 1, 2, 2, None, 0, None, 0, None, 0, None) == BAD_ARGUMENT
    lib.pfhe_tfhe_mbrot_destroy(None)
    lib.pfhe_tfhe32_mbrot_destroy(None)


def test_no_fallback_without_a_device(pfhe):
    """without a GPU the Python constructors raise NoDevice and compute nothing (it is the table's constructor that says so
    here, ahead of the rotation's; the rotation's own argument checks are covered above); with one they make a handle"""
    import torch
    if torch.cuda.is_available():
        ctx = pfhe.TfheMultiBitBlindRotateContext(pfhe.FullComplex64FftTable(10), pfhe.ApproxSignedBasis(32, 10, 2), 2)
        assert not ctx.in_use() and ctx.scratch_bytes() == 0
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.TfheMultiBitBlindRotateContext(pfhe.FullComplex64FftTable(10), pfhe.ApproxSignedBasis(32, 10, 2), 2)
    assert e.value.kind == "NoDevice"
