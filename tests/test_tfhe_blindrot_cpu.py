"""CPU-side checks of the blind rotation over the TFHE product (pfhe_tfhe{,32}_blindrot_*): its kernels are in the
compiler's resource report and use no scratch memory, the entry points are in the ctypes table, and argument errors are
reported with the product's statuses before the device is touched."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_")
         for g in ("blindrot_create", "blindrot_destroy", "blindrot_in_use", "blindrot_scratch_bytes", "blindrot_rotate_dev",
                   "blindrot_rotate", "mul_monomial_each_to_dev")]


def test_blindrot_kernels_are_reported_and_use_no_scratch():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_fft.hip"))
    by_name = {r["pretty"]: r for r in rows}
    must = ["tfhe_blindrot_loop_kernel<unsigned int>", "tfhe_blindrot_loop_kernel<unsigned long long>"]
    for w in ("unsigned int", "unsigned long long"):
        must += [f"tfhe_blindrot_glue_kernel<{w}, {flags}>" for flags in
                 ("false, false, 1", "false, true, 1", "true, true, 1", "true, true, 0", "false, false, 2")]
    for name in must:
        assert name in by_name, (name, sorted(by_name))
        assert by_name[name].get("ScratchSize", 0) == 0 and by_name[name].get("VGPRs Spill", 0) == 0, by_name[name]
    # three workgroups of four waves per CU is what the u64 / 2^11 LDS budget leaves: the registers must allow as many
    for name in must[:2]:
        assert by_name[name].get("Occupancy", 0) >= 3, by_name[name]
    # the fused product keeps its figures next to the new kernels
    assert by_name["tfhe_fused_kernel<unsigned int>"]["VGPRs"] <= 92
    assert by_name["tfhe_fused_kernel<unsigned long long>"]["VGPRs"] <= 106


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


def test_symbols_are_in_the_ctypes_table(pfhe):
    lib = pfhe.lib()
    for name in NAMES:
        f = getattr(lib, name)
        assert f.argtypes is not None, name
    assert lib.pfhe_tfhe_blindrot_rotate_dev.argtypes[3] == C.POINTER(C.c_double)
    for name in ("TfheBlindRotateContext", "tfhe_blind_rotate", "tfhe_blind_rotate_dev"):
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    assert hasattr(pfhe.FullComplex64FftTable, "mul_monomial_each_to_dev")


def test_create_reports_the_products_statuses_before_the_device(pfhe):
    import torch
    lib = pfhe.lib()
    h = C.c_void_p()
    # ApproxSignedBasis::new's assert!s first, with no table at all
    for fn, lb, length in (("pfhe_tfhe32_blindrot_create", 0, 0), ("pfhe_tfhe32_blindrot_create", 32, 0),
                           ("pfhe_tfhe32_blindrot_create", 10, 4), ("pfhe_tfhe_blindrot_create", 64, 0),
                           ("pfhe_tfhe_blindrot_create", 15, 5)):
        assert getattr(lib, fn)(None, 1, lb, length, 0, C.byref(h)) == 33, (fn, lb, length)   # PFHE_ERR_BAD_ARGUMENT
        assert not h.value
    # then the GLWE dimension, then the table
    assert lib.pfhe_tfhe_blindrot_create(None, 65, 15, 2, 0, C.byref(h)) == 36                # PFHE_ERR_UNSUPPORTED
    assert lib.pfhe_tfhe32_blindrot_create(None, 65, 10, 2, 0, C.byref(h)) == 36
    assert lib.pfhe_tfhe_blindrot_create(None, 1, 15, 2, 0, C.byref(h)) == 33
    assert lib.pfhe_tfhe32_blindrot_create(None, 1, 10, 2, 0, None) == 33
    # null handles
    assert lib.pfhe_tfhe_blindrot_in_use(None) == 0 and lib.pfhe_tfhe32_blindrot_scratch_bytes(None) == 0
    assert lib.pfhe_tfhe_blindrot_rotate_dev(None, None, 0, None, 0, None, 0, None) == 33
    assert lib.pfhe_tfhe32_blindrot_rotate(None, None, 0, None, 0, None, 0) == 33
    assert lib.pfhe_tfhe_mul_monomial_each_to_dev(None, None, 0, None, 1, None, None) == 33
    lib.pfhe_tfhe_blindrot_destroy(None)
    if not torch.cuda.is_available():
        with pytest.raises(pfhe.PfheError) as e:
            pfhe.TfheBlindRotateContext(pfhe.FullComplex64FftTable(10), pfhe.ApproxSignedBasis(32, 10, 2))
        assert e.value.kind == "NoDevice"
