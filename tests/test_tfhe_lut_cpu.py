"""CPU-side checks of the look-up table on encrypted bits (pfhe_tfhe{,32}_lut_*, _rotate_by_bits*, _lut_eval*): the 16 entry
points are in the ctypes table, declared in include/pfhe.h and mirrored in include/pfhe.hpp, the Python names are exported,
every refusal of create that precedes the device arrives in the stated order, tfhe_lut_table lays the entries out as the
model does, and the compiler's resource report shows the new kernels for both word types with no scratch memory, no spilled
register, no static LDS and the rotation loop's register budget."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("lut_create", "lut_destroy", "lut_in_use", "lut_scratch_bytes", "rotate_by_bits_dev", "rotate_by_bits", "lut_eval_dev",
         "lut_eval")
NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_") for g in CALLS]
PUBLIC = ("TfheLutContext", "tfhe_rotate_by_bits", "tfhe_rotate_by_bits_dev", "tfhe_lut_eval", "tfhe_lut_eval_dev",
          "tfhe_lut_table")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36


def test_lut_kernels_use_no_scratch_spill_nothing_and_keep_the_loops_budget():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_lut.hip"))
    by_name = {r["pretty"]: r for r in rows}
    words = ("unsigned int", "unsigned long long")
    want = ["%s<%s>" % (kern, w) for kern in ("tfhe_bitrot_loop_kernel", "tfhe_bitrot_monomial_kernel") for w in words]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    recorded = open(os.path.join(ROOT, "profiles", "tfhe_lut_a_kernel_resources.txt")).read()
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        # the digit spectrum and the accumulator are dynamic LDS sized by the launch: no kernel declares any of its own
        assert r.get("LDS Size", 0) == 0, r
        assert name in recorded, name
    for w in words:
        # four waves per SIMD, the rotation loop's figure: at most 128 registers
        assert by_name["tfhe_bitrot_loop_kernel<%s>" % w].get("VGPRs", 999) <= 128
        assert by_name["tfhe_bitrot_loop_kernel<%s>" % w].get("Occupancy", 0) >= 4


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


def test_symbols_are_in_the_ctypes_table_the_headers_and_the_package(pfhe):
    assert len(NAMES) == 16
    lib = pfhe.lib()
    header = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    import cpp_mirror
    mirror = cpp_mirror.mirror_symbols()       # tied to the compiled include/pfhe.hpp by test_cpp_header.py, which also
    for name in NAMES:                         # pins TfheLut and TfheLut32 as two types over the two C handles
        assert getattr(lib, name).argtypes is not None, name
        assert "%s(" % name in header and name in mirror, name
    # the note the CMUX entries carry: no reference counterpart, the rule is the project's own
    section = header[header.index("a look-up table on encrypted bits"):]
    assert "The reference has neither; the rules are this project's own (DESIGN.md §23)" in section
    for w in ("", "32"):
        for form in ("rotate_by_bits", "lut_eval"):
            dev, host = getattr(lib, f"pfhe_tfhe{w}_{form}_dev"), getattr(lib, f"pfhe_tfhe{w}_{form}")
            assert len(dev.argtypes) == len(host.argtypes) + 1
        assert getattr(lib, f"pfhe_tfhe{w}_lut_create").argtypes[2] == C.c_uint32
        assert len(getattr(lib, f"pfhe_tfhe{w}_lut_create").argtypes) == 10
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    import inspect
    params = inspect.signature(pfhe.TfheLutContext.__init__).parameters
    assert list(params)[1:] == ["fft", "basis", "glwe_dimension", "tree_depth", "rot_bits", "outputs", "log_stride", "chunk"]
    assert params["outputs"].default == 1 and params["log_stride"].default == 0 and params["chunk"].default == 0


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_create_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """a null out pointer; the product plan's checks in their order (the basis's assert!s, Unsupported above 64, the table);
    tree_depth above 16; rot_bits + log_stride above log N; no bit at all; no output; the grid of a launch; and only then the
    device.  A refusal leaves the handle null."""
    lib = pfhe.lib()
    _, fft = table                       # log N = 3
    create = getattr(lib, f"pfhe_tfhe{w}_lut_create")
    h = C.c_void_p(1)
    k, lb, ell = 1, 7, 3
    assert create(fft, k, lb, ell, 2, 2, 0, 1, 0, None) == BAD_ARGUMENT                     # nowhere to put the handle
    for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        h.value = 1
        assert create(None, 65, bad_lb, bad_len, 17, 9, 9, 0, 0, C.byref(h)) == BAD_ARGUMENT   # whatever else is wrong
        assert not h.value and "tree_depth" not in last_error(lib)
    assert create(None, 65, lb, ell, 17, 9, 9, 0, 0, C.byref(h)) == UNSUPPORTED              # before the table and the depth
    assert "glwe_dimension above 64" in last_error(lib)
    assert create(None, k, lb, ell, 17, 9, 9, 0, 0, C.byref(h)) == BAD_ARGUMENT              # no table, before the depth
    assert "tree_depth" not in last_error(lib)
    for depth in (17, 2 ** 40):
        h.value = 1
        assert create(fft, k, lb, ell, depth, 9, 9, 0, 0, C.byref(h)) == BAD_ARGUMENT and not h.value   # before r + s
        assert "tree_depth must be in 0..16" in last_error(lib)
    for r, s in ((4, 0), (3, 1), (0, 4), (2 ** 63, 2 ** 63), (1, 2 ** 64 - 1)):
        h.value = 1
        assert create(fft, k, lb, ell, 0, r, s, 0, 0, C.byref(h)) == BAD_ARGUMENT and not h.value       # before t + r = 0
        assert "rot_bits + log_stride must be at most log N" in last_error(lib)
    for s in (0, 3):
        assert create(fft, k, lb, ell, 0, 0, s, 0, 0, C.byref(h)) == BAD_ARGUMENT                        # before outputs
        assert "tree_depth + rot_bits must be at least 1" in last_error(lib)
    for t, r in ((1, 0), (0, 1), (16, 3)):
        h.value = 1
        assert create(fft, k, lb, ell, t, r, 0, 0, 2 ** 40, C.byref(h)) == BAD_ARGUMENT and not h.value  # before the grid
        assert "outputs must be at least 1" in last_error(lib)
    # a launch's grid holds chunk * o * 2^(t-1) nodes: BadLength for a chunk (or the outputs of one input) beyond it
    assert create(fft, k, lb, ell, 1, 0, 0, 1, 2 ** 31, C.byref(h)) == BAD_LENGTH
    assert create(fft, k, lb, ell, 0, 1, 0, 2 ** 16, 2 ** 15, C.byref(h)) == BAD_LENGTH
    assert create(fft, k, lb, ell, 16, 0, 0, 1, 2 ** 16, C.byref(h)) == BAD_LENGTH
    assert create(fft, k, lb, ell, 16, 0, 0, 2 ** 16, 0, C.byref(h)) == BAD_LENGTH
    assert create(fft, k, lb, ell, 0, 1, 0, 2 ** 31, 0, C.byref(h)) == BAD_LENGTH
    for args in ((0, 1, 0, 1, 0), (0, 3, 0, 1, 0), (0, 2, 1, 3, 5), (16, 0, 3, 1, 2 ** 15), (16, 3, 0, 2, 0), (1, 2, 1, 1, 2 ** 31 - 1)):
        h.value = 1
        assert create(fft, k, lb, ell, *args, C.byref(h)) == NO_DEVICE and not h.value       # the last check
    assert create(fft, 2, lb, 0, 2, 2, 0, 2, 5, C.byref(h)) == NO_DEVICE                     # the general form, the full length


@pytest.mark.parametrize("w", ["", "32"])
def test_calls_on_no_handle_are_refused(pfhe, w):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    keys = C.cast(buf, C.POINTER(C.c_double))
    assert getattr(lib, f"pfhe_tfhe{w}_rotate_by_bits_dev")(None, ptr, 8, keys, 8, 1, 0, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_rotate_by_bits")(None, ptr, 8, keys, 8, 1, 0, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_lut_eval_dev")(None, ptr, 8, keys, 8, 0, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_lut_eval")(None, ptr, 8, keys, 8, 0, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_tfhe{w}_lut_in_use")(None) == 0
    assert getattr(lib, f"pfhe_tfhe{w}_lut_scratch_bytes")(None) == 0
    getattr(lib, f"pfhe_tfhe{w}_lut_destroy")(None)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_lut_table_lays_the_entries_out_as_the_model(pfhe, dtype):
    import torch
    import tfhe_lut_model as lm
    rng = np.random.default_rng(5)
    for log_n, k, t, r, s, words in ((3, 1, 1, 2, 0, 0), (4, 2, 2, 2, 2, 3), (3, 1, 0, 3, 0, 0), (3, 1, 2, 0, 1, 2)):
        shape = (2, 1 << (t + r)) + ((words,) if words else ())
        values = rng.integers(0, 2 ** 31, shape).astype(dtype)
        want = lm.lut_table(values, log_n, k, t, r, s)
        got = pfhe.tfhe_lut_table(values, log_n, k, t, r, s)
        assert got.dtype == dtype and np.array_equal(got, want)
        signed = torch.from_numpy(values.astype(np.int64 if dtype == np.uint64 else np.int32))
        assert np.array_equal(pfhe.tfhe_lut_table(signed, log_n, k, t, r, s).numpy().astype(dtype), want)
    with pytest.raises(ValueError):
        pfhe.tfhe_lut_table(np.zeros((1, 8), dtype), 3, 1, 1, 1)                # 2^p is 4
    with pytest.raises(ValueError):
        pfhe.tfhe_lut_table(np.zeros((1, 4, 2), dtype), 3, 1, 1, 1, 0)          # two words need a stride
    with pytest.raises(ValueError):
        pfhe.tfhe_lut_table(np.zeros((1, 16), dtype), 3, 1, 0, 4)               # r above log N


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.FullComplex64FftTable(3)
    assert e.value.kind == "NoDevice"
