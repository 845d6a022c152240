"""CPU-side checks of the bootstrap around the TFHE blind rotation (pfhe_tfhe{,32}_modswitch_dev, _sample_extract*,
_keyswitch*, _bootstrap_*): the entry points are in the ctypes table and the Python names exported, argument errors are
reported before the device is touched, and the new kernels are in the compiler's resource report with no scratch memory."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = [pre + g for pre in ("pfhe_tfhe_", "pfhe_tfhe32_")
         for g in ("modswitch_dev", "sample_extract_dev", "sample_extract", "keyswitch_dev", "keyswitch", "bootstrap_create",
                   "bootstrap_destroy", "bootstrap_in_use", "bootstrap_scratch_bytes", "bootstrap_dev", "bootstrap")]
PYTHON_NAMES = ["lwe_modulus_switch_dev", "glwe_sample_extract", "glwe_sample_extract_dev", "lwe_keyswitch",
                "lwe_keyswitch_dev", "TfheBootstrapContext", "tfhe_bootstrap", "tfhe_bootstrap_dev"]
BAD_ARGUMENT, BAD_LENGTH, UNSUPPORTED = 33, 32, 36


def test_bootstrap_kernels_are_reported_and_use_no_scratch():
    import kernel_resources
    # the key switch is the file's own kernel; the switch, the accumulator and the extraction are csrc/pfhe_tfhe_stages.hip's
    csrc = os.path.join(ROOT, "primus-fhe_amd", "csrc")
    rows = kernel_resources.report(os.path.join(csrc, "pfhe_bootstrap.hip")) + kernel_resources.report(os.path.join(csrc, "pfhe_tfhe_stages.hip"))
    by_name = {r["pretty"]: r for r in rows}
    must = [kern % w for kern in ("tfhe_modswitch_kernel<%s>", "tfhe_acc_init_kernel<%s>", "tfhe_extract_kernel<%s, false>",
                                  "tfhe_keyswitch_kernel<%s>") for w in ("unsigned int", "unsigned long long")]
    for name in must:
        assert name in by_name, (name, sorted(by_name))
        assert by_name[name].get("ScratchSize", 0) == 0 and by_name[name].get("VGPRs Spill", 0) == 0, by_name[name]
    # the key switch keeps its 8 x 2 sums per thread in registers and the digits of its 32 ciphertexts in 64 x 32 words of LDS
    for w, lds in (("unsigned int", 8192), ("unsigned long long", 16384)):
        assert by_name[f"tfhe_keyswitch_kernel<{w}>"].get("LDS Size", 0) == lds


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


def test_symbols_are_in_the_ctypes_table(pfhe):
    assert len(NAMES) == 22
    lib = pfhe.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.pfhe_tfhe_bootstrap_dev.argtypes[3] == C.POINTER(C.c_double)
    assert lib.pfhe_tfhe32_keyswitch_dev.argtypes[0] == C.c_int
    for name in PYTHON_NAMES:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name


def test_stateless_calls_report_argument_errors_before_the_device(pfhe):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    for w in ("", "32"):
        ms = getattr(lib, f"pfhe_tfhe{w}_modswitch_dev")
        for log_n in (0, 15, 32):
            assert ms(0, ptr, 6, 5, log_n, ptr, 5, ptr, 1, None) == BAD_ARGUMENT, (w, log_n)
        assert ms(0, ptr, 6, 0, 10, ptr, 0, ptr, 6, None) == BAD_ARGUMENT           # lwe_dimension 0
        assert ms(0, ptr, 7, 5, 10, ptr, 5, ptr, 1, None) == BAD_LENGTH             # not a whole ciphertext
        assert ms(0, ptr, 12, 5, 10, ptr, 10, ptr, 1, None) == BAD_LENGTH           # neg_b of another batch
        assert ms(0, ptr, 12, 5, 10, ptr, 9, ptr, 2, None) == BAD_LENGTH
        assert ms(0, None, 6, 5, 10, ptr, 5, ptr, 1, None) == BAD_ARGUMENT          # null pointers
        assert ms(0, ptr, 6, 5, 10, None, 5, ptr, 1, None) == BAD_ARGUMENT
        assert ms(0, ptr, 6, 5, 10, ptr, 5, None, 1, None) == BAD_ARGUMENT
        assert ms(0, None, 0, 5, 10, None, 0, None, 0, None) == 0                   # an empty batch is a no-op
        bits = 64 if w == "" else 32
        for fn in (getattr(lib, f"pfhe_tfhe{w}_keyswitch_dev"), getattr(lib, f"pfhe_tfhe{w}_keyswitch")):
            tail = (None,) if fn.__name__.endswith("_dev") else ()
            # ApproxSignedBasis::new's assert!s first, whatever else is wrong
            for lb, length in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
                assert fn(0, None, 7, 0, None, 1, 0, lb, length, None, 3, *tail) == BAD_ARGUMENT, (w, lb, length)
            assert fn(0, ptr, 5, 0, ptr, 6, 2, 4, 2, ptr, 3, *tail) == BAD_ARGUMENT      # in_dimension 0
            assert fn(0, ptr, 5, 4, ptr, 8, 0, 4, 2, ptr, 1, *tail) == BAD_ARGUMENT      # out_dimension 0
            assert fn(0, ptr, 6, 4, ptr, 24, 2, 4, 2, ptr, 3, *tail) == BAD_LENGTH       # not a whole ciphertext
            assert fn(0, ptr, 5, 4, ptr, 23, 2, 4, 2, ptr, 3, *tail) == BAD_LENGTH       # key of another shape
            assert fn(0, ptr, 5, 4, ptr, 4 * (bits // 4) * 3, 2, 4, 0, ptr, 4, *tail) == BAD_LENGTH   # full length, wrong out
            assert fn(0, None, 5, 4, ptr, 24, 2, 4, 2, ptr, 3, *tail) == BAD_ARGUMENT    # null pointers
            assert fn(0, ptr, 5, 4, None, 24, 2, 4, 2, ptr, 3, *tail) == BAD_ARGUMENT
            assert fn(0, ptr, 5, 4, ptr, 24, 2, 4, 2, None, 3, *tail) == BAD_ARGUMENT
            assert fn(0, None, 0, 4, None, 24, 2, 4, 2, None, 0, *tail) == 0
        # sample extraction needs its table first
        assert getattr(lib, f"pfhe_tfhe{w}_sample_extract_dev")(None, 1, ptr, 32, 0, ptr, 17, None) == BAD_ARGUMENT
        assert getattr(lib, f"pfhe_tfhe{w}_sample_extract")(None, 1, ptr, 32, 0, ptr, 17) == BAD_ARGUMENT


def test_overlapping_key_switch_output_is_refused_before_the_device(pfhe):
    lib = pfhe.lib()
    buf = (C.c_uint32 * 256)()
    base = C.addressof(buf)
    at = lambda words: C.c_void_p(base + 4 * words)
    # in 4, out 2, ell 2: lwe_in 5 words, ksk 24, lwe_out 3
    assert lib.pfhe_tfhe32_keyswitch_dev(0, at(0), 5, 4, at(64), 24, 2, 4, 2, at(4), 3, None) == BAD_ARGUMENT
    assert lib.pfhe_tfhe32_keyswitch_dev(0, at(0), 5, 4, at(64), 24, 2, 4, 2, at(80), 3, None) == BAD_ARGUMENT


NO_DEVICE = 34


class TableStandIn(C.Structure):
    """What the library's table starts with: the device, log N and N.  With device -1 a call that passes every argument
    check ends in NoDevice, so the order of the refusals before it shows without a GPU; nothing is dereferenced."""
    _fields_ = [("device", C.c_int), ("log_n", C.c_uint32), ("n", C.c_size_t), ("tw", C.c_void_p)]


def last_error(lib):
    return lib.pfhe_last_error().decode(errors="replace")


@pytest.mark.parametrize("w, size", [("", 8), ("32", 4)])
def test_sample_extraction_refuses_its_arguments_in_order(pfhe, w, size):
    """the table, the dimension, the index, the lengths, the empty batch, null pointers, overlap (the device form only:
    the host form refuses none), and only then the device"""
    lib = pfhe.lib()
    t = TableStandIn(-1, 3, 8, None)                 # N = 8
    fft = C.cast(C.pointer(t), C.c_void_p)
    buf = (C.c_uint64 * 1024)()
    ptr = C.cast(buf, C.c_void_p)
    n, k = 8, 2
    glwe, lwe = 3 * (k + 1) * n, 3 * (k * n + 1)
    far = C.c_void_p(ptr.value + glwe * size)        # the first byte after the input
    for form, tail in (("sample_extract_dev", (None,)), ("sample_extract", ())):
        call = getattr(lib, f"pfhe_tfhe{w}_{form}")
        assert call(None, 0, None, 5, n, None, 3, *tail) == BAD_ARGUMENT        # the table before anything
        for kk in (0, 65, 2 ** 40):
            assert call(fft, kk, None, 5, n, None, 3, *tail) == BAD_ARGUMENT
            assert last_error(lib) == "sample extraction: glwe_dimension must be in 1..64"
        for index in (n, 2 ** 40):
            assert call(fft, k, None, 5, index, None, 3, *tail) == BAD_ARGUMENT
            assert last_error(lib) == "sample extraction: index must be below N"
        assert call(fft, k, ptr, glwe + 1, n - 1, far, lwe, *tail) == BAD_LENGTH
        assert call(fft, k, ptr, glwe, n - 1, far, lwe + 1, *tail) == BAD_LENGTH
        assert last_error(lib) == "sample extraction: glwe must be batch*(k+1)*N words and lwe batch*(k*N+1)"
        assert call(fft, k, None, 0, 0, None, 0, *tail) == 0                    # an empty batch: no pointer is looked at
        assert call(fft, k, None, glwe, 0, far, lwe, *tail) == BAD_ARGUMENT
        assert call(fft, k, ptr, glwe, 0, None, lwe, *tail) == BAD_ARGUMENT
        assert call(fft, k, ptr, glwe, 0, far, lwe, *tail) == NO_DEVICE         # the last check
    dev, host = getattr(lib, f"pfhe_tfhe{w}_sample_extract_dev"), getattr(lib, f"pfhe_tfhe{w}_sample_extract")
    for out in (ptr, C.c_void_p(far.value - 1), C.c_void_p(ptr.value - lwe * size + 1)):   # the same start, one byte shared
        assert dev(fft, k, ptr, glwe, 0, out, lwe, None) == BAD_ARGUMENT
        assert last_error(lib) == "sample extraction: the output must not overlap the input"
        assert host(fft, k, ptr, glwe, 0, out, lwe) == NO_DEVICE
    assert dev(fft, k, ptr, glwe, 0, C.c_void_p(ptr.value - lwe * size), lwe, None) == NO_DEVICE    # adjacent below


def test_the_stateless_calls_on_a_device_index_look_at_it_last(pfhe):
    """device -1: the null test and (device forms) the overlap test come before the device is asked about; the host form of
    the key switch refuses no overlap, the modulus switch refuses none at all, and inputs may overlap each other"""
    lib = pfhe.lib()
    buf = (C.c_uint64 * 256)()
    ptr = C.cast(buf, C.c_void_p)
    far, out = C.c_void_p(ptr.value + 512), C.c_void_p(ptr.value + 1024)
    for w in ("", "32"):
        ms = getattr(lib, f"pfhe_tfhe{w}_modswitch_dev")
        for log_n in (0, 15):
            assert ms(-1, ptr, 6, 5, log_n, far, 5, out, 1, None) == BAD_ARGUMENT
            assert last_error(lib) == "modulus switch: log_n must be in 1..14"
        for dim in (0, 2 ** 32 - 1):
            assert ms(-1, ptr, 6, dim, 10, far, 5, out, 1, None) == BAD_ARGUMENT
            assert last_error(lib) == "modulus switch: lwe_dimension must be in 1..2^32-2"
        assert ms(-1, None, 6, 5, 10, far, 5, out, 1, None) == BAD_ARGUMENT
        assert ms(-1, ptr, 6, 5, 10, far, 5, out, 1, None) == NO_DEVICE
        assert ms(-1, ptr, 6, 5, 10, ptr, 5, ptr, 1, None) == NO_DEVICE
        dev, host = getattr(lib, f"pfhe_tfhe{w}_keyswitch_dev"), getattr(lib, f"pfhe_tfhe{w}_keyswitch")
        for fn, tail in ((dev, (None,)), (host, ())):
            for din, dout in ((2 ** 31 - 1, 2), (4, 2 ** 31 - 1)):
                assert fn(-1, ptr, 5, din, far, 24, dout, 4, 2, out, 3, *tail) == BAD_ARGUMENT
                assert last_error(lib) == "key switch: both dimensions must be in 1..2^31-2"
            assert fn(-1, ptr, 5, 4, far, 23, 2, 4, 2, out, 3, *tail) == BAD_LENGTH
            assert last_error(lib).startswith("key switch: lwe_in must be batch*(in_dimension+1) words, ksk ")
            assert fn(-1, ptr, 5, 4, None, 24, 2, 4, 2, out, 3, *tail) == BAD_ARGUMENT
            assert fn(-1, ptr, 5, 4, far, 24, 2, 4, 2, out, 3, *tail) == NO_DEVICE
            assert fn(-1, ptr, 5, 4, ptr, 24, 2, 4, 2, out, 3, *tail) == NO_DEVICE     # the inputs overlap each other
        for a, b in ((ptr, far), (far, ptr)):                                          # the output on lwe_in, then on ksk
            assert dev(-1, a, 5, 4, b, 24, 2, 4, 2, ptr, 3, None) == BAD_ARGUMENT
            assert last_error(lib) == "key switch: the output must not overlap an input"
            assert host(-1, a, 5, 4, b, 24, 2, 4, 2, ptr, 3) == NO_DEVICE


def test_create_reports_the_rotations_statuses_first(pfhe):
    import torch
    lib = pfhe.lib()
    h = C.c_void_p()
    # the rotation's create runs first: ApproxSignedBasis::new's assert!s on the product's basis, with no table at all
    for fn, lb, length in (("pfhe_tfhe32_bootstrap_create", 0, 0), ("pfhe_tfhe32_bootstrap_create", 32, 0),
                           ("pfhe_tfhe32_bootstrap_create", 10, 4), ("pfhe_tfhe_bootstrap_create", 64, 0),
                           ("pfhe_tfhe_bootstrap_create", 15, 5)):
        assert getattr(lib, fn)(None, 1, lb, length, 630, 4, 3, 1, 0, C.byref(h)) == BAD_ARGUMENT, (fn, lb, length)
        assert not h.value
    # then the GLWE dimension, then the table
    assert lib.pfhe_tfhe_bootstrap_create(None, 65, 15, 2, 630, 4, 3, 1, 0, C.byref(h)) == UNSUPPORTED
    assert lib.pfhe_tfhe32_bootstrap_create(None, 65, 10, 2, 630, 4, 3, 1, 0, C.byref(h)) == UNSUPPORTED
    assert lib.pfhe_tfhe_bootstrap_create(None, 1, 15, 2, 630, 4, 3, 1, 0, C.byref(h)) == BAD_ARGUMENT
    assert lib.pfhe_tfhe32_bootstrap_create(None, 1, 10, 2, 630, 4, 3, 1, 0, None) == BAD_ARGUMENT
    # null handles
    assert lib.pfhe_tfhe_bootstrap_in_use(None) == 0 and lib.pfhe_tfhe32_bootstrap_scratch_bytes(None) == 0
    assert lib.pfhe_tfhe_bootstrap_dev(None, None, 0, None, 0, None, 0, None, 0, None, 0, None) == BAD_ARGUMENT
    assert lib.pfhe_tfhe32_bootstrap(None, None, 0, None, 0, None, 0, None, 0, None, 0) == BAD_ARGUMENT
    lib.pfhe_tfhe_bootstrap_destroy(None)
    lib.pfhe_tfhe32_bootstrap_destroy(None)
    if not torch.cuda.is_available():
        with pytest.raises(pfhe.PfheError) as e:
            pfhe.TfheBootstrapContext(pfhe.FullComplex64FftTable(10), pfhe.ApproxSignedBasis(32, 7, 3), 630,
                                      ks_basis=pfhe.ApproxSignedBasis(32, 4, 3))
        assert e.value.kind == "NoDevice"
