"""CPU-side checks of the linear layer with clear weights (pfhe_lwe{,32}_linear*): the 8 entry points are in the ctypes
table and declared in include/pfhe.h with their note, the width pairs have one signature up to the word, the C++ mirror's
templates leave exactly their own 8 symbols undefined, the Python names are exported with their defaults, every refusal that
precedes the device arrives in the stated order, and the compiler's resource report shows exactly the new kernels for both
word types with no scratch memory and no spilled register."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("linear_dev", "linear", "linear_i8_dev", "linear_i8")
NAMES = [pre + g for pre in ("pfhe_lwe_", "pfhe_lwe32_") for g in CALLS]
PUBLIC = ("lwe_linear", "lwe_linear_dev", "tfhe_dense_layer_dev")
OK, BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE = 0, 32, 33, 34
CSRC = os.path.join(ROOT, "primus-fhe_amd", "csrc")
WORD_TILES, I8_TILES = (1, 2, 4, 8), (1, 2)      # pfhe_linear.hip: outputs per thread, 16-output tiles per wave


def test_linear_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(CSRC, "pfhe_linear.hip"))
    by_name = {r["pretty"]: r for r in rows}
    words = {"unsigned int": 4, "unsigned long long": 8}
    want = ["lwe_linear_kernel<%s, %d>" % (w, r) for w in words for r in WORD_TILES] + \
           ["lwe_linear_i8_kernel<%s, %d>" % (w, t) for w in words for t in I8_TILES]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    recorded = open(os.path.join(ROOT, "profiles", "lwe_linear_a_kernel_resources.txt")).read()
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        assert r.get("Occupancy", 0) > 0
        assert name in recorded, name
    for w, size in words.items():        # the weights of a group: 64 inputs x (the tile's outputs + 1) words, at most 64 x 33
        for r in WORD_TILES:
            assert by_name["lwe_linear_kernel<%s, %d>" % (w, r)].get("LDS Size", 0) == 64 * (4 * r + 1) * size


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


def test_symbols_are_in_the_ctypes_table_the_headers_and_the_package(pfhe):
    assert len(NAMES) == 8
    lib = pfhe.lib()
    header = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
        assert "%s(" % name in header, name
    section = header[header.index("linear layer: clear integer weights on batches of LWE ciphertexts"):]
    assert "primus_lattice/src/lwe/single_message.rs:262-268" in section and "DESIGN.md §25" in section
    assert "out[e][o][c] = sum_{i < in_features} W[o][i] * in[e][i][c]  +  [c = dimension] * bias[o]" in section
    for status in ("PFHE_ERR_BAD_ARGUMENT", "PFHE_ERR_BAD_LENGTH", "an empty batch is a no-op", "the device"):
        assert status in section, status
    for w in ("", "32"):
        for entry in ("linear", "linear_i8"):
            dev, host = getattr(lib, f"pfhe_lwe{w}_{entry}_dev"), getattr(lib, f"pfhe_lwe{w}_{entry}")
            assert len(dev.argtypes) == len(host.argtypes) + 1 == 13
            assert dev.argtypes[0] == C.c_int and dev.restype == C.c_int
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    host = inspect.signature(pfhe.lwe_linear).parameters
    assert list(host) == ["lwe_in", "weights", "bias", "lwe_out", "dimension", "in_features", "out_features", "device"]
    assert host["device"].default == 0
    dev = inspect.signature(pfhe.lwe_linear_dev).parameters
    assert list(dev) == list(host) + ["stream"] and dev["device"].default is None and dev["stream"].default is None
    dense = inspect.signature(pfhe.tfhe_dense_layer_dev).parameters
    assert list(dense) == ["lwe_in", "weights", "bias", "bsk", "tv", "ksk", "lwe_out", "ctx", "in_features", "out_features",
                           "stream"]
    assert dense["stream"].default is None and "allocates" in pfhe.tfhe_dense_layer_dev.__doc__


def test_every_width_pair_of_the_family_has_one_signature_up_to_the_word():
    """The family has a prefix of its own, so the rule tests/test_boundary_static.py holds the pfhe_tfhe_ pairs to is held
    here for it, on that file's own reading of pfhe.h; the byte pointer of the i8 entries is spelled const int8_t *"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_boundary_static import header_signatures
    text = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    sigs = {n: v for n, v in header_signatures(text).items() if n.startswith("pfhe_lwe")}
    assert set(sigs) == set(NAMES)
    pairs = 0
    for name, (ret, params) in sigs.items():
        if name.startswith("pfhe_lwe32_"):
            continue
        other = "pfhe_lwe32_" + name[len("pfhe_lwe_"):]
        assert (ret, [t.replace("uint64_t", "uint32_t") for t in params]) == sigs[other], (name, sigs[name], sigs[other])
        assert params[4] == ("const int8_t *" if "_i8" in name else "const uint64_t *")
        pairs += 1
    assert pairs == 4
    ffi = open(os.path.join(ROOT, "integration", "primus_ntt_hip", "src", "ffi.rs")).read()
    assert len(re.findall(r"weights(?:_dev)?: \*const i8", ffi)) == 4


def test_mirror_templates_leave_exactly_their_own_symbols_undefined():
    import cpp_mirror
    support = os.path.join(ROOT, "tests", "support")
    own = set(open(os.path.join(support, "cpp_mirror_linear_symbols.txt")).read().split())
    assert own == set(NAMES)
    undefined = cpp_mirror.undefined_pfhe_symbols(os.path.join(support, "cpp_mirror_linear_instantiate.cpp"))
    old = cpp_mirror.mirror_symbols()
    assert not own & old
    assert undefined - old == own, sorted((undefined - old) ^ own)


def test_python_refuses_other_weight_dtypes_before_the_library(pfhe):
    x, out = np.zeros(6, np.uint32), np.zeros(2, np.uint32)
    for bad in (np.zeros(3, np.int16), np.zeros(3, np.uint64), np.zeros(3, np.float32), np.zeros(3, np.int32)):
        with pytest.raises(ValueError):
            pfhe.lwe_linear(x, bad, None, out, 1, 3, 1)


@pytest.mark.parametrize("w, word", [("", C.c_uint64), ("32", C.c_uint32)])
@pytest.mark.parametrize("entry", ["linear", "linear_i8"])
def test_calls_refuse_their_arguments_in_order(pfhe, w, word, entry):
    """the ranges; the lengths; the empty batch; a null pointer; a bias pointer with no length; the overlap (device form); and
    only then the device, which this machine may lack: device -1 is refused last whatever the machine"""
    lib = pfhe.lib()
    dim, in_f, out_f, batch = 5, 3, 2, 2
    row = dim + 1
    x, wt, bias, out = (word * (batch * in_f * row))(), (word * (out_f * in_f))(), (word * out_f)(), (word * (batch * out_f * row))()
    ptr = lambda a: C.cast(a, C.c_void_p)
    for form in ("_dev", ""):
        call = getattr(lib, "pfhe_lwe%s_%s%s" % (w, entry, form))
        good = [-1, ptr(x), len(x), dim, ptr(wt), len(wt), in_f, out_f, ptr(bias), out_f, ptr(out), len(out)] + ([None] if form else [])

        def with_(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return call(*a)

        for at in (3, 6, 7):
            for bad in (0, 2 ** 31 - 1, 2 ** 40):
                assert with_(**{"a%d" % at: bad, "a2": 1, "a5": 0, "a1": None}) == BAD_ARGUMENT, (at, bad)
                assert "1..2^31-2" in lib.pfhe_last_error().decode()
        assert with_(a2=len(x) - 1, a1=None) == BAD_LENGTH
        assert with_(a5=len(wt) + 1, a4=None) == BAD_LENGTH
        assert with_(a9=1, a8=None) == BAD_LENGTH
        assert with_(a11=len(out) - row, a10=None) == BAD_LENGTH
        assert with_(a11=len(out) + row) == BAD_LENGTH
        assert with_(a2=0, a11=0, a1=None, a10=None) == OK                 # the empty batch: a no-op, whatever the device
        for at in (1, 4, 8, 10):
            assert with_(**{"a%d" % at: None}) == BAD_ARGUMENT, at
        inside = C.c_void_p(C.addressof(x) + 8)                           # an output inside the input
        assert with_(a9=0, a10=inside) == BAD_ARGUMENT and "bias" in lib.pfhe_last_error().decode()
        if form:
            assert with_(a10=inside) == BAD_ARGUMENT and "overlap" in lib.pfhe_last_error().decode()
        assert with_() == NO_DEVICE                                        # the last check
        assert with_(a8=None, a9=0) == NO_DEVICE                           # no bias is no refusal
