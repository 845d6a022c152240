"""CPU-side checks of bit extraction (pfhe_bitext{,32}_*): the 12 entry points are in the ctypes table and
declared in include/pfhe.h with their note, the C++ mirror's new class leaves exactly its own 12 symbols undefined, the
Python names are exported with their defaults, every refusal of create that precedes the device arrives in the stated order,
calls on no handle are refused, and the compiler's resource report shows the new kernels for both word types with no
scratch memory, no spilled register, the tile's static LDS and no fewer waves than the plain key switch."""
import ctypes as C
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("create", "destroy", "in_use", "scratch_bytes", "extract_bits_dev", "extract_bits")
NAMES = [pre + g for pre in ("pfhe_bitext_", "pfhe_bitext32_") for g in CALLS]
PUBLIC = ("TfheBitExtractContext", "tfhe_extract_bits", "tfhe_extract_bits_dev", "tfhe_lut_on_integer_dev")
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36
CSRC = os.path.join(ROOT, "primus-fhe_amd", "csrc")
K_KS_MAX_ROWS, K_KS_TILE_M = 64, 32          # pfhe_tfhe_exact_device.hpp: kKsMaxRows, kKsTileM = kKsWaves * kKsRows


def test_bitext_kernels_use_no_scratch_spill_nothing_and_keep_the_key_switchs_waves():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(CSRC, "pfhe_bitext.hip"))
    by_name = {r["pretty"]: r for r in rows}
    words = {"unsigned int": 4, "unsigned long long": 8}
    want = ["tfhe_bitext_keyswitch_kernel<%s>" % w for w in words]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    # extract-and-subtract is the subtracting form of the extraction kernel of pfhe_tfhe_stages.hip
    stages = {r["pretty"]: r for r in kernel_resources.report(os.path.join(CSRC, "pfhe_tfhe_stages.hip"))}
    subtracting = ["tfhe_extract_kernel<%s, true>" % w for w in words]
    by_name.update({name: stages[name] for name in subtracting})
    want += subtracting
    recorded = open(os.path.join(ROOT, "profiles", "tfhe_bitext_a_kernel_resources.txt")).read()
    recorded += open(os.path.join(ROOT, "profiles", "tfhe_stages_a_kernel_resources.txt")).read()
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        assert name in recorded, name
    # the plain key switch of the same build, not a constant
    plain = {r["pretty"]: r for r in kernel_resources.report(os.path.join(CSRC, "pfhe_bootstrap.hip"))}
    for w, size in words.items():
        ks = by_name["tfhe_bitext_keyswitch_kernel<%s>" % w]
        assert ks.get("Occupancy", 0) >= plain["tfhe_keyswitch_kernel<%s>" % w]["Occupancy"] > 0, (ks, w)
        assert ks.get("LDS Size", 0) == K_KS_MAX_ROWS * K_KS_TILE_M * size, ks
        assert by_name["tfhe_extract_kernel<%s, true>" % w].get("LDS Size", 0) == 0
    header = open(os.path.join(CSRC, "pfhe_tfhe_exact_device.hpp")).read()
    assert "constexpr u32 kKsMaxRows = %d;" % K_KS_MAX_ROWS in header and "kKsRows = 8" in header


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
    assert len(NAMES) == 12
    lib = pfhe.lib()
    header = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
        assert "%s(" % name in header, name
    # the note the entries of the look-up carry: no reference counterpart, the rule is the project's own
    section = header[header.index("bit extraction: an LWE ciphertext of a multi-bit message"):]
    assert "The reference has none; the rule is this project's own (DESIGN.md §24)" in section
    assert "typedef struct pfhe_bitext pfhe_bitext;" in section and "typedef struct pfhe_bitext32 pfhe_bitext32;" in section
    for w in ("", "32"):
        dev, host = getattr(lib, f"pfhe_bitext{w}_extract_bits_dev"), getattr(lib, f"pfhe_bitext{w}_extract_bits")
        assert len(dev.argtypes) == len(host.argtypes) + 1 == 12
        assert dev.argtypes[7] == dev.argtypes[8] == C.c_uint32                  # delta_log, bits
        create = getattr(lib, f"pfhe_bitext{w}_create")
        assert len(create.argtypes) == 9 and create.argtypes[2] == create.argtypes[5] == C.c_uint32
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    params = inspect.signature(pfhe.TfheBitExtractContext.__init__).parameters
    assert list(params)[1:] == ["fft", "basis", "lwe_dimension", "glwe_dimension", "ks_basis", "chunk"]
    assert params["glwe_dimension"].default == 1 and params["ks_basis"].default is None and params["chunk"].default == 0
    assert list(inspect.signature(pfhe.tfhe_extract_bits).parameters) == \
        ["lwe_in", "bsk", "ksk", "bits_out", "ctx", "delta_log", "bits"]
    assert list(inspect.signature(pfhe.tfhe_extract_bits_dev).parameters) == \
        ["lwe_in", "bsk", "ksk", "bits_out", "ctx", "delta_log", "bits", "stream"]
    chain = inspect.signature(pfhe.tfhe_lut_on_integer_dev).parameters
    assert list(chain) == ["lwe_in", "bsk", "ksk", "pfksk", "table", "out", "bitext_ctx", "cbs_ctx", "lut_ctx", "delta_log",
                           "extract", "stream"]
    assert chain["extract"].default == 1 and chain["stream"].default is None
    assert "allocates" in pfhe.tfhe_lut_on_integer_dev.__doc__
    with pytest.raises(ValueError):              # no bit extraction without the key switch, before anything is created
        pfhe.TfheBitExtractContext(None, pfhe.ApproxSignedBasis(32, 7, 3), 4)


def test_every_width_pair_of_the_family_has_one_signature_up_to_the_word():
    """The family has a prefix of its own, so the rule tests/test_boundary_static.py holds the pfhe_tfhe_ pairs to is held
    here for it, on that file's own reading of pfhe.h: the u32 prototype of each pair is the u64 one with uint64_t ->
    uint32_t and pfhe_bitext -> pfhe_bitext32, no name lacks its twin, and both handle types are declared."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_boundary_static import header_signatures
    text = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    sigs = {n: v for n, v in header_signatures(text).items() if n.startswith("pfhe_bitext")}
    assert set(sigs) == set(NAMES)
    handles = set(re.findall(r"typedef struct (pfhe_\w+) \1;", text))
    assert {"pfhe_bitext", "pfhe_bitext32"} <= handles
    twin = lambda t: re.sub(r"\bpfhe_bitext\b", "pfhe_bitext32", t.replace("uint64_t", "uint32_t"))
    pairs = 0
    for name, (ret, params) in sigs.items():
        if name.startswith("pfhe_bitext32_"):
            assert "pfhe_bitext_" + name[len("pfhe_bitext32_"):] in sigs, name
            continue
        other = "pfhe_bitext32_" + name[len("pfhe_bitext_"):]
        assert (twin(ret), [twin(p) for p in params]) == sigs[other], (name, sigs[name], sigs[other])
        pairs += 1
    assert pairs == 6


def test_mirror_class_leaves_exactly_its_own_symbols_undefined():
    """TfheBitExtractT is a template only: the unit that instantiates it leaves undefined what a unit that only includes the
    header does (a subset of the 306 pinned by tests/test_cpp_header.py) plus the 12 of its own list"""
    import cpp_mirror
    support = os.path.join(ROOT, "tests", "support")
    own = set(open(os.path.join(support, "cpp_mirror_bitext_symbols.txt")).read().split())
    assert own == set(NAMES)
    undefined = cpp_mirror.undefined_pfhe_symbols(os.path.join(support, "cpp_mirror_bitext_instantiate.cpp"))
    old = cpp_mirror.mirror_symbols()
    assert not own & old
    assert undefined - old == own, sorted((undefined - old) ^ own)
    text = open(os.path.join(ROOT, "include", "pfhe.hpp")).read()
    assert "class TfheBitExtractT : public detail::Fns<W>::TfheBitext" in text
    assert "using TfheBitExtract = TfheBitExtractT<uint64_t>;" in text and "using TfheBitExtract32 = TfheBitExtractT<uint32_t>;" in text


@pytest.mark.parametrize("w, bits", [("", 64), ("32", 32)])
def test_create_refuses_its_arguments_in_order(pfhe, table, w, bits):
    """a null out pointer; the product plan's checks in their order (the basis's assert!s, Unsupported above 64, the table);
    the dimensions; the key-switch basis's assert!s; and only then the device.  A refusal leaves the handle null."""
    lib = pfhe.lib()
    _, fft = table                       # log N = 3
    create = getattr(lib, f"pfhe_bitext{w}_create")
    h = C.c_void_p(1)
    k, lb, ell, n, ks_lb, ks_ell = 1, 7, 3, 5, 4, 3
    assert create(fft, k, lb, ell, n, ks_lb, ks_ell, 0, None) == BAD_ARGUMENT                      # nowhere to put the handle
    for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        h.value = 1
        assert create(None, 65, bad_lb, bad_len, 0, 0, 0, 0, C.byref(h)) == BAD_ARGUMENT           # whatever else is wrong
        assert not h.value and ("log_basis" in last_error(lib) or "decompose_length" in last_error(lib))
    h.value = 1
    assert create(None, 65, lb, ell, 0, 0, 0, 0, C.byref(h)) == UNSUPPORTED and not h.value        # before the table
    assert "glwe_dimension above 64" in last_error(lib)
    assert create(None, k, lb, ell, 0, 0, 0, 0, C.byref(h)) == BAD_ARGUMENT                        # no table, before the dimensions
    assert "must be at least 1" not in last_error(lib)
    for bad_k, bad_n in ((0, n), (k, 0), (k, 2 ** 31 - 1), (k, 2 ** 40)):
        h.value = 1
        assert create(fft, bad_k, lb, ell, bad_n, 0, 99, 0, C.byref(h)) == BAD_ARGUMENT and not h.value   # before the key switch's basis
        assert "glwe_dimension must be at least 1 and lwe_dimension in 1..2^31-2" in last_error(lib)
    for bad_lb, bad_len in ((0, 0), (bits, 0), (10, bits // 10 + 1)):
        h.value = 1
        assert create(fft, k, lb, ell, n, bad_lb, bad_len, 0, C.byref(h)) == BAD_ARGUMENT and not h.value
        assert "log_basis" in last_error(lib) or "decompose_length" in last_error(lib)
    for args in ((k, lb, ell, n, ks_lb, ks_ell, 0), (2, lb, 0, 2 ** 31 - 2, ks_lb, 0, 3), (64, lb, ell, 1, bits - 1, 1, 5)):
        h.value = 1
        assert create(fft, *args, C.byref(h)) == NO_DEVICE and not h.value                        # the last check


@pytest.mark.parametrize("w", ["", "32"])
def test_calls_on_no_handle_are_refused(pfhe, w):
    lib = pfhe.lib()
    buf = (C.c_uint64 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    keys = C.cast(buf, C.POINTER(C.c_double))
    assert getattr(lib, f"pfhe_bitext{w}_extract_bits_dev")(None, ptr, 8, keys, 8, ptr, 8, 0, 0, ptr, 8, None) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_bitext{w}_extract_bits")(None, ptr, 8, keys, 8, ptr, 8, 3, 2, ptr, 8) == BAD_ARGUMENT
    assert getattr(lib, f"pfhe_bitext{w}_in_use")(None) == 0
    assert getattr(lib, f"pfhe_bitext{w}_scratch_bytes")(None) == 0
    getattr(lib, f"pfhe_bitext{w}_destroy")(None)


def test_no_fallback_without_a_device(pfhe):
    """without a GPU no table can be made, so nothing of this file's calls computes on the CPU"""
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pfhe.PfheError) as e:
        pfhe.FullComplex64FftTable(3)
    assert e.value.kind == "NoDevice"
