"""CPU-side checks of the random layer (pfhe_csprng_keystream_dev, pfhe_rand{,32}_*): the 19 entry points are in the ctypes
table and declared in include/pfhe.h with their note, the width pairs have one signature up to the word, the C++ mirror's
templates leave exactly their own symbols undefined, the Python names are exported, every refusal that precedes the device
arrives with no device present and in the stated order, and the compiler's resource report shows the new kernels for both
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

SAMPLERS = ("uniform_dev", "binary_dev", "ternary_dev", "tuniform_dev")
CALLS = SAMPLERS + ("fill_rows_dev", "lwe_encrypt_seeded", "lwe_encrypt_seeded_dev", "seeded_expand", "seeded_expand_dev")
NAMES = ["pfhe_csprng_keystream_dev"] + [pre + c for pre in ("pfhe_rand_", "pfhe_rand32_") for c in CALLS]
PUBLIC = ("RandSeed", "csprng_keystream_dev", "torus_uniform_dev", "torus_binary_dev", "torus_ternary_dev", "torus_tuniform_dev",
          "tfhe_fill_rows_dev", "lwe_encrypt_seeded", "lwe_encrypt_seeded_dev", "seeded_expand", "seeded_expand_dev",
          "tfhe_generate_ksk_seeded_dev")
OK, BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE = 0, 32, 33, 34
CSRC = os.path.join(ROOT, "primus-fhe_amd", "csrc")
CAP = (1 << 64) - (1 << 20)          # pfhe_csprng_device.hpp: kRandMaxIndex, the largest output index a call may end at


def test_csprng_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources
    rows = kernel_resources.report(os.path.join(CSRC, "pfhe_csprng.hip"))
    by_name = {r["pretty"]: r for r in rows}
    words = ("unsigned int", "unsigned long long")
    want = ["rand_fill_kernel<%s, %d>" % (w, s) for w in words for s in range(4)] + \
           ["%s<%s>" % (k, w) for k in ("rand_rows_kernel", "rand_lwe_seeded_kernel") for w in words]
    assert sorted(by_name) == sorted(want), sorted(by_name)
    for name in want:
        r = by_name[name]
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        assert r.get("Occupancy", 0) > 0
        # a workgroup's 256 blocks cross LDS at 17 words each; the fused kernel keeps its blocks in registers
        assert r.get("LDS Size", 0) == (0 if "seeded" in name else 256 * 17 * 4), r


def test_no_key_reaches_device_memory_or_a_message():
    """keys are host pointers read into a struct that is a kernel argument: the source copies no seed to the device, and no
    message it sets formats a word"""
    text = open(os.path.join(CSRC, "pfhe_csprng.hip")).read()
    assert "hipMemcpy" not in text and "upload" not in text and "printf" not in text
    assert re.findall(r"__global__[^\n]*\n?[^\n]*\(RandSeed \w+", text), "seeds are by-value kernel arguments"
    for message in re.findall(r'set_last_error\(([^;]*)\);', text):
        assert "%" not in message and "to_string" not in message and "key[" not in message, message


@pytest.fixture(scope="module")
def pfhe():
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        p.build()
    return p


def test_symbols_are_in_the_ctypes_table_the_headers_and_the_package(pfhe):
    assert len(NAMES) == 19
    lib = pfhe.lib()
    header = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
        assert "%s(" % name in header, name
    section = header[header.index("random layer: a device ChaCha20 stream"):]
    for cited in ("DESIGN.md §26", "RFC 8439", "primus_distr/src/common.rs:22-42", "common.rs:56-76", "UNVERIFIED",
                  "no primus_distr counterpart", "gathers no entropy", "PFHE_ERR_BAD_ARGUMENT", "PFHE_ERR_BAD_LENGTH",
                  "the device"):
        assert cited in section, cited
    for name in PUBLIC:
        assert hasattr(pfhe, name) and name in pfhe.__all__, name
    for name in ("torus_uniform", "torus_noise"):                      # the statistical fillers stay as they are
        assert "NOT CRYPTOGRAPHIC" in getattr(pfhe, name).__doc__
    dev = inspect.signature(pfhe.lwe_encrypt_seeded_dev).parameters
    host = inspect.signature(pfhe.lwe_encrypt_seeded).parameters
    assert list(host) == ["mask_seed", "noise_seed", "first_row", "key", "bound_log2", "bodies", "device"]
    assert list(dev) == list(host) + ["stream"] and host["device"].default == 0 and dev["device"].default is None
    fill = inspect.signature(pfhe.tfhe_fill_rows_dev).parameters
    assert list(fill) == ["mask_seed", "noise_seed", "first_row", "mask_len", "body_len", "bound_log2", "out", "add", "device",
                          "stream"] and fill["add"].default is False


def test_rand_seed_takes_the_callers_key_and_never_shows_it(pfhe):
    key = bytes(range(32))
    s = pfhe.RandSeed(key, 0x8000000000000001)
    assert list(s._key) == [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]
    assert list(s._nonce) == [1, 0x80000000] and s.nonce == 0x8000000000000001
    assert "key=<32 bytes>" in repr(s) and key.hex() not in repr(s) and "03020100" not in repr(s)
    t = s.with_nonce(5)
    assert list(t._key) == list(s._key) and t.nonce == 5
    a, b = pfhe.RandSeed.fresh(), pfhe.RandSeed.fresh(nonce=3)
    assert list(a._key) != list(b._key) and b.nonce == 3
    assert "os.urandom" in pfhe.RandSeed.fresh.__doc__ and "NO entropy" in pfhe.RandSeed.__doc__
    for bad in (b"short", "x" * 32, None):
        with pytest.raises(ValueError):
            pfhe.RandSeed(bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            pfhe.RandSeed(key, bad)
    with pytest.raises(TypeError):
        pfhe.seeded_expand(key, 0, 3, 1, np.zeros(2, np.uint32), np.zeros(8, np.uint32))


def test_every_width_pair_of_the_family_has_one_signature_up_to_the_word():
    """The family has a prefix of its own, so the rule tests/test_boundary_static.py holds the pfhe_tfhe_ pairs to is held
    here for it, on that file's own reading of pfhe.h: the u32 prototype of each pair is the u64 one with uint64_t ->
    uint32_t.  Keys and nonces are uint32_t words and indices size_t at both widths, so the replacement touches the torus
    words alone."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_boundary_static import header_signatures
    text = open(os.path.join(ROOT, "include", "pfhe.h")).read()
    sigs = {n: v for n, v in header_signatures(text).items() if n.startswith(("pfhe_rand", "pfhe_csprng"))}
    assert set(sigs) == set(NAMES)
    pairs = 0
    for name, (ret, params) in sigs.items():
        if not name.startswith("pfhe_rand_"):
            continue
        other = "pfhe_rand32_" + name[len("pfhe_rand_"):]
        assert (ret, [t.replace("uint64_t", "uint32_t") for t in params]) == sigs[other], (name, sigs[name], sigs[other])
        assert params[1:3] == ["const uint32_t *", "const uint32_t *"] and any("uint64_t *" in t for t in params)
        pairs += 1
    assert pairs == 9
    assert sigs["pfhe_csprng_keystream_dev"][1] == ["int", "const uint32_t *", "const uint32_t *", "size_t", "uint32_t *",
                                                    "size_t", "void *"]


def test_mirror_templates_leave_exactly_their_own_symbols_undefined():
    import cpp_mirror
    support = os.path.join(ROOT, "tests", "support")
    own = set(open(os.path.join(support, "cpp_mirror_csprng_symbols.txt")).read().split())
    assert own == set(NAMES)
    undefined = cpp_mirror.undefined_pfhe_symbols(os.path.join(support, "cpp_mirror_csprng_instantiate.cpp"))
    old = cpp_mirror.mirror_symbols()
    assert len(old) == 306 and not own & old
    assert undefined - old == own, sorted((undefined - old) ^ own)


# ---- refusals, all with no device present: device -1 is refused last, whatever the machine ----

def _ptr(a):
    return C.cast(a, C.c_void_p)


def _seeds():
    k1, k2 = (C.c_uint32 * 8)(*range(8)), (C.c_uint32 * 8)(*range(8))
    n1, n2 = (C.c_uint32 * 2)(1, 0), (C.c_uint32 * 2)(2, 0)
    return k1, n1, k2, n2


def _with(call, good):
    def run(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    return run


@pytest.mark.parametrize("w, word, bits", [("", C.c_uint64, 64), ("32", C.c_uint32, 32)])
def test_samplers_refuse_their_arguments_in_order(pfhe, w, word, bits):
    lib = pfhe.lib()
    k1, n1, _, _ = _seeds()
    out = (word * 40)()
    calls = [(getattr(lib, "pfhe_rand%s_%s" % (w, s)), s == "tuniform_dev") for s in SAMPLERS]
    if w == "32":
        calls.append((lib.pfhe_csprng_keystream_dev, False))
    for call, bounded in calls:
        lead = [-1, _ptr(k1), _ptr(n1), 5] + ([17] if bounded else [])
        at_out = len(lead)
        run = _with(call, lead + [_ptr(out), 40, None])
        assert run(a1=None, **{"a%d" % at_out: None}) == BAD_ARGUMENT and "key" in lib.pfhe_last_error().decode()
        assert run(a2=None) == BAD_ARGUMENT
        if bounded:
            assert run(a4=bits - 1, **{"a%d" % at_out: None}) == BAD_ARGUMENT and "BITS-2" in lib.pfhe_last_error().decode()
            assert run(a4=bits - 2) == NO_DEVICE
            assert run(a4=0) == NO_DEVICE
        assert run(a3=CAP - 39, **{"a%d" % at_out: None}) == BAD_LENGTH        # the last index passes the cap
        assert run(a3=(1 << 64) - 1, **{"a%d" % at_out: None}) == BAD_LENGTH          # offset + n wraps
        assert run(a3=CAP - 40) == NO_DEVICE
        assert run(**{"a%d" % at_out: None, "a%d" % (at_out + 1): 0}) == OK            # no outputs: a no-op
        assert run(**{"a%d" % at_out: None}) == BAD_ARGUMENT                          # a null buffer
        assert run() == NO_DEVICE                                                      # the last check


@pytest.mark.parametrize("w, word, bits", [("", C.c_uint64, 64), ("32", C.c_uint32, 32)])
def test_fill_rows_refuses_its_arguments_in_order(pfhe, w, word, bits):
    lib = pfhe.lib()
    k1, n1, k2, n2 = _seeds()
    out = (word * 24)()                                                               # 3 rows of 7 + 1
    run = _with(getattr(lib, "pfhe_rand%s_fill_rows_dev" % w),
                [-1, _ptr(k1), _ptr(n1), _ptr(k2), _ptr(n2), 0, 7, 1, 17, 0, _ptr(out), 24, None])
    for at in (1, 2, 3, 4):
        assert run(**{"a%d" % at: None, "a8": bits}) == BAD_ARGUMENT and "null" in lib.pfhe_last_error().decode()
    assert run(a4=_ptr(n1), a8=bits) == BAD_ARGUMENT and "differ" in lib.pfhe_last_error().decode()   # one stream for both
    assert run(a3=_ptr((C.c_uint32 * 8)(*range(8))), a4=_ptr((C.c_uint32 * 2)(1, 0))) == BAD_ARGUMENT  # equal by value
    assert run(a8=bits - 1, a6=0) == BAD_ARGUMENT and "BITS-2" in lib.pfhe_last_error().decode()
    for at in (6, 7):
        for bad in (0, 2 ** 31 - 1, 2 ** 40):
            assert run(**{"a%d" % at: bad, "a11": 23}) == BAD_ARGUMENT and "1..2^31-2" in lib.pfhe_last_error().decode()
    assert run(a11=23, a10=None) == BAD_LENGTH and "rows" in lib.pfhe_last_error().decode()
    assert run(a5=1 << 62, a10=None) == BAD_LENGTH and "2^64 - 2^20" in lib.pfhe_last_error().decode()
    assert run(a11=0, a10=None) == OK
    assert run(a10=None) == BAD_ARGUMENT
    assert run() == NO_DEVICE
    assert run(a9=1, a8=bits - 2) == NO_DEVICE


@pytest.mark.parametrize("w, word, bits", [("", C.c_uint64, 64), ("32", C.c_uint32, 32)])
def test_seeded_calls_refuse_their_arguments_in_order(pfhe, w, word, bits):
    lib = pfhe.lib()
    k1, n1, k2, n2 = _seeds()
    key, bodies, out = (word * 7)(), (word * 3)(), (word * 24)()
    for form in ("_dev", ""):
        tail = [None] if form else []
        run = _with(getattr(lib, "pfhe_rand%s_lwe_encrypt_seeded%s" % (w, form)),
                    [-1, _ptr(k1), _ptr(n1), _ptr(k2), _ptr(n2), 0, _ptr(key), 7, 17, _ptr(bodies), 3] + tail)
        for at in (1, 2, 3, 4):
            assert run(**{"a%d" % at: None, "a8": bits}) == BAD_ARGUMENT
        assert run(a3=_ptr(k1), a4=_ptr(n1), a8=bits) == BAD_ARGUMENT and "differ" in lib.pfhe_last_error().decode()
        assert run(a8=bits - 1, a7=0) == BAD_ARGUMENT and "BITS-2" in lib.pfhe_last_error().decode()
        for bad in (0, 2 ** 31 - 1):
            assert run(a7=bad, a6=None) == BAD_ARGUMENT and "1..2^31-2" in lib.pfhe_last_error().decode()
        assert run(a5=1 << 62, a6=None) == BAD_LENGTH
        assert run(a10=0, a6=None, a9=None) == OK
        assert run(a6=None) == BAD_ARGUMENT and run(a9=None) == BAD_ARGUMENT
        if form:
            inside = C.c_void_p(C.addressof(key) + C.sizeof(word))
            assert run(a9=inside) == BAD_ARGUMENT and "overlap" in lib.pfhe_last_error().decode()
        assert run() == NO_DEVICE

        run = _with(getattr(lib, "pfhe_rand%s_seeded_expand%s" % (w, form)),
                    [-1, _ptr(k1), _ptr(n1), 0, 7, 1, _ptr(bodies), 3, _ptr(out), 24] + tail)
        assert run(a1=None, a4=0) == BAD_ARGUMENT and run(a2=None, a4=0) == BAD_ARGUMENT
        for at in (4, 5):
            for bad in (0, 2 ** 31 - 1):
                assert run(**{"a%d" % at: bad, "a9": 23}) == BAD_ARGUMENT and "1..2^31-2" in lib.pfhe_last_error().decode()
        assert run(a9=23, a8=None) == BAD_LENGTH                                       # not a whole number of rows
        assert run(a9=16, a8=None) == BAD_LENGTH and run(a7=2, a6=None) == BAD_LENGTH  # bodies and out disagree on the rows
        assert run(a5=2, a6=None) == BAD_LENGTH                                        # 3 body words are not rows of 2
        assert run(a3=1 << 62, a6=None) == BAD_LENGTH
        assert run(a7=0, a9=0, a6=None, a8=None) == OK
        assert run(a6=None) == BAD_ARGUMENT and run(a8=None) == BAD_ARGUMENT
        if form:
            inside = C.c_void_p(C.addressof(out) + 8 * C.sizeof(word))
            assert run(a6=inside) == BAD_ARGUMENT and "overlap" in lib.pfhe_last_error().decode()
        assert run() == NO_DEVICE


def test_python_wrappers_refuse_before_the_library(pfhe):
    seed = pfhe.RandSeed(bytes(32))
    with pytest.raises(TypeError):
        pfhe.lwe_encrypt_seeded(seed, seed.with_nonce(1), 0, np.zeros(3, np.uint32), 5, np.zeros(2, np.uint64))
    with pytest.raises(pfhe.PfheError) as e:                                      # the library's own refusal, as an exception
        pfhe.lwe_encrypt_seeded(seed, seed, 0, np.zeros(3, np.uint32), 5, np.zeros(2, np.uint32))
    assert e.value.code == BAD_ARGUMENT
