"""Refusals of the four table constructors that are decided before the device is touched, and the NoDevice
status of a constructor whose arguments are good: status code and pfhe_last_error text, literally, per handle.
(The refusals of the other entry points need a created table: tests/test_gpu_table_statuses.py.)"""
import ctypes as C

import numpy as np
import pytest

OK, NO_PRIMITIVE_ROOT, MODULUS_TOO_LARGE = 0, 1, 5
BAD_LENGTH, BAD_ARGUMENT, NO_DEVICE, UNSUPPORTED = 32, 33, 34, 36

T_EMPTY = "empty modulus list"
T_NO_ROOT = "there is no primitive 2N-th root of unity modulo this modulus"
T_TOO_LARGE_32 = "modulus is too large for a u32 NTT table (max 30 bits)"

Q61 = (2305843009211596801, 2305843009210023937, 2305843009208713217)
Q30 = (1073479681, 1071513601, 1070727169)


def last_error(lib):
    return lib.pfhe_last_error().decode()


class Handle:
    def __init__(self, prefix, moduli, dtype, single, has_mul_to):
        self.prefix, self.moduli, self.dtype, self.single, self.has_mul_to = prefix, moduli, dtype, single, has_mul_to

    def create(self, lib, log_n, moduli, device, out, count=None):
        """The constructor of this family; `moduli` None passes a null list (with `count`)."""
        f = getattr(lib, self.prefix + "create")
        if self.single:
            return f(log_n, moduli[0], device, C.byref(out))
        ctype = C.c_uint64 if self.dtype is np.uint64 else C.c_uint32
        arr = None if moduli is None else (ctype * max(1, len(moduli)))(*moduli)
        return f(log_n, arr, len(moduli) if count is None else count, device, C.byref(out))


HANDLES = {
    "ntt": Handle("pfhe_ntt_", Q61[:1], np.uint64, True, True),
    "dcrt": Handle("pfhe_dcrt_", Q61, np.uint64, False, True),
    "ntt32": Handle("pfhe_ntt32_", Q30[:1], np.uint32, True, False),
    "dcrt32": Handle("pfhe_dcrt32_", Q30, np.uint32, False, False),
}


@pytest.fixture(scope="module")
def lib():
    import primus_fhe_amd as p
    p.build()
    return p.lib()


def refused(lib, h, status, text, log_n, moduli, device=0, count=None, clears_out=True):
    out = C.c_void_p(1)
    assert h.create(lib, log_n, moduli, device, out, count) == status, last_error(lib)
    assert bool(out.value) != clears_out, "a refused constructor leaves a null handle"
    if text is not None:
        assert last_error(lib) == text


def prime_of_shape(lo, step):
    """The first prime q = 1 (mod step) above lo."""
    q = lo + 1
    while not (q % step == 1 and all(q % p for p in range(3, int(q ** 0.5) + 2, 2))):
        q += 1 if q % step != 1 else step
    return q


@pytest.mark.parametrize("name", sorted(HANDLES))
def test_constructor_refusals_before_the_device(lib, name):
    h = HANDLES[name]
    # 2N does not divide q - 1 (log_n = 21: none of these primes has a 2^22-th root of unity)
    refused(lib, h, NO_PRIMITIVE_ROOT, T_NO_ROOT, 21, h.moduli)
    refused(lib, h, UNSUPPORTED, "log_n > 22 is not supported by this build", 23, h.moduli)
    null_out = getattr(lib, h.prefix + "create")
    if h.single:
        assert null_out(5, h.moduli[0], 0, None) == BAD_ARGUMENT
    else:
        assert null_out(5, None, 0, 0, None) == BAD_ARGUMENT
        refused(lib, h, BAD_ARGUMENT, T_EMPTY, 5, (), count=0)
        refused(lib, h, BAD_ARGUMENT, T_EMPTY, 5, None, count=0)
        # a null list with a count: the u32 table names the empty list; the u64 table refuses it with the null `out`,
        # before it writes a text or the handle
        refused(lib, h, NO_PRIMITIVE_ROOT, T_NO_ROOT, 21, h.moduli)
        if name == "dcrt32":
            refused(lib, h, BAD_ARGUMENT, T_EMPTY, 5, None, count=3)
        else:
            refused(lib, h, BAD_ARGUMENT, T_NO_ROOT, 5, None, count=3, clears_out=False)
        # the second modulus is the bad one
        refused(lib, h, NO_PRIMITIVE_ROOT, T_NO_ROOT, 5, (h.moduli[0], 15, h.moduli[2]))


def test_u32_modulus_bound_is_reported_after_the_root_search(lib):
    q_ok = prime_of_shape(1 << 30, 1 << 12)     # a prime above 2^30 with a 2^12-th root of unity
    assert (1 << 30) < q_ok < (1 << 31)
    q_no_root = (1 << 30) + 3                   # 2N does not divide q - 1, and q is above the bound as well
    for name in ("ntt32", "dcrt32"):
        h = HANDLES[name]
        with_big = (q_ok,) if h.single else (h.moduli[0], q_ok)
        refused(lib, h, MODULUS_TOO_LARGE, T_TOO_LARGE_32, 10, with_big)
        without_root = (q_no_root,) if h.single else (h.moduli[0], q_no_root)
        refused(lib, h, NO_PRIMITIVE_ROOT, T_NO_ROOT, 10, without_root)
        # the largest modulus the table takes gets as far as the device
        out = C.c_void_p()
        status = h.create(lib, 10, h.moduli, 1 << 20, out)
        assert status == NO_DEVICE and not out.value


@pytest.mark.parametrize("name", sorted(HANDLES))
def test_good_arguments_reach_the_device_check(lib, name):
    """No device, or an index past the last one: NoDevice with the text of the case, never a fallback."""
    h = HANDLES[name]
    count = C.c_int(-1)
    assert lib.pfhe_device_count(C.byref(count)) == OK
    text = "device index out of range" if count.value > 0 else "no HIP device available (libpfhe_hip has no CPU fallback)"
    refused(lib, h, NO_DEVICE, text, 5, h.moduli, device=1 << 20)
    refused(lib, h, NO_DEVICE, text, 5, h.moduli, device=-1)
    if count.value == 0:
        refused(lib, h, NO_DEVICE, text, 5, h.moduli, device=0)
