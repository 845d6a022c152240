"""Refusals of the four table handles (pfhe_ntt, pfhe_dcrt, pfhe_ntt32, pfhe_dcrt32) through the C ABI.

Every entry point the four handles share is driven with each kind of bad input — null table, null data with a
non-zero length, unaligned device pointer, length that is not a multiple of L*N, multiplicand length, monomial
length, unreduced monomial coefficient — and the status code and the pfhe_last_error text are compared literally,
per handle.  A refusal that writes no text must leave the previous text alone: each such case is preceded by a
refusal with a known text.  A valid zero-length call returns PFHE_OK on every handle.  The calls go through lib()
directly, so the Python mirror's own checks are not in the way.
"""
import ctypes as C

import numpy as np
import pytest

from test_table_statuses_cpu import BAD_ARGUMENT, BAD_LENGTH, HANDLES, OK, last_error

pytestmark = pytest.mark.gpu

T_SLICE = "slice length is not a multiple of the polynomial length"
T_MULTIPLICAND = "multiplicand must have the same length or exactly one polynomial"
T_MONOMIAL_LEN = "monomial output must be exactly one polynomial"
T_MONOMIAL_COEFF = "monomial coefficient must be reduced modulo every modulus"
SLICES = ("transform_slice", "inverse_transform_slice", "lazy_transform_slice", "lazy_inverse_transform_slice")
LOG_N = 5


class Table:
    """One created handle of the family `name`, with device and host buffers of two units."""

    def __init__(self, name):
        import torch
        import primus_fhe_amd as p

        self.name, self.h = name, HANDLES[name]
        self.lib = p.lib()
        self.handle = C.c_void_p()
        assert self.h.create(self.lib, LOG_N, self.h.moduli, 0, self.handle) == OK, last_error(self.lib)
        self.unit = (1 << LOG_N) * len(self.h.moduli)
        self.size = self.h.dtype().itemsize
        tdt = torch.int64 if self.size == 8 else torch.int32
        self.bufs = [torch.zeros(2 * self.unit + 8, dtype=tdt, device="cuda") for _ in range(4)]
        self.host = np.zeros(2 * self.unit + 1, self.h.dtype)

    def close(self):
        self.f("destroy")(self.handle)

    def f(self, entry):
        return getattr(self.lib, self.h.prefix + entry)

    def dev(self, i, odd=False):
        """An aligned device pointer, or (odd) one word past it: not 16-byte aligned."""
        return C.c_void_p(self.bufs[i].data_ptr() + (self.size if odd else 0))

    def hostp(self):
        return self.host.ctypes.data_as(C.c_void_p)

    def prime(self):
        """Leave a known text behind, so that a refusal that writes none can be told from one that does."""
        assert self.f("transform_dev")(self.handle, self.dev(0), 1, 0, None) == BAD_LENGTH
        assert last_error(self.lib) == T_SLICE

    def refused(self, status, text, entry, *args):
        """`entry(*args)` returns `status`; the last error is `text`, or (text None) what it was before the call."""
        if text is None:
            self.prime()
            text = T_SLICE
        else:  # make sure the text is written by this call
            assert self.f("transform_monomial")(self.handle, 0, 0, self.hostp(), self.unit + 1) == BAD_LENGTH
            assert last_error(self.lib) == T_MONOMIAL_LEN
            if text == T_MONOMIAL_LEN:
                self.prime()
        assert self.f(entry)(*args) == status, (self.name, entry, last_error(self.lib))
        assert last_error(self.lib) == text, (self.name, entry)


@pytest.fixture(scope="module", params=sorted(HANDLES))
def tab(request):
    t = Table(request.param)
    yield t
    t.close()


def test_null_table(tab):
    u, d, hp = tab.unit, tab.dev, tab.hostp()
    assert tab.f("poly_length")(None) == 0
    assert tab.f("device")(None) == -1
    tab.f("destroy")(None)
    for e in SLICES:
        tab.refused(BAD_ARGUMENT, None, e, None, hp, u)
    tab.refused(BAD_ARGUMENT, None, "transform_monomial", None, 1, 0, hp, u)
    tab.refused(BAD_ARGUMENT, None, "transform_coeff_one_monomial", None, 0, hp, u)
    tab.refused(BAD_ARGUMENT, None, "transform_coeff_minus_one_monomial", None, 0, hp, u)
    tab.refused(BAD_ARGUMENT, None, "transform_dev", None, d(0), u, 0, None)
    tab.refused(BAD_ARGUMENT, None, "inverse_transform_dev", None, d(0), u, 0, None)
    tab.refused(BAD_ARGUMENT, None, "mul_assign_dev", None, d(0), u, d(1), u, None)
    tab.refused(BAD_ARGUMENT, None, "add_mul_assign_dev", None, d(0), d(1), u, d(2), u, None)
    if tab.h.has_mul_to:
        tab.refused(BAD_ARGUMENT, None, "mul_to_dev", None, d(0), u, d(1), u, d(2), None)
        tab.refused(BAD_ARGUMENT, None, "mul_add_to_dev", None, d(0), u, d(1), u, d(2), d(3), None)


def test_null_data_with_a_length(tab):
    h, u, d = tab.handle, tab.unit, tab.dev
    for e in SLICES:
        tab.refused(BAD_ARGUMENT, None, e, h, None, u)
        tab.refused(BAD_ARGUMENT, None, e, h, None, u + 1)  # before the length check
    for e in ("transform_dev", "inverse_transform_dev"):
        tab.refused(BAD_ARGUMENT, None, e, h, None, u, 0, None)
        tab.refused(BAD_ARGUMENT, None, e, h, None, u + 1, 1, None)
    tab.refused(BAD_ARGUMENT, None, "mul_assign_dev", h, None, u, d(1), u, None)
    tab.refused(BAD_ARGUMENT, None, "mul_assign_dev", h, d(0), u, None, u, None)
    tab.refused(BAD_ARGUMENT, None, "mul_assign_dev", h, d(0, odd=True), u, None, u, None)  # before the alignment check
    tab.refused(BAD_ARGUMENT, None, "add_mul_assign_dev", h, None, d(1), u, d(2), u, None)
    tab.refused(BAD_ARGUMENT, None, "add_mul_assign_dev", h, d(0), None, u, d(2), u, None)
    tab.refused(BAD_ARGUMENT, None, "add_mul_assign_dev", h, d(0), d(1), u, None, u, None)
    # the monomial forms refuse a null output whatever the length
    tab.refused(BAD_ARGUMENT, None, "transform_monomial", h, 1, 0, None, u)
    tab.refused(BAD_ARGUMENT, None, "transform_monomial", h, 1, 0, None, 0)
    tab.refused(BAD_ARGUMENT, None, "transform_coeff_one_monomial", h, 0, None, u)
    tab.refused(BAD_ARGUMENT, None, "transform_coeff_minus_one_monomial", h, 0, None, u)
    if tab.h.has_mul_to:
        tab.refused(BAD_ARGUMENT, None, "mul_to_dev", h, None, u, d(1), u, d(2), None)
        tab.refused(BAD_ARGUMENT, None, "mul_to_dev", h, d(0), u, None, u, d(2), None)
        tab.refused(BAD_ARGUMENT, None, "mul_to_dev", h, d(0), u, d(1), u, None, None)
        tab.refused(BAD_ARGUMENT, None, "mul_add_to_dev", h, d(0), u, d(1), u, None, d(3), None)
        tab.refused(BAD_ARGUMENT, None, "mul_add_to_dev", h, d(0), u, d(1), u, d(2), None, None)


def test_unaligned_device_pointer(tab):
    h, u, d = tab.handle, tab.unit, tab.dev
    for e in ("transform_dev", "inverse_transform_dev"):
        tab.refused(BAD_ARGUMENT, "data must be 16-byte aligned", e, h, d(0, odd=True), u, 0, None)
        tab.refused(BAD_ARGUMENT, "data must be 16-byte aligned", e, h, d(0, odd=True), u + 1, 0, None)  # before the length
    tab.refused(BAD_ARGUMENT, "acc must be 16-byte aligned", "mul_assign_dev", h, d(0, odd=True), u, d(1), u, None)
    tab.refused(BAD_ARGUMENT, "b must be 16-byte aligned", "mul_assign_dev", h, d(0), u, d(1, odd=True), u, None)
    tab.refused(BAD_ARGUMENT, "acc must be 16-byte aligned", "mul_assign_dev", h, d(0, odd=True), u, d(1, odd=True), u, None)
    tab.refused(BAD_ARGUMENT, "acc must be 16-byte aligned", "add_mul_assign_dev", h, d(0, odd=True), d(1), u, d(2), u, None)
    tab.refused(BAD_ARGUMENT, "a must be 16-byte aligned", "add_mul_assign_dev", h, d(0), d(1, odd=True), u, d(2), u, None)
    tab.refused(BAD_ARGUMENT, "b must be 16-byte aligned", "add_mul_assign_dev", h, d(0), d(1), u, d(2, odd=True), u, None)
    tab.refused(BAD_ARGUMENT, "a must be 16-byte aligned", "add_mul_assign_dev", h, d(0), d(1, odd=True), u + 1, d(2), u, None)
    if tab.h.has_mul_to:
        tab.refused(BAD_ARGUMENT, "out must be 16-byte aligned", "mul_to_dev", h, d(0), u, d(1), u, d(2, odd=True), None)
        tab.refused(BAD_ARGUMENT, "a must be 16-byte aligned", "mul_to_dev", h, d(0, odd=True), u, d(1), u, d(2), None)
        tab.refused(BAD_ARGUMENT, "b must be 16-byte aligned", "mul_to_dev", h, d(0), u, d(1, odd=True), u, d(2), None)
        tab.refused(BAD_ARGUMENT, "c must be 16-byte aligned", "mul_add_to_dev", h, d(0), u, d(1), u, d(2, odd=True), d(3), None)
        tab.refused(BAD_ARGUMENT, "out must be 16-byte aligned", "mul_add_to_dev", h, d(0), u, d(1), u, d(2, odd=True),
                    d(3, odd=True), None)


def test_length_not_a_multiple_of_the_unit(tab):
    h, u, d, hp = tab.handle, tab.unit, tab.dev, tab.hostp()
    for e in SLICES:
        tab.refused(BAD_LENGTH, T_SLICE, e, h, hp, u + 1)
        tab.refused(BAD_LENGTH, T_SLICE, e, h, hp, u - 1)
    for e in ("transform_dev", "inverse_transform_dev"):
        tab.refused(BAD_LENGTH, T_SLICE, e, h, d(0), u + 4, 0, None)
        tab.refused(BAD_LENGTH, T_SLICE, e, h, d(0), 1, 1, None)
    tab.refused(BAD_LENGTH, T_SLICE, "mul_assign_dev", h, d(0), u + 4, d(1), u + 4, None)
    tab.refused(BAD_LENGTH, T_SLICE, "mul_assign_dev", h, d(0), u + 4, d(1), 3, None)  # before the multiplicand length
    tab.refused(BAD_LENGTH, T_SLICE, "add_mul_assign_dev", h, d(0), d(1), u + 4, d(2), u, None)
    if tab.h.has_mul_to:
        tab.refused(BAD_LENGTH, T_SLICE, "mul_to_dev", h, d(0), u + 4, d(1), u, d(2), None)
        tab.refused(BAD_LENGTH, T_SLICE, "mul_add_to_dev", h, d(0), u + 4, d(1), 3, d(2), d(3), None)


def test_multiplicand_length(tab):
    h, u, d = tab.handle, tab.unit, tab.dev
    tab.refused(BAD_LENGTH, T_MULTIPLICAND, "mul_assign_dev", h, d(0), 2 * u, d(1), u + 4, None)
    tab.refused(BAD_LENGTH, T_MULTIPLICAND, "mul_assign_dev", h, d(0), 2 * u, d(1), 0, None)
    tab.refused(BAD_LENGTH, T_MULTIPLICAND, "mul_assign_dev", h, d(0), u, d(1), 2 * u, None)
    tab.refused(BAD_LENGTH, T_MULTIPLICAND, "mul_assign_dev", h, None, 0, None, 2 * u, None)  # checked at length 0 too
    tab.refused(BAD_LENGTH, T_MULTIPLICAND, "add_mul_assign_dev", h, d(0), d(1), 2 * u, d(2), u - 1, None)
    if tab.h.has_mul_to:
        tab.refused(BAD_LENGTH, T_MULTIPLICAND, "mul_to_dev", h, d(0), 2 * u, d(1), u + 4, d(2), None)
        tab.refused(BAD_LENGTH, T_MULTIPLICAND, "mul_add_to_dev", h, d(0), u, d(1), 2 * u, d(2), d(3), None)


def test_monomial(tab):
    h, u, hp = tab.handle, tab.unit, tab.hostp()
    q = min(tab.h.moduli)  # reduced modulo the other limbs, not this one
    tab.refused(BAD_LENGTH, T_MONOMIAL_LEN, "transform_monomial", h, 1, 0, hp, u + 1)
    tab.refused(BAD_LENGTH, T_MONOMIAL_LEN, "transform_monomial", h, 1, 0, hp, 2 * u)
    tab.refused(BAD_LENGTH, T_MONOMIAL_LEN, "transform_monomial", h, 1, 0, hp, 0)
    tab.refused(BAD_LENGTH, T_MONOMIAL_LEN, "transform_monomial", h, q, 0, hp, u + 1)  # before the coefficient
    tab.refused(BAD_LENGTH, T_MONOMIAL_LEN, "transform_coeff_one_monomial", h, 0, hp, 2 * u)
    tab.refused(BAD_LENGTH, T_MONOMIAL_LEN, "transform_coeff_minus_one_monomial", h, 0, hp, u - 1)
    tab.refused(BAD_ARGUMENT, T_MONOMIAL_COEFF, "transform_monomial", h, q, 0, hp, u)
    tab.refused(BAD_ARGUMENT, T_MONOMIAL_COEFF, "transform_monomial", h, max(tab.h.moduli), 3, hp, u)
    # the valid forms, against each other: -X^d is (q_i - 1) X^d on every limb
    n = 1 << LOG_N
    one, minus = np.zeros(u, tab.h.dtype), np.zeros(u, tab.h.dtype)
    assert tab.f("transform_coeff_one_monomial")(h, 3, one.ctypes.data_as(C.c_void_p), u) == OK
    assert tab.f("transform_coeff_minus_one_monomial")(h, 3, minus.ctypes.data_as(C.c_void_p), u) == OK
    for i, qi in enumerate(tab.h.moduli):
        a, b = one[i * n:(i + 1) * n].astype(object), minus[i * n:(i + 1) * n].astype(object)
        assert all(x != 0 for x in a) and all((x + y) % qi == 0 for x, y in zip(a, b))


def test_zero_length_calls_are_ok(tab):
    h = tab.handle
    for e in SLICES:
        assert tab.f(e)(h, None, 0) == OK
        assert tab.f(e)(h, tab.hostp(), 0) == OK
    for e in ("transform_dev", "inverse_transform_dev"):
        assert tab.f(e)(h, None, 0, 0, None) == OK
        assert tab.f(e)(h, tab.dev(0), 0, 1, None) == OK
    assert tab.f("mul_assign_dev")(h, None, 0, None, 0, None) == OK
    assert tab.f("mul_assign_dev")(h, tab.dev(0), 0, tab.dev(1), tab.unit, None) == OK
    assert tab.f("add_mul_assign_dev")(h, None, None, 0, None, 0, None) == OK
    if tab.h.has_mul_to:
        assert tab.f("mul_to_dev")(h, None, 0, None, 0, None, None) == OK
        assert tab.f("mul_add_to_dev")(h, None, 0, None, 0, None, None, None) == OK
    import torch
    torch.cuda.synchronize()


def test_getters(tab):
    h = tab.handle
    assert tab.f("poly_length")(h) == 1 << LOG_N
    assert tab.f("device")(h) == 0
    if tab.h.single:
        assert tab.f("log_n")(h) == LOG_N and tab.f("modulus")(h) == tab.h.moduli[0]
        assert tab.f("log_n")(None) == 0 and tab.f("modulus")(None) == 0 and tab.f("root")(None) == 0
        assert tab.f("inv_root")(None) == 0 and tab.f("inv_n")(None) == 0
        q, n = tab.h.moduli[0], 1 << LOG_N
        assert tab.f("root")(h) * tab.f("inv_root")(h) % q == 1 and tab.f("inv_n")(h) * n % q == 1
    else:
        L = len(tab.h.moduli)
        assert tab.f("moduli_count")(h) == L and tab.f("crt_poly_length")(h) == tab.unit
        assert [tab.f("modulus")(h, i) for i in range(L)] == list(tab.h.moduli)
        assert tab.f("modulus")(h, L) == 0 and tab.f("root")(h, L) == 0  # past the last limb
        assert tab.f("moduli_count")(None) == 0 and tab.f("crt_poly_length")(None) == 0
        assert tab.f("modulus")(None, 0) == 0 and tab.f("root")(None, 0) == 0
