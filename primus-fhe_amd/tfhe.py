"""Torus FFT tables and the TFHE external product — host-side mirror of primus_fft / primus_lattice::tfhe.

Reference: FullComplex64FftTable (primus_fft/src/complex64/table.rs:47-130) behind the FftTable trait (table.rs),
TorusFftValue (torus.rs:32-58), ApproxSignedBasis<T> with a power-of-two modulus (primus_decompose/src/primitive/basis.rs),
TfheFftContext (primus_lattice/src/context/tfhe.rs), external_product_to (tfhe/external_product.rs:36-93) and the
write_fourier_form conversions of GLWE / GLev / GGSW (tfhe/convert.rs).

Layouts are the reference's: a torus polynomial is N words (uint32 or uint64), a Fourier polynomial N complex values
(fourier_length == poly_length), a GLWE (k+1) polynomials, a Fourier GGSW (k+1) x ell x (k+1) Fourier polynomials.  Fourier
values are complex128 arrays, or the interleaved float64 view of one (re, im, re, im, ...).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import PfheError, check, lib
from .ntt import _stream

_WORD = {np.dtype(np.uint64): "", np.dtype(np.uint32): "32"}


def _host_words(a: np.ndarray):
    if not isinstance(a, np.ndarray) or a.dtype not in _WORD or not a.flags.c_contiguous:
        raise TypeError("expected a C-contiguous numpy uint32 or uint64 array")
    return a.ctypes.data_as(C.c_void_p), a.size, _WORD[a.dtype]


def _host_fourier(a: np.ndarray):
    """(pointer, complex count) of a complex128 array or its interleaved float64 view"""
    if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
        raise TypeError("expected a C-contiguous numpy complex128 / float64 array")
    if a.dtype == np.complex128:
        return a.ctypes.data_as(C.POINTER(C.c_double)), a.size
    if a.dtype == np.float64 and a.size % 2 == 0:
        return a.ctypes.data_as(C.POINTER(C.c_double)), a.size // 2
    raise TypeError("expected complex128 values or an interleaved float64 view")


def _dev_words(t, suffix=None):
    """(pointer, words, suffix) of a contiguous CUDA tensor of 32-bit (u32 torus) or 64-bit (u64 torus) elements"""
    if isinstance(t, tuple):
        ptr, words, sfx = t
        return C.c_void_p(int(ptr)), int(words), sfx
    if not hasattr(t, "data_ptr") or not t.is_cuda or not t.is_contiguous() or t.element_size() not in (4, 8) \
            or t.is_floating_point() or t.is_complex():
        raise TypeError("expected a contiguous 32- or 64-bit integer CUDA tensor")
    return C.c_void_p(t.data_ptr()), t.numel(), "32" if t.element_size() == 4 else ""


def _dev_fourier(t):
    """(pointer, complex count) of a contiguous complex128 or float64 (interleaved) CUDA tensor"""
    import torch
    if isinstance(t, tuple):
        return C.cast(C.c_void_p(int(t[0])), C.POINTER(C.c_double)), int(t[1])
    if not t.is_cuda or not t.is_contiguous() or t.dtype not in (torch.complex128, torch.float64):
        raise TypeError("expected a contiguous complex128 or float64 CUDA tensor")
    n = t.numel() if t.dtype == torch.complex128 else t.numel() // 2
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double)), n


def _dev_exps(t):
    """(pointer, count) of a contiguous int32 / uint32 CUDA tensor of exponents, or a (ptr, count) tuple"""
    if isinstance(t, tuple):
        return C.c_void_p(int(t[0])), int(t[1])
    if not hasattr(t, "data_ptr") or not t.is_cuda or not t.is_contiguous() or t.element_size() != 4 \
            or t.is_floating_point():
        raise TypeError("expected a contiguous int32 / uint32 CUDA tensor of exponents")
    return C.c_void_p(t.data_ptr()), t.numel()


def _host_exps(exps):
    """(pointer, count) of the exponents of a host form"""
    if not isinstance(exps, np.ndarray) or exps.dtype != np.uint32 or not exps.flags.c_contiguous:
        raise TypeError("expected a C-contiguous numpy uint32 array of exponents")
    return exps.ctypes.data_as(C.c_void_p), exps.size


def _same_width(message: str, *widths) -> str:
    """the one width suffix of all the word arrays of a call (and of its context), or TypeError(message)"""
    if len(set(widths)) != 1:
        raise TypeError(message)
    return widths[0]


class FullComplex64FftTable:
    """primus_fft::FullComplex64FftTable — negacyclic torus FFT of N = 2^log_n (1 <= log_n <= 14), u32 and u64 words."""

    def __init__(self, log_n: int, device: int = 0):
        h = C.c_void_p()
        check(lib().pfhe_fft_create(log_n, device, C.byref(h)))
        self._h, self.log_n, self.device = h, log_n, device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().pfhe_fft_destroy(h)
            self._h = None

    def poly_length(self) -> int:
        return int(lib().pfhe_fft_poly_length(self._h))

    def fourier_length(self) -> int:
        return int(lib().pfhe_fft_fourier_length(self._h))

    # ---- host slices (FftTable::forward_torus_slice / inverse_torus_slice, over one or more polynomials) ----
    def forward_torus_slice(self, inp: np.ndarray, out: np.ndarray) -> None:
        pi, ni, w = _host_words(inp)
        po, no = _host_fourier(out)
        check(getattr(lib(), "pfhe_fft_forward_torus" + w + "_slice")(self._h, pi, ni, po, no))

    def inverse_torus_slice(self, inp: np.ndarray, out: np.ndarray) -> None:
        pi, ni = _host_fourier(inp)
        po, no, w = _host_words(out)
        check(getattr(lib(), "pfhe_fft_inverse_torus" + w + "_slice")(self._h, pi, ni, po, no))

    # ---- device tensors: int32 / uint32 words select the u32 torus, int64 / uint64 the u64 torus ----
    def forward_torus_dev(self, inp, out, stream=None) -> None:
        pi, ni, w = _dev_words(inp)
        po, no = _dev_fourier(out)
        check(getattr(lib(), "pfhe_fft_forward_torus" + w + "_dev")(self._h, pi, ni, po, no, _stream(stream)))

    def inverse_torus_dev(self, inp, out, stream=None) -> None:
        pi, ni = _dev_fourier(inp)
        po, no, w = _dev_words(out)
        check(getattr(lib(), "pfhe_fft_inverse_torus" + w + "_dev")(self._h, pi, ni, po, no, _stream(stream)))

    def mul_monomial_each_to_dev(self, a, exps, out, polys_per_exp: int = 1, stream=None) -> None:
        """out = X^{exps[e]} * element e for elements of `polys_per_exp` torus polynomials each (exponents modulo 2N): the
        per-ciphertext X^{-b_e} * TV that starts a bootstrap.  out must not overlap a."""
        pa, na, wa = _dev_words(a)
        po, no, wo = _dev_words(out)
        pe, _ne = _dev_exps(exps)
        if wa != wo or na != no:
            raise TypeError("a and out must have the same width and length")
        check(getattr(lib(), "pfhe_tfhe" + wa + "_mul_monomial_each_to_dev")(self._h, pa, na, pe, polys_per_exp, po,
                                                                              _stream(stream)))


class ApproxSignedBasis:
    """primus_decompose::ApproxSignedBasis<T> with modulus None (2^BITS): a host-side value object.  `bits` is 32 or 64
    (the torus word); reverse_length limits the number of levels (basis.rs:47-177).  The reference's assert!s raise
    PfheError BadArgument here."""

    def __init__(self, bits: int, log_basis: int, reverse_length: int | None = None):
        if bits not in (32, 64):
            raise PfheError(33, "bits must be 32 or 64")
        if not 0 < log_basis < bits:
            raise PfheError(33, "log_basis must be in 1..BITS-1")
        full = bits // log_basis
        if reverse_length is not None and not 0 < reverse_length <= full:
            raise PfheError(33, "reverse_length must be in 1..BITS/log_basis")
        self.bits, self._log_basis = bits, log_basis
        self._length = full if reverse_length is None else reverse_length

    def log_basis(self) -> int:
        return self._log_basis

    def decompose_length(self) -> int:
        return self._length

    def drop_bits(self) -> int:
        return self.bits - self._length * self._log_basis


class _TorusContext:
    """What the four torus contexts share: the C handle, released with the object, and the sizes that follow from the table,
    the basis and the GLWE dimension.  Every create starts with (table, glwe_dimension, log_basis, decompose_length) and
    ends with the handle (`lead`: what a create takes between the dimension and the basis); `prefix` is what the context's calls start with, `calls` what its create, destroy, in-use and
    scratch calls are named behind it."""

    def _open(self, fft, basis, glwe_dimension, prefix, args, calls=("create", "destroy", "in_use", "scratch_bytes"), lead=(),
              family=None):
        self._w = "" if basis.bits == 64 else "32"
        # family: a handle whose entry points have a prefix of their own, family + width, instead of pfhe_tfhe{,32}_<prefix>
        self._pre = family + self._w if family else "pfhe_tfhe" + self._w + "_" + prefix
        self._destroy, self._in_use, self._scratch = calls[1:]
        h = C.c_void_p()
        check(getattr(lib(), self._pre + calls[0])(fft._h, glwe_dimension, *lead, basis.log_basis(), basis.decompose_length(),
                                                   *args, C.byref(h)))
        self._h = h
        self.fft, self.basis, self.glwe_dimension = fft, basis, glwe_dimension

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            getattr(lib(), self._pre + self._destroy)(h)
            self._h = None

    def dtype(self):
        return np.uint64 if self.basis.bits == 64 else np.uint32

    def scratch_bytes(self) -> int:
        return int(getattr(lib(), self._pre + self._scratch)(self._h))

    def in_use(self) -> bool:
        return bool(getattr(lib(), self._pre + self._in_use)(self._h))

    def glwe_len(self) -> int:
        return (self.glwe_dimension + 1) * self.fft.poly_length()

    def key_len(self) -> int:
        """complex values of one Fourier GGSW key (one step of a rotation)"""
        return (self.glwe_dimension + 1) * self.basis.decompose_length() * self.glwe_len()


class TfheFftContext(_TorusContext):
    """TfheFftContext<T> bundled with its basis and table (context/tfhe.rs): owns the device scratch of the product.  One
    holder at a time: a call from a second thread while one is inside raises PfheError (Busy)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int = 1, chunk: int = 0):
        self._open(fft, basis, glwe_dimension, "", (chunk,), ("plan_create", "plan_destroy", "plan_in_use", "plan_scratch_bytes"))


def tfhe_external_product_to(inp: np.ndarray, key: np.ndarray, out: np.ndarray, ctx: TfheFftContext) -> None:
    """external_product_to (tfhe/external_product.rs:36-93) on host arrays: out = inp (x) key for a batch of GLWE
    ciphertexts (batch*(k+1)*N words of the context's width) and one Fourier GGSW key."""
    pi, ni, wi = _host_words(inp)
    po, no, wo = _host_words(out)
    pk, nk = _host_fourier(key)
    _same_width("input / output words must match the basis width", wi, wo, ctx._w)
    check(getattr(lib(), ctx._pre + "external_product_to")(ctx._h, pi, ni, pk, nk, po, no))


def tfhe_external_product_to_dev(inp, key, out, ctx: TfheFftContext, stream=None) -> None:
    """the device form: inp / out 32- or 64-bit integer CUDA tensors (the context's width), key complex128 or float64"""
    pi, ni, wi = _dev_words(inp)
    po, no, wo = _dev_words(out)
    pk, nk = _dev_fourier(key)
    _same_width("input / output words must match the basis width", wi, wo, ctx._w)
    check(getattr(lib(), ctx._pre + "external_product_to_dev")(ctx._h, pi, ni, pk, nk, po, no, _stream(stream)))


class TfheBlindRotateContext(_TorusContext):
    """Handle of the batched blind rotation over the TFHE product (include/pfhe.h, pfhe_tfhe{,32}_blindrot_*): for every
    step i and ciphertext e, ACC_e += external_product_to(X^{exps[e*n_steps+i]} * ACC_e - ACC_e, BSK_i) on torus words.
    Owns a product plan and whatever glue buffers its form needs for `chunk` ciphertexts (0 = the default); one holder at
    a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int = 1, chunk: int = 0):
        self._open(fft, basis, glwe_dimension, "blindrot_", (chunk,))


def tfhe_blind_rotate(acc: np.ndarray, bsk: np.ndarray, exps: np.ndarray, ctx: TfheBlindRotateContext) -> None:
    """Batched blind rotation on host arrays, acc updated in place.  acc: batch GLWE ciphertexts of the context's width;
    bsk: n_steps Fourier GGSW keys end to end; exps: uint32, batch x n_steps, ciphertext-major, every exponent below 2N."""
    pa, na, wa = _host_words(acc)
    pk, nk = _host_fourier(bsk)
    _same_width("accumulator words must match the basis width", wa, ctx._w)
    pe, ne = _host_exps(exps)
    check(getattr(lib(), ctx._pre + "rotate")(ctx._h, pa, na, pk, nk, pe, ne))


def tfhe_blind_rotate_dev(acc, bsk, exps, ctx: TfheBlindRotateContext, stream=None) -> None:
    """the device form (acc a 32- or 64-bit integer CUDA tensor of the context's width, bsk complex128 or float64, exps
    int32 / uint32), asynchronous; every exponent is taken modulo 2N on the device"""
    pa, na, wa = _dev_words(acc)
    pk, nk = _dev_fourier(bsk)
    pe, ne = _dev_exps(exps)
    _same_width("accumulator words must match the basis width", wa, ctx._w)
    check(getattr(lib(), ctx._pre + "rotate_dev")(ctx._h, pa, na, pk, nk, pe, ne, _stream(stream)))


class TfheMultiBitBlindRotateContext(_TorusContext):
    """Handle of the multi-bit blind rotation (include/pfhe.h, pfhe_tfhe{,32}_mbrot_*): the mask is consumed
    `grouping_factor` (1..4) elements at a time; for every group t and ciphertext e,
    ACC_e = external_product_to(ACC_e, sum_j X^{r_j} * BSK[t][j]) with r_j the subset sum of the group's exponents at the set
    bits of j.  Assumes binary LWE keys: key [t][j] encrypts the indicator that the key bits of group t equal pattern j.
    Owns the scratch of its form for `chunk` ciphertexts (0 = the default); one holder at a time (Busy for a second
    thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, grouping_factor: int, glwe_dimension: int = 1,
                 chunk: int = 0):
        self._open(fft, basis, glwe_dimension, "mbrot_", (grouping_factor, chunk))
        self.grouping_factor = grouping_factor


    def group_len(self) -> int:
        """complex values of the 2^g keys of one group"""
        return self.key_len() << self.grouping_factor


def tfhe_multibit_blind_rotate(acc: np.ndarray, bsk: np.ndarray, exps: np.ndarray, ctx: TfheMultiBitBlindRotateContext) -> None:
    """Multi-bit blind rotation on host arrays, acc updated in place.  acc: batch GLWE ciphertexts of the context's width;
    bsk: groups x 2^g Fourier GGSW keys end to end; exps: uint32, batch x groups*g, ciphertext-major, every exponent below
    2N."""
    pa, na, wa = _host_words(acc)
    pk, nk = _host_fourier(bsk)
    _same_width("accumulator words must match the basis width", wa, ctx._w)
    pe, ne = _host_exps(exps)
    check(getattr(lib(), ctx._pre + "rotate")(ctx._h, pa, na, pk, nk, pe, ne))


def tfhe_multibit_blind_rotate_dev(acc, bsk, exps, ctx: TfheMultiBitBlindRotateContext, stream=None) -> None:
    """the device form, asynchronous; every exponent is taken modulo 2N on the device"""
    pa, na, wa = _dev_words(acc)
    pk, nk = _dev_fourier(bsk)
    pe, ne = _dev_exps(exps)
    _same_width("accumulator words must match the basis width", wa, ctx._w)
    check(getattr(lib(), ctx._pre + "rotate_dev")(ctx._h, pa, na, pk, nk, pe, ne, _stream(stream)))


def tfhe_multibit_combine_key_dev(keys, exps, out, fft: FullComplex64FftTable, decompose_length: int, grouping_factor: int,
                                  glwe_dimension: int = 1, stream=None) -> None:
    """The combined key of one ciphertext and one group as a key in the reference's layout: keys the group's 2^g Fourier
    GGSW keys, exps its g exponents, out one key that tfhe_external_product_to_dev takes; the rotation equals this call
    followed by the product, word for word."""
    pk, nk = _dev_fourier(keys)
    pe, ne = _dev_exps(exps)
    po, no = _dev_fourier(out)
    check(lib().pfhe_tfhe_mb_combine_key_dev(fft._h, glwe_dimension, decompose_length, grouping_factor, pk, nk, pe, ne, po, no,
                                             _stream(stream)))


# ---- the programmable bootstrap around the rotation (include/pfhe.h: modswitch, sample_extract, keyswitch, bootstrap) ----

def _dev_index(t, device) -> int:
    if device is not None:
        return int(device)
    return int(t.device.index or 0) if hasattr(t, "device") else 0


def _stateless(name, dev, arrays, message, args, stream=None) -> None:
    """One stateless step in its host (dev false) or device form.  `arrays`: numpy arrays or CUDA tensors of one word width w
    (TypeError(message) otherwise); args(w, (pointer, words) per array) gives the C arguments, and the device form takes
    the stream after them."""
    words = [(_dev_words if dev else _host_words)(a) for a in arrays]
    w = _same_width(message, *(x[2] for x in words))
    tail = (_stream(stream),) if dev else ()
    check(getattr(lib(), "pfhe_tfhe" + w + name + ("_dev" if dev else ""))(*args(w, *(x[:2] for x in words)), *tail))


def lwe_modulus_switch_dev(lwe, lwe_dimension: int, log_n: int, exps, neg_b, device=None, stream=None) -> None:
    """The project's own modulus switch (the reference has none): for a batch of LWE ciphertexts (a[0..n), b) of 32- or
    64-bit torus words, exps[e*n + i] = sw(a_{e,i}) and neg_b[e] = (2N - sw(b_e)) mod 2N, with
    sw(w) = (((w >> (shift-1)) + 1) >> 1) & (2N-1), shift = BITS - log_n - 1 (round to nearest, ties up).  exps is what
    tfhe_blind_rotate_dev takes; neg_b the exponents of the accumulator's X^{-b} * TV."""
    pl, nl, w = _dev_words(lwe)
    pe, ne = _dev_exps(exps)
    pb, nb = _dev_exps(neg_b)
    check(getattr(lib(), "pfhe_tfhe" + w + "_modswitch_dev")(_dev_index(lwe, device), pl, nl, lwe_dimension, log_n, pe, ne,
                                                            pb, nb, _stream(stream)))


def lwe_modulus_switch_strided_dev(lwe, lwe_dimension: int, log_n: int, log_stride: int, exps, neg_b, device=None,
                                   stream=None) -> None:
    """The modulus switch to multiples of 2^log_stride (0 <= log_stride <= log_n), what a many-LUT rotation takes:
    exps[e*n + i] = sw_v(a_{e,i}) and neg_b[e] = (2N - sw_v(b_e)) mod 2N with
    sw_v(w) = ((((w >> (BITS - log_n - 2 + v)) + 1) >> 1) << v) & (2N-1): w * 2N / 2^v / 2^BITS rounded to nearest, ties up,
    times 2^v; a word that rounds up to 2N wraps to 0.  log_stride 0 is lwe_modulus_switch_dev, word for word."""
    pl, nl, w = _dev_words(lwe)
    pe, ne = _dev_exps(exps)
    pb, nb = _dev_exps(neg_b)
    check(getattr(lib(), "pfhe_tfhe" + w + "_modswitch_stride_dev")(_dev_index(lwe, device), pl, nl, lwe_dimension, log_n,
                                                                   log_stride, pe, ne, pb, nb, _stream(stream)))


def tfhe_many_lut_test_vector(tvs):
    """The test vector of a many-LUT bootstrap from 2^v ordinary ones: tvs is a (2^v, ..., N) torch tensor (or a sequence of
    2^v tensors of one shape) of test vectors, polynomial coefficients last, and TV[c] = tvs[c mod 2^v][c - (c mod 2^v)]
    for every polynomial.  The strided switch makes the rotated phase p a multiple of 2^v, so coefficient i < 2^v of
    ACC = X^{-p} * TV is TV[p + i] = tvs[i][p] for p < N and -TV[p - N + i] = -tvs[i][p - N] otherwise: output i of the
    bootstrap is what an ordinary bootstrap with tvs[i] gives at the stride-rounded phase, with one sign for all i."""
    import torch
    t = torch.stack(list(tvs)) if not hasattr(tvs, "shape") else tvs
    luts, n = t.shape[0], t.shape[-1]
    if luts == 0 or luts & (luts - 1) or n % luts:
        raise ValueError("expected 2^v test vectors of N coefficients, 2^v dividing N")
    c = torch.arange(n, device=t.device)
    low = c % luts
    return t[low, ..., c - low].movedim(0, -1).contiguous()


def _sample_extract(dev, glwe, lwe, fft, glwe_dimension, index, stream=None) -> None:
    _stateless("_sample_extract", dev, (glwe, lwe), "glwe and lwe must have the same word width",
               lambda w, g, o: (fft._h, glwe_dimension, *g, index, *o), stream)


def glwe_sample_extract(glwe: np.ndarray, lwe: np.ndarray, fft: FullComplex64FftTable, glwe_dimension: int = 1,
                        index: int = 0) -> None:
    """Rlwe::extract_lwe_with_index (rlwe/coeff.rs:194-227) per mask polynomial, on host arrays: batch GLWE ciphertexts of
    (k+1)*N words -> batch LWE ciphertexts of k*N + 1 words under the GLWE key polynomials end to end."""
    _sample_extract(False, glwe, lwe, fft, glwe_dimension, index)


def glwe_sample_extract_dev(glwe, lwe, fft: FullComplex64FftTable, glwe_dimension: int = 1, index: int = 0,
                            stream=None) -> None:
    """the device form; lwe must not overlap glwe"""
    _sample_extract(True, glwe, lwe, fft, glwe_dimension, index, stream)


def _basis_args(basis, width: str):
    if (basis.bits == 64) != (width == ""):
        raise TypeError("the basis width must match the torus words")
    return basis.log_basis(), basis.decompose_length()


def _keyswitch(dev, lwe_in, ksk, lwe_out, in_dimension, out_dimension, basis, device, stream=None) -> None:
    _stateless("_keyswitch", dev, (lwe_in, ksk, lwe_out), "lwe_in, ksk and lwe_out must have the same word width",
               lambda w, i, k, o: (_dev_index(lwe_in, device) if dev else device, *i, in_dimension, *k, out_dimension,
                                   *_basis_args(basis, w), *o), stream)


def lwe_keyswitch(lwe_in: np.ndarray, ksk: np.ndarray, lwe_out: np.ndarray, in_dimension: int, out_dimension: int,
                  basis: ApproxSignedBasis, device: int = 0) -> None:
    """LWE key switch on host arrays: out = (0, b) - sum_i sum_j d_{i,j} * KSK[i][j] modulo 2^BITS, d the signed digits of
    a_i under `basis`; ksk is in_dimension x ell x (out_dimension+1) words, row (i, j) an LWE ciphertext of
    s_i * 2^(drop_bits + j*log_basis) under the output key, levels least significant first."""
    _keyswitch(False, lwe_in, ksk, lwe_out, in_dimension, out_dimension, basis, device)


def lwe_keyswitch_dev(lwe_in, ksk, lwe_out, in_dimension: int, out_dimension: int, basis: ApproxSignedBasis, device=None,
                      stream=None) -> None:
    """the device form, asynchronous; lwe_out must not overlap an input and may be uninitialised"""
    _keyswitch(True, lwe_in, ksk, lwe_out, in_dimension, out_dimension, basis, device, stream)


# ---- the linear layer with clear weights (include/pfhe.h: pfhe_lwe{,32}_linear*) ----

def _linear_weights(dev, weights, w: str):
    """(pointer, count, entry suffix) of the weights: dtype int8 takes the i8 entry, the word's dtype (for a tensor, the
    integer dtype of the word's size) the word entry; anything else is a ValueError before the library is called"""
    if dev:
        import torch
        if not hasattr(weights, "data_ptr") or not weights.is_cuda or not weights.is_contiguous():
            raise TypeError("expected a contiguous CUDA tensor of weights")
        if weights.dtype == torch.int8:
            return C.c_void_p(weights.data_ptr()), weights.numel(), "_i8"
        if weights.is_floating_point() or weights.is_complex() or weights.dtype == torch.bool \
                or weights.element_size() != (4 if w == "32" else 8):
            raise ValueError("weights must be int8 or of the ciphertext words' dtype")
        return C.c_void_p(weights.data_ptr()), weights.numel(), ""
    if not isinstance(weights, np.ndarray) or not weights.flags.c_contiguous:
        raise TypeError("expected a C-contiguous numpy array of weights")
    if weights.dtype == np.int8:
        return weights.ctypes.data_as(C.c_void_p), weights.size, "_i8"
    if _WORD.get(weights.dtype) != w:
        raise ValueError("weights must be int8 or of the ciphertext words' dtype")
    return weights.ctypes.data_as(C.c_void_p), weights.size, ""


def _linear(dev, lwe_in, weights, bias, lwe_out, dimension, in_features, out_features, device, stream=None) -> None:
    words = _dev_words if dev else _host_words
    pi, ni, wi = words(lwe_in)
    po, no, wo = words(lwe_out)
    pb, nb, wb = words(bias) if bias is not None else (None, 0, wi)
    w = _same_width("lwe_in, bias and lwe_out must have the same word width", wi, wo, wb)
    pw, nw, entry = _linear_weights(dev, weights, w)
    tail = (_stream(stream),) if dev else ()
    check(getattr(lib(), "pfhe_lwe" + w + "_linear" + entry + ("_dev" if dev else ""))(
        _dev_index(lwe_in, device) if dev else device, pi, ni, dimension, pw, nw, in_features, out_features, pb, nb, po, no,
        *tail))


def lwe_linear(lwe_in: np.ndarray, weights: np.ndarray, bias, lwe_out: np.ndarray, dimension: int, in_features: int,
               out_features: int, device: int = 0) -> None:
    """A linear layer with clear integer weights on host arrays, modulo 2^BITS: lwe_in is batch x in_features ciphertexts of
    dimension + 1 words, weights out_features x in_features (row-major, shared by the batch), bias out_features torus words
    added to the bodies or None, and out[e][o] = sum_i weights[o][i] * in[e][i] + (0, bias[o]): out_features chains of
    Lwe::add_mul_scalar_assign (lwe/single_message.rs:262-268) per input vector.  Weights of dtype int8 run on the matrix
    cores and give the words of the sign-extended weights; weights of the words' dtype are the reference's scalars, a
    negative weight in two's complement.  Any other dtype is a ValueError."""
    _linear(False, lwe_in, weights, bias, lwe_out, dimension, in_features, out_features, device)


def lwe_linear_dev(lwe_in, weights, bias, lwe_out, dimension: int, in_features: int, out_features: int, device=None,
                   stream=None) -> None:
    """the device form, asynchronous; lwe_out must not overlap an input and may be uninitialised"""
    _linear(True, lwe_in, weights, bias, lwe_out, dimension, in_features, out_features, device, stream)


class TfheBootstrapContext(_TorusContext):
    """Handle of the batched programmable bootstrap (include/pfhe.h, pfhe_tfhe{,32}_bootstrap_*): modulus switch,
    ACC = X^{-b~} * TV, the blind rotation over lwe_dimension steps (grouping_factor above 1: the multi-bit rotation over
    lwe_dimension / grouping_factor groups, on the multi-bit key), sample extraction at index 0 and, when ks_basis is
    given, the key switch back to lwe_dimension.  log_luts = v above 0 (at most log N) is the many-LUT bootstrap: the
    modulus switch is lwe_modulus_switch_strided_dev with v, the accumulator is extracted at every index i < 2^v, and
    lwe_out holds batch * 2^v ciphertexts, output (e, i) at e * 2^v + i; tfhe_many_lut_test_vector builds its test vector.
    Owns a blind-rotation handle and every buffer between the stages for `chunk` ciphertexts (0 = the default); one holder
    at a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, lwe_dimension: int, glwe_dimension: int = 1,
                 ks_basis: ApproxSignedBasis | None = None, chunk: int = 0, grouping_factor: int = 1, log_luts: int = 0):
        if ks_basis is not None and ks_basis.bits != basis.bits:
            raise TypeError("both bases must have the width of the torus words")
        args = (lwe_dimension, ks_basis.log_basis() if ks_basis else 0, ks_basis.decompose_length() if ks_basis else 0,
                1 if ks_basis else 0)
        calls = ("_destroy", "_in_use", "_scratch_bytes")
        if log_luts:    # many-LUT: the switch to multiples of 2^log_luts and 2^log_luts outputs per input
            self._open(fft, basis, glwe_dimension, "bootstrap", args + (grouping_factor, log_luts, chunk),
                       ("_create_many_lut",) + calls)
        elif grouping_factor == 1:
            self._open(fft, basis, glwe_dimension, "bootstrap", args + (chunk,), ("_create",) + calls)
        else:   # the multi-bit rotation: bsk is (lwe_dimension / g) * 2^g keys
            self._open(fft, basis, glwe_dimension, "bootstrap", args + (grouping_factor, chunk), ("_create_multibit",) + calls)
        self.grouping_factor, self.ks_basis, self.lwe_dimension = grouping_factor, ks_basis, lwe_dimension
        self.log_luts = log_luts


    def bsk_len(self) -> int:
        """complex values of the whole bootstrapping key: lwe_dimension keys, or (lwe_dimension / g) * 2^g multi-bit keys"""
        g = self.grouping_factor
        return (self.lwe_dimension if g == 1 else (self.lwe_dimension // g) << g) * self.key_len()

    def extracted_dimension(self) -> int:
        return self.glwe_dimension * self.fft.poly_length()

    def ksk_len(self) -> int:
        """words of the key-switch key (0 without a key switch)"""
        if self.ks_basis is None:
            return 0
        return self.extracted_dimension() * self.ks_basis.decompose_length() * (self.lwe_dimension + 1)

    def out_len(self) -> int:
        """words of one output ciphertext"""
        return (self.lwe_dimension if self.ks_basis is not None else self.extracted_dimension()) + 1


def tfhe_bootstrap(lwe_in: np.ndarray, bsk: np.ndarray, tv: np.ndarray, ksk, lwe_out: np.ndarray,
                   ctx: TfheBootstrapContext) -> None:
    """Batched programmable bootstrap on host arrays.  lwe_in: batch x (n+1) words; bsk: n Fourier GGSW keys end to end;
    tv: one GLWE test vector ((k+1)*N words) or one per ciphertext; ksk: the key-switch key, None without a key switch;
    lwe_out: batch x ctx.out_len() words."""
    pi, ni, wi = _host_words(lwe_in)
    pk, nk = _host_fourier(bsk)
    pt, nt, wt = _host_words(tv)
    po, no, wo = _host_words(lwe_out)
    ps, ns, ws = _host_words(ksk) if ksk is not None else (None, 0, ctx._w)
    _same_width("every word array must have the width of the context's basis", wi, wt, wo, ws, ctx._w)
    check(getattr(lib(), ctx._pre)(ctx._h, pi, ni, pk, nk, pt, nt, ps, ns, po, no))


def tfhe_bootstrap_dev(lwe_in, bsk, tv, ksk, lwe_out, ctx: TfheBootstrapContext, stream=None) -> None:
    """the device form (32- or 64-bit integer CUDA tensors of the context's width, bsk complex128 or float64),
    asynchronous; lwe_out must not overlap an input"""
    pi, ni, wi = _dev_words(lwe_in)
    pk, nk = _dev_fourier(bsk)
    pt, nt, wt = _dev_words(tv)
    po, no, wo = _dev_words(lwe_out)
    ps, ns, ws = _dev_words(ksk) if ksk is not None else (None, 0, ctx._w)
    _same_width("every word tensor must have the width of the context's basis", wi, wt, wo, ws, ctx._w)
    check(getattr(lib(), ctx._pre + "_dev")(ctx._h, pi, ni, pk, nk, pt, nt, ps, ns, po, no, _stream(stream)))


def tfhe_dense_layer_dev(lwe_in, weights, bias, bsk, tv, ksk, lwe_out, ctx: TfheBootstrapContext, in_features: int,
                         out_features: int, stream=None) -> None:
    """A dense layer of encrypted inference as two public calls: lwe_linear_dev (the weighted sums of every input vector,
    with the bias) and tfhe_bootstrap_dev on the batch * out_features sums (the activation, as the test vector tv: one, or
    one per output ciphertext).  ctx is a bootstrap context with its key switch, so lwe_out (batch x out_features
    ciphertexts of lwe_dimension + 1 words) feeds the next layer.  Plain Python, not a handle: every call allocates the
    intermediate sums with torch on lwe_in's device; allocation and the current-stream semantics of torch apply, so pass the
    stream torch is on, or None on the default stream."""
    import torch
    if ctx.ks_basis is None:
        raise ValueError("a dense layer needs a bootstrap context with its key switch")
    row = ctx.lwe_dimension + 1
    if lwe_in.numel() % (in_features * row) != 0:
        raise ValueError("lwe_in must be batch x in_features x (lwe_dimension + 1) words")
    batch = lwe_in.numel() // (in_features * row)
    sums = torch.empty(batch * out_features * row, dtype=lwe_in.dtype, device=lwe_in.device)
    lwe_linear_dev(lwe_in, weights, bias, sums, ctx.lwe_dimension, in_features, out_features, stream=stream)
    tfhe_bootstrap_dev(sums, bsk, tv, ksk, lwe_out, ctx, stream)


def write_fourier_form(coeff, fourier, fft: FullComplex64FftTable, stream=None) -> None:
    """Glwe / Glev / Ggsw::write_fourier_form (tfhe/convert.rs): the Fourier containers are polynomial after polynomial,
    so each is one batched forward transform.  numpy arrays take the host form, CUDA tensors the device form."""
    if isinstance(coeff, np.ndarray):
        fft.forward_torus_slice(coeff, fourier)
    else:
        fft.forward_torus_dev(coeff, fourier, stream)


# ---- key generation, encryption and phase (include/pfhe.h: lwe_body_mac, glwe_body_mac, ggsw_add_gadget, bsk / ksk) ----
# No call below draws a random number: masks and noise are what the caller put into the buffers (tfhe_fill_rows_dev, at the
# end of this file, fills them from a ChaCha20 stream; torus_uniform and torus_noise are statistical fillers for tests).

def _lwe_body(dev, lwe, key, subtract: int, device, stream=None) -> None:
    _stateless("_lwe_body_mac", dev, (lwe, key), "ciphertexts and key must have the same word width",
               lambda w, l, k: (_dev_index(lwe, device) if dev else device, *l, k[1], *k, subtract), stream)


def lwe_encrypt(lwe: np.ndarray, key: np.ndarray, device: int = 0) -> None:
    """Lwe::generate_random_zero_sample (lwe/single_message.rs:94-125) with the caller's randomness, on host arrays and in
    place: lwe holds batch x (len(key)+1) words, masks uniform and body slots noise + message; b_e += <a_e, key>."""
    _lwe_body(False, lwe, key, 0, device)


def lwe_encrypt_dev(lwe, key, device=None, stream=None) -> None:
    """the device form, asynchronous"""
    _lwe_body(True, lwe, key, 0, device, stream)


def lwe_phase(lwe: np.ndarray, key: np.ndarray, device: int = 0) -> None:
    """b_e -= <a_e, key> in place: every body slot becomes the phase b - <a,s> = noise + message"""
    _lwe_body(False, lwe, key, 1, device)


def lwe_phase_dev(lwe, key, device=None, stream=None) -> None:
    """the device form, asynchronous"""
    _lwe_body(True, lwe, key, 1, device, stream)


def _glwe_body(dev, glwe, key, fft, glwe_dimension: int, subtract: int, stream=None) -> None:
    _stateless("_glwe_body_mac", dev, (glwe, key), "ciphertexts and key must have the same word width",
               lambda w, g, k: (fft._h, glwe_dimension, *g, *k, subtract), stream)


def glwe_encrypt(glwe: np.ndarray, key: np.ndarray, fft: FullComplex64FftTable, glwe_dimension: int = 1) -> None:
    """Rlwe::generate_random_zero_sample (rlwe/coeff.rs:92-121) with the caller's randomness, on host arrays and in place:
    glwe holds batch x (k+1) x N words, mask polynomials uniform and body polynomials noise + message; key the k key
    polynomials end to end; B_e += sum_j A_{e,j} * z_j modulo X^N + 1."""
    _glwe_body(False, glwe, key, fft, glwe_dimension, 0)


def glwe_encrypt_dev(glwe, key, fft: FullComplex64FftTable, glwe_dimension: int = 1, stream=None) -> None:
    """the device form, asynchronous"""
    _glwe_body(True, glwe, key, fft, glwe_dimension, 0, stream)


def glwe_phase(glwe: np.ndarray, key: np.ndarray, fft: FullComplex64FftTable, glwe_dimension: int = 1) -> None:
    """B_e -= sum_j A_{e,j} * z_j in place: every body polynomial becomes the phase"""
    _glwe_body(False, glwe, key, fft, glwe_dimension, 1)


def glwe_phase_dev(glwe, key, fft: FullComplex64FftTable, glwe_dimension: int = 1, stream=None) -> None:
    """the device form, asynchronous"""
    _glwe_body(True, glwe, key, fft, glwe_dimension, 1, stream)


def ggsw_add_gadget_dev(ggsw, messages, fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int = 1,
                        stream=None) -> None:
    """Adds m * 2^(drop_bits + l*log_basis) to coefficient 0 of component r of row (r, l) of every torus-form GGSW of the
    batch ((k+1) x ell x (k+1) x N words each), one message word per GGSW."""
    pg, ng, wg = _dev_words(ggsw)
    pm, nm, wm = _dev_words(messages)
    _same_width("GGSWs and messages must have the same word width", wg, wm)
    lb, ell = _basis_args(basis, wg)
    check(getattr(lib(), "pfhe_tfhe" + wg + "_ggsw_add_gadget_dev")(fft._h, glwe_dimension, lb, ell, pg, ng, pm, nm,
                                                                  _stream(stream)))


class TfheKeyShape:
    """The shape of a bootstrapping key without a handle: what tfhe_generate_bsk_dev reads from a TfheBootstrapContext.
    grouping_factor 0 is the classic layout (lwe_dimension keys), 1..4 the multi-bit one ((lwe_dimension / g) * 2^g keys)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, lwe_dimension: int, glwe_dimension: int = 1,
                 grouping_factor: int = 0):
        self.fft, self.basis, self.lwe_dimension = fft, basis, lwe_dimension
        self.glwe_dimension, self.grouping_factor = glwe_dimension, grouping_factor

    def keys(self) -> int:
        g = self.grouping_factor
        return (self.lwe_dimension // g) << g if g else self.lwe_dimension

    def bsk_len(self) -> int:
        """torus words of the whole key, and complex values of its Fourier form"""
        rows = self.glwe_dimension + 1
        return self.keys() * rows * self.basis.decompose_length() * rows * self.fft.poly_length()


def _key_shape(ctx_or_shape) -> TfheKeyShape:
    if isinstance(ctx_or_shape, TfheKeyShape):
        return ctx_or_shape
    c = ctx_or_shape    # a TfheBootstrapContext: grouping_factor 1 is its classic rotation
    return TfheKeyShape(c.fft, c.basis, c.lwe_dimension, c.glwe_dimension, 0 if c.grouping_factor == 1 else c.grouping_factor)


def tfhe_generate_bsk_dev(ctx_or_shape, lwe_key, glwe_key, rand, out=None, stream=None):
    """The bootstrapping key a TfheBootstrapContext (or a TfheKeyShape) takes, generated on the device.  lwe_key: the n key
    words; glwe_key: the k key polynomials end to end; rand: shape.bsk_len() torus words holding the randomness (masks
    uniform, bodies noise), which becomes the torus-form key in place; out: as many complex128 values (allocated when
    None), which becomes its Fourier form, bit for bit what write_fourier_form gives.  Returns out.  Asynchronous."""
    import torch
    sh = _key_shape(ctx_or_shape)
    ps, ns, ws = _dev_words(lwe_key)
    pz, nz, wz = _dev_words(glwe_key)
    pr, nr, wr = _dev_words(rand)
    _same_width("both keys and the randomness must have the same word width", ws, wz, wr)
    lb, ell = _basis_args(sh.basis, wr)
    if out is None:
        out = torch.empty(nr, dtype=torch.complex128, device=rand.device)
    po, no = _dev_fourier(out)
    check(getattr(lib(), "pfhe_tfhe" + wr + "_bsk_generate_dev")(sh.fft._h, sh.glwe_dimension, lb, ell, sh.grouping_factor, ps,
                                                               ns, pz, nz, pr, nr, po, no, _stream(stream)))
    return out


def tfhe_generate_ksk_dev(key_in, key_out, basis: ApproxSignedBasis, rand, device=None, stream=None) -> None:
    """The key-switch key lwe_keyswitch_dev takes, from key_in (len(key_in) words) to key_out, generated in place in rand:
    len(key_in) x ell rows of len(key_out)+1 words holding the randomness (masks uniform, bodies noise); row (i, j) becomes
    b += <a, key_out> + key_in[i] * 2^(drop_bits + j*log_basis).  Asynchronous."""
    pi, ni, wi = _dev_words(key_in)
    po, no, wo = _dev_words(key_out)
    pr, nr, wr = _dev_words(rand)
    _same_width("both keys and the randomness must have the same word width", wi, wo, wr)
    lb, ell = _basis_args(basis, wr)
    check(getattr(lib(), "pfhe_tfhe" + wr + "_ksk_generate_dev")(_dev_index(rand, device), pi, ni, po, no, lb, ell, pr, nr,
                                                               _stream(stream)))


# ---- packing: LWE ciphertexts back into a GLWE, and multi-message extraction (include/pfhe.h: pack_keyswitch, pksk_generate,
# sample_extract_first_few, multimsg_extract) ----

def _pack_keyswitch(dev, lwe_in, pksk, glwe_out, in_dimension, count, fft, basis, glwe_dimension, stream=None) -> None:
    _stateless("_pack_keyswitch", dev, (lwe_in, pksk, glwe_out), "lwe_in, pksk and glwe_out must have the same word width",
               lambda w, i, k, o: (fft._h, glwe_dimension, *i, in_dimension, count, *k, *_basis_args(basis, w), *o), stream)


def lwe_pack_keyswitch(lwe_in: np.ndarray, pksk: np.ndarray, glwe_out: np.ndarray, in_dimension: int, count: int,
                       fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int = 1) -> None:
    """Packing key switch on host arrays: every group of `count` LWE ciphertexts (in_dimension+1 words each) becomes one GLWE
    ciphertext whose message polynomial holds their messages in coefficients 0..count-1,
    out = (0, .., 0, sum_i b_i X^i) - sum_i X^i sum_j sum_l d_l(a_{i,j}) * pksk[j][l] modulo 2^BITS and X^N + 1, d the
    signed digits of `basis`; pksk is in_dimension x ell x (k+1) x N words, row (j, l) a GLWE ciphertext of
    s_j * 2^(drop_bits + l*log_basis) under the output key, levels least significant first.  1 <= count <= N."""
    _pack_keyswitch(False, lwe_in, pksk, glwe_out, in_dimension, count, fft, basis, glwe_dimension)


def lwe_pack_keyswitch_dev(lwe_in, pksk, glwe_out, in_dimension: int, count: int, fft: FullComplex64FftTable,
                           basis: ApproxSignedBasis, glwe_dimension: int = 1, stream=None) -> None:
    """the device form, asynchronous and stateless; glwe_out must not overlap an input and may be uninitialised"""
    _pack_keyswitch(True, lwe_in, pksk, glwe_out, in_dimension, count, fft, basis, glwe_dimension, stream)


def tfhe_generate_pksk_dev(key_in, glwe_key, fft: FullComplex64FftTable, basis: ApproxSignedBasis, rand,
                           glwe_dimension: int = 1, stream=None) -> None:
    """The packing key lwe_pack_keyswitch_dev takes, from key_in (len(key_in) words) to glwe_key (the k key polynomials end
    to end), generated in place in rand: len(key_in) x ell GLWE rows of (k+1)*N words holding the randomness (mask
    polynomials uniform, body polynomials noise); row (j, l) becomes B += sum_r A_r * z_r, and
    key_in[j] * 2^(drop_bits + l*log_basis) on coefficient 0.  A second call adds the body a second time.  Asynchronous."""
    pi, ni, wi = _dev_words(key_in)
    pz, nz, wz = _dev_words(glwe_key)
    pr, nr, wr = _dev_words(rand)
    _same_width("both keys and the randomness must have the same word width", wi, wz, wr)
    lb, ell = _basis_args(basis, wr)
    check(getattr(lib(), "pfhe_tfhe" + wr + "_pksk_generate_dev")(fft._h, glwe_dimension, pi, ni, pz, nz, lb, ell, pr, nr,
                                                                _stream(stream)))


class TfhePackFftContext(_TorusContext):
    """Handle of the packing key switch in the Fourier domain (include/pfhe.h, pfhe_tfhe{,32}_packfft_*): the rule of
    lwe_pack_keyswitch_dev computed as one external product of in_dimension * ell rows against the half-spectrum key of
    tfhe_pack_key_fourier_dev.  Approximate as the TFHE product is, cheaper than the exact call when count approaches N, and
    opt-in: 1 <= log N <= 11 and 1 <= glwe_dimension <= 3 (Unsupported otherwise; the exact call serves every shape).  Owns the
    partial sums of `chunk` groups (0 = the default); one holder at a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, in_dimension: int, glwe_dimension: int = 1,
                 chunk: int = 0):
        self._open(fft, basis, glwe_dimension, "packfft_", (chunk,),
                   ("plan_create", "plan_destroy", "plan_in_use", "plan_scratch_bytes"), lead=(in_dimension,))
        self.in_dimension = in_dimension

    @property
    def fkey_len(self) -> int:
        """complex values of the Fourier packing key: in_dimension x ell x (k+1) x N/2"""
        return self.in_dimension * self.basis.decompose_length() * self.glwe_len() // 2

    def pksk_len(self) -> int:
        """words of the torus packing key it is converted from"""
        return self.in_dimension * self.basis.decompose_length() * self.glwe_len()


def tfhe_pack_key_fourier_dev(pksk, fkey, ctx: TfhePackFftContext, stream=None) -> None:
    """The Fourier packing key of lwe_pack_keyswitch_fft_dev from the torus key tfhe_generate_pksk_dev wrote: the half
    spectrum of every key polynomial, ctx.fkey_len complex128 values (or their interleaved float64 view).  Asynchronous."""
    pk, nk, wk = _dev_words(pksk)
    pf, nf = _dev_fourier(fkey)
    _same_width("the packing key must have the width of the context's basis", wk, ctx._w)
    check(getattr(lib(), ctx._pre + "key_dev")(ctx._h, pk, nk, pf, nf, _stream(stream)))


def lwe_pack_keyswitch_fft(lwe_in: np.ndarray, fkey: np.ndarray, glwe_out: np.ndarray, count: int,
                           ctx: TfhePackFftContext) -> None:
    """lwe_pack_keyswitch through the Fourier domain, on host arrays: lwe_in and glwe_out as the exact call takes them, fkey
    the Fourier packing key (complex128, or the interleaved float64 view)."""
    pi, ni, wi = _host_words(lwe_in)
    pf, nf = _host_fourier(fkey)
    po, no, wo = _host_words(glwe_out)
    _same_width("lwe_in and glwe_out must have the width of the context's basis", wi, wo, ctx._w)
    check(getattr(lib(), "pfhe_tfhe" + ctx._w + "_pack_keyswitch_fft")(ctx._h, pi, ni, count, pf, nf, po, no))


def lwe_pack_keyswitch_fft_dev(lwe_in, fkey, glwe_out, count: int, ctx: TfhePackFftContext, stream=None) -> None:
    """the device form, asynchronous; glwe_out must not overlap an input and may be uninitialised"""
    pi, ni, wi = _dev_words(lwe_in)
    pf, nf = _dev_fourier(fkey)
    po, no, wo = _dev_words(glwe_out)
    _same_width("lwe_in and glwe_out must have the width of the context's basis", wi, wo, ctx._w)
    check(getattr(lib(), "pfhe_tfhe" + ctx._w + "_pack_keyswitch_fft_dev")(ctx._h, pi, ni, count, pf, nf, po, no,
                                                                          _stream(stream)))


def _extract_pair(name, src, dst, fft, count, glwe_dimension, dev, stream=None):
    _stateless(name, dev, (src, dst), "input and output must have the same word width",
               lambda w, a, b: (fft._h, glwe_dimension, *a, count, *b), stream)


def glwe_sample_extract_first_few(glwe: np.ndarray, out: np.ndarray, fft: FullComplex64FftTable, count: int,
                                  glwe_dimension: int = 1) -> None:
    """Rlwe::extract_first_few_lwe (rlwe/coeff.rs:231-260) per mask polynomial, on host arrays: batch GLWE ciphertexts of
    (k+1)*N words -> batch MultiMsgLwe layouts of k*N + count words, each mask polynomial as [a_0, -a_{N-1}, ..., -a_1],
    then b_0 .. b_{count-1}."""
    _extract_pair("_sample_extract_first_few", glwe, out, fft, count, glwe_dimension, False)


def glwe_sample_extract_first_few_dev(glwe, out, fft: FullComplex64FftTable, count: int, glwe_dimension: int = 1,
                                      stream=None) -> None:
    """the device form; out must not overlap glwe"""
    _extract_pair("_sample_extract_first_few", glwe, out, fft, count, glwe_dimension, True, stream)


def multimsg_lwe_extract(multi: np.ndarray, lwe_out: np.ndarray, fft: FullComplex64FftTable, count: int,
                         glwe_dimension: int = 1) -> None:
    """MultiMsgLwe::extract_rlwe_mode (lwe/multiple_message.rs:250-263) for every index h < count, on host arrays: batch
    layouts of k*N + count words -> batch x count LWE ciphertexts of k*N + 1 words; ciphertext h equals
    glwe_sample_extract(..., index=h) of the GLWE the layout came from."""
    _extract_pair("_multimsg_extract", multi, lwe_out, fft, count, glwe_dimension, False)


def multimsg_lwe_extract_dev(multi, lwe_out, fft: FullComplex64FftTable, count: int, glwe_dimension: int = 1,
                             stream=None) -> None:
    """the device form; lwe_out must not overlap multi"""
    _extract_pair("_multimsg_extract", multi, lwe_out, fft, count, glwe_dimension, True, stream)


# ---- the circuit bootstrap: an encrypted bit becomes a GGSW (include/pfhe.h: private_keyswitch, pfksk_generate, cbs) ----

def _private_keyswitch(dev, lwe_in, pfksk, out, in_dimension, levels, fft, basis, glwe_dimension, stream=None) -> None:
    _stateless("_private_keyswitch", dev, (lwe_in, pfksk, out), "lwe_in, pfksk and out must have the same word width",
               lambda w, i, k, o: (fft._h, glwe_dimension, *i, in_dimension, levels, *k, *_basis_args(basis, w), *o), stream)


def lwe_private_keyswitch(lwe_in: np.ndarray, pfksk: np.ndarray, out: np.ndarray, in_dimension: int, levels: int,
                          fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int = 1) -> None:
    """Private functional key switch on host arrays: batch x levels LWE ciphertexts (in_dimension+1 words, ciphertext (e, l)
    at e*levels + l) become batch GGSW-shaped blocks of (k+1) x levels x (k+1)*N words,
    out[e][u][l] = - sum_{j <= in_dimension} sum_t d_t(c_{e,l,j}) * pfksk[u][j][t] modulo 2^BITS, c = (a, b) with the body
    decomposed as one more mask word and d the signed digits of `basis`; pfksk is (k+1) x (in_dimension+1) x ell GLWE rows,
    row (u, j, t) an encryption of f_u(s'_j * 2^(drop_bits + t*log_basis)), s' = (s_in, -1), f_u(x) = -z_u*x for u < k and
    x on coefficient 0 for u = k: the phase of out[e][u][l] is f_u of the phase of input (e, l).  1 <= levels <= 64."""
    _private_keyswitch(False, lwe_in, pfksk, out, in_dimension, levels, fft, basis, glwe_dimension)


def lwe_private_keyswitch_dev(lwe_in, pfksk, out, in_dimension: int, levels: int, fft: FullComplex64FftTable,
                              basis: ApproxSignedBasis, glwe_dimension: int = 1, stream=None) -> None:
    """the device form, asynchronous and stateless; out must not overlap an input and may be uninitialised"""
    _private_keyswitch(True, lwe_in, pfksk, out, in_dimension, levels, fft, basis, glwe_dimension, stream)


def tfhe_generate_pfksk_dev(key_in, glwe_key, fft: FullComplex64FftTable, basis: ApproxSignedBasis, rand,
                            glwe_dimension: int = 1, stream=None) -> None:
    """The key lwe_private_keyswitch_dev takes, from key_in (len(key_in) words) to glwe_key (the k key polynomials end to
    end), generated in place in rand: (k+1) x (len(key_in)+1) x ell GLWE rows of (k+1)*N words holding the randomness (mask
    polynomials uniform, body polynomials noise).  Every row becomes B += sum_r A_r * z_r; then, with s' = (key_in, -1) and
    g_t = 2^(drop_bits + t*log_basis), row (k, j, t) gets s'_j*g_t on coefficient 0 of the body and row (u, j, t), u < k,
    gets -s'_j*g_t*z_u[i] on every body coefficient i.  A second call adds both a second time.  Asynchronous."""
    pi, ni, wi = _dev_words(key_in)
    pz, nz, wz = _dev_words(glwe_key)
    pr, nr, wr = _dev_words(rand)
    _same_width("both keys and the randomness must have the same word width", wi, wz, wr)
    lb, ell = _basis_args(basis, wr)
    check(getattr(lib(), "pfhe_tfhe" + wr + "_pfksk_generate_dev")(fft._h, glwe_dimension, pi, ni, pz, nz, lb, ell, pr, nr,
                                                                 _stream(stream)))


class TfheCircuitBootstrapContext(_TorusContext):
    """Handle of the batched circuit bootstrap (include/pfhe.h, pfhe_tfhe{,32}_cbs_*): an LWE ciphertext of a bit m encoded
    as m*2^(BITS-1) becomes a torus-form GGSW of m under the GLWE key, in `cbs_basis`.  Per input and level l of cbs_basis:
    the modulus switch of (a, b + 2^(BITS-2)), ACC = X^{-b~} * (0, .., 0, -g_l/2 on every coefficient), the blind rotation
    over lwe_dimension steps under `basis`, sample extraction at index 0 with g_l/2 added to the body, and the private
    functional key switch under `pfks_basis` with levels = cbs_basis.decompose_length().  cbs_basis must drop at least
    one bit.  grouping_factor above 1 runs the multi-bit rotation on the multi-bit key of tfhe_generate_bsk_dev.
    shared_rotation runs ONE rotation per input for all levels (many-LUT): with v = ceil(log2 ell_cb) the switch is
    lwe_modulus_switch_strided_dev with v, the test vector's body coefficient c is -g_{c mod 2^v}/2 (0 where the basis has no
    such level), and level l is extracted at index l; ell_cb must be at most N.  The switch then rounds every word to a
    multiple of 2^v: its worst-case margin shrinks by that factor.  Owns a blind-rotation handle and every
    buffer between the stages for `chunk` inputs (0 = the default); one holder at a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, lwe_dimension: int, glwe_dimension: int,
                 cbs_basis: ApproxSignedBasis, pfks_basis: ApproxSignedBasis, chunk: int = 0, grouping_factor: int = 1,
                 shared_rotation: bool = False):
        if cbs_basis.bits != basis.bits or pfks_basis.bits != basis.bits:
            raise TypeError("every basis must have the width of the torus words")
        args = (lwe_dimension, cbs_basis.log_basis(), cbs_basis.decompose_length(), pfks_basis.log_basis(),
                pfks_basis.decompose_length())
        calls = ("_destroy", "_in_use", "_scratch_bytes")
        if grouping_factor == 1 and not shared_rotation:
            self._open(fft, basis, glwe_dimension, "cbs", args + (chunk,), ("_create",) + calls)
        else:
            self._open(fft, basis, glwe_dimension, "cbs", args + (grouping_factor, 1 if shared_rotation else 0, chunk),
                       ("_create_with",) + calls)
        self.lwe_dimension, self.cbs_basis, self.pfks_basis = lwe_dimension, cbs_basis, pfks_basis
        self.grouping_factor, self.shared_rotation = grouping_factor, bool(shared_rotation)

    def bsk_len(self) -> int:
        """complex values of the bootstrapping key: lwe_dimension Fourier GGSW keys, or (lwe_dimension / g) * 2^g multi-bit keys"""
        g = self.grouping_factor
        return (self.lwe_dimension if g == 1 else (self.lwe_dimension // g) << g) * self.key_len()

    def extracted_dimension(self) -> int:
        return self.glwe_dimension * self.fft.poly_length()

    def pfksk_len(self) -> int:
        """words of the private key-switch key"""
        return (self.glwe_dimension + 1) * (self.extracted_dimension() + 1) * self.pfks_basis.decompose_length() \
            * self.glwe_len()

    def ggsw_len(self) -> int:
        """words of one output GGSW: (k+1) x ell_cb x (k+1) x N"""
        return (self.glwe_dimension + 1) * self.cbs_basis.decompose_length() * self.glwe_len()


def tfhe_circuit_bootstrap(lwe_in: np.ndarray, bsk: np.ndarray, pfksk: np.ndarray, ggsw_out: np.ndarray,
                           ctx: TfheCircuitBootstrapContext) -> None:
    """Batched circuit bootstrap on host arrays.  lwe_in: batch x (n+1) words; bsk: n Fourier GGSW keys end to end; pfksk:
    ctx.pfksk_len() words as tfhe_generate_pfksk_dev writes them for key_in = the GLWE key polynomials end to end;
    ggsw_out: batch x ctx.ggsw_len() words."""
    pi, ni, wi = _host_words(lwe_in)
    pk, nk = _host_fourier(bsk)
    pp, np_, wp = _host_words(pfksk)
    po, no, wo = _host_words(ggsw_out)
    _same_width("every word array must have the width of the context's basis", wi, wp, wo, ctx._w)
    check(getattr(lib(), ctx._pre)(ctx._h, pi, ni, pk, nk, pp, np_, po, no))


def tfhe_circuit_bootstrap_dev(lwe_in, bsk, pfksk, ggsw_out, ctx: TfheCircuitBootstrapContext, stream=None) -> None:
    """the device form (32- or 64-bit integer CUDA tensors of the context's width, bsk complex128 or float64),
    asynchronous; ggsw_out must not overlap an input and may be uninitialised.  write_fourier_form of ggsw_out is what
    tfhe_external_product_to_dev takes with a TfheFftContext on cbs_basis."""
    pi, ni, wi = _dev_words(lwe_in)
    pk, nk = _dev_fourier(bsk)
    pp, np_, wp = _dev_words(pfksk)
    po, no, wo = _dev_words(ggsw_out)
    _same_width("every word tensor must have the width of the context's basis", wi, wp, wo, ctx._w)
    check(getattr(lib(), ctx._pre + "_dev")(ctx._h, pi, ni, pk, nk, pp, np_, po, no, _stream(stream)))


# ---- the CMUX with a selector per group, and the CMUX tree (include/pfhe.h: cmux_tree_*, cmux, cmux_dev) ----

class TfheCmuxTreeContext(_TorusContext):
    """Handle of the batched CMUX and of the CMUX tree (include/pfhe.h, pfhe_tfhe{,32}_cmux_tree_*): a tree of `depth`
    (1..16) levels selects one of 2^depth GLWE ciphertexts by depth Fourier GGSW selectors per input, the vertical packing
    of a look-up table; tfhe_cmux(_dev) is one level with a key per group as a call of its own.  `basis` is the selectors'
    (the circuit bootstrap's cbs_basis when they come from there).  Owns the node buffers of `chunk` inputs (0 = the
    default) and, off the fused shape, a product plan; one holder at a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int, depth: int, chunk: int = 0):
        self._open(fft, basis, glwe_dimension, "cmux_tree", (depth, chunk), ("_create", "_destroy", "_in_use", "_scratch_bytes"))
        self.depth = depth


def _cmux(words, fourier, d0, d1, keys, out, per_key, ctx, name, tail):
    p0, n0, w0 = words(d0)
    p1, n1, w1 = words(d1)
    po, no, wo = words(out)
    pk, nk = fourier(keys)
    _same_width("d0, d1 and out must have the width of the context's basis", w0, w1, wo, ctx._w)
    check(getattr(lib(), "pfhe_tfhe" + ctx._w + name)(ctx._h, p0, n0, p1, n1, pk, nk, per_key, po, no, *tail))


def tfhe_cmux(d0: np.ndarray, d1: np.ndarray, keys: np.ndarray, out: np.ndarray, ctx: TfheCmuxTreeContext,
              per_key: int = 1) -> None:
    """Batched CMUX on host arrays: out[i] = d0[i] + external_product_to(d1[i] - d0[i], keys[i // per_key]) modulo 2^BITS
    for count GLWE ciphertexts and count / per_key Fourier GGSW keys end to end (ctx.key_len() complex values each): a key
    of the bit m selects d_m.  Word for word the subtraction, tfhe_external_product_to per key group and the addition."""
    _cmux(_host_words, _host_fourier, d0, d1, keys, out, per_key, ctx, "_cmux", ())


def tfhe_cmux_dev(d0, d1, keys, out, ctx: TfheCmuxTreeContext, per_key: int = 1, stream=None) -> None:
    """the device form, asynchronous; out may be exactly d0 or exactly d1, any other overlap with an input is refused"""
    _cmux(_dev_words, _dev_fourier, d0, d1, keys, out, per_key, ctx, "_cmux_dev", (_stream(stream),))


def _cmux_tree(words, fourier, table, selectors, out, ctx, name, tail):
    pt, nt, wt = words(table)
    po, no, wo = words(out)
    ps, ns = fourier(selectors)
    _same_width("table and out must have the width of the context's basis", wt, wo, ctx._w)
    check(getattr(lib(), ctx._pre + name)(ctx._h, pt, nt, ps, ns, po, no, *tail))


def tfhe_cmux_tree(table: np.ndarray, selectors: np.ndarray, out: np.ndarray, ctx: TfheCmuxTreeContext) -> None:
    """The CMUX tree on host arrays.  table: 2^depth GLWE ciphertexts shared by the batch, or batch * 2^depth, input-major;
    selectors: batch x depth Fourier GGSW keys, the key of input e and bit j at e*depth + j (what
    tfhe_circuit_bootstrap_dev on inputs in that order, then write_fourier_form, gives); out: batch ciphertexts, out[e] the
    leaf sum_j m_{e,j} 2^j of e's table.  Word for word depth calls of tfhe_cmux with per_key = 2^(depth-1-j)."""
    _cmux_tree(_host_words, _host_fourier, table, selectors, out, ctx, "", ())


def tfhe_cmux_tree_dev(table, selectors, out, ctx: TfheCmuxTreeContext, stream=None) -> None:
    """the device form, asynchronous; out must not overlap an input and may be uninitialised"""
    _cmux_tree(_dev_words, _dev_fourier, table, selectors, out, ctx, "_dev", (_stream(stream),))


# ---- a look-up table on encrypted bits: tree, rotation by bits, extraction (include/pfhe.h: lut_*, rotate_by_bits, lut_eval) ----

class TfheLutContext(_TorusContext):
    """Handle of the look-up table on encrypted bits (include/pfhe.h, pfhe_tfhe{,32}_lut_*): a CMUX tree of
    `tree_depth` t (0..16) levels over the high bits, a rotation by the `rot_bits` r (0..log N) low bits at stride
    2^`log_stride` (r + s <= log N), and sample extraction, for `outputs` o >= 1 tables per input; p = t + r >= 1 bits per
    input.  `basis` is the selectors' (the circuit bootstrap's cbs_basis when they come from there).  Owns the buffers of
    `chunk` inputs (0 = the default); one holder at a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int, tree_depth: int,
                 rot_bits: int, outputs: int = 1, log_stride: int = 0, chunk: int = 0):
        self._open(fft, basis, glwe_dimension, "lut", (tree_depth, rot_bits, log_stride, outputs, chunk),
                   ("_create", "_destroy", "_in_use", "_scratch_bytes"))
        self.tree_depth, self.rot_bits, self.log_stride, self.outputs = tree_depth, rot_bits, log_stride, outputs

    def bits(self) -> int:
        """p = tree_depth + rot_bits, the selectors per input"""
        return self.tree_depth + self.rot_bits


def _rotate_by_bits(words, fourier, inp, keys, out, ctx, keys_per_input, first_key, name, tail):
    pi, ni, wi = words(inp)
    po, no, wo = words(out)
    pk, nk = fourier(keys)
    _same_width("inp and out must have the width of the context's basis", wi, wo, ctx._w)
    kpi = ctx.rot_bits if keys_per_input is None else keys_per_input
    check(getattr(lib(), "pfhe_tfhe" + ctx._w + name)(ctx._h, pi, ni, pk, nk, kpi, first_key, po, no, *tail))


def tfhe_rotate_by_bits(inp: np.ndarray, keys: np.ndarray, out: np.ndarray, ctx: TfheLutContext,
                        keys_per_input: int | None = None, first_key: int = 0) -> None:
    """The rotation by encrypted bits on host arrays.  inp, out: count = batch * outputs GLWE ciphertexts, accumulator a of
    input a // outputs; keys: batch * keys_per_input Fourier GGSW keys (default rot_bits per input), of which input e uses
    keys[e * keys_per_input + first_key + j] for bit j < rot_bits:
    acc += external_product_to(X^{2N - 2^(j + log_stride)} acc - acc, that key), so out[a] = X^{-x 2^log_stride} inp[a] for
    key bits x = sum_j m_j 2^j.  Word for word, per step, mul_monomial_each_to_dev and tfhe_cmux_dev with per_key = outputs."""
    _rotate_by_bits(_host_words, _host_fourier, inp, keys, out, ctx, keys_per_input, first_key, "_rotate_by_bits", ())


def tfhe_rotate_by_bits_dev(inp, keys, out, ctx: TfheLutContext, keys_per_input: int | None = None, first_key: int = 0,
                            stream=None) -> None:
    """the device form, asynchronous; out may be exactly inp, any other overlap is refused"""
    _rotate_by_bits(_dev_words, _dev_fourier, inp, keys, out, ctx, keys_per_input, first_key, "_rotate_by_bits_dev",
                    (_stream(stream),))


def _lut_eval(words, fourier, table, selectors, out, ctx, extract, name, tail):
    pt, nt, wt = words(table)
    po, no, wo = words(out)
    ps, ns = fourier(selectors)
    _same_width("table and out must have the width of the context's basis", wt, wo, ctx._w)
    check(getattr(lib(), ctx._pre + name)(ctx._h, pt, nt, ps, ns, extract, po, no, *tail))


def tfhe_lut_eval(table: np.ndarray, selectors: np.ndarray, out: np.ndarray, ctx: TfheLutContext, extract: int = 0) -> None:
    """A look-up table of 2^p entries on p encrypted bits, on host arrays.  table: outputs * 2^tree_depth GLWE ciphertexts
    shared by the batch, or batch times as many, leaf (output u, index i) at u * 2^tree_depth + i (tfhe_lut_table builds
    them); selectors: batch x p Fourier GGSW keys, the key of input e and bit j at e*p + j (what tfhe_circuit_bootstrap_dev,
    then write_fourier_form, gives); bits 0..rot_bits-1 rotate, the others walk the tree.  out: batch * outputs GLWE
    ciphertexts (extract = 0), or batch * outputs * extract LWE ciphertexts of k*N + 1 words, row (e * outputs + u) * extract
    + i what glwe_sample_extract writes at index i: index 0 of output (e, u) is entry sum_j m_{e,j} 2^j of table u."""
    _lut_eval(_host_words, _host_fourier, table, selectors, out, ctx, extract, "_eval", ())


def tfhe_lut_eval_dev(table, selectors, out, ctx: TfheLutContext, extract: int = 0, stream=None) -> None:
    """the device form, asynchronous; out must not overlap an input and may be uninitialised"""
    _lut_eval(_dev_words, _dev_fourier, table, selectors, out, ctx, extract, "_eval_dev", (_stream(stream),))


def tfhe_lut_table(values, log_n: int, k: int, tree_depth: int, rot_bits: int, log_stride: int = 0):
    """The trivial GLWE leaves of tfhe_lut_eval from clear entries.  values: a torch or numpy integer array of shape
    (outputs, 2^p) or (outputs, 2^p, words), words <= 2^log_stride, the torus words of entry x of every output.  Returns an
    array of the same kind and dtype of shape (outputs, 2^tree_depth, k+1, N): masks zero, word w of entry x at body
    coefficient (x mod 2^rot_bits) * 2^log_stride + w of leaf x >> rot_bits, every other coefficient zero."""
    n, p = 1 << log_n, tree_depth + rot_bits
    if values.ndim == 2:
        values = values[:, :, None]
    if values.ndim != 3 or values.shape[1] != 1 << p or not 1 <= values.shape[2] <= 1 << log_stride \
            or rot_bits + log_stride > log_n:
        raise ValueError("expected values of shape (outputs, 2^(tree_depth + rot_bits)[, words <= 2^log_stride]) and "
                         "rot_bits + log_stride <= log_n")
    outputs, words = values.shape[0], values.shape[2]
    shape = (outputs, 1 << tree_depth, k + 1, n)
    if isinstance(values, np.ndarray):
        leaves = np.zeros(shape, dtype=values.dtype)
    else:
        import torch
        leaves = torch.zeros(shape, dtype=values.dtype, device=values.device)
    body = leaves[:, :, k, :(1 << rot_bits) << log_stride].reshape(outputs, 1 << tree_depth, 1 << rot_bits, 1 << log_stride)
    body[..., :words] = values.reshape(outputs, 1 << tree_depth, 1 << rot_bits, words)
    leaves[:, :, k, :(1 << rot_bits) << log_stride] = body.reshape(outputs, 1 << tree_depth, -1)
    return leaves


# ---- bit extraction of a multi-bit LWE message, and the look-up on an encrypted integer (include/pfhe.h: pfhe_bitext{,32}_*) ----

class TfheBitExtractContext(_TorusContext):
    """Handle of the batched bit extraction (include/pfhe.h, pfhe_bitext{,32}_*): an LWE ciphertext of
    k*N + 1 words under the extracted GLWE key with phase m*2^delta_log + e becomes `bits` LWE ciphertexts of
    lwe_dimension + 1 words under the LWE key, bit i encoded as m_i*2^(BITS-1): what tfhe_circuit_bootstrap_dev takes.
    Per bit: the key switch under `ks_basis` of the running ciphertext shifted left, and unless it is the last bit a
    blind rotation under `basis` that clears the bit from the running ciphertext.  Owns a blind-rotation handle and every
    buffer between the stages for `chunk` inputs (0 = the default); one holder at a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, lwe_dimension: int, glwe_dimension: int = 1,
                 ks_basis: ApproxSignedBasis | None = None, chunk: int = 0):
        if ks_basis is None:
            raise ValueError("bit extraction needs ks_basis: every bit leaves through the key switch")
        if ks_basis.bits != basis.bits:
            raise TypeError("ks_basis must have the width of the torus words")
        self._open(fft, basis, glwe_dimension, "bitext",
                   (lwe_dimension, ks_basis.log_basis(), ks_basis.decompose_length(), chunk),
                   ("_create", "_destroy", "_in_use", "_scratch_bytes"), family="pfhe_bitext")
        self.lwe_dimension, self.ks_basis = lwe_dimension, ks_basis

    def bsk_len(self) -> int:
        """complex values of the bootstrapping key: lwe_dimension Fourier GGSW keys"""
        return self.lwe_dimension * self.key_len()

    def extracted_dimension(self) -> int:
        return self.glwe_dimension * self.fft.poly_length()

    def ksk_len(self) -> int:
        """words of the key-switch key from the extracted key to the LWE key"""
        return self.extracted_dimension() * self.ks_basis.decompose_length() * (self.lwe_dimension + 1)


def _extract_bits(words, fourier, lwe_in, bsk, ksk, bits_out, ctx, delta_log, bits, name, tail):
    pi, ni, wi = words(lwe_in)
    pk, nk = fourier(bsk)
    ps, ns, ws = words(ksk)
    po, no, wo = words(bits_out)
    _same_width("every word array must have the width of the context's basis", wi, ws, wo, ctx._w)
    check(getattr(lib(), ctx._pre + name)(ctx._h, pi, ni, pk, nk, ps, ns, delta_log, bits, po, no, *tail))


def tfhe_extract_bits(lwe_in: np.ndarray, bsk: np.ndarray, ksk: np.ndarray, bits_out: np.ndarray,
                      ctx: TfheBitExtractContext, delta_log: int, bits: int) -> None:
    """Batched bit extraction on host arrays.  lwe_in: batch x (k*N + 1) words, phase m*2^delta_log + e; bsk: n Fourier
    GGSW keys end to end; ksk: ctx.ksk_len() words as tfhe_generate_ksk_dev writes them; bits_out: batch x bits x (n+1)
    words, bit i (0 the least significant) of input e at row e*bits + i with phase m_i*2^(BITS-1) plus noise.
    1 <= delta_log, 1 <= bits, delta_log + bits <= BITS; higher message bits are shifted out."""
    _extract_bits(_host_words, _host_fourier, lwe_in, bsk, ksk, bits_out, ctx, delta_log, bits, "_extract_bits", ())


def tfhe_extract_bits_dev(lwe_in, bsk, ksk, bits_out, ctx: TfheBitExtractContext, delta_log: int, bits: int,
                          stream=None) -> None:
    """the device form (32- or 64-bit integer CUDA tensors of the context's width, bsk complex128 or float64),
    asynchronous; bits_out must not overlap an input and may be uninitialised; lwe_in is read only"""
    _extract_bits(_dev_words, _dev_fourier, lwe_in, bsk, ksk, bits_out, ctx, delta_log, bits, "_extract_bits_dev",
                  (_stream(stream),))


def tfhe_lut_on_integer_dev(lwe_in, bsk, ksk, pfksk, table, out, bitext_ctx: TfheBitExtractContext,
                            cbs_ctx: TfheCircuitBootstrapContext, lut_ctx: TfheLutContext, delta_log: int, extract: int = 1,
                            stream=None) -> None:
    """A look-up table on an encrypted integer without a padding bit, as a chain of three public calls: tfhe_extract_bits_dev
    with bits = lut_ctx.bits(), tfhe_circuit_bootstrap_dev + write_fourier_form on the batch*bits bit ciphertexts, and
    tfhe_lut_eval_dev with those selectors.  lwe_in: batch x (k*N + 1) words with phase m*2^delta_log + e; out: what
    tfhe_lut_eval_dev writes for `extract` (with extract >= 1 its rows are inputs of the next such call).  lut_ctx's basis
    is cbs_ctx.cbs_basis.  Plain Python, not a handle: every call allocates its intermediates with torch (the bit
    ciphertexts, the torus GGSWs and their Fourier form) on lwe_in's device; allocation and the current-stream semantics
    of torch apply, so pass the stream torch is on, or None on the default stream."""
    import torch
    p = lut_ctx.bits()
    ext = bitext_ctx.extracted_dimension() + 1
    if lwe_in.numel() % ext != 0:
        raise ValueError("lwe_in must be batch x (k*N + 1) words")
    batch = lwe_in.numel() // ext
    bit_cts = torch.empty(batch * p * (bitext_ctx.lwe_dimension + 1), dtype=lwe_in.dtype, device=lwe_in.device)
    ggsw = torch.empty(batch * p * cbs_ctx.ggsw_len(), dtype=lwe_in.dtype, device=lwe_in.device)
    selectors = torch.empty(ggsw.numel(), dtype=torch.complex128, device=lwe_in.device)
    tfhe_extract_bits_dev(lwe_in, bsk, ksk, bit_cts, bitext_ctx, delta_log, p, stream)
    tfhe_circuit_bootstrap_dev(bit_cts, bsk, pfksk, ggsw, cbs_ctx, stream)
    write_fourier_form(ggsw, selectors, cbs_ctx.fft, stream)
    tfhe_lut_eval_dev(table, selectors, out, lut_ctx, extract, stream)


# ---- GLWE key switch, automorphism and trace; their keys; the LWE embedding (include/pfhe.h: glwe_trace_*, glwe_automorphism,
# gksk_generate_dev, lwe_embed) ----

class TfheGlweTraceContext(_TorusContext):
    """Handle of the GLWE automorphism X -> X^t with its key switch and of the homomorphic trace built from it
    (include/pfhe.h, pfhe_tfhe{,32}_glwe_trace_*).  Created and checked as TfheFftContext; owns, off the fused shape
    (k = 1, N <= 2^11), the buffers of `chunk` ciphertexts (0 = the default); one holder at a time (Busy for a second
    thread).  A key has k*ell rows, the mask rows of a Fourier GGSW: key_len() complex values."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int = 1, chunk: int = 0):
        self._open(fft, basis, glwe_dimension, "glwe_trace", (chunk,), ("_create", "_destroy", "_in_use", "_scratch_bytes"))

    def key_len(self) -> int:
        """complex values (and torus words) of one key: k * ell rows of a GLWE ciphertext each"""
        return self.glwe_dimension * self.basis.decompose_length() * self.glwe_len()

    def trace_exponents(self, steps: int | None = None) -> list:
        """the exponents t_s = 2^(log N - s + 1) + 1, s = 1..steps (default log N), whose keys glwe_trace takes in this order"""
        log_n = self.fft.log_n
        steps = log_n if steps is None else steps
        if not 1 <= steps <= log_n:
            raise PfheError(33, "steps must be in 1..log N")
        return [(1 << (log_n - s + 1)) + 1 for s in range(1, steps + 1)]


def _glwe_automorphism(words, fourier, inp, key, out, t, ctx, name, tail):
    pi, ni, wi = words(inp)
    po, no, wo = words(out)
    pk, nk = fourier(key)
    _same_width("inp and out must have the width of the context's basis", wi, wo, ctx._w)
    check(getattr(lib(), "pfhe_tfhe" + ctx._w + name)(ctx._h, pi, ni, pk, nk, t, po, no, *tail))


def glwe_automorphism(inp: np.ndarray, key: np.ndarray, out: np.ndarray, t: int, ctx: TfheGlweTraceContext) -> None:
    """The automorphism X -> X^t (t odd, 1..2N-1) with its key switch, on host arrays:
    out[e] = (0, .., 0, sigma_t(B_e)) - to_torus(sum_j sum_l d_l(sigma_t(A_{e,j})) * key[j][l]) modulo 2^BITS for a batch of
    GLWE ciphertexts and one key of ctx.key_len() complex values (tfhe_generate_gksk_dev).  Word for word the exact
    permutation sigma_t, tfhe_external_product_to against the key padded with ell zero body rows, and the subtraction."""
    _glwe_automorphism(_host_words, _host_fourier, inp, key, out, t, ctx, "_glwe_automorphism", ())


def glwe_automorphism_dev(inp, key, out, t: int, ctx: TfheGlweTraceContext, stream=None) -> None:
    """the device form, asynchronous; out must not overlap inp (the operation is a gather)"""
    _glwe_automorphism(_dev_words, _dev_fourier, inp, key, out, t, ctx, "_glwe_automorphism_dev", (_stream(stream),))


def glwe_keyswitch(inp: np.ndarray, key: np.ndarray, out: np.ndarray, ctx: TfheGlweTraceContext) -> None:
    """GLWE key switch on host arrays: glwe_automorphism with t = 1, key from tfhe_generate_gksk_dev(.., exponents=[1])"""
    glwe_automorphism(inp, key, out, 1, ctx)


def glwe_keyswitch_dev(inp, key, out, ctx: TfheGlweTraceContext, stream=None) -> None:
    """the device form, asynchronous; out must not overlap inp"""
    glwe_automorphism_dev(inp, key, out, 1, ctx, stream)


def _glwe_trace(words, fourier, inp, keys, out, ctx, steps, name, tail):
    pi, ni, wi = words(inp)
    po, no, wo = words(out)
    pk, nk = fourier(keys)
    _same_width("inp and out must have the width of the context's basis", wi, wo, ctx._w)
    m = ctx.fft.log_n if steps is None else steps
    check(getattr(lib(), ctx._pre + name)(ctx._h, pi, ni, pk, nk, m, po, no, *tail))


def glwe_trace(inp: np.ndarray, keys: np.ndarray, out: np.ndarray, ctx: TfheGlweTraceContext, steps: int | None = None) -> None:
    """The homomorphic trace of `steps` = m steps (1..log N, default log N) on host arrays: ACC_0 = inp[e],
    ACC_s = ACC_{s-1} + automorphism(ACC_{s-1}, keys[s-1], t_s), out[e] = ACC_m, with t_s = ctx.trace_exponents(m)[s-1] and
    keys the m keys end to end; word for word m calls of glwe_automorphism with a wrapping addition after each.  The phase
    of out is 2^m times the phase of inp at the coefficients that are multiples of 2^m and (up to the key switches' noise)
    zero elsewhere; m = log N leaves N times coefficient 0 alone.  The factor 2^m is NOT removed here: scaling the message
    by 1 / 2^m beforehand is the caller's business."""
    _glwe_trace(_host_words, _host_fourier, inp, keys, out, ctx, steps, "", ())


def glwe_trace_dev(inp, keys, out, ctx: TfheGlweTraceContext, steps: int | None = None, stream=None) -> None:
    """the device form, asynchronous; out may be exactly inp, any other overlap is refused.  The factor 2^m stays in
    the result, as in glwe_trace."""
    _glwe_trace(_dev_words, _dev_fourier, inp, keys, out, ctx, steps, "_dev", (_stream(stream),))


def tfhe_generate_gksk_dev(key_in, key_out, fft: FullComplex64FftTable, basis: ApproxSignedBasis, rand, exponents,
                           glwe_dimension: int = 1, out=None, stream=None):
    """The keys glwe_automorphism_dev / glwe_trace_dev take, generated on the device: for every odd exponent t_x of
    `exponents`, a key that switches sigma_{t_x} of a ciphertext under key_in to key_out (both the k key polynomials end to
    end).  rand: len(exponents) x k*ell x (k+1)*N torus words holding the randomness (mask polynomials uniform, body
    polynomials noise), which becomes the torus-form keys in place: row (j, l) of key x gets B += sum_c A_c * key_out_c and
    B += sigma_{t_x}(key_in_j) * 2^(drop_bits + l*log_basis); out: as many complex128 values (allocated when None), the
    Fourier form, bit for bit what write_fourier_form gives.  exponents=[1] is a plain GLWE key switch key;
    ctx.trace_exponents(m) with key_in == key_out the trace's keys.  Returns out.  Asynchronous."""
    import torch
    pi, ni, wi = _dev_words(key_in)
    pz, nz, wz = _dev_words(key_out)
    pr, nr, wr = _dev_words(rand)
    _same_width("both keys and the randomness must have the same word width", wi, wz, wr)
    lb, ell = _basis_args(basis, wr)
    ex = np.ascontiguousarray(list(exponents), dtype=np.uint32)
    if out is None:
        out = torch.empty(nr, dtype=torch.complex128, device=rand.device)
    po, no = _dev_fourier(out)
    check(getattr(lib(), "pfhe_tfhe" + wr + "_gksk_generate_dev")(fft._h, glwe_dimension, lb, ell, pi, ni, pz, nz,
                                                                ex.ctypes.data_as(C.c_void_p), ex.size, pr, nr, po, no,
                                                                _stream(stream)))
    return out


def _lwe_embed(dev, lwe, glwe_out, fft, glwe_dimension, stream=None) -> None:
    _stateless("_lwe_embed", dev, (lwe, glwe_out), "lwe and glwe_out must have the same word width",
               lambda w, l, g: (fft._h, glwe_dimension, *l, *g), stream)


def lwe_embed_glwe(lwe: np.ndarray, glwe_out: np.ndarray, fft: FullComplex64FftTable, glwe_dimension: int = 1) -> None:
    """Embeds LWE ciphertexts (a[0..kN), b) under the GLWE key polynomials end to end into GLWE ciphertexts whose phase has
    the LWE phase on coefficient 0 (and no meaning elsewhere), on host arrays: A_j[0] = a[jN], A_j[N - i] = -a[jN + i],
    B = (b, 0, .., 0).  Exact; glwe_sample_extract at index 0 gives the LWE ciphertext back word for word; followed by
    the full glwe_trace it is the LWE-to-GLWE conversion (times N)."""
    _lwe_embed(False, lwe, glwe_out, fft, glwe_dimension)


def lwe_embed_glwe_dev(lwe, glwe_out, fft: FullComplex64FftTable, glwe_dimension: int = 1, stream=None) -> None:
    """the device form, asynchronous and stateless; glwe_out must not overlap lwe and may be uninitialised"""
    _lwe_embed(True, lwe, glwe_out, fft, glwe_dimension, stream)


# ---- ring packing of LWE ciphertexts by automorphisms (include/pfhe.h: pfhe_ringpack{,32}_*) ----

class TfheRingPackContext(_TorusContext):
    """Handle of ring packing (include/pfhe.h, pfhe_ringpack{,32}_*): up to `max_count` (default N)
    LWE ciphertexts under the GLWE key polynomials end to end become ONE GLWE ciphertext, by pairwise merges with one
    automorphism each and the remaining trace steps, on the key set glwe_trace takes.  Created and checked as
    TfheGlweTraceContext, then max_count in 1..N; owns the node buffer of chunk * max(1, 2^(M-1)) ciphertexts,
    M = ceil(log2 max_count), and off the fused shape (k = 1, N <= 2^11) the general form's buffers; `chunk` counts
    output ciphertexts (0 = the default); one holder at a time (Busy for a second thread)."""

    def __init__(self, fft: FullComplex64FftTable, basis: ApproxSignedBasis, glwe_dimension: int = 1,
                 max_count: int | None = None, chunk: int = 0):
        self.max_count = fft.poly_length() if max_count is None else max_count
        self._open(fft, basis, glwe_dimension, "ringpack", (self.max_count, chunk),
                   ("_create", "_destroy", "_in_use", "_scratch_bytes"), family="pfhe_ringpack")

    def key_len(self) -> int:
        """complex values (and torus words) of one key: k * ell rows of a GLWE ciphertext each"""
        return self.glwe_dimension * self.basis.decompose_length() * self.glwe_len()

    def lwe_len(self) -> int:
        return self.glwe_dimension * self.fft.poly_length() + 1

    def trace_exponents(self) -> list:
        """the exponents t_s = 2^(log N - s + 1) + 1, s = 1..log N, whose keys lwe_ring_pack takes in this order: all of
        them, whatever the count (tfhe_generate_gksk_dev with key_in == key_out)"""
        log_n = self.fft.log_n
        return [(1 << (log_n - s + 1)) + 1 for s in range(1, log_n + 1)]

    def slot(self, i: int, count: int) -> int:
        """the coefficient of the packed phase that holds N times the phase of LWE ciphertext i of `count`: i * N / 2^m,
        m = ceil(log2 count)"""
        if not 0 <= i < count <= self.max_count:
            raise PfheError(33, "need 0 <= i < count <= max_count")
        return i * (self.fft.poly_length() >> (count - 1).bit_length())


def _glwe_ring_merge(words, fourier, even, odd, key, out, level, ctx, name, tail):
    pe, ne, we = words(even)
    pd, nd, wd = words(odd)
    po, no, wo = words(out)
    pk, nk = fourier(key)
    _same_width("even, odd and out must have the width of the context's basis", we, wd, wo, ctx._w)
    check(getattr(lib(), ctx._pre + name)(ctx._h, pe, ne, pd, nd, pk, nk, level, po, no, *tail))


def glwe_ring_merge(even: np.ndarray, odd: np.ndarray, key: np.ndarray, out: np.ndarray, level: int,
                    ctx: TfheRingPackContext) -> None:
    """The merge of ring packing at `level` l in 1..log N, on host arrays, with s = N / 2^l and t = 2^l + 1:
    D = even[e] - X^s odd[e], S = even[e] + X^s odd[e], out[e] = S + automorphism(D, key, t) modulo 2^BITS, for a batch of
    pairs and one key of ctx.key_len() complex values (the key of t).  Word for word tfhe_mul_monomial_each_to_dev, a
    wrapping subtraction and addition, glwe_automorphism and a wrapping addition.  Where the phases of both inputs are
    fixed by sigma_t up to a sign at the multiples of 2 s (what the previous level leaves), the phase of out is twice the
    phase of even at the even multiples of s and twice the phase of odd, moved by s, at the odd ones."""
    _glwe_ring_merge(_host_words, _host_fourier, even, odd, key, out, level, ctx, "_merge", ())


def glwe_ring_merge_dev(even, odd, key, out, level: int, ctx: TfheRingPackContext, stream=None) -> None:
    """the device form, asynchronous; out may be exactly even, any other overlap (and any with odd or key) is refused"""
    _glwe_ring_merge(_dev_words, _dev_fourier, even, odd, key, out, level, ctx, "_merge_dev", (_stream(stream),))


def _lwe_ring_pack(words, fourier, lwe_in, keys, glwe_out, count, ctx, name, tail):
    pi, ni, wi = words(lwe_in)
    po, no, wo = words(glwe_out)
    pk, nk = fourier(keys)
    _same_width("lwe_in and glwe_out must have the width of the context's basis", wi, wo, ctx._w)
    check(getattr(lib(), ctx._pre + name)(ctx._h, pi, ni, pk, nk, count, po, no, *tail))


def lwe_ring_pack(lwe_in: np.ndarray, keys: np.ndarray, glwe_out: np.ndarray, count: int, ctx: TfheRingPackContext) -> None:
    """Ring packing on host arrays: lwe_in holds batch * count LWE ciphertexts of k*N + 1 words (group e is ciphertexts
    e*count .. e*count + count - 1), keys the log N keys of ctx.trace_exponents() end to end (ALL of them, whatever the
    count), glwe_out batch GLWE ciphertexts.  With m = ceil(log2 count): node_0[i] = lwe_embed_glwe(lwe_in[e*count + i])
    (all zero for count <= i < 2^m), node_l[r] = glwe_ring_merge(node_{l-1}[r], node_{l-1}[r + 2^(m-l)], keys[log N - l],
    level l) for l = 1..m, glwe_out[e] = glwe_trace(node_m[0], keys[0 .. log N - m), steps = log N - m); word for word
    that composition.  The phase of glwe_out[e] is N times the phase of ciphertext i at coefficient ctx.slot(i, count) =
    i * N / 2^m and (up to the key switches' noise) zero elsewhere: the stride is N / 2^m, where lwe_pack_keyswitch fills
    coefficients 0..count-1.  The factor N is NOT removed, as the trace's 2^m is not: the message has to sit log N bits
    lower in the inputs than it is wanted in the output, which is the price against the packing key switch (whose key is
    about 50 times larger)."""
    _lwe_ring_pack(_host_words, _host_fourier, lwe_in, keys, glwe_out, count, ctx, "_pack", ())


def lwe_ring_pack_dev(lwe_in, keys, glwe_out, count: int, ctx: TfheRingPackContext, stream=None) -> None:
    """the device form, asynchronous; glwe_out must overlap neither lwe_in nor keys.  The factor N stays in the result and
    the message has to sit log N bits lower, as in lwe_ring_pack."""
    _lwe_ring_pack(_dev_words, _dev_fourier, lwe_in, keys, glwe_out, count, ctx, "_pack_dev", (_stream(stream),))


def _torus_dtype(bits: int):
    import torch
    if bits not in (32, 64):
        raise PfheError(33, "bits must be 32 or 64")
    return torch.int32 if bits == 32 else torch.int64


def torus_uniform(size, bits: int, device="cuda", generator=None):
    """`size` uniform torus words of `bits` bits as an int32 / int64 tensor (the words are the two's-complement bit
    patterns).  NOT CRYPTOGRAPHIC: torch's generator is a statistical one (Philox / Mersenne twister), fit for tests and
    measurements only; fill the buffers from a cryptographic generator for real keys and ciphertexts."""
    import torch
    half = 1 << (bits - 1)
    dtype = _torus_dtype(bits)
    if bits == 32:
        return torch.randint(-half, half, (size,), dtype=torch.int64, device=device, generator=generator).to(dtype)
    # randint's exclusive upper bound cannot be 2^63: two 32-bit halves instead
    hi = torch.randint(-(1 << 31), 1 << 31, (size,), dtype=torch.int64, device=device, generator=generator)
    lo = torch.randint(0, 1 << 32, (size,), dtype=torch.int64, device=device, generator=generator)
    return (hi << 32) | lo


def torus_noise(size, bits: int, device="cuda", std=None, bound=None, generator=None):
    """`size` noise words as an int32 / int64 tensor: a rounded Gaussian of standard deviation `std` (in units of one torus
    word, i.e. 2^-BITS of the torus), or integers uniform in [-bound, bound]; exactly one of the two.  NOT CRYPTOGRAPHIC:
    torch's generator is a statistical one, and the Gaussian is rounded from float64, so its tail ends near 2^53."""
    import torch
    dtype = _torus_dtype(bits)
    if (std is None) == (bound is None):
        raise TypeError("give exactly one of std and bound")
    if bound is not None:
        return torch.randint(-int(bound), int(bound) + 1, (size,), dtype=torch.int64, device=device,
                             generator=generator).to(dtype)
    g = torch.empty(size, dtype=torch.float64, device=device).normal_(0.0, float(std), generator=generator)
    return torch.round(g).to(torch.int64).to(dtype)


# ---- the random layer: a ChaCha20 stream on the device, samplers, rows, seeded ciphertexts (include/pfhe.h: pfhe_csprng_*,
# pfhe_rand{,32}_*) ----

class RandSeed:
    """The identity of one ChaCha20 stream: a 32-byte key and a 64-bit nonce (the key's bytes are the state words 4..11
    little-endian, as in RFC 8439; the nonce is state words 14 and 15).  Every output of every sampler is a closed form of
    (key, nonce, index), so the same seed gives the same words in any call, of any length, on any launch.

    The library gathers NO entropy of its own: `key` is the caller's, and fresh() takes it from os.urandom.  A mask seed
    may be published (a seeded ciphertext carries it); a noise seed is a secret and must differ from the mask seed in key
    or nonce.  Neither repr() nor an error message shows a key."""

    def __init__(self, key: bytes, nonce: int = 0):
        if not isinstance(key, (bytes, bytearray)) or len(key) != 32:
            raise ValueError("the key must be 32 bytes")
        if not 0 <= int(nonce) < 1 << 64:
            raise ValueError("the nonce must be in 0..2^64-1")
        self.nonce = int(nonce)
        self._key = (C.c_uint32 * 8)(*(int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)))
        self._nonce = (C.c_uint32 * 2)(self.nonce & 0xffffffff, self.nonce >> 32)

    @classmethod
    def fresh(cls, nonce: int = 0) -> "RandSeed":
        """a seed whose key is 32 bytes of os.urandom: the operating system's entropy, not the library's"""
        import os
        return cls(os.urandom(32), nonce)

    def with_nonce(self, nonce: int) -> "RandSeed":
        """the same key under another nonce: an independent stream"""
        return RandSeed(b"".join(int(w).to_bytes(4, "little") for w in self._key), nonce)

    def __repr__(self) -> str:
        return "RandSeed(key=<32 bytes>, nonce=%d)" % self.nonce

    def _args(self):
        return C.cast(self._key, C.c_void_p), C.cast(self._nonce, C.c_void_p)


def _seed_args(*seeds):
    for s in seeds:
        if not isinstance(s, RandSeed):
            raise TypeError("expected a RandSeed")
    return tuple(a for s in seeds for a in s._args())


def csprng_keystream_dev(seed: RandSeed, word_offset: int, out, device=None, stream=None) -> None:
    """u32 words [word_offset, word_offset + out.numel()) of the seed's ChaCha20 stream into a 32-bit integer CUDA tensor:
    word j is little-endian word j mod 16 of block j div 16.  Asynchronous."""
    po, no, w = _dev_words(out)
    if w != "32":
        raise TypeError("the keystream is written as 32-bit words")
    check(lib().pfhe_csprng_keystream_dev(_dev_index(out, device), *_seed_args(seed), word_offset, po, no, _stream(stream)))


def _sampler(name, seed, offset, out, device, stream, *lead) -> None:
    po, no, w = _dev_words(out)
    check(getattr(lib(), "pfhe_rand" + w + "_" + name + "_dev")(_dev_index(out, device), *_seed_args(seed), offset, *lead, po,
                                                             no, _stream(stream)))


def torus_uniform_dev(seed: RandSeed, offset: int, out, device=None, stream=None) -> None:
    """out[i] = stream word offset + i of the tensor's width (32- or 64-bit integer CUDA tensor; a u64 stream word is u32
    words 2j, low half, and 2j + 1): uniform torus words from a cryptographic stream.  Asynchronous."""
    _sampler("uniform", seed, offset, out, device, stream)


def torus_binary_dev(seed: RandSeed, offset: int, out, device=None, stream=None) -> None:
    """out[i] = bit (offset + i) mod 32 of u32 stream word (offset + i) div 32, as a torus word 0 or 1: the values of
    sample_binary_values_to (primus_distr/src/common.rs:22-42) on the same word stream.  Asynchronous."""
    _sampler("binary", seed, offset, out, device, stream)


def torus_ternary_dev(seed: RandSeed, offset: int, out, device=None, stream=None) -> None:
    """out[i] = [0, 0, 1, -1][(w >> 2 (j mod 16)) & 3] with j = offset + i and w u32 stream word j div 16, -1 the all-ones
    word: sample_ternary_values_to (common.rs:56-76).  Asynchronous."""
    _sampler("ternary", seed, offset, out, device, stream)


def torus_tuniform_dev(seed: RandSeed, offset: int, bound_log2: int, out, device=None, stream=None) -> None:
    """Bounded noise TUniform(b), b = bound_log2 in 0..BITS-2: out[i] takes u64 stream word offset + i at both widths, r its
    low b + 2 bits, and is (r >> 1) + (r & 1) - 2^b modulo 2^BITS: support [-2^b, 2^b], the two ends with probability
    2^-(b+2), every other value 2^-(b+1), variance (2^(2b+1) + 1) / 6.  Asynchronous."""
    _sampler("tuniform", seed, offset, out, device, stream, bound_log2)


def tfhe_fill_rows_dev(mask_seed: RandSeed, noise_seed: RandSeed, first_row: int, mask_len: int, body_len: int,
                       bound_log2: int, out, add: bool = False, device=None, stream=None) -> None:
    """The randomness of whole ciphertext rows in one launch: out holds rows x (mask_len + body_len) words; for absolute row
    R = first_row + r, mask word j is uniform output R*mask_len + j of the mask stream and body word j gets TUniform(bound_log2)
    output R*body_len + j of the noise stream, stored, or added when `add` (so that messages can be placed first).  LWE rows
    are (n, 1), GLWE rows (k*N, N); the `rand` argument of tfhe_generate_bsk_dev, _ksk_dev, _pksk_dev, _pfksk_dev and
    _gksk_dev is rows of one of the two.  Rows [a, a + b) written alone are that slice of rows [0, R).  The two seeds must
    differ.  Asynchronous."""
    po, no, w = _dev_words(out)
    check(getattr(lib(), "pfhe_rand" + w + "_fill_rows_dev")(_dev_index(out, device), *_seed_args(mask_seed, noise_seed),
                                                           first_row, mask_len, body_len, bound_log2, int(bool(add)), po, no,
                                                           _stream(stream)))


def _encrypt_seeded(dev, mask_seed, noise_seed, first_row, key, bound_log2, bodies, device, stream=None) -> None:
    words = _dev_words if dev else _host_words
    pk, nk, wk = words(key)
    pb, nb, wb = words(bodies)
    w = _same_width("key and bodies must have the same word width", wk, wb)
    tail = (_stream(stream),) if dev else ()
    check(getattr(lib(), "pfhe_rand" + w + "_lwe_encrypt_seeded" + ("_dev" if dev else ""))(
        _dev_index(bodies, device) if dev else device, *_seed_args(mask_seed, noise_seed), first_row, pk, nk, bound_log2, pb,
        nb, *tail))


def lwe_encrypt_seeded(mask_seed: RandSeed, noise_seed: RandSeed, first_row: int, key: np.ndarray, bound_log2: int,
                       bodies: np.ndarray, device: int = 0) -> None:
    """Seeded LWE encryption on host arrays, in place: bodies[r] += <mask(R), key> + noise(R) for R = first_row + r, where
    mask(R) is uniform outputs [R*n, (R+1)*n) of the mask stream (n = len(key)) and noise(R) TUniform(bound_log2) output R of
    the noise stream.  bodies holds the encoded messages on entry and the ciphertext bodies on exit: with (mask_seed,
    first_row) they ARE the ciphertexts, one word each instead of n + 1.  The mask is generated in registers and never
    stored; the result is word for word tfhe_fill_rows_dev(add=True) followed by lwe_encrypt_dev.  The key is any words."""
    _encrypt_seeded(False, mask_seed, noise_seed, first_row, key, bound_log2, bodies, device)


def lwe_encrypt_seeded_dev(mask_seed: RandSeed, noise_seed: RandSeed, first_row: int, key, bound_log2: int, bodies,
                           device=None, stream=None) -> None:
    """the device form, asynchronous; the key must not overlap the bodies"""
    _encrypt_seeded(True, mask_seed, noise_seed, first_row, key, bound_log2, bodies, device, stream)


def _seeded_expand(dev, mask_seed, first_row, mask_len, body_len, bodies, out, device, stream=None) -> None:
    words = _dev_words if dev else _host_words
    pb, nb, wb = words(bodies)
    po, no, wo = words(out)
    w = _same_width("bodies and out must have the same word width", wb, wo)
    tail = (_stream(stream),) if dev else ()
    check(getattr(lib(), "pfhe_rand" + w + "_seeded_expand" + ("_dev" if dev else ""))(
        _dev_index(out, device) if dev else device, *_seed_args(mask_seed), first_row, mask_len, body_len, pb, nb, po, no,
        *tail))


def seeded_expand(mask_seed: RandSeed, first_row: int, mask_len: int, body_len: int, bodies: np.ndarray, out: np.ndarray,
                  device: int = 0) -> None:
    """What the receiving side of seeded ciphertexts runs, on host arrays: out becomes rows x (mask_len + body_len) words,
    the masks from the mask stream (as tfhe_fill_rows_dev writes them) and the bodies copied from `bodies` (rows x body_len
    words).  It takes no noise seed."""
    _seeded_expand(False, mask_seed, first_row, mask_len, body_len, bodies, out, device)


def seeded_expand_dev(mask_seed: RandSeed, first_row: int, mask_len: int, body_len: int, bodies, out, device=None,
                      stream=None) -> None:
    """the device form, asynchronous; out must not overlap bodies and may be uninitialised"""
    _seeded_expand(True, mask_seed, first_row, mask_len, body_len, bodies, out, device, stream)


def tfhe_generate_ksk_seeded_dev(mask_seed: RandSeed, noise_seed: RandSeed, key_in, key_out, basis: ApproxSignedBasis,
                                 bound_log2: int, first_row: int = 0, device=None, stream=None):
    """The key-switch key lwe_keyswitch_dev takes, in seeded form: len(key_in) * ell words instead of len(key_in) * ell *
    (len(key_out) + 1).  Row (i, j) is absolute row first_row + i*ell + j of the two streams; its body starts as the message
    key_in[i] * 2^(drop_bits + j*log_basis) (placed by torch) and lwe_encrypt_seeded_dev adds <mask, key_out> + noise.
    seeded_expand_dev(mask_seed, first_row, len(key_out), 1, bodies, ksk) then gives exactly what tfhe_generate_ksk_dev makes
    of tfhe_fill_rows_dev's buffer.  Returns the bodies (allocates them).  Asynchronous on `stream`'s device; torch places the
    messages on its current stream."""
    import torch
    _, _, wi = _dev_words(key_in)
    _, _, wo = _dev_words(key_out)
    _basis_args(basis, _same_width("both keys must have the same word width", wi, wo))
    bits, half = basis.bits, 1 << (basis.bits - 1)
    factors = [1 << (basis.drop_bits() + j * basis.log_basis()) for j in range(basis.decompose_length())]
    gadget = torch.tensor([f - (1 << bits) if f >= half else f for f in factors], dtype=key_in.dtype, device=key_in.device)
    bodies = (key_in.reshape(-1, 1) * gadget.reshape(1, -1)).reshape(-1).contiguous()   # wrapping products modulo 2^BITS
    lwe_encrypt_seeded_dev(mask_seed, noise_seed, first_row, key_out, bound_log2, bodies, device, stream)
    return bodies
