"""Reference model of the torus FFT and the TFHE external product (include/pfhe.h, pfhe_fft_* / pfhe_tfhe_*), shared by
the CPU model test and the GPU parity tests.

A numpy restatement of:
  - FullComplex64FftTable (primus_fft/src/complex64/table.rs:47-130): forward = FFT_N(centred(x_j) * psi^j), psi = e^{i pi/N};
    inverse = Re(IFFT_N(Y) * conj(psi^j) / N) rounded and wrapped to the torus;
  - TorusFftValue (primus_fft/src/torus.rs:32-58): centring by a signed reinterpretation, and from_f64_wrapping_rounded
    (round half away from zero, then `as i64 as u32` / `as i128 as u64`, i.e. saturate, then wrap);
  - the power-of-two ApproxSignedBasis (primus_decompose/src/primitive/basis.rs:47-177, 391-407; common.rs:219-274):
    init_carry_slice + decompose_iter;
  - external_product_to (primus_lattice/src/tfhe/external_product.rs:36-93);
and an exact integer schoolbook of the same product (the reference test's naive_external_product_u32, carried out mod 2^64
so that it serves u32 and u64 alike).
"""
import numpy as np

UINT = {32: np.uint32, 64: np.uint64}
SINT = {32: np.int32, 64: np.int64}


def twist(log_n: int) -> np.ndarray:
    """psi^j = cis(pi * j / N), j < N, with one rounding of the angle (complex64/table.rs:76-81)."""
    n = 1 << log_n
    ang = np.pi * np.arange(n, dtype=np.float64) / float(n)
    return np.cos(ang) + 1j * np.sin(ang)


def centred(x: np.ndarray, bits: int) -> np.ndarray:
    """TorusFftValue::into_f64_centered: the word reinterpreted as signed, widened to f64."""
    return np.asarray(x).astype(UINT[bits]).view(SINT[bits]).astype(np.float64)


def round_half_away(v: np.ndarray) -> np.ndarray:
    """f64::round: half-way cases away from zero (v - trunc(v) is exact)."""
    v = np.asarray(v, np.float64)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def from_f64_wrapping_rounded(v, bits: int) -> np.ndarray:
    """TorusFftValue::from_f64_wrapping_rounded: u32 = round() as i64 as u32 (saturates at +-2^63 first), u64 = round() as
    i128 as u64 (saturates at +-2^127, otherwise the exact value mod 2^64).  NaN gives 0."""
    r = round_half_away(np.atleast_1d(v)).ravel()
    sat = 63 if bits == 32 else 127
    out = np.zeros(r.size, np.uint64)
    small = np.abs(r) < 2.0 ** 62
    out[small] = r[small].astype(np.int64).view(np.uint64)
    for i in np.nonzero(~small)[0]:
        x = r[i]
        if np.isnan(x):
            iv = 0
        elif x >= 2.0 ** sat:
            iv = (1 << sat) - 1
        elif x <= -(2.0 ** sat):
            iv = -(1 << sat)
        else:
            iv = int(x)  # exact: a double is an integer here
        out[i] = iv % (1 << 64)
    return out.astype(UINT[bits])


class FullComplex64FftTable:
    """FullComplex64FftTable: fourier_length == poly_length == N."""

    def __init__(self, log_n: int):
        self.log_n = log_n
        self.n = 1 << log_n
        self.tw = twist(log_n)

    def poly_length(self):
        return self.n

    def fourier_length(self):
        return self.n

    def forward(self, x: np.ndarray, bits: int) -> np.ndarray:
        """forward_torus_slice over one polynomial or a batch (the last axis is the polynomial)."""
        return np.fft.fft(centred(x, bits) * self.tw, axis=-1)

    def inverse_f64(self, y: np.ndarray) -> np.ndarray:
        """the f64 value before the conversion: Re(IFFT_N(Y) * conj(psi^j) / N), rustfft's unscaled inverse"""
        buf = np.fft.ifft(np.asarray(y, np.complex128), axis=-1) * self.n
        return (buf * (np.conj(self.tw) / self.n)).real

    def inverse(self, y: np.ndarray, bits: int) -> np.ndarray:
        v = self.inverse_f64(y)
        return from_f64_wrapping_rounded(v, bits).reshape(v.shape)


# ---- the folded half-size transform the kernels rest on ----

def folded_forward(x: np.ndarray, bits: int) -> np.ndarray:
    """Y[2m], m < N/2, as FFT_{N/2}((x_m + i x_{m+N/2}) e^{i pi m/N})."""
    n = x.shape[-1]
    h = n // 2
    c = centred(x, bits)
    z = (c[..., :h] + 1j * c[..., h:]) * twist(int(np.log2(n)))[:h]
    return np.fft.fft(z, axis=-1)


def hermitian_even(y: np.ndarray) -> np.ndarray:
    """H[2m] = (Y[2m] + conj(Y[(1 - 2m) mod N])) / 2 for m < N/2."""
    n = y.shape[-1]
    m = np.arange(n // 2)
    return (y[..., 2 * m] + np.conj(y[..., (1 - 2 * m) % n])) / 2


def folded_inverse_f64(h_even: np.ndarray) -> np.ndarray:
    """the N reals whose folded transform is h_even (N/2 values): z = IFFT_{N/2}(H) e^{-i pi l/N}, x_l = Re, x_{l+N/2} = Im"""
    h = h_even.shape[-1]
    n = 2 * h
    z = np.fft.ifft(h_even, axis=-1) * np.conj(twist(int(np.log2(n)))[:h])
    return np.concatenate([z.real, z.imag], axis=-1)


# ---- ApproxSignedBasis<T> with modulus None (power of two) ----

class ApproxSignedBasis:
    def __init__(self, bits: int, log_basis: int, reverse_length=None):
        assert 0 < log_basis < bits, "log_basis must be in 1..BITS-1"
        self.bits, self.log_basis = bits, log_basis
        length = bits // log_basis
        drop = bits - length * log_basis
        if reverse_length is not None:
            assert length >= reverse_length
            length, drop = reverse_length, bits - reverse_length * log_basis
        assert length > 0
        self.decompose_length, self.drop_bits = length, drop

    def digits(self, values: np.ndarray):
        """init_carry_slice + decompose_iter: the signed digits, least significant kept level first, as signed int64"""
        v = np.asarray(values).astype(np.uint64)
        B = 1 << self.log_basis
        carry = ((v >> np.uint64(self.drop_bits - 1)) & np.uint64(1)).astype(np.int64) if self.drop_bits else \
            np.zeros(v.shape, np.int64)
        out = []
        for lvl in range(self.decompose_length):
            shift = np.uint64(self.drop_bits + lvl * self.log_basis)
            temp = ((v >> shift) & np.uint64(B - 1)).astype(np.int64) + carry
            if self.log_basis == 1:
                nc = (temp & 2) != 0
            else:
                nc = (temp & (B | (B >> 1))) != 0
            d = np.where(nc, np.where(temp > B - 1, 0, temp - B), temp)
            carry = nc.astype(np.int64)
            out.append(d)
        return out


def external_product(inp: np.ndarray, key: np.ndarray, basis: ApproxSignedBasis, log_n: int, k: int):
    """external_product_to for one GLWE: inp (k+1)*N words, key (k+1)*ell*(k+1)*N complex (the reference's layout);
    returns (output words, the f64 values before the conversion)."""
    bits, n, ell = basis.bits, 1 << log_n, basis.decompose_length
    fft = FullComplex64FftTable(log_n)
    key = np.asarray(key, np.complex128).reshape(k + 1, ell, k + 1, n)
    acc = np.zeros((k + 1, n), np.complex128)
    polys = np.asarray(inp).reshape(k + 1, n)
    for r in range(k + 1):
        for lvl, d in enumerate(basis.digits(polys[r])):
            dft = fft.forward(d.astype(UINT[bits]), bits)
            acc += dft[None, :] * key[r, lvl]
    v = fft.inverse_f64(acc)
    return from_f64_wrapping_rounded(v, bits).reshape(k + 1, n).reshape(-1), v.reshape(-1)


def negacyclic_u64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a * b mod (X^N + 1) with wrapping uint64 arithmetic: exact mod 2^64"""
    n = a.size
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    out = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        for i in range(n):
            if a[i] == 0:
                continue
            prod = b * a[i]
            out[i:] += prod[:n - i]
            out[:i] -= prod[n - i:]
    return out


def schoolbook(inp: np.ndarray, key_coeff: np.ndarray, basis: ApproxSignedBasis, log_n: int, k: int) -> np.ndarray:
    """the exact product with a coefficient-domain key (naive_external_product_u32, widened): digits and key words as
    signed integers, everything mod 2^BITS"""
    bits, n, ell = basis.bits, 1 << log_n, basis.decompose_length
    kc = np.asarray(key_coeff).astype(UINT[bits]).view(SINT[bits]).astype(np.int64).view(np.uint64)
    kc = kc.reshape(k + 1, ell, k + 1, n)
    out = np.zeros((k + 1, n), np.uint64)
    polys = np.asarray(inp).reshape(k + 1, n)
    with np.errstate(over="ignore"):
        for r in range(k + 1):
            for lvl, d in enumerate(basis.digits(polys[r])):
                du = d.astype(np.int64).view(np.uint64)
                for c in range(k + 1):
                    out[c] += negacyclic_u64(du, kc[r, lvl, c])
    return out.reshape(-1).astype(UINT[bits])


def centred_error(a: np.ndarray, b: np.ndarray, bits: int) -> np.ndarray:
    """|a - b| as centred torus distances"""
    d = (np.asarray(a).astype(UINT[bits]) - np.asarray(b).astype(UINT[bits])).view(SINT[bits])
    return np.abs(d.astype(np.float64))
