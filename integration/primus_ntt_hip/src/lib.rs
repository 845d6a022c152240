//! `NttTable` / `DcrtTable` implementations that delegate to hand-written HIP kernels for MI355X
//! through the C ABI of libpfhe_hip.so (include/pfhe.h).  UNTESTED SOURCE — see Cargo.toml.
//!
//! Replaces, behind the same traits:
//!   * `U64NttTable`  (crates/primus_ntt/src/ntt/prime64/table.rs:41)  -> [`HipNttTable`]
//!   * `U64DcrtTable` (crates/primus_ntt/src/dcrt/prime64.rs:11)       -> [`HipDcrtTable`]
//!   * `U32NttTable`  (crates/primus_ntt/src/ntt/prime32/table.rs:37)  -> [`HipU32NttTable`]
//! so that every function of primus_lattice that is generic over `Table: NttTable` / `DcrtTable`
//! runs on the GPU unchanged (one host->device->host round trip per `&mut [T]` call), and adds the
//! batched, device-resident external product as [`HipExternalProduct`].  `FullComplex64FftTable`
//! (crates/primus_fft/src/complex64/table.rs:47) -> [`HipFftTable`] behind `FftTable`, and the TFHE product in the
//! Fourier domain as [`HipTfheExternalProduct`] / [`HipTfheExternalProduct32`], with the blind rotation over it as
//! [`HipTfheBlindRotate`] / [`HipTfheBlindRotate32`], its multi-bit form as [`HipTfheMultiBitBlindRotate`] /
//! [`HipTfheMultiBitBlindRotate32`], and the programmable bootstrap around that as
//! [`HipTfheBootstrap`] / [`HipTfheBootstrap32`].
mod ffi;

use core::ffi::{c_int, CStr};

use num_complex::Complex64;
use primus_data::{DataMut, RawData};
use primus_fft::{FftError, FftTable, TorusFftValue};
use primus_ntt::{DcrtTable, NttError, NttTable};
use primus_poly::{CrtPolynomial, DcrtPolynomial, NttPolynomial, Polynomial};
use primus_reduce::FieldContext;

fn device() -> c_int {
    std::env::var("PFHE_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0)
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(ffi::pfhe_last_error()) }.to_string_lossy().into_owned()
}

/// pfhe_status -> NttError (crates/primus_ntt/src/error.rs:7-49; include/pfhe.h status codes 1..5).
fn status_to_err<T: From<u32> + Copy>(code: c_int, n: usize, q: T, max_bits: u32) -> NttError<T> {
    match code {
        1 => NttError::NoPrimitiveRoot { degree: T::from(2 * n as u32), modulus: q },
        2 => NttError::DegreeConversionErr { degree: n, modulus: q },
        3 => NttError::DegreeTooLarge { degree: n, modulus: q },
        5 => NttError::ModulusTooLarge { modulus: q, max_bits },
        _ => NttError::NttTableErr, // incl. PFHE_ERR_NO_DEVICE / PFHE_ERR_HIP: no CPU fallback
    }
}

/// The reference's transforms are infallible (`table.rs:541-563` only debug_asserts lengths); a
/// non-zero status here is a length mismatch or a device failure, i.e. a state the reference would
/// panic on as well.
fn expect_ok(rc: c_int, what: &str) {
    assert_eq!(rc, ffi::PFHE_OK, "{what}: {}", last_error());
}

// ------------------------------------------------------------------------------------------------
// U64NttTable
// ------------------------------------------------------------------------------------------------
pub struct HipNttTable {
    h: *mut ffi::pfhe_ntt,
}
// handles are immutable after creation and usable from several host threads (pfhe.h "Conventions")
unsafe impl Send for HipNttTable {}
unsafe impl Sync for HipNttTable {}
impl Drop for HipNttTable {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_ntt_destroy(self.h) }
    }
}

/// The inherent getters of `U64NttTable` (crates/primus_ntt/src/ntt/prime64/table.rs:127-161).
impl HipNttTable {
    pub fn modulus(&self) -> u64 {
        unsafe { ffi::pfhe_ntt_modulus(self.h) }
    }
    pub fn log_n(&self) -> u32 {
        unsafe { ffi::pfhe_ntt_log_n(self.h) }
    }
    pub fn n(&self) -> usize {
        unsafe { ffi::pfhe_ntt_poly_length(self.h) }
    }
    pub fn root(&self) -> u64 {
        unsafe { ffi::pfhe_ntt_root(self.h) }
    }
    pub fn inv_root(&self) -> u64 {
        unsafe { ffi::pfhe_ntt_inv_root(self.h) }
    }
    pub fn inv_n(&self) -> u64 {
        unsafe { ffi::pfhe_ntt_inv_n(self.h) }
    }
}

impl NttTable for HipNttTable {
    type ValueT = u64;

    fn new<M: FieldContext<u64>>(log_n: u32, modulus: M) -> Result<Self, NttError<u64>> {
        let q = modulus.value().ok_or(NttError::NttTableErr)?; // table.rs:313-315
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_ntt_create(log_n, q, device(), &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(status_to_err(e, 1usize << log_n, q, 62)),
        }
    }
    fn poly_length(&self) -> usize {
        unsafe { ffi::pfhe_ntt_poly_length(self.h) }
    }
    fn transform_inplace<S: RawData<Elem = u64> + DataMut>(&self, mut poly: Polynomial<S>) -> NttPolynomial<S> {
        self.transform_slice(poly.as_mut_slice()); // table.rs:523-530
        NttPolynomial::new(poly.0)
    }
    fn inverse_transform_inplace<S: RawData<Elem = u64> + DataMut>(&self, mut values: NttPolynomial<S>) -> Polynomial<S> {
        self.inverse_transform_slice(values.as_mut_slice()); // table.rs:532-539
        Polynomial::new(values.0)
    }
    fn lazy_transform_slice(&self, poly: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_ntt_lazy_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "lazy_transform_slice")
    }
    fn transform_slice(&self, poly: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_ntt_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "transform_slice")
    }
    fn lazy_inverse_transform_slice(&self, values: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_ntt_lazy_inverse_transform_slice(self.h, values.as_mut_ptr(), values.len()) },
                  "lazy_inverse_transform_slice")
    }
    fn inverse_transform_slice(&self, values: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_ntt_inverse_transform_slice(self.h, values.as_mut_ptr(), values.len()) },
                  "inverse_transform_slice")
    }
    fn transform_monomial(&self, coeff: u64, degree: usize, values: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_ntt_transform_monomial(self.h, coeff, degree, values.as_mut_ptr(), values.len()) },
                  "transform_monomial")
    }
    fn transform_coeff_one_monomial(&self, degree: usize, values: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_ntt_transform_coeff_one_monomial(self.h, degree, values.as_mut_ptr(), values.len()) },
                  "transform_coeff_one_monomial")
    }
    fn transform_coeff_minus_one_monomial(&self, degree: usize, values: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_ntt_transform_coeff_minus_one_monomial(self.h, degree, values.as_mut_ptr(), values.len()) },
                  "transform_coeff_minus_one_monomial")
    }
}

// ------------------------------------------------------------------------------------------------
// U64DcrtTable
// ------------------------------------------------------------------------------------------------
pub struct HipDcrtTable {
    h: *mut ffi::pfhe_dcrt,
    limbs: Vec<HipNttTable>, // DcrtTable::ntt_tables() hands out per-limb tables (dcrt/mod.rs:31-35)
    poly_length: usize,
}
unsafe impl Send for HipDcrtTable {}
unsafe impl Sync for HipDcrtTable {}
impl Drop for HipDcrtTable {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_dcrt_destroy(self.h) }
    }
}
impl HipDcrtTable {
    /// Raw handle for the device-resident entry points (`pfhe_dcrt_*_dev`, `pfhe_extprod_*`).
    pub fn handle(&self) -> *const ffi::pfhe_dcrt {
        self.h
    }

    // Device-resident element-wise forms of CrtGlwe / CrtPolynomial methods for a batch in one slice
    // (crates/primus_lattice/src/macros/mod.rs:367-531, glwe/crt.rs:59-175, primus_poly/src/crt/mul.rs:102-127).
    // All pointers are device pointers to `len` words; `out` may alias `a`.

    /// `CrtGlwe::add_element_wise_to` / `add_element_wise_assign`.
    pub unsafe fn add_element_wise_to_dev(&self, a: *const u64, b: *const u64, out: *mut u64, len: usize,
                                          stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        status(unsafe { ffi::pfhe_dcrt_add_to_dev(self.h, a, b, out, len, stream) })
    }
    /// `CrtGlwe::sub_element_wise_to` / `sub_element_wise_assign`.
    pub unsafe fn sub_element_wise_to_dev(&self, a: *const u64, b: *const u64, out: *mut u64, len: usize,
                                          stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        status(unsafe { ffi::pfhe_dcrt_sub_to_dev(self.h, a, b, out, len, stream) })
    }
    /// `CrtGlwe::mul_scalar_to` / `mul_scalar_assign` (`scalar_residue`: one residue per modulus, on the host).
    pub unsafe fn mul_scalar_to_dev(&self, a: *const u64, scalar_residue: &[u64], out: *mut u64, len: usize,
                                    stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        assert_eq!(scalar_residue.len(), self.limbs.len());
        status(unsafe { ffi::pfhe_dcrt_mul_scalar_to_dev(self.h, a, scalar_residue.as_ptr(), out, len, stream) })
    }
    /// `CrtGlwe::mul_monic_monomial_assign(r)` written to a second buffer (`self * X^r`, `r < 2N`).
    pub unsafe fn mul_monic_monomial_to_dev(&self, a: *const u64, r: usize, out: *mut u64, len: usize,
                                            stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        status(unsafe { ffi::pfhe_dcrt_mul_monomial_to_dev(self.h, a, r, out, len, stream) })
    }
    /// `DcrtPolynomial::inv_to`; `Err(PFHE_ERR_NO_INVERSE)` where the reference panics.
    pub unsafe fn inv_to_dev(&self, a: *const u64, out: *mut u64, len: usize, stream: *mut core::ffi::c_void)
                             -> Result<(), c_int> {
        status(unsafe { ffi::pfhe_dcrt_inv_to_dev(self.h, a, out, len, stream) })
    }
}

fn status(rc: c_int) -> Result<(), c_int> {
    if rc == ffi::PFHE_OK { Ok(()) } else { Err(rc) }
}

impl DcrtTable for HipDcrtTable {
    type ValueT = u64;
    type NttTables = HipNttTable;

    fn new<M: FieldContext<u64>>(log_n: u32, moduli: &[M]) -> Result<Self, NttError<u64>> {
        let qs: Vec<u64> = moduli.iter().map(|m| m.value().ok_or(NttError::NttTableErr)).collect::<Result<_, _>>()?;
        let limbs = moduli.iter().map(|m| HipNttTable::new(log_n, *m)).collect::<Result<Vec<_>, _>>()?;
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_dcrt_create(log_n, qs.as_ptr(), qs.len(), device(), &mut h) } {
            ffi::PFHE_OK => Ok(Self { h, limbs, poly_length: 1usize << log_n }),
            e => Err(status_to_err(e, 1usize << log_n, qs.first().copied().unwrap_or(0), 62)),
        }
    }
    fn ntt_tables(&self) -> &[HipNttTable] {
        &self.limbs
    }
    fn iter(&self) -> std::slice::Iter<'_, HipNttTable> {
        self.limbs.iter()
    }
    fn poly_length(&self) -> usize {
        self.poly_length
    }
    fn moduli_count(&self) -> usize {
        self.limbs.len()
    }
    fn crt_poly_length(&self) -> usize {
        self.poly_length * self.limbs.len()
    }
    fn transform_inplace<S: RawData<Elem = u64> + DataMut>(&self, mut crt_poly: CrtPolynomial<S>) -> DcrtPolynomial<S> {
        self.transform_slice(crt_poly.as_mut_slice()); // one launch for all limbs (dcrt/prime64.rs:71-83 loops)
        DcrtPolynomial::new(crt_poly.0)
    }
    fn inverse_transform_inplace<S: RawData<Elem = u64> + DataMut>(&self, mut dcrt_poly: DcrtPolynomial<S>) -> CrtPolynomial<S> {
        self.inverse_transform_slice(dcrt_poly.as_mut_slice());
        CrtPolynomial::new(dcrt_poly.0)
    }
    fn lazy_transform_slice(&self, poly: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_dcrt_lazy_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "dcrt lazy_transform_slice")
    }
    fn transform_slice(&self, poly: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_dcrt_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "dcrt transform_slice")
    }
    fn lazy_inverse_transform_slice(&self, poly: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_dcrt_lazy_inverse_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) },
                  "dcrt lazy_inverse_transform_slice")
    }
    fn inverse_transform_slice(&self, poly: &mut [u64]) {
        expect_ok(unsafe { ffi::pfhe_dcrt_inverse_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) },
                  "dcrt inverse_transform_slice")
    }
    // transform_monomial & co: the trait's provided methods (dcrt/mod.rs:107-134) call the per-limb tables
}

// ------------------------------------------------------------------------------------------------
// U32NttTable
// ------------------------------------------------------------------------------------------------
pub struct HipU32NttTable {
    h: *mut ffi::pfhe_ntt32,
}
unsafe impl Send for HipU32NttTable {}
unsafe impl Sync for HipU32NttTable {}
impl Drop for HipU32NttTable {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_ntt32_destroy(self.h) }
    }
}

impl NttTable for HipU32NttTable {
    type ValueT = u32;

    fn new<M: FieldContext<u32>>(log_n: u32, modulus: M) -> Result<Self, NttError<u32>> {
        let q = modulus.value().ok_or(NttError::NttTableErr)?;
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_ntt32_create(log_n, q, device(), &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(status_to_err(e, 1usize << log_n, q, 30)), // prime32/table.rs:195-200
        }
    }
    fn poly_length(&self) -> usize {
        unsafe { ffi::pfhe_ntt32_poly_length(self.h) }
    }
    fn transform_inplace<S: RawData<Elem = u32> + DataMut>(&self, mut poly: Polynomial<S>) -> NttPolynomial<S> {
        self.transform_slice(poly.as_mut_slice());
        NttPolynomial::new(poly.0)
    }
    fn inverse_transform_inplace<S: RawData<Elem = u32> + DataMut>(&self, mut values: NttPolynomial<S>) -> Polynomial<S> {
        self.inverse_transform_slice(values.as_mut_slice());
        Polynomial::new(values.0)
    }
    fn lazy_transform_slice(&self, poly: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_ntt32_lazy_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "u32 lazy_transform_slice")
    }
    fn transform_slice(&self, poly: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_ntt32_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "u32 transform_slice")
    }
    fn lazy_inverse_transform_slice(&self, values: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_ntt32_lazy_inverse_transform_slice(self.h, values.as_mut_ptr(), values.len()) },
                  "u32 lazy_inverse_transform_slice")
    }
    fn inverse_transform_slice(&self, values: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_ntt32_inverse_transform_slice(self.h, values.as_mut_ptr(), values.len()) },
                  "u32 inverse_transform_slice")
    }
    fn transform_monomial(&self, coeff: u32, degree: usize, values: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_ntt32_transform_monomial(self.h, coeff, degree, values.as_mut_ptr(), values.len()) },
                  "u32 transform_monomial")
    }
    fn transform_coeff_one_monomial(&self, degree: usize, values: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_ntt32_transform_coeff_one_monomial(self.h, degree, values.as_mut_ptr(), values.len()) },
                  "u32 transform_coeff_one_monomial")
    }
    fn transform_coeff_minus_one_monomial(&self, degree: usize, values: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_ntt32_transform_coeff_minus_one_monomial(self.h, degree, values.as_mut_ptr(), values.len()) },
                  "u32 transform_coeff_minus_one_monomial")
    }
}

// ------------------------------------------------------------------------------------------------
// U32DcrtTable (crates/primus_ntt/src/dcrt/prime32.rs:11-128)
// ------------------------------------------------------------------------------------------------
pub struct HipU32DcrtTable {
    h: *mut ffi::pfhe_dcrt32,
    limbs: Vec<HipU32NttTable>,
    poly_length: usize,
}
unsafe impl Send for HipU32DcrtTable {}
unsafe impl Sync for HipU32DcrtTable {}
impl Drop for HipU32DcrtTable {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_dcrt32_destroy(self.h) }
    }
}
impl HipU32DcrtTable {
    /// Raw handle for the device-resident entry points (`pfhe_dcrt32_*_dev`, `pfhe_extprod32_*`).
    pub fn handle(&self) -> *const ffi::pfhe_dcrt32 {
        self.h
    }
}

impl DcrtTable for HipU32DcrtTable {
    type ValueT = u32;
    type NttTables = HipU32NttTable;

    fn new<M: FieldContext<u32>>(log_n: u32, moduli: &[M]) -> Result<Self, NttError<u32>> {
        let qs: Vec<u32> = moduli.iter().map(|m| m.value().ok_or(NttError::NttTableErr)).collect::<Result<_, _>>()?;
        let limbs = moduli.iter().map(|m| HipU32NttTable::new(log_n, *m)).collect::<Result<Vec<_>, _>>()?;
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_dcrt32_create(log_n, qs.as_ptr(), qs.len(), device(), &mut h) } {
            ffi::PFHE_OK => Ok(Self { h, limbs, poly_length: 1usize << log_n }),
            e => Err(status_to_err(e, 1usize << log_n, qs.first().copied().unwrap_or(0), 30)),
        }
    }
    fn ntt_tables(&self) -> &[HipU32NttTable] {
        &self.limbs
    }
    fn iter(&self) -> std::slice::Iter<'_, HipU32NttTable> {
        self.limbs.iter()
    }
    fn poly_length(&self) -> usize {
        self.poly_length
    }
    fn moduli_count(&self) -> usize {
        self.limbs.len()
    }
    fn crt_poly_length(&self) -> usize {
        self.poly_length * self.limbs.len()
    }
    fn transform_inplace<S: RawData<Elem = u32> + DataMut>(&self, mut crt_poly: CrtPolynomial<S>) -> DcrtPolynomial<S> {
        self.transform_slice(crt_poly.as_mut_slice());
        DcrtPolynomial::new(crt_poly.0)
    }
    fn inverse_transform_inplace<S: RawData<Elem = u32> + DataMut>(&self, mut dcrt_poly: DcrtPolynomial<S>) -> CrtPolynomial<S> {
        self.inverse_transform_slice(dcrt_poly.as_mut_slice());
        CrtPolynomial::new(dcrt_poly.0)
    }
    fn lazy_transform_slice(&self, poly: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_dcrt32_lazy_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "dcrt32 lazy_transform_slice")
    }
    fn transform_slice(&self, poly: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_dcrt32_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) }, "dcrt32 transform_slice")
    }
    fn lazy_inverse_transform_slice(&self, poly: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_dcrt32_lazy_inverse_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) },
                  "dcrt32 lazy_inverse_transform_slice")
    }
    fn inverse_transform_slice(&self, poly: &mut [u32]) {
        expect_ok(unsafe { ffi::pfhe_dcrt32_inverse_transform_slice(self.h, poly.as_mut_ptr(), poly.len()) },
                  "dcrt32 inverse_transform_slice")
    }
}

// ------------------------------------------------------------------------------------------------
// Batched, device-resident RNS gadget external product:
//   CrtGlwe::mul_dcrt_ggsw_to (crates/primus_lattice/src/glwe/crt.rs:200-227) for `batch` ciphertexts
// ------------------------------------------------------------------------------------------------
/// Owns what the reference passes as `&BigUintApproxSignedBasis`, `&RNSBase` and `&mut DcrtGlevContext`
/// (scratch): one per stream, like the `&mut` context it mirrors.
pub struct HipExternalProduct {
    rns: *mut ffi::pfhe_rns,
    basis: *mut ffi::pfhe_basis,
    plan: *mut ffi::pfhe_extprod_plan,
}
impl HipExternalProduct {
    pub fn new(table: &HipDcrtTable, moduli: &[u64], log_basis: u32, glwe_dimension: usize) -> Result<Self, c_int> {
        let (mut rns, mut basis, mut plan) = (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut());
        unsafe {
            let rc = ffi::pfhe_rns_create(moduli.as_ptr(), moduli.len(), device(), &mut rns);
            if rc != ffi::PFHE_OK { return Err(rc); }
            let rc = ffi::pfhe_basis_create(rns, log_basis, 0, &mut basis);
            if rc != ffi::PFHE_OK { ffi::pfhe_rns_destroy(rns); return Err(rc); }
            let rc = ffi::pfhe_extprod_plan_create(table.handle(), rns, basis, glwe_dimension, 0, &mut plan);
            if rc != ffi::PFHE_OK { ffi::pfhe_basis_destroy(basis); ffi::pfhe_rns_destroy(rns); return Err(rc); }
        }
        Ok(Self { rns, basis, plan })
    }
    /// `crt_glwe_dev`: batch x (k+1) x L x N words on the device; `dcrt_ggsw_dev`: one GGSW
    /// ((k+1) x ell x (k+1) x L x N words, shared) or one per ciphertext; `result_dev` like `crt_glwe_dev`.
    pub unsafe fn mul_dcrt_ggsw_to_dev(&mut self, crt_glwe_dev: *const u64, len_glwe: usize, dcrt_ggsw_dev: *const u64,
                                       len_ggsw: usize, result_dev: *mut u64, into_coeff_form: bool,
                                       stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        match unsafe { ffi::pfhe_extprod_mul_dcrt_ggsw_to_dev(self.plan, crt_glwe_dev, len_glwe, dcrt_ggsw_dev, len_ggsw,
                                                             result_dev, len_glwe, into_coeff_form as c_int, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipExternalProduct {
    fn drop(&mut self) {
        unsafe {
            ffi::pfhe_extprod_plan_destroy(self.plan);
            ffi::pfhe_basis_destroy(self.basis);
            ffi::pfhe_rns_destroy(self.rns);
        }
    }
}

/// The same over `U32DcrtTable`: `CrtGlwe::<u32>::mul_dcrt_ggsw_to` with `RNSBase<u32>` and
/// `BigUintApproxSignedBasis<u32>` (u32 words on the device; moduli below 2^30, log_basis below 32).
pub struct HipExternalProduct32 {
    rns: *mut ffi::pfhe_rns32,
    basis: *mut ffi::pfhe_basis32,
    plan: *mut ffi::pfhe_extprod32_plan,
}
impl HipExternalProduct32 {
    pub fn new(table: &HipU32DcrtTable, moduli: &[u32], log_basis: u32, glwe_dimension: usize) -> Result<Self, c_int> {
        let (mut rns, mut basis, mut plan) = (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut());
        unsafe {
            let rc = ffi::pfhe_rns32_create(moduli.as_ptr(), moduli.len(), device(), &mut rns);
            if rc != ffi::PFHE_OK { return Err(rc); }
            let rc = ffi::pfhe_basis32_create(rns, log_basis, 0, &mut basis);
            if rc != ffi::PFHE_OK { ffi::pfhe_rns32_destroy(rns); return Err(rc); }
            let rc = ffi::pfhe_extprod32_plan_create(table.handle(), rns, basis, glwe_dimension, 0, &mut plan);
            if rc != ffi::PFHE_OK { ffi::pfhe_basis32_destroy(basis); ffi::pfhe_rns32_destroy(rns); return Err(rc); }
        }
        Ok(Self { rns, basis, plan })
    }
    pub unsafe fn mul_dcrt_ggsw_to_dev(&mut self, crt_glwe_dev: *const u32, len_glwe: usize, dcrt_ggsw_dev: *const u32,
                                       len_ggsw: usize, result_dev: *mut u32, into_coeff_form: bool,
                                       stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        status(unsafe { ffi::pfhe_extprod32_mul_dcrt_ggsw_to_dev(self.plan, crt_glwe_dev, len_glwe, dcrt_ggsw_dev, len_ggsw,
                                                                 result_dev, len_glwe, into_coeff_form as c_int, stream) })
    }
}
impl Drop for HipExternalProduct32 {
    fn drop(&mut self) {
        unsafe {
            ffi::pfhe_extprod32_plan_destroy(self.plan);
            ffi::pfhe_basis32_destroy(self.basis);
            ffi::pfhe_rns32_destroy(self.rns);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Batched blind rotation over the external product (the CMUX loop of a bootstrap): for every step i and ciphertext e,
//   ACC_e += coeff_form(((X^{exps[e*n_steps+i]} - 1) * ACC_e) (x) BSK_i)
// (CrtGlwe::mul_monic_monomial_assign, glwe/crt.rs:76-114; CrtGlwe::mul_dcrt_ggsw_to, glwe/crt.rs:200-227)
// ------------------------------------------------------------------------------------------------
/// Owns the basis, the RNS base and the rotation handle (its product plan and glue buffers): one per stream.
pub struct HipBlindRotate {
    rns: *mut ffi::pfhe_rns,
    basis: *mut ffi::pfhe_basis,
    h: *mut ffi::pfhe_blindrot,
}
impl HipBlindRotate {
    pub fn new(table: &HipDcrtTable, moduli: &[u64], log_basis: u32, glwe_dimension: usize) -> Result<Self, c_int> {
        let (mut rns, mut basis, mut h) = (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut());
        unsafe {
            let rc = ffi::pfhe_rns_create(moduli.as_ptr(), moduli.len(), device(), &mut rns);
            if rc != ffi::PFHE_OK { return Err(rc); }
            let rc = ffi::pfhe_basis_create(rns, log_basis, 0, &mut basis);
            if rc != ffi::PFHE_OK { ffi::pfhe_rns_destroy(rns); return Err(rc); }
            let rc = ffi::pfhe_blindrot_create(table.handle(), rns, basis, glwe_dimension, 0, &mut h);
            if rc != ffi::PFHE_OK { ffi::pfhe_basis_destroy(basis); ffi::pfhe_rns_destroy(rns); return Err(rc); }
        }
        Ok(Self { rns, basis, h })
    }
    /// `acc_dev`: batch x (k+1) x L x N words (coefficient form, updated in place); `bsk_dev`: n_steps GGSWs end to end;
    /// `exps_dev`: batch x n_steps exponents, ciphertext-major (taken modulo 2N).
    pub unsafe fn rotate_dev(&mut self, acc_dev: *mut u64, len_acc: usize, bsk_dev: *const u64, len_bsk: usize,
                             exps_dev: *const u32, len_exps: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        status(unsafe { ffi::pfhe_blindrot_rotate_dev(self.h, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream) })
    }
}
impl Drop for HipBlindRotate {
    fn drop(&mut self) {
        unsafe {
            ffi::pfhe_blindrot_destroy(self.h);
            ffi::pfhe_basis_destroy(self.basis);
            ffi::pfhe_rns_destroy(self.rns);
        }
    }
}

/// The same over `U32DcrtTable` (u32 words on the device).
pub struct HipBlindRotate32 {
    rns: *mut ffi::pfhe_rns32,
    basis: *mut ffi::pfhe_basis32,
    h: *mut ffi::pfhe_blindrot32,
}
impl HipBlindRotate32 {
    pub fn new(table: &HipU32DcrtTable, moduli: &[u32], log_basis: u32, glwe_dimension: usize) -> Result<Self, c_int> {
        let (mut rns, mut basis, mut h) = (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut());
        unsafe {
            let rc = ffi::pfhe_rns32_create(moduli.as_ptr(), moduli.len(), device(), &mut rns);
            if rc != ffi::PFHE_OK { return Err(rc); }
            let rc = ffi::pfhe_basis32_create(rns, log_basis, 0, &mut basis);
            if rc != ffi::PFHE_OK { ffi::pfhe_rns32_destroy(rns); return Err(rc); }
            let rc = ffi::pfhe_blindrot32_create(table.handle(), rns, basis, glwe_dimension, 0, &mut h);
            if rc != ffi::PFHE_OK { ffi::pfhe_basis32_destroy(basis); ffi::pfhe_rns32_destroy(rns); return Err(rc); }
        }
        Ok(Self { rns, basis, h })
    }
    pub unsafe fn rotate_dev(&mut self, acc_dev: *mut u32, len_acc: usize, bsk_dev: *const u32, len_bsk: usize,
                             exps_dev: *const u32, len_exps: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        status(unsafe { ffi::pfhe_blindrot32_rotate_dev(self.h, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream) })
    }
}
impl Drop for HipBlindRotate32 {
    fn drop(&mut self) {
        unsafe {
            ffi::pfhe_blindrot32_destroy(self.h);
            ffi::pfhe_basis32_destroy(self.basis);
            ffi::pfhe_rns32_destroy(self.rns);
        }
    }
}

/// `FftTable` (crates/primus_fft/src/table.rs) over the host-slice forms of the torus FFT: the drop-in replacement of
/// `FullComplex64FftTable` (complex64/table.rs:47-130; fourier_length == poly_length == N).  u32 and u64 torus values;
/// 1 <= log_n <= 14 (the table's `new` refuses more with `FftError::InvalidLogN { max: 14 }`).  The batched,
/// device-resident product is [`HipTfheExternalProduct`].
pub struct HipFftTable {
    fft: *mut ffi::pfhe_fft,
    n: usize,
}
unsafe impl Send for HipFftTable {}
unsafe impl Sync for HipFftTable {}
impl Drop for HipFftTable {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_fft_destroy(self.fft) }
    }
}
impl HipFftTable {
    pub fn handle(&self) -> *mut ffi::pfhe_fft {
        self.fft
    }
}
impl FftTable for HipFftTable {
    fn new(log_n: u32) -> Result<Self, FftError> {
        let mut fft = core::ptr::null_mut();
        match unsafe { ffi::pfhe_fft_create(log_n, device(), &mut fft) } {
            ffi::PFHE_OK => Ok(Self { fft, n: 1usize << log_n }),
            ffi::PFHE_ERR_UNSUPPORTED => Err(FftError::InvalidLogN { log_n, max: 14 }),
            e => panic!("pfhe_fft_create: status {e}: {}", last_error()),
        }
    }
    fn poly_length(&self) -> usize {
        self.n
    }
    fn fourier_length(&self) -> usize {
        self.n
    }
    fn forward_torus_slice<T: TorusFftValue>(&self, input: &[T], output: &mut [Complex64]) {
        // Complex64 is #[repr(C)] { re, im }: the interleaved layout of the C ABI
        let out = output.as_mut_ptr() as *mut f64;
        let rc = unsafe {
            match core::mem::size_of::<T>() {
                8 => ffi::pfhe_fft_forward_torus_slice(self.fft, input.as_ptr() as *const u64, input.len(), out, output.len()),
                4 => ffi::pfhe_fft_forward_torus32_slice(self.fft, input.as_ptr() as *const u32, input.len(), out, output.len()),
                _ => panic!("HipFftTable: u32 and u64 torus values only"),
            }
        };
        assert_eq!(rc, ffi::PFHE_OK, "pfhe_fft_forward_torus_slice: {}", last_error());
    }
    fn inverse_torus_slice<T: TorusFftValue>(&self, input: &[Complex64], output: &mut [T]) {
        let inp = input.as_ptr() as *const f64;
        let rc = unsafe {
            match core::mem::size_of::<T>() {
                8 => ffi::pfhe_fft_inverse_torus_slice(self.fft, inp, input.len(), output.as_mut_ptr() as *mut u64, output.len()),
                4 => ffi::pfhe_fft_inverse_torus32_slice(self.fft, inp, input.len(), output.as_mut_ptr() as *mut u32, output.len()),
                _ => panic!("HipFftTable: u32 and u64 torus values only"),
            }
        };
        assert_eq!(rc, ffi::PFHE_OK, "pfhe_fft_inverse_torus_slice: {}", last_error());
    }
}

/// `external_product_to` (crates/primus_lattice/src/tfhe/external_product.rs:36-93) for a batch of u64-torus GLWE
/// ciphertexts and one Fourier GGSW key, with its `ApproxSignedBasis::<u64>::new(None, log_basis, reverse_length)` and
/// `TfheFftContext` in one plan (`decompose_length` 0 = the full length).  [`HipTfheExternalProduct32`]: the u32 torus.
pub struct HipTfheExternalProduct {
    plan: *mut ffi::pfhe_tfhe_plan,
}
impl HipTfheExternalProduct {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize) -> Result<Self, c_int> {
        let mut plan = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe_plan_create(fft.handle(), glwe_dimension, log_basis, decompose_length, 0, &mut plan) } {
            ffi::PFHE_OK => Ok(Self { plan }),
            e => Err(e),
        }
    }
    /// `input_dev` / `output_dev`: batch x (k+1) x N words; `key_dev`: (k+1) x ell x (k+1) x N complex values
    pub unsafe fn external_product_to_dev(&mut self, input_dev: *const u64, len_input: usize, key_dev: *const f64,
                                          len_key: usize, output_dev: *mut u64, stream: *mut core::ffi::c_void)
                                          -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe_external_product_to_dev(self.plan, input_dev, len_input, key_dev, len_key, output_dev,
                                                             len_input, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheExternalProduct {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe_plan_destroy(self.plan) }
    }
}

pub struct HipTfheExternalProduct32 {
    plan: *mut ffi::pfhe_tfhe32_plan,
}
impl HipTfheExternalProduct32 {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize) -> Result<Self, c_int> {
        let mut plan = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe32_plan_create(fft.handle(), glwe_dimension, log_basis, decompose_length, 0, &mut plan) } {
            ffi::PFHE_OK => Ok(Self { plan }),
            e => Err(e),
        }
    }
    pub unsafe fn external_product_to_dev(&mut self, input_dev: *const u32, len_input: usize, key_dev: *const f64,
                                          len_key: usize, output_dev: *mut u32, stream: *mut core::ffi::c_void)
                                          -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe32_external_product_to_dev(self.plan, input_dev, len_input, key_dev, len_key,
                                                               output_dev, len_input, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheExternalProduct32 {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe32_plan_destroy(self.plan) }
    }
}

/// The batched blind rotation over the TFHE product: for every step i and ciphertext e,
/// `ACC_e += external_product_to(X^{exps[e*n_steps+i]} * ACC_e - ACC_e, BSK_i)` on u64-torus words, the whole loop on the
/// device (one launch per chunk for k = 1, N <= 2^11).  Takes [`HipTfheExternalProduct`]'s arguments and owns its plan.
/// [`HipTfheBlindRotate32`]: the u32 torus.
pub struct HipTfheBlindRotate {
    h: *mut ffi::pfhe_tfhe_blindrot,
}
impl HipTfheBlindRotate {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize) -> Result<Self, c_int> {
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe_blindrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, 0, &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(e),
        }
    }
    /// `acc_dev`: batch x (k+1) x N words, updated in place; `bsk_dev`: n_steps x (k+1) x ell x (k+1) x N complex values
    /// (`len_bsk` counts them); `exps_dev`: batch x n_steps exponents, taken modulo 2N
    pub unsafe fn rotate_dev(&mut self, acc_dev: *mut u64, len_acc: usize, bsk_dev: *const f64, len_bsk: usize,
                             exps_dev: *const u32, len_exps: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe_blindrot_rotate_dev(self.h, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheBlindRotate {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe_blindrot_destroy(self.h) }
    }
}

pub struct HipTfheBlindRotate32 {
    h: *mut ffi::pfhe_tfhe32_blindrot,
}
impl HipTfheBlindRotate32 {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize) -> Result<Self, c_int> {
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe32_blindrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, 0, &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(e),
        }
    }
    /// `acc_dev`: batch x (k+1) x N words, updated in place; `bsk_dev`: n_steps x (k+1) x ell x (k+1) x N complex values
    /// (`len_bsk` counts them); `exps_dev`: batch x n_steps exponents, taken modulo 2N
    pub unsafe fn rotate_dev(&mut self, acc_dev: *mut u32, len_acc: usize, bsk_dev: *const f64, len_bsk: usize,
                             exps_dev: *const u32, len_exps: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe32_blindrot_rotate_dev(self.h, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheBlindRotate32 {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe32_blindrot_destroy(self.h) }
    }
}

/// The multi-bit blind rotation over the TFHE product: the mask is consumed `grouping_factor` (1..4) elements at a time, and
/// for every group t and ciphertext e `ACC_e = external_product_to(ACC_e, sum_j X^{r_j} * BSK[t][j])`, r_j the subset sum of
/// the group's exponents at the set bits of j.  Binary LWE keys; the key holds groups x 2^g Fourier GGSW keys.
/// [`HipTfheMultiBitBlindRotate32`]: the u32 torus.
pub struct HipTfheMultiBitBlindRotate {
    h: *mut ffi::pfhe_tfhe_mbrot,
}
impl HipTfheMultiBitBlindRotate {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize,
               grouping_factor: usize) -> Result<Self, c_int> {
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe_mbrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor, 0, &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(e),
        }
    }
    /// `acc_dev`: batch x (k+1) x N words, updated in place; `bsk_dev`: groups x 2^g keys of (k+1) x ell x (k+1) x N complex
    /// values (`len_bsk` counts them); `exps_dev`: batch x groups*g exponents, taken modulo 2N
    pub unsafe fn rotate_dev(&mut self, acc_dev: *mut u64, len_acc: usize, bsk_dev: *const f64, len_bsk: usize,
                             exps_dev: *const u32, len_exps: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe_mbrot_rotate_dev(self.h, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheMultiBitBlindRotate {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe_mbrot_destroy(self.h) }
    }
}

pub struct HipTfheMultiBitBlindRotate32 {
    h: *mut ffi::pfhe_tfhe32_mbrot,
}
impl HipTfheMultiBitBlindRotate32 {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize,
               grouping_factor: usize) -> Result<Self, c_int> {
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe32_mbrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor, 0, &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(e),
        }
    }
    /// `acc_dev`: batch x (k+1) x N words, updated in place; `bsk_dev`: groups x 2^g keys of (k+1) x ell x (k+1) x N complex
    /// values (`len_bsk` counts them); `exps_dev`: batch x groups*g exponents, taken modulo 2N
    pub unsafe fn rotate_dev(&mut self, acc_dev: *mut u32, len_acc: usize, bsk_dev: *const f64, len_bsk: usize,
                             exps_dev: *const u32, len_exps: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe32_mbrot_rotate_dev(self.h, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheMultiBitBlindRotate32 {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe32_mbrot_destroy(self.h) }
    }
}

/// The batched programmable bootstrap around [`HipTfheBlindRotate`]: modulus switch, `ACC = X^{-b~} * TV`, the blind
/// rotation over `lwe_dimension` steps, sample extraction at index 0 and, with a key switch, the switch back to
/// `lwe_dimension`, all queued on the caller's stream.  Takes [`HipTfheBlindRotate`]'s arguments plus the LWE dimension and
/// the key-switch basis; owns its rotation handle and every buffer between the stages.
/// [`HipTfheBootstrap32`]: the u32 torus.
pub struct HipTfheBootstrap {
    h: *mut ffi::pfhe_tfhe_bootstrap_handle,
}
impl HipTfheBootstrap {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize, lwe_dimension: usize,
               ks_log_basis: u32, ks_decompose_length: usize, with_keyswitch: bool) -> Result<Self, c_int> {
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe_bootstrap_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension,
                                                       ks_log_basis, ks_decompose_length, with_keyswitch as c_int, 0, &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(e),
        }
    }
    /// `lwe_in_dev`: batch x (n+1) words; `bsk_dev`: n Fourier GGSW keys (`len_bsk` counts complex values); `tv_dev`: one
    /// GLWE test vector or one per ciphertext; `ksk_dev`: k*N x ell x (n+1) words, null with `len_ksk` 0 without a key
    /// switch; `lwe_out_dev`: batch x (n+1) words (batch x (k*N+1) without a key switch), disjoint from every input
    pub unsafe fn bootstrap_dev(&mut self, lwe_in_dev: *const u64, len_in: usize, bsk_dev: *const f64, len_bsk: usize,
                                tv_dev: *const u64, len_tv: usize, ksk_dev: *const u64, len_ksk: usize, lwe_out_dev: *mut u64,
                                len_out: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe_bootstrap_dev(self.h, lwe_in_dev, len_in, bsk_dev, len_bsk, tv_dev, len_tv, ksk_dev,
                                                    len_ksk, lwe_out_dev, len_out, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheBootstrap {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe_bootstrap_destroy(self.h) }
    }
}

/// The stateless steps of a bootstrap on the u64 torus: the project's own modulus switch (the reference has none), sample
/// extraction (`Rlwe::extract_lwe_with_index`, rlwe/coeff.rs:194-227, per mask polynomial) and the LWE key switch
/// (`Lwe::add_mul_scalar_assign`, lwe/single_message.rs:262-268, with `ApproxSignedBasis`'s digits).
pub unsafe fn tfhe_modswitch_dev(device: c_int, lwe_dev: *const u64, len_lwe: usize, lwe_dimension: usize, log_n: u32,
                                 exps_dev: *mut u32, len_exps: usize, neg_b_dev: *mut u32, len_neg_b: usize,
                                 stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_modswitch_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, exps_dev, len_exps, neg_b_dev,
                                                len_neg_b, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe_sample_extract_dev(fft: &HipFftTable, glwe_dimension: usize, glwe_dev: *const u64, len_glwe: usize,
                                      index: usize, lwe_dev: *mut u64, len_lwe: usize, stream: *mut core::ffi::c_void)
                                      -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_sample_extract_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, index, lwe_dev, len_lwe,
                                                     stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe_keyswitch_dev(device: c_int, lwe_in_dev: *const u64, len_in: usize, in_dimension: usize,
                                 ksk_dev: *const u64, len_ksk: usize, out_dimension: usize, log_basis: u32,
                                 decompose_length: usize, lwe_out_dev: *mut u64, len_out: usize,
                                 stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_keyswitch_dev(device, lwe_in_dev, len_in, in_dimension, ksk_dev, len_ksk, out_dimension,
                                                log_basis, decompose_length, lwe_out_dev, len_out, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}

pub struct HipTfheBootstrap32 {
    h: *mut ffi::pfhe_tfhe32_bootstrap_handle,
}
impl HipTfheBootstrap32 {
    pub fn new(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize, lwe_dimension: usize,
               ks_log_basis: u32, ks_decompose_length: usize, with_keyswitch: bool) -> Result<Self, c_int> {
        let mut h = core::ptr::null_mut();
        match unsafe { ffi::pfhe_tfhe32_bootstrap_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension,
                                                       ks_log_basis, ks_decompose_length, with_keyswitch as c_int, 0, &mut h) } {
            ffi::PFHE_OK => Ok(Self { h }),
            e => Err(e),
        }
    }
    /// `lwe_in_dev`: batch x (n+1) words; `bsk_dev`: n Fourier GGSW keys (`len_bsk` counts complex values); `tv_dev`: one
    /// GLWE test vector or one per ciphertext; `ksk_dev`: k*N x ell x (n+1) words, null with `len_ksk` 0 without a key
    /// switch; `lwe_out_dev`: batch x (n+1) words (batch x (k*N+1) without a key switch), disjoint from every input
    pub unsafe fn bootstrap_dev(&mut self, lwe_in_dev: *const u32, len_in: usize, bsk_dev: *const f64, len_bsk: usize,
                                tv_dev: *const u32, len_tv: usize, ksk_dev: *const u32, len_ksk: usize, lwe_out_dev: *mut u32,
                                len_out: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
        match unsafe { ffi::pfhe_tfhe32_bootstrap_dev(self.h, lwe_in_dev, len_in, bsk_dev, len_bsk, tv_dev, len_tv, ksk_dev,
                                                    len_ksk, lwe_out_dev, len_out, stream) } {
            ffi::PFHE_OK => Ok(()),
            e => Err(e),
        }
    }
}
impl Drop for HipTfheBootstrap32 {
    fn drop(&mut self) {
        unsafe { ffi::pfhe_tfhe32_bootstrap_destroy(self.h) }
    }
}

/// The stateless steps of a bootstrap on the u32 torus: the project's own modulus switch (the reference has none), sample
/// extraction (`Rlwe::extract_lwe_with_index`, rlwe/coeff.rs:194-227, per mask polynomial) and the LWE key switch
/// (`Lwe::add_mul_scalar_assign`, lwe/single_message.rs:262-268, with `ApproxSignedBasis`'s digits).
pub unsafe fn tfhe32_modswitch_dev(device: c_int, lwe_dev: *const u32, len_lwe: usize, lwe_dimension: usize, log_n: u32,
                                 exps_dev: *mut u32, len_exps: usize, neg_b_dev: *mut u32, len_neg_b: usize,
                                 stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_modswitch_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, exps_dev, len_exps, neg_b_dev,
                                                len_neg_b, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe32_sample_extract_dev(fft: &HipFftTable, glwe_dimension: usize, glwe_dev: *const u32, len_glwe: usize,
                                      index: usize, lwe_dev: *mut u32, len_lwe: usize, stream: *mut core::ffi::c_void)
                                      -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_sample_extract_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, index, lwe_dev, len_lwe,
                                                     stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe32_keyswitch_dev(device: c_int, lwe_in_dev: *const u32, len_in: usize, in_dimension: usize,
                                 ksk_dev: *const u32, len_ksk: usize, out_dimension: usize, log_basis: u32,
                                 decompose_length: usize, lwe_out_dev: *mut u32, len_out: usize,
                                 stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_keyswitch_dev(device, lwe_in_dev, len_in, in_dimension, ksk_dev, len_ksk, out_dimension,
                                                log_basis, decompose_length, lwe_out_dev, len_out, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}

/// Key generation, encryption and phase for the bootstrap on the u64 torus.  No random number is drawn: the buffers arrive
/// holding the caller's randomness (masks uniform, bodies noise + message).  The body calls are
/// `Lwe::generate_random_zero_sample` (lwe/single_message.rs:94-125) and `Rlwe::generate_random_zero_sample`
/// (rlwe/coeff.rs:92-121) without their sampling, with `subtract` the phase; the gadget term and the two key generators
/// have no reference counterpart.  `grouping_factor` 0: the classic key layout, 1..4: the multi-bit one.
pub unsafe fn tfhe_lwe_body_mac_dev(device: c_int, lwe_dev: *mut u64, len_lwe: usize, dimension: usize, key_dev: *const u64,
                                  len_key: usize, subtract: bool, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_lwe_body_mac_dev(device, lwe_dev, len_lwe, dimension, key_dev, len_key, subtract as c_int, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe_glwe_body_mac_dev(fft: &HipFftTable, glwe_dimension: usize, glwe_dev: *mut u64, len_glwe: usize,
                                   key_dev: *const u64, len_key: usize, subtract: bool, stream: *mut core::ffi::c_void)
                                   -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_glwe_body_mac_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, key_dev, len_key,
                                                 subtract as c_int, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe_ggsw_add_gadget_dev(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize,
                                     ggsw_dev: *mut u64, len_ggsw: usize, messages_dev: *const u64, len_messages: usize,
                                     stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_ggsw_add_gadget_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, ggsw_dev, len_ggsw,
                                                   messages_dev, len_messages, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe_bsk_generate_dev(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize,
                                  grouping_factor: usize, lwe_key_dev: *const u64, lwe_dimension: usize,
                                  glwe_key_dev: *const u64, len_glwe_key: usize, ggsw_torus_dev: *mut u64, len_ggsw: usize,
                                  bsk_out_dev: *mut f64, len_bsk: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_bsk_generate_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor,
                                                lwe_key_dev, lwe_dimension, glwe_key_dev, len_glwe_key, ggsw_torus_dev, len_ggsw,
                                                bsk_out_dev, len_bsk, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe_ksk_generate_dev(device: c_int, key_in_dev: *const u64, in_dimension: usize, key_out_dev: *const u64,
                                  out_dimension: usize, log_basis: u32, decompose_length: usize, ksk_dev: *mut u64,
                                  len_ksk: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe_ksk_generate_dev(device, key_in_dev, in_dimension, key_out_dev, out_dimension, log_basis,
                                                decompose_length, ksk_dev, len_ksk, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}

/// The same calls on the u32 torus.
pub unsafe fn tfhe32_lwe_body_mac_dev(device: c_int, lwe_dev: *mut u32, len_lwe: usize, dimension: usize, key_dev: *const u32,
                                  len_key: usize, subtract: bool, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_lwe_body_mac_dev(device, lwe_dev, len_lwe, dimension, key_dev, len_key, subtract as c_int, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe32_glwe_body_mac_dev(fft: &HipFftTable, glwe_dimension: usize, glwe_dev: *mut u32, len_glwe: usize,
                                   key_dev: *const u32, len_key: usize, subtract: bool, stream: *mut core::ffi::c_void)
                                   -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_glwe_body_mac_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, key_dev, len_key,
                                                 subtract as c_int, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe32_ggsw_add_gadget_dev(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize,
                                     ggsw_dev: *mut u32, len_ggsw: usize, messages_dev: *const u32, len_messages: usize,
                                     stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_ggsw_add_gadget_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, ggsw_dev, len_ggsw,
                                                   messages_dev, len_messages, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe32_bsk_generate_dev(fft: &HipFftTable, glwe_dimension: usize, log_basis: u32, decompose_length: usize,
                                  grouping_factor: usize, lwe_key_dev: *const u32, lwe_dimension: usize,
                                  glwe_key_dev: *const u32, len_glwe_key: usize, ggsw_torus_dev: *mut u32, len_ggsw: usize,
                                  bsk_out_dev: *mut f64, len_bsk: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_bsk_generate_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor,
                                                lwe_key_dev, lwe_dimension, glwe_key_dev, len_glwe_key, ggsw_torus_dev, len_ggsw,
                                                bsk_out_dev, len_bsk, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
pub unsafe fn tfhe32_ksk_generate_dev(device: c_int, key_in_dev: *const u32, in_dimension: usize, key_out_dev: *const u32,
                                  out_dimension: usize, log_basis: u32, decompose_length: usize, ksk_dev: *mut u32,
                                  len_ksk: usize, stream: *mut core::ffi::c_void) -> Result<(), c_int> {
    match unsafe { ffi::pfhe_tfhe32_ksk_generate_dev(device, key_in_dev, in_dimension, key_out_dev, out_dimension, log_basis,
                                                decompose_length, ksk_dev, len_ksk, stream) } {
        ffi::PFHE_OK => Ok(()),
        e => Err(e),
    }
}
