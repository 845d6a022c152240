// pfhe_handles.hpp — what a table handle owns.
#pragma once
#include <memory>
#include <vector>

#include "pfhe_common.hpp"
#include "pfhe_device_buffers.hpp"
#include "pfhe_ntt_device.hpp"
#include "pfhe_pointwise.hpp"

namespace pfhe {

// One or more per-prime NTT tables living on one GPU (U64NttTable / U32NttTable = 1, U64DcrtTable / U32DcrtTable = L).
struct TableSet {
    int device = 0;
    u32 log_n = 0;
    size_t n = 1;
    u32 L = 0;
    bool pm = false;                       // every prime has the pseudo-Mersenne shape
    int ntt_arith = 0;                     // policy of the plain transforms: kArithPm, kArithMont (generic primes below 2^61) or kArithShoup
    // tuning switches, read from the environment once, when the handle is created
    NttTuning tune;
    std::vector<NttPrime> primes;          // host copies (device pointers inside)
    const NttPrime *primes_dev = nullptr;  // the same array on the device
    const u64 *moduli_dev = nullptr;
    std::vector<u64> roots, inv_roots;
    DeviceBuffers bufs;                    // every device table above
};

// The four table handles of the C ABI (pfhe_ntt, pfhe_dcrt, pfhe_ntt32, pfhe_dcrt32: pfhe_capi_internal.hpp) are empty
// structs over this one.
struct TableHandle {
    std::unique_ptr<TableSet> t;
};

// Table construction for both widths (pfhe_tables.cpp).
int make_table_set(u32 log_n, const u64 *moduli, size_t count, int device, std::unique_ptr<TableSet> &out);
int make_table_set32(u32 log_n, const u32 *moduli, size_t count, int device, std::unique_ptr<TableSet> &out);

// The host layer of the tables, one definition over the word type W (u64 or u32): pfhe_capi.hip, except
// transform_host (pfhe_staging.cpp, next to the staging code it drives).
int check_len(const TableSet &t, size_t len, u64 &units);  // len must be a multiple (0 included) of the unit, L*N words
template <class W> int transform_dev(const TableSet &t, W *data, size_t len, bool inverse, bool lazy, hipStream_t s);
template <class W> int transform_host(const TableSet &t, W *host, size_t len, bool inverse, bool lazy);
// mode 0: acc = acc*b; mode 1: acc = a*b + acc
template <class W>
int pointwise(const TableSet &t, int mode, W *acc, const W *a, size_t len_a, const W *b, size_t len_b, hipStream_t s);
// minus_one: the coefficient of limb i is q_i - 1 (DcrtTable::transform_coeff_minus_one_monomial,
// primus_ntt/src/dcrt/mod.rs:124-134); otherwise `coeff` for every limb.
template <class W>
int monomial(const TableSet &t, W coeff, size_t degree, W *values, size_t len, bool host, hipStream_t s,
             bool minus_one = false);

// What is specific to a width: which launcher runs (the u32 ones sit with their kernels in pfhe_u32.hip) and the
// quotient word of MonomialScalars (the u32 kernel reduces with the table's Barrett constant and reads none).
inline int launch_transform(const TableSet &t, u64 *data, u64 npolys, bool inverse, bool lazy, hipStream_t s) {
    return inverse ? ntt_inverse_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, data, npolys, lazy, s, t.tune)
                   : ntt_forward_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, data, npolys, lazy, s, t.tune);
}
inline int launch_transform(const TableSet &t, u32 *data, u64 npolys, bool inverse, bool lazy, hipStream_t s) {
    return ntt32_transform_dev(t.primes_dev, t.L, t.log_n, data, npolys, inverse, lazy, s, t.tune);
}
inline int launch_pointwise(const TableSet &t, int mode, u64 *acc, const u64 *a, const u64 *b, u64 len, u64 len_b,
                            hipStream_t s) {
    return mode == 0 ? pointwise_dev(acc, acc, b, nullptr, t.primes_dev, t.L, t.log_n, len, len_b, s, 0, t.pm)
                     : pointwise_dev(acc, a, b, acc, t.primes_dev, t.L, t.log_n, len, len_b, s, 0, t.pm);
}
int launch_pointwise(const TableSet &t, int mode, u32 *acc, const u32 *a, const u32 *b, u64 len, u64 len_b, hipStream_t s);
inline int launch_monomial(u64 *out, const NttPrime *primes, u32 L, u32 log_n, u64 degree, const MonomialScalars &sc,
                           hipStream_t s) {
    return monomial_dev(out, primes, L, log_n, degree, sc, s);
}
int launch_monomial(u32 *out, const NttPrime *primes, u32 L, u32 log_n, u64 degree, const MonomialScalars &sc, hipStream_t s);
inline u64 monomial_quotient(u64 c, u64 q) { return (u64)(((unsigned __int128)c << 64) / q); }
inline u64 monomial_quotient(u32, u32) { return 0; }

}  // namespace pfhe
