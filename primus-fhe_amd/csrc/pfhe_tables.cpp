// pfhe_tables.cpp — construction of a TableSet for both widths: the host tables of every modulus (pfhe_hosttables.cpp),
// brought into the forms the transforms read and uploaded.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pfhe_capi_internal.hpp"
#include "pfhe_common.hpp"
#include "pfhe_handles.hpp"
#include "pfhe_staging.hpp"

namespace pfhe {

// One device table: as many elements as `v` holds, allocated into the table's own typed pointer and filled from `v`.
template <class V, class T>
static int upload(TableSet &ts, const V &v, T *&dst) {
    PFHE_TRY(ts.bufs.add(dst, v.size()));
    static_assert(sizeof(typename V::value_type) == sizeof(T), "the table's element is the vector's");
    PFHE_HIP(hipMemcpy((void *)dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PFHE_OK;
}

// The twiddles of the closing register pass, re-ordered so that the 64 lanes of a wave load 64 consecutive entries
// (NttPrime::fwd_last / inv_last, fwd_last_w / inv_last_w): entry (slot * G + g) belongs to group g of 16.
//
// u64 tables: the four stages at distances 8, 4, 2, 1 — 15 twiddles per group of 16 coefficients.
static void last_order(size_t n, const std::vector<ulonglong2> &fwd, const std::vector<ulonglong2> &inv,
                       std::vector<ulonglong2> &fl, std::vector<ulonglong2> &il) {
    const size_t groups = n / 16;
    fl.assign(15 * groups, ulonglong2{0, 0});
    il.assign(15 * groups, ulonglong2{0, 0});
    for (int j = 3; j >= 0; --j) {
        const size_t per = (size_t)8 >> j;  // twiddles per group at distance 2^j
        for (size_t u = 0; u < per; ++u)
            for (size_t g = 0; g < groups; ++g) {
                const size_t off = (per - 1 + u) * groups + g;
                fl[off] = fwd[(n >> (j + 1)) + g * per + u];
                il[off] = inv[1 + n - (n >> j) + g * per + u];
            }
    }
}

// u32 tables: a thread owns 16 consecutive WORDS (stages at word distances 8, 4, 2, 1: 15 twiddles per group of 16
// words) plus the intra-word stage (one twiddle per word: 16 more).  The gathers kept the u32 block pass at 3.6 TB/s
// whatever its instruction count.  Word units: nw = N/2 words per polynomial; pn / pi are the packed negated-forward and
// inverse tables.
static void last_order32(size_t nw, const std::vector<u64> &pn, const std::vector<u64> &pi, std::vector<u64> &fl,
                         std::vector<u64> &il) {
    const size_t G = nw / 16;
    fl.assign(31 * G, 0);
    il.assign(31 * G, 0);
    for (int j = 3; j >= 0; --j) {
        const size_t per = (size_t)8 >> j;
        for (size_t u = 0; u < per; ++u)
            for (size_t g = 0; g < G; ++g) {
                const size_t off = (per - 1 + u) * G + g;
                fl[off] = pn[(nw >> (j + 1)) + g * per + u];
                il[off] = pi[nw + 1 + nw - (nw >> j) + g * per + u];
            }
    }
    for (size_t k = 0; k < 16; ++k)
        for (size_t g = 0; g < G; ++g) {
            fl[(15 + k) * G + g] = pn[nw + 16 * g + k];  // fwd_intra: roots[N/2 + word]
            il[(15 + k) * G + g] = pi[1 + 16 * g + k];   // inv_intra: inv_roots[1 + word]
        }
}

// Builds host tables for every modulus, uploads them, and fills `out`.
int make_table_set(u32 log_n, const u64 *moduli, size_t count, int device, std::unique_ptr<TableSet> &out) {
    if (count == 0) {
        set_last_error("empty modulus list");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    std::vector<HostTable> host(count);
    for (size_t i = 0; i < count; ++i) PFHE_TRY(build_host_table(log_n, moduli[i], host[i]));
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;

    auto ts = std::make_unique<TableSet>();
    ts->device = device;
    ts->log_n = log_n;
    ts->n = (size_t)1 << log_n;
    ts->L = (u32)count;
    ts->primes.resize(count);
    ts->tune = NttTuning::from_env();
    bool all_pm = std::getenv("PFHE_DISABLE_PM") == nullptr;  // tuning switch: force the generic path
    bool all_mont = std::getenv("PFHE_DISABLE_MONT") == nullptr;  // tuning switch: generic primes keep the Shoup transforms
    for (size_t i = 0; i < count; ++i) {
        u32 pk = 0;
        u64 pc = 0;
        if (!pm_shape(host[i].q, pk, pc)) all_pm = false;
        if (!mont_shape(host[i].q)) all_mont = false;
    }
    const bool use_mont = !all_pm && all_mont && log_n >= 4;
    ts->bufs.bind(device);
    for (size_t i = 0; i < count; ++i) {
        NttPrime &P = ts->primes[i];
        std::memset(&P, 0, sizeof P);
        PFHE_TRY(upload(*ts, host[i].fwd, P.fwd));
        PFHE_TRY(upload(*ts, host[i].inv, P.inv));
        P.q = host[i].q;
        P.two_q = host[i].q << 1;
        P.q3 = 3 * host[i].q;
        P.inv_n = host[i].inv_n;
        P.inv_n_p = (u64)(((unsigned __int128)host[i].inv_n << 64) / host[i].q);
        P.inv_n_w = host[i].inv_n_w;
        P.inv_n_w_p = (u64)(((unsigned __int128)host[i].inv_n_w << 64) / host[i].q);
        P.bar_lo = host[i].bar_lo;
        P.bar_hi = host[i].bar_hi;
        u32 pk = 0;
        u64 pc = 0;
        P.pm_k = pm_shape(P.q, pk, pc) ? pk : 0;
        P.pm_c = P.pm_k ? pc : 0;
        std::vector<ulonglong2> fl, il;
        if (P.pm_k) {
            // {w, w * 2^32 mod q}: the twiddle product of PmArith splits the multiplicand, not the twiddle
            const auto shifted = [&](u64 w) { return (u64)(((unsigned __int128)w << 32) % P.q); };
            std::vector<ulonglong2> fw(ts->n), iw(ts->n);
            for (size_t k = 0; k < ts->n; ++k) {
                fw[k] = ulonglong2{host[i].fwd[k].x, shifted(host[i].fwd[k].x)};
                iw[k] = ulonglong2{host[i].inv[k].x, shifted(host[i].inv[k].x)};
            }
            PFHE_TRY(upload(*ts, fw, P.fwd_p));
            PFHE_TRY(upload(*ts, iw, P.inv_p));
            P.inv_n_2 = shifted(P.inv_n);
            P.inv_n_w_2 = shifted(P.inv_n_w);
            if (all_pm && log_n >= 4) last_order(ts->n, fw, iw, fl, il);
        }
        if (!all_pm && log_n >= 4) last_order(ts->n, host[i].fwd, host[i].inv, fl, il);
        if (use_mont) {
            // {w * 2^32 mod q, w * 2^64 mod q}: the one-word Montgomery product of MontArith (pfhe_mont_asm.hpp)
            const u64 q = P.q;
            const auto mform = [&](u64 w) {
                const u64 a = (u64)(((unsigned __int128)w << 32) % q);
                return ulonglong2{a, (u64)(((unsigned __int128)a << 32) % q)};
            };
            std::vector<ulonglong2> fm(ts->n), im(ts->n), flm, ilm;
            for (size_t k = 0; k < ts->n; ++k) {
                fm[k] = mform(host[i].fwd[k].x);
                im[k] = mform(host[i].inv[k].x);
            }
            last_order(ts->n, fm, im, flm, ilm);
            PFHE_TRY(upload(*ts, fm, P.fwd_m));
            PFHE_TRY(upload(*ts, im, P.inv_m));
            PFHE_TRY(upload(*ts, flm, P.fwd_last_m));
            PFHE_TRY(upload(*ts, ilm, P.inv_last_m));
            const ulonglong2 nm = mform(P.inv_n), nwm = mform(P.inv_n_w);
            P.inv_n_m = nm.x, P.inv_n_m2 = nm.y, P.inv_n_w_m = nwm.x, P.inv_n_w_m2 = nwm.y;
            u32 inv = 1;  // Newton: q^-1 mod 2^32
            for (int it = 0; it < 5; ++it) inv *= 2u - (u32)q * inv;
            P.qinv32 = 0u - inv;
            P.mont_qest = (u32)((1ull << (63 - __builtin_clzll(q))) / ((q >> 32) + 1));
            P.mont_qf = ((1ull << 63) / q) * q;
        }
        if (!fl.empty()) {
            PFHE_TRY(upload(*ts, fl, P.fwd_last));
            PFHE_TRY(upload(*ts, il, P.inv_last));
        }
        ts->roots.push_back(host[i].root);
        ts->inv_roots.push_back(host[i].inv_root);
    }
    ts->pm = all_pm;
    ts->ntt_arith = all_pm ? kArithPm : (use_mont ? kArithMont : kArithShoup);
    PFHE_TRY(upload(*ts, ts->primes, ts->primes_dev));
    PFHE_TRY(upload(*ts, std::vector<u64>(moduli, moduli + count), ts->moduli_dev));
    out = std::move(ts);
    return PFHE_OK;
}

// U32NttTable::new for every modulus (table.rs:184-333), uploaded in the packed layout B32Arith
// reads: one 64-bit entry {w, floor(w*2^32/q)} per twiddle.
int make_table_set32(u32 log_n, const u32 *moduli, size_t count, int device, std::unique_ptr<TableSet> &out) {
    if (count == 0 || !moduli) {
        set_last_error("empty modulus list");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    std::vector<HostTable> host(count);
    for (size_t i = 0; i < count; ++i) {
        // root search first (table.rs:189), then the q < 2^30 requirement (:195-200)
        PFHE_TRY(build_host_table(log_n, moduli[i], host[i]));
        if (moduli[i] >= (1u << 30)) {
            set_last_error("modulus is too large for a u32 NTT table (max 30 bits)");
            return PFHE_ERR_MODULUS_TOO_LARGE;
        }
    }
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;

    auto ts = std::make_unique<TableSet>();
    ts->device = device;
    ts->log_n = log_n;
    ts->n = (size_t)1 << log_n;
    ts->L = (u32)count;
    ts->tune = NttTuning::from_env();  // u32 tables read the tuning switches at creation too
    ts->primes.resize(count);
    const size_t n = ts->n;
    ts->bufs.bind(device);
    for (size_t i = 0; i < count; ++i) {
        const u64 q = host[i].q;
        NttPrime &P = ts->primes[i];
        std::memset(&P, 0, sizeof P);
        P.q = q;
        P.two_q = q << 1;
        P.inv_n = host[i].inv_n;
        P.inv_n_p = (host[i].inv_n << 32) / q;
        P.inv_n_w = host[i].inv_n_w;
        P.inv_n_w_p = (host[i].inv_n_w << 32) / q;
        P.bar_lo = (u64)(((unsigned __int128)1 << 64) / q);
        const auto pack_of = [&](const std::vector<ulonglong2> &src, bool negate) {
            std::vector<u64> v(n);
            for (size_t k = 0; k < n; ++k)
                v[k] = (negate ? (u64)(u32)(0u - (u32)src[k].x) : src[k].x) | (((src[k].x << 32) / q) << 32);
            return v;
        };
        // forward, inverse, forward with the twiddle negated (B32Arith::mul1_neg)
        const std::vector<u64> pf = pack_of(host[i].fwd, false), pi = pack_of(host[i].inv, false), pn = pack_of(host[i].fwd, true);
        const u64 *dinv = nullptr;
        PFHE_TRY(upload(*ts, pf, P.fwd_w));
        PFHE_TRY(upload(*ts, pi, dinv));
        P.inv_w = dinv + n / 2;  // the word kernels index the inverse table in units of words: biased by N/2 entries
        PFHE_TRY(upload(*ts, pn, P.fwd_wn));
        if (n / 2 >= 16) {
            std::vector<u64> fl, il;
            last_order32(n / 2, pn, pi, fl, il);
            PFHE_TRY(upload(*ts, fl, P.fwd_last_w));
            PFHE_TRY(upload(*ts, il, P.inv_last_w));
        }
        ts->roots.push_back(host[i].root);
        ts->inv_roots.push_back(host[i].inv_root);
    }
    PFHE_TRY(upload(*ts, ts->primes, ts->primes_dev));
    out = std::move(ts);
    return PFHE_OK;
}

}  // namespace pfhe
