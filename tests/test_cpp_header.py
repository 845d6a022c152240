"""The C++ mirror (include/pfhe.hpp) compiles against the C ABI and links to libpfhe_hip.so;
without a GPU its constructors report NoDevice through pfhe::Error (no CPU fallback)."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include <cstdio>
#include "pfhe.hpp"
int main() {
    try {
        pfhe::U64DcrtTable t(10, {2305843009211596801ull, 2305843009210023937ull, 2305843009208713217ull});
        std::vector<uint64_t> a(3 * 1024, 1), b = a;
        t.transform_slice(a.data(), a.size());
        t.inverse_transform_slice(a.data(), a.size());
        pfhe::U32DcrtTable t32(10, {1073479681u, 1071513601u});
        std::vector<uint32_t> c(2 * 1024, 7), d = c;
        t32.transform_slice(c.data(), c.size());
        t32.inverse_transform_slice(c.data(), c.size());
        pfhe::RNSBase in({17, 19, 23}), out2({29, 31});
        pfhe::BaseConverter conv(in, out2);
        std::vector<uint64_t> res = {1, 2, 3}, conv_out(2);   // one coefficient, residues (1,2,3)
        conv.fast_convert_array(res.data(), 3, conv_out.data(), 2, 1);
        // the <u32> operators: compose(decompose(v)) == v over a nine-modulus base (constants in a device table),
        // and an external product with a zero GGSW is zero
        pfhe::RNSBase32 wide({1073707009u, 1073698817u, 1073692673u, 1073682433u, 1073668097u, 1073655809u, 1073651713u,
                              1073643521u, 1073620993u});
        const size_t wl = wide.big_uint_value_len();
        std::vector<uint32_t> big(4 * wl, 0), res32(9 * 4), back(4 * wl, 1);
        for (size_t i = 0; i < 4; ++i) { big[i * wl] = 12345u + (uint32_t)i; big[i * wl + 1] = 99u * (uint32_t)i; }
        wide.decompose_big_uint_values_to(big.data(), big.size(), res32.data(), res32.size(), 4);
        wide.compose_multiple_values_to(res32.data(), res32.size(), back.data(), back.size(), 4);
        pfhe::RNSBase32 in32({17u, 19u, 23u}), out32b({29u, 31u});
        pfhe::BaseConverter32 conv32(in32, out32b);
        std::vector<uint32_t> r32 = {1, 2, 3}, c32(2);
        conv32.fast_convert_array(r32.data(), 3, c32.data(), 2, 1);
        const bool conv32_ok = conv32.output_moduli_count() == 2 && c32[0] < 29 && c32[1] < 31;
        pfhe::RNSBase32 base32({1073479681u, 1071513601u});
        pfhe::BigUintApproxSignedBasis32 basis32(base32, 20);
        pfhe::DcrtGlevContext32 ctx32(t32, base32, basis32);
        const size_t ell32 = basis32.decompose_length(), cl = t32.crt_poly_length();
        std::vector<uint32_t> glwe32(2 * cl, 5), ggsw32(2 * ell32 * 2 * cl, 0), out32(2 * cl, 9);
        pfhe::mul_dcrt_ggsw_to(glwe32.data(), glwe32.size(), ggsw32.data(), ggsw32.size(), out32.data(), out32.size(), ctx32);
        bool u32_ok = conv32_ok && big == back && wide.moduli_count() == 9 && !ctx32.in_use();
        for (uint32_t w : out32) u32_ok = u32_ok && w == 0;
        // element-wise family on device buffers: ((a + b) - b) * X^5 * X^(2N-5) == a, and -(-a) == a
        void *da = nullptr, *db = nullptr, *dx = nullptr;
        const size_t bytes = a.size() * sizeof(uint64_t);
        pfhe::check(pfhe_device_malloc(0, bytes, &da));
        pfhe::check(pfhe_device_malloc(0, bytes, &db));
        pfhe::check(pfhe_device_malloc(0, bytes, &dx));
        std::vector<uint64_t> e(a.size());
        for (size_t i = 0; i < e.size(); ++i) e[i] = 1000003ull * i + 17;
        pfhe::check(pfhe_memcpy_h2d(0, da, e.data(), bytes, nullptr));
        pfhe::check(pfhe_memcpy_h2d(0, db, b.data(), bytes, nullptr));
        uint64_t *pa = (uint64_t *)da, *pb = (uint64_t *)db, *px = (uint64_t *)dx;
        t.add_to_dev(pa, pb, px, e.size());
        t.sub_to_dev(px, pb, px, e.size());
        t.mul_monomial_assign_dev(px, 5, e.size());
        t.mul_monomial_to_dev(px, 2 * 1024 - 5, pb, e.size());
        t.neg_to_dev(pb, pb, e.size());
        t.neg_to_dev(pb, pb, e.size());
        t.mul_scalar_to_dev(pb, {2, 2, 2}, px, e.size());
        std::vector<uint64_t> f(e.size());
        pfhe::check(pfhe_memcpy_d2h(0, f.data(), dx, bytes, nullptr));
        bool ew_ok = true;
        for (size_t i = 0; i < e.size(); ++i) ew_ok = ew_ok && f[i] == 2 * e[i];
        pfhe_device_free(0, da); pfhe_device_free(0, db); pfhe_device_free(0, dx);
        const bool ok = ew_ok && u32_ok && a == b && c == d && conv.input_moduli_count() == 3 && conv_out[0] < 29 && conv_out[1] < 31;
        std::printf(ok ? "roundtrip ok\n" : "roundtrip MISMATCH\n");
        return ok ? 0 : 1;
    } catch (const pfhe::Error &e) {
        std::printf("pfhe::Error %d: %s\n", e.status(), e.what());
        return e.status() == PFHE_ERR_NO_DEVICE ? 42 : 2;
    }
}
'''


def test_cpp_mirror_compiles_and_runs():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    import primus_fhe_amd as p
    lib_dir = os.path.dirname(p.library_path())
    if not os.path.exists(p.library_path()):
        pytest.skip("libpfhe_hip.so not built")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write(SRC)
        exe = os.path.join(d, "t")
        subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib_dir, "-lpfhe_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        import torch
        if torch.cuda.is_available():
            assert r.returncode == 0 and "roundtrip ok" in r.stdout, r.stdout + r.stderr
        else:
            assert r.returncode == 42 and "NO_DEVICE" not in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mirror_on_gpu():
    """The same program on the GPU box: transforms, base conversion and the element-wise family round-trip."""
    test_cpp_mirror_compiles_and_runs()


# The torus side of the mirror, written once over the word type and run for both: log N = 3, k = 1, log_basis 8, two
# levels, a batch of 2 — the smallest shape at which every index of the layouts is distinct.  Every expectation is exact.
TORUS_SRC = r'''
#include <cstdio>
#include "pfhe.hpp"

template <class W>
struct DeviceWords {   // a device buffer of words, filled from the host
    explicit DeviceWords(const std::vector<W> &host) : bytes(host.size() * sizeof(W)) {
        pfhe::check(pfhe_device_malloc(0, bytes, &p));
        pfhe::check(pfhe_memcpy_h2d(0, p, host.data(), bytes, nullptr));
    }
    ~DeviceWords() { pfhe_device_free(0, p); }
    W *words() const { return static_cast<W *>(p); }
    std::vector<W> host() const {
        std::vector<W> out(bytes / sizeof(W));
        pfhe::check(pfhe_memcpy_d2h(0, out.data(), p, bytes, nullptr));
        return out;
    }
    size_t bytes;
    void *p = nullptr;
};

static bool expect(bool ok, const char *what, size_t bits) {
    if (!ok) std::printf("MISMATCH u%zu: %s\n", bits, what);
    return ok;
}

template <class W>
bool run() {
    const size_t bits = 8 * sizeof(W), n = 8, k = 1, ell = 2, batch = 2;
    const uint32_t log_basis = 8;
    const size_t glwe_len = batch * (k + 1) * n, key_len = (k + 1) * ell * (k + 1) * n;   // words; complex values
    bool ok = true;
    pfhe::FullComplex64FftTable fft(3);
    ok &= expect(fft.poly_length() == n && fft.fourier_length() == n, "table lengths", bits);

    // words below 2^20, all distinct
    std::vector<W> glwe(glwe_len);
    for (size_t i = 0; i < glwe_len; ++i) glwe[i] = static_cast<W>((40503u * (i + 1) + 977u) & 0xFFFFFu);

    // slices: forward then inverse is the identity
    std::vector<double> spectrum(2 * glwe_len, -1.0);
    std::vector<W> back(glwe_len, 1);
    fft.forward_torus_slice(glwe.data(), glwe.size(), spectrum.data(), glwe_len);
    fft.inverse_torus_slice(spectrum.data(), glwe_len, back.data(), back.size());
    ok &= expect(back == glwe, "forward_torus_slice then inverse_torus_slice", bits);

    // device buffers: the same
    {
        DeviceWords<W> in(glwe), out(std::vector<W>(glwe_len, 1));
        DeviceWords<double> mid(std::vector<double>(2 * glwe_len, -1.0));
        fft.forward_torus_dev(in.words(), glwe_len, mid.words(), glwe_len);
        fft.inverse_torus_dev(mid.words(), glwe_len, out.words(), glwe_len);
        ok &= expect(out.host() == glwe, "forward_torus_dev then inverse_torus_dev", bits);
    }

    // the product with an all-zero key is zero, and the context is free afterwards
    const std::vector<double> zero_key(2 * key_len, 0.0);
    {
        pfhe::TfheFftContextT<W> ctx(fft, k, log_basis, ell);
        std::vector<W> out(glwe_len, 9);
        pfhe::external_product_to(glwe.data(), glwe.size(), zero_key.data(), key_len, out.data(), out.size(), ctx);
        ok &= expect(out == std::vector<W>(glwe_len, 0), "external_product_to with a zero key", bits);
        ok &= expect(!ctx.in_use(), "in_use() after the product", bits);
    }

    // three steps of the blind rotation with all-zero keys leave the accumulator as it was
    {
        const size_t steps = 3;
        pfhe::TfheBlindRotateT<W> rot(fft, k, log_basis, ell);
        const std::vector<double> bsk(steps * 2 * key_len, 0.0);
        const std::vector<uint32_t> exps = {1, 5, 15, 0, 8, 9};   // batch x steps, below 2N
        std::vector<W> acc = glwe;
        rot.rotate(acc.data(), acc.size(), bsk.data(), steps * key_len, exps.data(), exps.size());
        ok &= expect(acc == glwe, "rotate with zero keys", bits);
        ok &= expect(!rot.in_use(), "in_use() after the rotation", bits);
    }

    // the CMUX with all-zero selectors returns d0
    {
        pfhe::TfheCmuxTreeT<W> tree(fft, k, log_basis, ell, 1);
        std::vector<W> d1(glwe_len), out(glwe_len, 3);
        for (size_t i = 0; i < glwe_len; ++i) d1[i] = static_cast<W>(~glwe[i]);
        const std::vector<double> keys(batch * 2 * key_len, 0.0);
        tree.cmux(glwe.data(), glwe.size(), d1.data(), d1.size(), keys.data(), batch * key_len, 1, out.data(), out.size());
        ok &= expect(out == glwe, "cmux with zero selectors", bits);
    }

    // the LWE key switch with an all-zero key returns (0, .., 0, b)
    {
        const size_t in_dim = k * n, out_dim = 3;
        std::vector<W> lwe(batch * (in_dim + 1)), out(batch * (out_dim + 1), 7);
        for (size_t i = 0; i < lwe.size(); ++i) lwe[i] = glwe[i];
        const std::vector<W> ksk(in_dim * ell * (out_dim + 1), 0);
        pfhe::lwe_keyswitch(0, lwe.data(), lwe.size(), in_dim, ksk.data(), ksk.size(), out_dim, log_basis, ell, out.data(),
                            out.size());
        std::vector<W> want(out.size(), 0);
        for (size_t e = 0; e < batch; ++e) want[e * (out_dim + 1) + out_dim] = lwe[e * (in_dim + 1) + in_dim];
        ok &= expect(out == want, "lwe_keyswitch with a zero key", bits);
    }

    // sample extraction at index 0: [a_0, -a_{N-1}, .., -a_1, b_0]
    {
        std::vector<W> lwe(batch * (k * n + 1), 5), want(lwe.size());
        pfhe::glwe_sample_extract(fft, k, glwe.data(), glwe.size(), 0, lwe.data(), lwe.size());
        for (size_t e = 0; e < batch; ++e) {
            const W *a = glwe.data() + e * 2 * n, *b = a + n;
            W *w = want.data() + e * (n + 1);
            w[0] = a[0];
            for (size_t i = 1; i < n; ++i) w[i] = static_cast<W>(0 - a[n - i]);
            w[n] = b[0];
        }
        ok &= expect(lwe == want, "glwe_sample_extract at index 0", bits);
    }

    // a moved-from handle destroys nothing: both objects go out of scope here
    {
        pfhe::TfheLutT<W> lut(fft, k, log_basis, ell, 1, 1);
        pfhe::TfheLutT<W> moved(std::move(lut));
        ok &= expect(moved.handle() != nullptr && lut.handle() == nullptr, "the move takes the handle", bits);
        pfhe::FullComplex64FftTable other(3);
        pfhe::FullComplex64FftTable taken(std::move(other));
        ok &= expect(taken.poly_length() == n, "a moved table", bits);
    }
    return ok;
}

int main() {
    try {
        const bool ok64 = run<uint64_t>();
        const bool ok32 = run<uint32_t>();
        std::printf(ok64 && ok32 ? "torus mirror ok\n" : "torus mirror MISMATCH\n");
        return ok64 && ok32 ? 0 : 1;
    } catch (const pfhe::Error &e) {
        std::printf("pfhe::Error %d: %s\n", e.status(), e.what());
        return e.status() == PFHE_ERR_NO_DEVICE ? 42 : 2;
    }
}
'''


def test_cpp_mirror_uses_the_c_functions_it_used_before_the_widths_were_folded():
    """Every class template for both word types and every free function template once per word type, compiled only: the
    pfhe_* symbols left undefined are the committed list, none missing and none extra.  The handle types are distinct and
    the prototypes typed, so an entry bound to another handle's function or a changed argument fails this compile."""
    import cpp_mirror
    want = cpp_mirror.mirror_symbols()
    assert len(want) == 306
    got = cpp_mirror.undefined_pfhe_symbols(cpp_mirror.INSTANTIATE)
    assert got == want, (sorted(want - got), sorted(got - want))


def test_cpp_torus_mirror_compiles_and_runs():
    import cpp_mirror
    r = cpp_mirror.build_and_run(TORUS_SRC)
    import torch
    if torch.cuda.is_available():
        assert r.returncode == 0 and "torus mirror ok" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 42 and "NO_DEVICE" not in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_torus_mirror_on_gpu():
    """The torus program on the GPU box, for uint64_t and uint32_t: the transforms round-trip on slices and on device
    buffers, zero keys leave the product zero, the accumulator and d0 as they are, the key switch returns (0, .., 0, b),
    sample extraction at index 0 is [a_0, -a_{N-1}, .., -a_1, b_0], and a moved-from handle destroys nothing."""
    test_cpp_torus_mirror_compiles_and_runs()
