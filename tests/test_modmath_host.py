"""barrett_reduce128 / mul_add_mod_barrett (primus-fhe_amd/csrc/pfhe_modmath.hpp) over the WHOLE 128-bit range, on the CPU.

The functions are PFHE_HD, so the host compiler builds the very code the kernels run; here it is compiled into a small shared
object (tests/support/modmath_host_shim.cpp, the recipe of test_oracle_sanitize.py without the sanitizers) and compared with
Python integers.  What this pins: the reduction is exact for EVERY (hi:lo), not only below q * 2^64 — dot_mod
(pfhe_convert.hip) hands it sums up to 2^128 - 1 and gadget_mulacc_kernel (pfhe_rns.hip) sums up to 2^127 with q * 2^64 as
small as 2^126 or less; there the quotient estimate no longer fits 64 bits and wraps, and the remainder must not notice.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from primes import ntt_primes_below
from pyref import Q61
from test_gpu_fuzz import pm_prime
from test_gpu_ntt import MULTIPASS_PRIMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
M64, M128 = (1 << 64) - 1, (1 << 128) - 1

# the 61-bit primes the suite uses: the three of BASELINE, the pseudo-Mersenne pair of the multi-pass plans, the wide bases'
# primes just below 2^61 and the pseudo-Mersenne prime with the largest admissible c
IN_USE_61 = list(Q61) + list(MULTIPASS_PRIMES["pm"]) + ntt_primes_below(32, 61, 4) + [pm_prime(61, 12, True)]
MODULI = [3, ntt_primes_below(1, 31, 4)[0], max(IN_USE_61), min(IN_USE_61), ntt_primes_below(1, 62, 0)[0]]
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    assert os.path.exists(CLANG), "ROCm's clang (hipcc's host compiler) is needed to build the shim"
    so = str(tmp_path_factory.mktemp("modmath") / "libmodmath_shim.so")
    cmd = [CLANG, "-std=c++17", "-O2", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I", os.path.join(ROOT, "primus-fhe_amd", "csrc"), os.path.join(ROOT, "tests", "support", "modmath_host_shim.cpp"),
           "-o", so]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return C.CDLL(so)


def arr(values):
    return np.array(values, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(u64p)


def ratio(q):
    mu = (1 << 128) // q     # fits 128 bits for q >= 2
    return C.c_uint64(q), C.c_uint64(mu & M64), C.c_uint64(mu >> 64)


def wide_inputs(q, rng):
    """128-bit operands: both ends, both sides of the documented precondition q * 2^64, multiples of q at the smallest
    quotient, at the first quotient whose estimate needs 64 bits and at the largest one, a full top word, random words."""
    xs = [0, M128, q * (1 << 64) - 1, q * (1 << 64), q * (1 << 64) + 1, M64 << 64, M128]
    for k in (1, M64, M128 // q):
        xs += [k * q - 1, k * q, k * q + 1]
    xs = [x for x in xs if 0 <= x <= M128]
    rnd = rng.integers(0, 1 << 64, (2, 100_000), dtype=np.uint64)
    lo = np.concatenate([arr([x & M64 for x in xs]), rnd[0]])
    hi = np.concatenate([arr([x >> 64 for x in xs]), rnd[1]])
    return xs, lo, hi


def test_the_moduli_are_the_sizes_named():
    assert [q.bit_length() for q in MODULI] == [2, 31, 61, 61, 62] and MODULI[2] > MODULI[3]


@pytest.mark.parametrize("q", MODULI)
def test_barrett_reduce128_is_exact_for_every_128_bit_value(shim, q):
    rng = np.random.default_rng(q % 1000)
    xs, lo, hi = wide_inputs(q, rng)
    # the table reaches past the precondition, and past the point where the quotient estimate wraps 64 bits
    assert any(x >= q << 64 for x in xs) and any(x // q > M64 for x in xs)
    out = np.empty_like(lo)
    shim.shim_barrett_reduce128(ptr(lo), ptr(hi), C.c_size_t(lo.size), *ratio(q), ptr(out))
    exp = arr([((int(h) << 64) | int(l)) % q for l, h in zip(lo, hi)])
    bad = np.nonzero(out != exp)[0]
    assert bad.size == 0, [(hex(int(hi[i])), hex(int(lo[i])), int(out[i]), int(exp[i])) for i in bad[:5]]


@pytest.mark.parametrize("q", MODULI)
def test_mul_add_mod_barrett_takes_any_64_bit_multiplicand(shim, q):
    """a up to 2^64 - 1 (the RAW transform outputs of the lazy forward passes are below 4q, not below q), b, c < q."""
    rng = np.random.default_rng(q % 1000 + 1)
    edge_a = [0, 1, q - 1, q, q + 1, 2 * q, 4 * q - 1, 4 * q, (1 << 63), M64 - 1, M64]
    edge_a = [a & M64 for a in edge_a]
    edge_bc = [0, 1, q // 2, q - 2, q - 1]
    trip = [(a, b, c) for a in edge_a for b in edge_bc for c in edge_bc]
    n = 100_000
    a = np.concatenate([arr([t[0] for t in trip]), rng.integers(0, 1 << 64, n, dtype=np.uint64)])
    b = np.concatenate([arr([t[1] for t in trip]), rng.integers(0, q, n, dtype=np.uint64)])
    c = np.concatenate([arr([t[2] for t in trip]), rng.integers(0, q, n, dtype=np.uint64)])
    out = np.empty_like(a)
    shim.shim_mul_add_mod_barrett(ptr(a), ptr(b), ptr(c), C.c_size_t(a.size), *ratio(q), ptr(out))
    exp = arr([(int(x) * int(y) + int(z)) % q for x, y, z in zip(a, b, c)])
    bad = np.nonzero(out != exp)[0]
    assert bad.size == 0, [(int(a[i]), int(b[i]), int(c[i]), int(out[i]), int(exp[i])) for i in bad[:5]]
    out2 = np.empty_like(a)
    shim.shim_mul_mod_barrett(ptr(a), ptr(b), C.c_size_t(a.size), *ratio(q), ptr(out2))
    assert np.array_equal(out2, arr([(int(x) * int(y)) % q for x, y in zip(a, b)]))
