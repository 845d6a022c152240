#!/usr/bin/env python3
"""TFHE external product (pfhe_tfhe{,32}_external_product_to_dev) and the standalone torus FFTs: products/s at batch 8192
and batch 1, forward / inverse transforms per second, and the RNS small-ring product (DcrtGlevContext, one 61-bit prime)
at the same N, k and ell beside it.  Prints one JSON object per row; `--json FILE` also writes them all."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402
from primus_fhe_amd._lib import check, u64p  # noqa: E402

SHAPES = [  # bits, log_n, k, log_basis, ell
    (32, 10, 1, 7, 3), (32, 10, 1, 10, 2), (32, 11, 1, 7, 3), (32, 11, 1, 10, 2),
    (64, 11, 1, 23, 1), (64, 11, 1, 15, 2),
    (64, 12, 1, 15, 2), (32, 10, 2, 7, 3),   # the general form
]
Q61 = 2305843009211596801


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def words(bits, count, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dt = torch.int32 if bits == 32 else torch.int64
    lo, hi = (-2 ** 31, 2 ** 31) if bits == 32 else (-2 ** 63, 2 ** 63 - 1)
    return torch.randint(lo, hi, (count,), dtype=dt, device="cuda", generator=g)


def tfhe_row(bits, log_n, k, lb, ell, batch):
    n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    ctx = p.TfheFftContext(fft, p.ApproxSignedBasis(bits, lb, ell), k)
    g = words(bits, ctx.key_len(), 2)
    key = torch.empty(ctx.key_len(), dtype=torch.complex128, device="cuda")
    fft.forward_torus_dev(g, key)
    x = words(bits, batch * (k + 1) * n, 1)
    out = torch.empty_like(x)
    dt = timed(lambda: p.tfhe_external_product_to_dev(x, key, out, ctx), 20 if batch > 1 else 500)
    row = {"what": "tfhe_extprod", "bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "batch": batch,
           "form": "fused" if ctx.scratch_bytes() == 0 else "general", "seconds": dt, "products_per_s": batch / dt}
    return row


def fft_rows(bits, log_n, batch):
    n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    x = words(bits, batch * n, 3)
    y = torch.empty(batch * n, dtype=torch.complex128, device="cuda")
    back = torch.empty_like(x)
    fwd = timed(lambda: fft.forward_torus_dev(x, y), 20)
    inv = timed(lambda: fft.inverse_torus_dev(y, back), 20)
    return [{"what": "fft_forward", "bits": bits, "log_n": log_n, "batch": batch, "seconds": fwd, "per_s": batch / fwd},
            {"what": "fft_inverse", "bits": bits, "log_n": log_n, "batch": batch, "seconds": inv, "per_s": batch / inv}]


def rns_row(log_n, k, ell, batch):
    """the RNS small-ring product, one 61-bit prime, log_basis chosen so that it has the same ell"""
    n = 1 << log_n
    t, base = p.U64DcrtTable(log_n, [Q61]), p.RNSBase([Q61])
    lb = next(b for b in range(1, 62) if p.BigUintApproxSignedBasis(base, b).decompose_length() <= ell)
    basis = p.BigUintApproxSignedBasis(base, lb)
    ctx = p.DcrtGlevContext(t, base, basis, k)
    mods = np.array([Q61], np.uint64)

    def fill(count, seed):
        x = torch.empty(count, dtype=torch.int64, device="cuda")
        check(p.lib().pfhe_fill_uniform_dev(0, C.c_void_p(x.data_ptr()), count, mods.ctypes.data_as(u64p), 1, n, seed, None))
        return x

    glwe, ggsw = fill(batch * (k + 1) * n, 1), fill(ctx.ggsw_len(), 2)
    out = torch.empty_like(glwe)
    dt = timed(lambda: p.mul_dcrt_ggsw_to_dev(glwe, ggsw, out, ctx, into_coeff_form=True), 20 if batch > 1 else 500)
    return {"what": "rns_extprod", "log_n": log_n, "k": k, "log_basis": lb, "ell": basis.decompose_length(), "batch": batch,
            "seconds": dt, "products_per_s": batch / dt}


def main():
    rows = []
    for bits, log_n, k, lb, ell in SHAPES:
        for batch in (8192, 1):
            rows.append(tfhe_row(bits, log_n, k, lb, ell, batch))
            print(json.dumps(rows[-1]), flush=True)
            rows.append(rns_row(log_n, k, ell, batch))
            print(json.dumps(rows[-1]), flush=True)
    for bits in (32, 64):
        for log_n in (10, 11, 14):
            for r in fft_rows(bits, log_n, 8192 if log_n < 14 else 1024):
                rows.append(r)
                print(json.dumps(r), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
