#!/usr/bin/env python3
"""Batched blind rotation (pfhe_blindrot_*): steps per second against the standalone external product and against the
same loop built from public calls, timed with device events after a warm-up.

    python tools/perf_blind_rotate.py [--steps 64] [--reps 3] [--shapes 0,1] [--json out.json]

For every shape: blind-rotation steps/s (batch x n_steps / time), the rate of mul_dcrt_ggsw_to_dev(into_coeff_form=1)
on the same shape and batch, the rate of the public-call loop (per-ciphertext monomial, sub_to, the product in coefficient
form, add_to; u64 only: the u32 tables have no element-wise family), and the bytes a step moves by the shapes (ACC read
twice and written once, BSK_i once; the public-call loop adds the two full-batch temporaries D and E, each written and
read again).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402
from primus_fhe_amd._lib import check, u64p  # noqa: E402

Q61 = [2305843009211596801, 2305843009210023937, 2305843009208713217]
Q30 = [1073479681, 1071513601, 1070727169]
# (word bits, log_n, moduli, log_basis, batch, n_steps or None for --steps)
SHAPES = [
    (64, 10, Q61[:1], 10, 8192, None),
    (64, 11, Q61[:1], 10, 8192, None),
    (64, 11, Q61[:2], 20, 8192, None),
    (64, 16, Q61, 30, 8, 4),
    (32, 16, Q30, 15, 8, 4),
]


def timed(fn, reps):
    fn()  # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def fill(words, mods, n, seed, bits):
    x = torch.empty(words, dtype=torch.int64, device="cuda")
    m = np.array(mods, np.uint64)
    check(p.lib().pfhe_fill_uniform_dev(0, C.c_void_p(x.data_ptr()), words, m.ctypes.data_as(u64p), len(mods), n, seed, None))
    return x if bits == 64 else x.to(torch.int32)  # u32 residues (< 2^30) keep their value


def run(bits, log_n, mods, log_basis, batch, n_steps, reps):
    n, L, k = 1 << log_n, len(mods), 1
    if bits == 64:
        t, base = p.U64DcrtTable(log_n, mods), p.RNSBase(mods)
        basis = p.BigUintApproxSignedBasis(base, log_basis)
        ctx, prod = p.BlindRotateContext(t, base, basis, k), p.DcrtGlevContext(t, base, basis, k)
    else:
        t, base = p.U32DcrtTable(log_n, mods), p.RNSBase32(mods)
        basis = p.BigUintApproxSignedBasis32(base, log_basis)
        ctx, prod = p.BlindRotateContext32(t, base, basis, k), p.DcrtGlevContext32(t, base, basis, k)
    W, G = ctx.glwe_len(), ctx.ggsw_len()
    acc = fill(batch * W, mods, n, 1, bits)
    bsk = fill(n_steps * G, mods, n, 2, bits)
    exps = torch.from_numpy(np.random.default_rng(3).integers(0, 2 * n, batch * n_steps).astype(np.int32)).cuda()
    t_rot = timed(lambda: p.blind_rotate_dev(acc, bsk, exps, ctx), reps)
    d, e = torch.empty_like(acc), torch.empty_like(acc)
    key0 = bsk[:G]
    t_prod = timed(lambda: p.mul_dcrt_ggsw_to_dev(acc, key0, e, prod, into_coeff_form=True), reps * n_steps) * n_steps
    res = {"word_bits": bits, "log_n": log_n, "L": L, "log_basis": log_basis, "ell": basis.decompose_length(), "batch": batch,
           "n_steps": n_steps, "rotate_ms": t_rot * 1e3, "rotate_steps_per_s": batch * n_steps / t_rot,
           "product_steps_per_s": batch * n_steps / t_prod}
    w = 8 if bits == 64 else 4
    res["step_bytes_fused"] = (3 * batch * W + G) * w  # glue-free form: ACC gathered + read + written, BSK_i
    res["step_bytes_public_loop"] = (3 * batch * W + G + 4 * batch * W) * w
    if bits == 64:
        rot = torch.empty_like(acc)
        ex_step = exps[:batch].contiguous()

        def public_loop():
            for i in range(n_steps):
                t.mul_monomial_each_to_dev(acc, ex_step, k + 1, rot)
                t.sub_to_dev(rot, acc, d)
                p.mul_dcrt_ggsw_to_dev(d, bsk[i * G:(i + 1) * G], e, prod, into_coeff_form=True)
                t.add_to_dev(acc, e, acc)
        t_pub = timed(public_loop, reps)
        res["public_loop_steps_per_s"] = batch * n_steps / t_pub
    res["rotate_vs_product"] = res["rotate_steps_per_s"] / res["product_steps_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    rows = []
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    for bits, log_n, mods, log_basis, batch, steps in pick:
        r = run(bits, log_n, mods, log_basis, batch, steps or a.steps, a.reps)
        rows.append(r)
        pub = f"{r['public_loop_steps_per_s'] / 1e6:8.3f} M/s" if "public_loop_steps_per_s" in r else "     n/a    "
        print(f"u{bits} N=2^{log_n} L={r['L']} logB={log_basis} ell={r['ell']} batch={batch} steps={r['n_steps']}: "
              f"rotate {r['rotate_steps_per_s'] / 1e6:8.3f} M steps/s | product {r['product_steps_per_s'] / 1e6:8.3f} M/s "
              f"(rotate/product {r['rotate_vs_product']:.3f}) | public loop {pub} | "
              f"step bytes fused-form {r['step_bytes_fused'] / 2**20:.1f} MiB, public loop {r['step_bytes_public_loop'] / 2**20:.1f} MiB",
              flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
