#!/usr/bin/env python3
"""The packing key switch in the Fourier domain (pfhe_tfhe{,32}_pack_keyswitch_fft_dev) beside the exact call
(pfhe_tfhe{,32}_pack_keyswitch_dev) in the same run on the same inputs: time per output GLWE at the two shapes of
tools/perf_tfhe_pack.py with n = 630 and the key switch's basis (log B 4, ell 3), for count 1, 32 and N and batch 1 and 64 —
device events after a warm-up, five rounds, median and spread.  The key conversion is timed on its own.

    python tools/perf_tfhe_pack_fft.py [--rounds 5] [--shapes 0,1] [--lwe 630] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  `faster` says whether the Fourier call's median is below
the exact call's by more than the two spreads (spread x median of each, added): the expectation to check at count = N.
No threshold is judged here.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, key-switch log_basis, key-switch ell): the two shapes of tools/perf_tfhe_pack.py
SHAPES = [
    (32, 10, 1, 4, 3),
    (64, 11, 1, 4, 3),
]
BATCHES = (1, 64)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def summary(times):
    med = statistics.median(times)
    return {"s": med, "rounds_s": times, "spread": (max(times) - min(times)) / med}


def measure(fn, rounds):
    fn()  # warm-up
    return summary([timed(fn) for _ in range(rounds)])


def run(bits, log_n, k, lb, ell, n, rounds):
    big_n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    basis = p.ApproxSignedBasis(bits, lb, ell)
    ell = basis.decompose_length()
    row = (k + 1) * big_n
    ctx = p.TfhePackFftContext(fft, basis, n, k)
    pksk = p.torus_uniform(n * ell * row, bits)          # full-range words: the cost does not depend on them
    fkey = torch.empty(ctx.fkey_len, dtype=torch.complex128, device="cuda")
    conv = measure(lambda: p.tfhe_pack_key_fourier_dev(pksk, fkey, ctx), rounds)
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "in_dimension": n,
           "scratch_bytes": ctx.scratch_bytes(), "key_conversion": conv, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} n={n} logB={lb} ell={ell}  packing key {pksk.numel() * pksk.element_size() / 2 ** 20:.0f} MiB, "
          f"Fourier key {fkey.numel() * 16 / 2 ** 20:.0f} MiB, plan scratch {ctx.scratch_bytes() / 2 ** 20:.0f} MiB")
    print(f"  key conversion {conv['s'] * 1e3:10.3f} ms  spread {100 * conv['spread']:5.2f} %")
    for count in (1, 32, big_n):
        for batch in BATCHES:
            lwe = p.torus_uniform(batch * count * (n + 1), bits)
            out = torch.empty(batch * row, dtype=lwe.dtype, device="cuda")
            f = measure(lambda: p.lwe_pack_keyswitch_fft_dev(lwe, fkey, out, count, ctx), rounds)
            x = measure(lambda: p.lwe_pack_keyswitch_dev(lwe, pksk, out, n, count, fft, basis, k), rounds)
            margin = f["spread"] * f["s"] + x["spread"] * x["s"]
            f.update(count=count, batch=batch, s_per_glwe=f["s"] / batch, exact=x, exact_s_per_glwe=x["s"] / batch,
                     ratio=x["s"] / f["s"], faster=bool(x["s"] - f["s"] > margin))
            res["forms"][f"count={count} batch={batch}"] = f
            print(f"  count {count:5d} batch {batch:3d}  fft {f['s'] * 1e3:10.3f} ms/call {f['s_per_glwe'] * 1e6:10.1f} us/GLWE spread "
                  f"{100 * f['spread']:5.2f} %  |  exact {x['s'] * 1e3:10.3f} ms/call {x['s'] / batch * 1e6:10.1f} us/GLWE spread "
                  f"{100 * x['spread']:5.2f} %  |  exact / fft {f['ratio']:8.2f}  faster by more than the spreads: {f['faster']}",
                  flush=True)
            del lwe, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lwe", type=int, default=630, help="the LWE dimension n of the inputs")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    rows = [run(*shape, a.lwe, a.rounds) for shape in pick]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
