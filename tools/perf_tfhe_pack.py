#!/usr/bin/env python3
"""The packing key switch (pfhe_tfhe{,32}_pack_keyswitch_dev): time per output GLWE and word multiply-adds per second at the
two shapes of tools/perf_tfhe_keygen.py with n = 630 and the key switch's basis (log B 4, ell 3), for count 1, 32 and N and
batch 1 and 64 — device events after a warm-up, five rounds, median and spread.

    python tools/perf_tfhe_pack.py [--rounds 5] [--shapes 0,1] [--lwe 630] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  No threshold is judged: nothing was measured before.
`mac/s` counts count * n * ell * (k+1) * N word multiply-adds per output GLWE, the zero digits of a padded step excluded.

In the same run, as a yardstick of the multiply-add rate on the same box (reported, not judged): lwe_keyswitch_dev on the
same batch * count input ciphertexts, the same in_dimension and basis, to out_dimension (k+1) N - 1, so that a row of its
key is as long as a row of the packing key and the two calls count the same multiply-adds.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, key-switch log_basis, key-switch ell): the two shapes of tools/perf_tfhe_keygen.py
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


def run(bits, log_n, k, lb, ell, n, rounds):
    big_n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    basis = p.ApproxSignedBasis(bits, lb, ell)
    ell = basis.decompose_length()
    row = (k + 1) * big_n
    pksk = p.torus_uniform(n * ell * row, bits)          # full-range words: the cost does not depend on them
    ksk = p.torus_uniform(n * ell * row, bits)           # the yardstick's key: rows of out_dimension + 1 = (k+1) N words
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "in_dimension": n, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} n={n} logB={lb} ell={ell}  packing key {pksk.numel() * pksk.element_size() / 2 ** 20:.0f} MiB")
    for count in (1, 32, big_n):
        for batch in BATCHES:
            lwe = p.torus_uniform(batch * count * (n + 1), bits)
            out = torch.empty(batch * row, dtype=lwe.dtype, device="cuda")
            fn = lambda: p.lwe_pack_keyswitch_dev(lwe, pksk, out, n, count, fft, basis, k)
            fn()  # warm-up
            f = summary([timed(fn) for _ in range(rounds)])
            macs = batch * count * n * ell * row
            f.update(count=count, batch=batch, s_per_glwe=f["s"] / batch, mac_per_s=macs / f["s"])
            ks_out = torch.empty(batch * count * row, dtype=lwe.dtype, device="cuda")
            ks = lambda: p.lwe_keyswitch_dev(lwe, ksk, ks_out, n, row - 1, basis)
            ks()
            y = summary([timed(ks) for _ in range(rounds)])
            y.update(mac_per_s=macs / y["s"])
            f["lwe_keyswitch_yardstick"] = y
            res["forms"][f"count={count} batch={batch}"] = f
            print(f"  count {count:5d} batch {batch:3d}  {f['s'] * 1e3:10.3f} ms/call  {f['s_per_glwe'] * 1e6:12.1f} us/GLWE  spread "
                  f"{100 * f['spread']:5.2f} %  {f['mac_per_s'] / 1e12:7.3f} T mac/s   |  lwe_keyswitch on the same inputs "
                  f"{y['s'] * 1e3:10.3f} ms  spread {100 * y['spread']:5.2f} %  {y['mac_per_s'] / 1e12:7.3f} T mac/s", flush=True)
            del lwe, out, ks_out
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
