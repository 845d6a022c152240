#!/usr/bin/env python3
"""Multi-bit bootstrap against the classic one (pfhe_tfhe{,32}_bootstrap_create_multibit / _create): seconds per call of the
classic handle and of the multi-bit handle at g = 2 and g = 3 on the same inputs — device events after a warm-up, the
forms in alternation within one process.

    python tools/perf_tfhe_multibit.py [--rounds 5] [--reps 1] [--shapes 0,1] [--batches 1,64,8192] [--lwe 630] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  `ratio` is classic time / multi-bit time (above 1: the
multi-bit handle is faster); `beyond spread` says whether the two medians differ by more than the larger of the two
spreads.  No threshold is judged: the figures are recorded against the classic handle of the same process and box.
The keys are full-torus random words (the timing does not depend on their values); the multi-bit key has
(n / g) * 2^g of them, the classic one n.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, log_basis, ell, key-switch log_basis, key-switch ell): the two shapes of tools/perf_tfhe_bootstrap.py
SHAPES = [
    (32, 10, 1, 7, 3, 4, 3),
    (64, 11, 1, 15, 2, 4, 3),
]
GROUPINGS = (2, 3)


def timed(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def rand_words(bits, words, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-2 ** 31, 2 ** 31, (words * bits // 32,), dtype=torch.int32, device="cuda", generator=g)
    return x if bits == 32 else x.view(torch.int64)


def random_keys(fft, bits, count, key_len, seed):
    """`count` full-torus Fourier GGSW keys end to end, 32 keys per forward call to bound the input"""
    out = torch.empty(count * key_len, dtype=torch.complex128, device="cuda")
    for i in range(0, count, 32):
        c = min(32, count - i)
        fft.forward_torus_dev(rand_words(bits, c * key_len, seed + i), out[i * key_len:(i + c) * key_len])
    return out


def run(bits, log_n, k, lb, ell, ks_lb, ks_ell, n, batches, rounds, reps):
    dtype = torch.int32 if bits == 32 else torch.int64
    fft = p.FullComplex64FftTable(log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, ks_lb, ks_ell)
    ctxs = {"classic": p.TfheBootstrapContext(fft, basis, n, k, ks_basis)}
    for g in GROUPINGS:
        assert n % g == 0
        ctxs[f"multibit g={g}"] = p.TfheBootstrapContext(fft, basis, n, k, ks_basis, grouping_factor=g)
    keys = {name: random_keys(fft, bits, c.bsk_len() // c.key_len(), c.key_len(), 100 * len(name)) for name, c in ctxs.items()}
    classic = ctxs["classic"]
    tv = rand_words(bits, classic.glwe_len(), 2)
    ksk = rand_words(bits, classic.ksk_len(), 3)
    rows = []
    for batch in batches:
        lwe = rand_words(bits, batch * (n + 1), 1)
        out = torch.empty(batch * (n + 1), dtype=dtype, device="cuda")
        forms = {name: (lambda c=c, key=keys[name]: p.tfhe_bootstrap_dev(lwe, key, tv, ksk, out, c)) for name, c in ctxs.items()}
        for fn in forms.values():
            fn()  # warm-up
        torch.cuda.synchronize()
        times = {name: [] for name in forms}
        for _ in range(rounds):          # same-process alternation
            for name, fn in forms.items():
                times[name].append(timed(fn, reps))
        res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": basis.decompose_length(), "lwe_dimension": n,
               "batch": batch, "forms": {}}
        for name, t in times.items():
            med = statistics.median(t)
            res["forms"][name] = {"s": med, "rounds_s": t, "per_s": batch / med, "spread": (max(t) - min(t)) / med,
                                  "bsk_MiB": keys[name].numel() * 16 / 2 ** 20, "scratch_bytes": ctxs[name].scratch_bytes()}
        base = res["forms"]["classic"]
        for name, f in res["forms"].items():
            f["ratio"] = base["s"] / f["s"]
            f["beyond_spread"] = abs(base["s"] - f["s"]) > max(base["spread"], f["spread"]) * max(base["s"], f["s"])
        rows.append(res)
        print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={res['ell']} n={n} batch={batch}")
        for name, f in res["forms"].items():
            print(f"  {name:14s} {f['s'] * 1e3:10.3f} ms/call  {f['per_s']:12.1f} bootstraps/s  spread {100 * f['spread']:5.2f} %  "
                  f"classic / this {f['ratio']:.4f}  beyond spread: {f['beyond_spread']}  key {f['bsk_MiB']:.0f} MiB", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--batches", default="1,64,8192")
    ap.add_argument("--lwe", type=int, default=630, help="the LWE dimension n (a multiple of 2 and 3)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    rows = []
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    for shape in pick:
        rows += run(*shape, a.lwe, [int(b) for b in a.batches.split(",")], a.rounds, a.reps)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
