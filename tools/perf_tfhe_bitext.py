#!/usr/bin/env python3
"""Bit extraction (pfhe_tfhe{,32}_extract_bits_dev): time per call at the two shapes of tools/perf_tfhe_bootstrap.py with
n = 630 and a key switch of log B 4, ell 3, for 4 and 8 bits and batch 1, 64 and 1024 — device events after a warm-up, five
rounds, median and spread.

    python tools/perf_tfhe_bitext.py [--rounds 5] [--shapes 0,1] [--bits 4,8] [--batches 1,64,1024] [--limit 900] [--json out.json]

Every (shape, bits) runs in a process of its own under its own time limit (--limit seconds); the first one that fails ends
the run.  `spread` is (max - min) / median of a form's rounds in this run.  The two forms are timed in turn within every
round, odd rounds in reverse order:
  - the handle: one tfhe_extract_bits_dev;
  - the composition of public calls, per bit: a torch left shift, lwe_keyswitch_dev, b += 2^(BITS-2), lwe_modulus_switch_dev,
    mul_monomial_each_to_dev on TV_i, tfhe_blind_rotate_dev, glwe_sample_extract_dev at 0, body += 2^(delta+i-1) and a torch
    subtraction, on buffers allocated before the clock starts.
JUDGED on every line: the handle's median must not be longer than the composition's by more than the larger of the two
spreads (taken of the composition's median); the line ends in `ok` or `SLOWER`.  Both forms are checked to give the same
words in the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (word bits, log_n, k, log_basis, ell): the two shapes of tools/perf_tfhe_bootstrap.py
SHAPES = [
    (32, 10, 1, 7, 3),
    (64, 11, 1, 15, 2),
]
LWE_DIMENSION, KS_BASIS = 630, (4, 3)


def summary(times):
    med = statistics.median(times)
    return {"s": med, "rounds_s": times, "spread": (max(times) - min(times)) / med}


def run(bits, log_n, k, lb, ell, nbits, rounds, batches):
    sys.path.insert(0, ROOT)
    import torch

    import primus_fhe_amd as p

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3

    def signed(v):
        v %= 1 << bits
        return v - (1 << bits) if v >> (bits - 1) else v

    n, big_n = LWE_DIMENSION, 1 << log_n
    glwe, ext = (k + 1) * big_n, k * big_n + 1
    delta = bits - nbits - 1
    fft, basis, ks_basis = p.FullComplex64FftTable(log_n), p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *KS_BASIS)
    ctx = p.TfheBitExtractContext(fft, basis, n, k, ks_basis)
    rot = p.TfheBlindRotateContext(fft, basis, k)
    bsk = torch.empty(ctx.bsk_len(), dtype=torch.complex128, device="cuda")
    per_key = ctx.key_len()
    for i in range(0, n, 32):                                # 32 keys per forward call bound the torus form
        c = min(32, n - i)
        p.write_fourier_form(p.torus_uniform(c * per_key, bits), bsk[i * per_key:(i + c) * per_key], fft)
    ksk = p.torus_uniform(ctx.ksk_len(), bits)
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "lwe_dimension": n, "bits": nbits,
           "delta_log": delta, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={ell} n={n} key switch {KS_BASIS}  bits {nbits} at delta {delta}  "
          f"bsk {ctx.bsk_len() * 16 / 2 ** 20:.0f} MiB  ksk {ctx.ksk_len() * bits / 8 / 2 ** 20:.1f} MiB  "
          f"handle scratch {ctx.scratch_bytes() / 2 ** 20:.0f} MiB", flush=True)
    for batch in batches:
        lwe = p.torus_uniform(batch * ext, bits)             # full-range words: the cost does not depend on them
        out, out_c = (torch.empty(batch * nbits * (n + 1), dtype=lwe.dtype, device="cuda") for _ in range(2))
        run_c, shifted, lwe_ext = (torch.empty(batch * ext, dtype=lwe.dtype, device="cuda") for _ in range(3))
        switched = torch.empty(batch * (n + 1), dtype=lwe.dtype, device="cuda")
        exps = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        neg_b = torch.empty(batch, dtype=torch.int32, device="cuda")
        acc = torch.empty(batch * glwe, dtype=lwe.dtype, device="cuda")
        tvs = []
        for i in range(nbits - 1):
            tv = torch.zeros((batch, k + 1, big_n), dtype=lwe.dtype, device="cuda")
            tv[:, k, :] = signed(-(1 << (delta + i - 1)))
            tvs.append(tv.view(-1))

        def composition():
            cur = lwe
            view = out_c.view(batch, nbits, n + 1)
            for i in range(nbits):
                torch.bitwise_left_shift(cur, bits - 1 - delta - i, out=shifted)
                p.lwe_keyswitch_dev(shifted, ksk, switched, ext - 1, n, ks_basis)
                view[:, i] = switched.view(batch, n + 1)
                if i + 1 == nbits:
                    break
                switched.view(batch, n + 1)[:, n] += signed(1 << (bits - 2))
                p.lwe_modulus_switch_dev(switched, n, log_n, exps, neg_b)
                fft.mul_monomial_each_to_dev(tvs[i], neg_b, acc, polys_per_exp=k + 1)
                p.tfhe_blind_rotate_dev(acc, bsk, exps, rot)
                p.glwe_sample_extract_dev(acc, lwe_ext, fft, k, 0)
                lwe_ext.view(batch, ext)[:, ext - 1] += signed(1 << (delta + i - 1))
                torch.sub(cur, lwe_ext, out=run_c)
                cur = run_c

        forms = {
            "handle": lambda: p.tfhe_extract_bits_dev(lwe, bsk, ksk, out, ctx, delta, nbits),
            "composition": composition,
        }
        times = {name: [] for name in forms}
        for fn in forms.values():
            fn()  # warm-up
        same = bool(torch.equal(out, out_c))
        for i in range(rounds):
            order = list(forms.items())
            for name, fn in (reversed(order) if i % 2 else order):
                times[name].append(timed(fn))
        h, c = summary(times["handle"]), summary(times["composition"])
        margin = max(h["spread"], c["spread"]) * c["s"]
        holds = h["s"] - c["s"] <= margin
        h.update(batch=batch, composition=c, same_words=same, holds=holds)
        res["forms"][f"batch={batch}"] = h
        print(f"  batch {batch:5d}  handle {h['s'] * 1e3:10.3f} ms/call  spread {100 * h['spread']:5.2f} %  |  composition "
              f"{c['s'] * 1e3:10.3f} ms ({100 * c['spread']:5.2f} %)  x{c['s'] / h['s']:6.2f}  {'ok' if holds else 'SLOWER'}  |  "
              f"same words {same}", flush=True)
        del lwe, out, out_c, run_c, shifted, lwe_ext, switched, exps, neg_b, acc, tvs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bits", default="4,8")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--limit", type=int, default=900, help="seconds one (shape, bits) may take")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)        # "shape index,bits": the child's work
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    if a.one:
        shape, nbits = (int(v) for v in a.one.split(","))
        print("JSON " + json.dumps(run(*SHAPES[shape], nbits, a.rounds, batches)))
        return
    pick = [int(i) for i in a.shapes.split(",")] if a.shapes else range(len(SHAPES))
    rows = []
    for shape in pick:
        for nbits in (int(v) for v in a.bits.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{shape},{nbits}", "--rounds", str(a.rounds), "--batches",
                   a.batches]
            child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
            limit = threading.Timer(a.limit, child.kill)
            limit.start()
            for line in child.stdout:      # passed on line by line, as the child prints
                if line.startswith("JSON "):
                    rows.append(json.loads(line[5:]))
                else:
                    print(line, end="", flush=True)
            child.wait()
            limit.cancel()
            if child.returncode != 0:      # nothing more is started on the device after a failure or a time limit
                sys.exit(f"shape {shape} bits {nbits} ended with status {child.returncode}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
