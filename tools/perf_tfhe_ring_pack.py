#!/usr/bin/env python3
"""Ring packing (pfhe_ringpack{,32}_pack_dev): time per call at the two shapes of tools/perf_tfhe_trace.py (k = 1: the
fused form), counts 16 and N, output batch 1 and 64 — device events after a warm-up, five rounds, median and spread.

    python tools/perf_tfhe_ring_pack.py [--rounds 5] [--shapes 0,1] [--batches 1,64] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  The four forms are timed in turn within every round, on
the same inputs:
  - the handle (chunk = the batch: one launch per level);
  - the composition from public calls: lwe_embed_glwe_dev, per level mul_monomial_each_to_dev, a subtraction and an
    addition, glwe_automorphism_dev and an addition, batched over the nodes, then glwe_trace_dev; the same words are checked
    in the run.  JUDGED at batch 64: the handle's median may exceed the composition's by no more than the larger of the two
    spreads; the line ends in `ok` or `SLOWER` (batch 1 is reported only);
  - lwe_pack_keyswitch_fft_dev and lwe_pack_keyswitch_dev at in_dimension = N, the two packing key switches (reported, not
    judged; they fill coefficients 0..count-1 and keep no factor N).  By transform count ring packing costs
    (2^m - 1 + log N - m) (ell + 2) half transforms against about N ell.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, log_basis, ell): the two shapes of tools/perf_tfhe_trace.py
SHAPES = [
    (32, 10, 1, 7, 3),
    (64, 11, 1, 15, 2),
]


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


def composition(lwe, keys, out, count, trace):
    """rule B as public calls: the embedding, the levels batched over nodes and groups, the trailing trace"""
    fft, k = trace.fft, trace.glwe_dimension
    n, log_n, glwe, key_len = fft.poly_length(), fft.log_n, trace.glwe_len(), trace.key_len()
    batch = lwe.numel() // (count * (k * n + 1))
    m = (count - 1).bit_length()
    leaves = torch.empty(batch * count * glwe, dtype=lwe.dtype, device="cuda")
    p.lwe_embed_glwe_dev(lwe, leaves, fft, k)
    nodes = torch.zeros((batch, 1 << m, glwe), dtype=lwe.dtype, device="cuda")
    nodes[:, :count] = leaves.view(batch, count, glwe)
    for level in range(1, m + 1):
        half = 1 << (m - level)
        even, odd = nodes[:, :half].reshape(-1), nodes[:, half:2 * half].reshape(-1)
        exps = torch.full((batch * half,), n >> level, dtype=torch.int32, device="cuda")
        shifted = torch.empty_like(odd)
        fft.mul_monomial_each_to_dev(odd, exps, shifted, polys_per_exp=k + 1)
        d, s = even - shifted, even + shifted
        auto = torch.empty_like(d)
        p.glwe_automorphism_dev(d, keys[(log_n - level) * key_len:(log_n - level + 1) * key_len], auto, (1 << level) + 1, trace)
        nodes = (s + auto).view(batch, half, glwe)
    out.copy_(nodes[:, 0].reshape(-1))
    if m < log_n:
        p.glwe_trace_dev(out, keys[:(log_n - m) * key_len], out, trace, log_n - m)


def run(bits, log_n, k, lb, ell, rounds, batches):
    n = 1 << log_n
    fft, basis = p.FullComplex64FftTable(log_n), p.ApproxSignedBasis(bits, lb, ell)
    trace = p.TfheGlweTraceContext(fft, basis, k)
    glwe, key_len, word = trace.glwe_len(), trace.key_len(), bits // 8
    keys = torch.empty(log_n * key_len, dtype=torch.complex128, device="cuda")
    p.write_fourier_form(p.torus_uniform(log_n * key_len, bits), keys, fft)
    pf = p.TfhePackFftContext(fft, basis, k * n, k)
    pksk = p.torus_uniform(k * n * ell * glwe, bits)      # full-range words: the cost does not depend on them
    fkey = torch.empty(pf.fkey_len, dtype=torch.complex128, device="cuda")
    p.tfhe_pack_key_fourier_dev(pksk, fkey, pf)
    key_bytes = {"ring": keys.numel() * 16, "pack_fft": fkey.numel() * 16, "pack_exact": pksk.numel() * word}
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "key_bytes": key_bytes, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={ell}  keys: ring packing {key_bytes['ring'] / 2 ** 20:.2f} MiB, Fourier packing "
          f"key {key_bytes['pack_fft'] / 2 ** 20:.1f} MiB (x{key_bytes['pack_fft'] / key_bytes['ring']:.0f}), exact packing key "
          f"{key_bytes['pack_exact'] / 2 ** 20:.1f} MiB")
    for count in (16, n):
        m = (count - 1).bit_length()
        expected = (2 ** m - 1 + log_n - m) * (ell + 2) / (n * ell)
        for batch in batches:
            ctx = p.TfheRingPackContext(fft, basis, k, max_count=count, chunk=batch)
            lwe = p.torus_uniform(batch * count * (k * n + 1), bits)
            out, out_c, out_f, out_x = (torch.empty(batch * glwe, dtype=lwe.dtype, device="cuda") for _ in range(4))
            forms = {
                "handle": lambda: p.lwe_ring_pack_dev(lwe, keys, out, count, ctx),
                "composition": lambda: composition(lwe, keys, out_c, count, trace),
                "pack_fft": lambda: p.lwe_pack_keyswitch_fft_dev(lwe, fkey, out_f, count, pf),
                "pack_exact": lambda: p.lwe_pack_keyswitch_dev(lwe, pksk, out_x, k * n, count, fft, basis, k),
            }
            times = {name: [] for name in forms}
            for fn in forms.values():
                fn()  # warm-up
            same = bool(torch.equal(out, out_c))
            for _ in range(rounds):
                for name, fn in forms.items():
                    times[name].append(timed(fn))
            h, c, f, x = (summary(times[name]) for name in forms)
            judged = batch >= 64
            holds = h["s"] <= c["s"] * (1 + max(h["spread"], c["spread"]))
            h.update(count=count, batch=batch, composition=c, pack_fft=f, pack_exact=x, same_words=same, judged=judged,
                     condition_holds=holds, expected_ratio_to_pack_fft=expected)
            res["forms"][f"count={count} batch={batch}"] = h
            verdict = ("ok" if holds else "SLOWER") if judged else "-"
            print(f"  count {count:5d} batch {batch:3d}  handle {h['s'] * 1e3:10.3f} ms/call  spread {100 * h['spread']:5.2f} %  |  "
                  f"composition {c['s'] * 1e3:10.3f} ms ({100 * c['spread']:5.2f} %)  x{c['s'] / h['s']:6.2f}  {verdict}  same words "
                  f"{same}  |  pack fft {f['s'] * 1e3:9.3f} ms ({100 * f['spread']:5.2f} %)  handle / fft {h['s'] / f['s']:7.2f} "
                  f"(by transforms {expected:5.2f})  |  pack exact {x['s'] * 1e3:9.3f} ms ({100 * x['spread']:5.2f} %)  handle / "
                  f"exact {h['s'] / x['s']:7.2f}", flush=True)
            del lwe, out, out_c, out_f, out_x, ctx
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    batches = [int(v) for v in a.batches.split(",")]
    rows = [run(*shape, a.rounds, batches) for shape in pick]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
