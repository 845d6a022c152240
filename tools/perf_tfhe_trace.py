#!/usr/bin/env python3
"""The homomorphic trace (pfhe_tfhe{,32}_glwe_trace_dev): time per call of the full trace (log N steps) at the two shapes of
tools/perf_tfhe_bootstrap.py (k = 1: the fused form), batch 1, 64 and 1024 — device events after a warm-up, five rounds,
median and spread.

    python tools/perf_tfhe_trace.py [--rounds 5] [--shapes 0,1] [--batches 1,64,1024] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  The three forms are timed in turn within every round:
  - the handle;
  - the composition: the same trace from the calls there were before the handle: per step a torch gather for sigma_t,
    tfhe_external_product_to_dev on the key padded with ell zero body rows, a subtraction and an addition; the same words
    are checked in the run.  JUDGED at batch 64 and 1024: the handle's median may exceed the composition's by no more than
    the larger of the two spreads; the line ends in `ok` or `SLOWER` (batch 1 is reported only);
  - as a yardstick (reported, not judged): log N calls of tfhe_external_product_to_dev with one key on the batch.  By
    transform count (ell forward and 2 inverse transforms a step against 2 ell and 2) one expects (ell + 2) / (2 ell + 2).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, log_basis, ell): the two shapes of tools/perf_tfhe_bootstrap.py
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


def composition(inp, padded, out, plan, exps, n, scratch):
    """the trace as the calls of before: per step a gather, the product on the padded key, a subtraction and an addition"""
    k = plan.glwe_dimension
    acc = inp
    for s, t in enumerate(exps):
        u = (torch.arange(n, device="cuda") * pow(t, -1, 2 * n)) % (2 * n)
        g = acc.view(-1, n)[:, u % n]
        sig = torch.where(u < n, g, -g).reshape(-1)
        p.tfhe_external_product_to_dev(sig, padded[s], scratch, plan)
        body = torch.zeros_like(sig).view(-1, k + 1, n)
        body[:, k] = sig.view(-1, k + 1, n)[:, k]
        acc = acc + (body.view(-1) - scratch)
    out.copy_(acc)


def run(bits, log_n, k, lb, ell, rounds, batches):
    fft, basis = p.FullComplex64FftTable(log_n), p.ApproxSignedBasis(bits, lb, ell)
    plan, ctx = p.TfheFftContext(fft, basis, k), p.TfheGlweTraceContext(fft, basis, k)
    glwe, key_len, n = ctx.glwe_len(), ctx.key_len(), 1 << log_n
    exps = ctx.trace_exponents()
    word = bits // 8
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={ell}  {log_n} steps  ciphertext {glwe * word / 1024:.0f} KiB  "
          f"key {key_len * 16 / 1024:.0f} KiB a step  expected handle / yardstick {(ell + 2) / (2 * ell + 2):.2f}")
    keys = torch.empty(log_n * key_len, dtype=torch.complex128, device="cuda")
    p.write_fourier_form(p.torus_uniform(log_n * key_len, bits), keys, fft)
    padded = torch.zeros(log_n, plan.key_len(), dtype=torch.complex128, device="cuda")
    padded[:, :key_len] = keys.view(log_n, key_len)
    for batch in batches:
        inp = p.torus_uniform(batch * glwe, bits)          # full-range words: the cost does not depend on them
        out, out_c, scratch, many_out = (torch.empty_like(inp) for _ in range(4))

        def yardstick():
            for s in range(log_n):
                p.tfhe_external_product_to_dev(inp, padded[s], many_out, plan)

        forms = {
            "handle": lambda: p.glwe_trace_dev(inp, keys, out, ctx),
            "composition": lambda: composition(inp, padded, out_c, plan, exps, n, scratch),
            "yardstick": yardstick,
        }
        times = {name: [] for name in forms}
        for fn in forms.values():
            fn()  # warm-up
        same = bool(torch.equal(out, out_c))
        for _ in range(rounds):
            for name, fn in forms.items():
                times[name].append(timed(fn))
        h, c, y = (summary(times[name]) for name in ("handle", "composition", "yardstick"))
        judged = batch > 1
        holds = h["s"] <= c["s"] * (1 + max(h["spread"], c["spread"]))
        h.update(batch=batch, composition=c, yardstick=y, same_words=same, judged=judged, condition_holds=holds,
                 ratio_to_yardstick=h["s"] / y["s"])
        res["forms"][f"batch={batch}"] = h
        verdict = ("ok" if holds else "SLOWER") if judged else "-"
        print(f"  batch {batch:5d}  handle {h['s'] * 1e3:10.3f} ms/call  spread {100 * h['spread']:5.2f} %  |  composition "
              f"{c['s'] * 1e3:10.3f} ms ({100 * c['spread']:5.2f} %)  x{c['s'] / h['s']:7.2f}  {verdict}  same words {same}  |  "
              f"{log_n} products one key {y['s'] * 1e3:9.3f} ms ({100 * y['spread']:5.2f} %)  handle / yardstick "
              f"{h['ratio_to_yardstick']:5.2f}", flush=True)
        del inp, out, out_c, scratch, many_out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,64,1024")
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
