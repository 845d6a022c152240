#!/usr/bin/env python3
"""The circuit bootstrap with its options (pfhe_tfhe{,32}_cbs_create_with): the existing handle, the shared rotation
(many-LUT), the multi-bit rotation with grouping factor 2, and both — time per call at the two shapes of
tools/perf_tfhe_cbs.py (n = 630, k = 1), an output basis of 2 and 4 levels (log B 4), the key switch's basis log B 4 ell 3,
and batch 1, 64 and 1024.  Device events after a warm-up, five rounds, median and spread; the four forms are timed in turn
within every round of one process (odd rounds in reverse order), so that drift of the clock falls on all of them alike and
no form always runs behind the same other one.

    timeout -k 10 900 python tools/perf_tfhe_cbs_shared.py --shapes 0 [--rounds 5] [--lwe 630] [--batches 1,64,1024] [--json out.json]
    timeout -k 10 900 python tools/perf_tfhe_cbs_shared.py --shapes 1

One shape per process, each under its own time limit.  `spread` is (max - min) / median of a form's rounds in this run.

JUDGED, at batch 1024 only: the shared handle's median must be shorter than the existing handle's of the same line by more
than the larger of their two spreads (in seconds); the line ends in `ok` or `MISSED`.  Beside it stand the ratio seen and the
ratio expected from the accumulator count: the rotation's share r of the existing call falls by ell_cb and the rest (the key
switch and the small stages) stays, expected = r / ell_cb + (1 - r), with r measured in the same run as
tfhe_bootstrap_dev without a key switch on batch * ell_cb ciphertexts over the existing handle.  Nothing is judged at batch 1
and 64, where the call is bound by the latency of n dependent steps, nor on the multi-bit lines, whose job is those batches.

Reported, not judged, at batch 64 and 1024: the many-LUT bootstrap (log_luts = log2 ell_cb, no key switch) against the
classic bootstrap on 2^v times as many ciphertexts.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, rotation log_basis, ell): the two shapes of tools/perf_tfhe_cbs.py
SHAPES = [
    (32, 10, 1, 7, 3),
    (64, 11, 1, 15, 2),
]
CBS_LOG_BASIS, CBS_LEVELS = 4, (2, 4)
PFKS_BASIS = (4, 3)
GROUPING = 2
JUDGED_BATCH = 1024


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


def measure_in_turn(forms, rounds):
    """forms: name -> callable; every round times each of them once, in turn, odd rounds in reverse order: a form's time
    depends a little on which keys the call before it left in the Infinity Cache (a circuit bootstrap ends in its key
    switch, whose key evicts the bootstrapping key; a bare bootstrap leaves it there), so no form keeps one predecessor"""
    for fn in forms.values():
        fn()  # warm-up
    times = {name: [] for name in forms}
    names = list(forms)
    for r in range(rounds):
        for name in (names[::-1] if r % 2 else names):
            times[name].append(timed(forms[name]))
    return {name: summary(t) for name, t in times.items()}


def fourier_key(fft, words, bits):
    torus = p.torus_uniform(words, bits)     # full-range words: the cost does not depend on them
    key = torch.empty(words, dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, key, fft)
    return key


def run(bits, log_n, k, lb, ell, n, rounds, batches):
    big_n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    basis, pfks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *PFKS_BASIS)
    glwe, ext = (k + 1) * big_n, k * big_n + 1
    bsk = fourier_key(fft, p.TfheKeyShape(fft, basis, n, k, 0).bsk_len(), bits)
    bsk_mb = fourier_key(fft, p.TfheKeyShape(fft, basis, n, k, GROUPING).bsk_len(), bits)
    pfksk = p.torus_uniform((k + 1) * ext * pfks_basis.decompose_length() * glwe, bits)
    tv = p.torus_uniform(glwe, bits)
    boot = p.TfheBootstrapContext(fft, basis, n, k)             # without a key switch
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "lwe_dimension": n, "lines": {}}
    print(f"u{bits} N=2^{log_n} k={k} n={n} rotation logB={lb} ell={ell}  pfks logB={PFKS_BASIS[0]} ell={PFKS_BASIS[1]}  "
          f"g={GROUPING}")
    for levels in CBS_LEVELS:
        cbs_basis = p.ApproxSignedBasis(bits, CBS_LOG_BASIS, levels)
        log_luts = (levels - 1).bit_length()
        make = lambda **kw: p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, **kw)  # noqa: E731
        ctxs = {"existing": (make(), bsk), "shared": (make(shared_rotation=True), bsk),
                "g2": (make(grouping_factor=GROUPING), bsk_mb),
                "shared+g2": (make(grouping_factor=GROUPING, shared_rotation=True), bsk_mb)}
        many_ctx = p.TfheBootstrapContext(fft, basis, n, k, log_luts=log_luts)
        for batch in batches:
            lwe = p.torus_uniform(batch * (n + 1), bits)
            out = torch.empty(batch * ctxs["existing"][0].ggsw_len(), dtype=lwe.dtype, device="cuda")
            many = p.torus_uniform(batch * levels * (n + 1), bits)
            extracted = torch.empty(batch * levels * ext, dtype=lwe.dtype, device="cuda")
            forms = {name: (lambda c=c, key=key: p.tfhe_circuit_bootstrap_dev(lwe, key, pfksk, out, c))
                     for name, (c, key) in ctxs.items()}
            forms["rotation_alone"] = lambda: p.tfhe_bootstrap_dev(many, bsk, tv, None, extracted, boot)
            if batch >= 64:
                forms["many_lut"] = lambda: p.tfhe_bootstrap_dev(lwe, bsk, tv, None, extracted[:(batch << log_luts) * ext],
                                                                 many_ctx)
                wide = many[:(batch << log_luts) * (n + 1)]
                forms["classic_x_luts"] = lambda: p.tfhe_bootstrap_dev(wide, bsk, tv, None, extracted[:(batch << log_luts) * ext],
                                                                       boot)
            t = measure_in_turn(forms, rounds)
            ex, sh = t["existing"], t["shared"]
            share = min(1.0, t["rotation_alone"]["s"] / ex["s"])
            line = dict(levels=levels, batch=batch, forms=t, rotation_share=share, expected_ratio=share / levels + 1 - share,
                        seen_ratio=sh["s"] / ex["s"], scratch_bytes={nm: c.scratch_bytes() for nm, (c, _) in ctxs.items()})
            text = "  ".join(f"{nm} {t[nm]['s'] * 1e3:9.3f} ms ({100 * t[nm]['spread']:5.2f} %)" for nm in ctxs)
            verdict = ""
            if batch == JUDGED_BATCH:
                margin = max(ex["spread"] * ex["s"], sh["spread"] * sh["s"])
                line["shorter"] = sh["s"] < ex["s"] - margin
                verdict = "  " + ("ok" if line["shorter"] else "MISSED")
            print(f"  ell_cb {levels} batch {batch:5d}  {text}  |  shared/existing seen {line['seen_ratio']:.3f} expected "
                  f"{line['expected_ratio']:.3f} (rotation share {share:.3f}){verdict}", flush=True)
            if "many_lut" in t:
                a, b = t["many_lut"], t["classic_x_luts"]
                print(f"      many-LUT bootstrap x{1 << log_luts} {a['s'] * 1e3:9.3f} ms ({100 * a['spread']:5.2f} %)  classic on "
                      f"{batch << log_luts} {b['s'] * 1e3:9.3f} ms ({100 * b['spread']:5.2f} %)", flush=True)
            res["lines"][f"levels={levels} batch={batch}"] = line
            del lwe, out, many, extracted, forms
        del ctxs, many_ctx
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lwe", type=int, default=630, help="the LWE dimension n of the inputs (a multiple of 2)")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    batches = [int(v) for v in a.batches.split(",")]
    rows = [run(*shape, a.lwe, a.rounds, batches) for shape in pick]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
