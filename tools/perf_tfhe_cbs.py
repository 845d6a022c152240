#!/usr/bin/env python3
"""The circuit bootstrap (pfhe_tfhe{,32}_cbs_dev) and the private functional key switch under it
(pfhe_tfhe{,32}_private_keyswitch_dev): time per call and per input bit at the two shapes of tools/perf_tfhe_bootstrap.py
(n = 630, k = 1), for an output basis of 2 and 4 levels (log B 4), the key switch's basis log B 4 ell 3, and batch 1, 64 and
1024 — device events after a warm-up, five rounds, median and spread.

    python tools/perf_tfhe_cbs.py [--rounds 5] [--shapes 0,1] [--lwe 630] [--batches 1,64,1024] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  In the same run:
  - tfhe_bootstrap_dev without a key switch on batch * ell_cb ciphertexts, and the stateless private key switch on its
    outputs: the two calls whose work the handle queues.  JUDGED: the handle's median must not exceed the sum of their
    medians by more than the larger of their two spreads (in seconds); the line ends in `ok` or `SLOWER`.  As measured
    (profiles/tfhe_cbs_a_perf.txt) it is met at u32 and MISSED at u64 on every line, by 0.5 to 1.8 ms: timed apart, each call
    finds its own key in the Infinity Cache, which the two keys of the u64 shape (384 + 158 MiB) cannot share; the handle
    equals the pair timed as one region (tools/perf_tfhe_cbs_pair.py).
  - the private key switch alone in word multiply-adds per second, counting batch * ell_cb * (k N + 1) * ell_pf * (k+1)^2 * N;
  - as a yardstick of the multiply-add rate on the same box (reported, not judged): lwe_keyswitch_dev on as many
    ciphertexts with in_dimension k N + 1 and out_dimension (k+1)^2 N - 1, so that its key has the rows and the words of the
    private key-switch key and the two calls count the same multiply-adds.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, rotation log_basis, ell): the two shapes of tools/perf_tfhe_bootstrap.py
SHAPES = [
    (32, 10, 1, 7, 3),
    (64, 11, 1, 15, 2),
]
CBS_LOG_BASIS, CBS_LEVELS = 4, (2, 4)
PFKS_BASIS = (4, 3)


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


def run(bits, log_n, k, lb, ell, n, rounds, batches):
    big_n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    basis, pfks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, *PFKS_BASIS)
    glwe, ext = (k + 1) * big_n, k * big_n + 1
    torus = p.torus_uniform(n * (k + 1) * ell * glwe, bits)     # full-range words: the cost does not depend on them
    bsk = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, bsk, fft)
    del torus
    pf_ell = pfks_basis.decompose_length()
    pfksk = p.torus_uniform((k + 1) * ext * pf_ell * glwe, bits)
    ksk = p.torus_uniform(ext * pf_ell * (k + 1) * glwe, bits)  # the yardstick's key: as many rows and words
    tv = p.torus_uniform(glwe, bits)
    boot = p.TfheBootstrapContext(fft, basis, n, k)             # without a key switch
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "lwe_dimension": n, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} n={n} rotation logB={lb} ell={ell}  pfks logB={PFKS_BASIS[0]} ell={pf_ell}  "
          f"private key-switch key {pfksk.numel() * pfksk.element_size() / 2 ** 20:.0f} MiB")
    for levels in CBS_LEVELS:
        cbs_basis = p.ApproxSignedBasis(bits, CBS_LOG_BASIS, levels)
        ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
        for batch in batches:
            rows = batch * levels
            lwe = p.torus_uniform(batch * (n + 1), bits)
            out = torch.empty(batch * ctx.ggsw_len(), dtype=lwe.dtype, device="cuda")
            f = measure(lambda: p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx), rounds)
            many = p.torus_uniform(rows * (n + 1), bits)
            extracted = torch.empty(rows * ext, dtype=lwe.dtype, device="cuda")
            b = measure(lambda: p.tfhe_bootstrap_dev(many, bsk, tv, None, extracted, boot), rounds)
            ks = measure(lambda: p.lwe_private_keyswitch_dev(extracted, pfksk, out, k * big_n, levels, fft, pfks_basis, k), rounds)
            macs = rows * ext * pf_ell * (k + 1) * glwe
            ks.update(mac_per_s=macs / ks["s"])
            wide = p.torus_uniform(rows * (ext + 1), bits)
            wide_out = torch.empty(rows * (k + 1) * glwe, dtype=lwe.dtype, device="cuda")
            y = measure(lambda: p.lwe_keyswitch_dev(wide, ksk, wide_out, ext, (k + 1) * glwe - 1, pfks_basis), rounds)
            y.update(mac_per_s=macs / y["s"])
            allowed = b["s"] + ks["s"] + max(b["spread"] * b["s"], ks["spread"] * ks["s"])
            f.update(levels=levels, batch=batch, s_per_bit=f["s"] / batch, bootstrap_without_keyswitch=b, private_keyswitch=ks,
                     lwe_keyswitch_yardstick=y, allowed_s=allowed, within=f["s"] <= allowed)
            res["forms"][f"levels={levels} batch={batch}"] = f
            print(f"  ell_cb {levels} batch {batch:5d}  handle {f['s'] * 1e3:10.3f} ms/call  {f['s_per_bit'] * 1e6:10.1f} us/bit  "
                  f"spread {100 * f['spread']:5.2f} %  |  bootstrap x{rows} {b['s'] * 1e3:10.3f} ms ({100 * b['spread']:5.2f} %)  + "
                  f"private key switch {ks['s'] * 1e3:9.3f} ms ({100 * ks['spread']:5.2f} %)  {ks['mac_per_s'] / 1e12:6.3f} T mac/s  "
                  f"=> allowed {allowed * 1e3:10.3f} ms  {'ok' if f['within'] else 'SLOWER'}  |  lwe_keyswitch of the same size "
                  f"{y['s'] * 1e3:9.3f} ms ({100 * y['spread']:5.2f} %)  {y['mac_per_s'] / 1e12:6.3f} T mac/s", flush=True)
            del lwe, out, many, extracted, wide, wide_out
        del ctx
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lwe", type=int, default=630, help="the LWE dimension n of the inputs")
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
