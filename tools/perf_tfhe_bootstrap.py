#!/usr/bin/env python3
"""Batched programmable bootstrap (pfhe_tfhe{,32}_bootstrap_*): bootstraps per second of the handle, of the same stages run
as public calls (modulus switch, mul_monomial_each on a broadcast test vector, blind rotation, sample extraction, key
switch) and of the blind rotation alone — device events after a warm-up, the three forms in alternation within one process.

    python tools/perf_tfhe_bootstrap.py [--rounds 5] [--reps 1] [--shapes 0,1] [--batch 8192] [--lwe 630] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  The handle does the composition's work minus one
broadcast copy of the test vector and one allocation per buffer and call, so its median is expected at or above the
composition's; `handle_within_spread` is false when it is below by more than the larger of the two spreads — find out why
before relying on the handle.  `outside_rotation` is the share of the handle's device time not spent in the rotation,
1 - (rotation-alone time) / (handle time), from the same rounds.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

# (word bits, log_n, k, log_basis, ell, key-switch log_basis, key-switch ell)
SHAPES = [
    (32, 10, 1, 7, 3, 4, 3),
    (64, 11, 1, 15, 2, 4, 3),
]


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


def run(bits, log_n, k, lb, ell, ks_lb, ks_ell, n, batch, rounds, reps):
    big_n = 1 << log_n
    dtype = torch.int32 if bits == 32 else torch.int64
    fft = p.FullComplex64FftTable(log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, ks_lb, ks_ell)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis)
    rot = p.TfheBlindRotateContext(fft, basis, k)
    W, G, ext = ctx.glwe_len(), ctx.key_len(), ctx.extracted_dimension()
    lwe = rand_words(bits, batch * (n + 1), 1)
    bsk = torch.empty(n * G, dtype=torch.complex128, device="cuda")
    for i in range(n):                                             # full-torus keys, a key at a time to bound the input
        fft.forward_torus_dev(rand_words(bits, G, 100 + i), bsk[i * G:(i + 1) * G])
    tv = rand_words(bits, W, 2)
    ksk = rand_words(bits, ctx.ksk_len(), 3)
    out = torch.empty(batch * (n + 1), dtype=dtype, device="cuda")
    want = torch.empty_like(out)
    # the rotation alone runs on exponents and an accumulator prepared once (it rotates whatever the accumulator holds)
    exps0 = torch.empty(batch * n, dtype=torch.int32, device="cuda")
    neg_b0 = torch.empty(batch, dtype=torch.int32, device="cuda")
    p.lwe_modulus_switch_dev(lwe, n, log_n, exps0, neg_b0)
    acc0 = rand_words(bits, batch * W, 4)

    def handle():
        p.tfhe_bootstrap_dev(lwe, bsk, tv, ksk, out, ctx)

    def composition():
        exps = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        neg_b = torch.empty(batch, dtype=torch.int32, device="cuda")
        p.lwe_modulus_switch_dev(lwe, n, log_n, exps, neg_b)
        acc = torch.empty(batch * W, dtype=dtype, device="cuda")
        fft.mul_monomial_each_to_dev(tv.repeat(batch), neg_b, acc, polys_per_exp=k + 1)
        p.tfhe_blind_rotate_dev(acc, bsk, exps, rot)
        lwe_ext = torch.empty(batch * (ext + 1), dtype=dtype, device="cuda")
        p.glwe_sample_extract_dev(acc, lwe_ext, fft, k, 0)
        p.lwe_keyswitch_dev(lwe_ext, ksk, want, ext, n, ks_basis)

    def rotation():
        p.tfhe_blind_rotate_dev(acc0, bsk, exps0, rot)

    forms = {"handle": handle, "composition": composition, "rotation": rotation}
    for fn in forms.values():
        fn()  # warm-up
    torch.cuda.synchronize()
    same = bool(torch.equal(out, want))
    times = {name: [] for name in forms}
    for _ in range(rounds):          # same-process alternation
        for name, fn in forms.items():
            times[name].append(timed(fn, reps))
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": basis.decompose_length(), "lwe_dimension": n,
           "ks_log_basis": ks_lb, "ks_ell": ks_basis.decompose_length(), "batch": batch,
           "handle_equals_composition": same, "handle_scratch_bytes": ctx.scratch_bytes()}
    for name, t in times.items():
        med = statistics.median(t)
        res[name + "_s"] = med
        res[name + "_rounds_s"] = t
        res[name + "_per_s"] = batch / med
        res[name + "_spread"] = (max(t) - min(t)) / med
    spread = max(res["handle_spread"], res["composition_spread"])
    res["handle_vs_composition"] = res["handle_per_s"] / res["composition_per_s"]
    res["handle_within_spread"] = res["handle_per_s"] >= res["composition_per_s"] * (1 - spread)
    res["outside_rotation"] = 1 - res["rotation_s"] / res["handle_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--lwe", type=int, default=630, help="the LWE dimension n (steps of the rotation)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    rows = []
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    for shape in pick:
        r = run(*shape, a.lwe, a.batch, a.rounds, a.reps)
        rows.append(r)
        print(f"u{r['word_bits']} N=2^{r['log_n']} k={r['k']} logB={r['log_basis']} ell={r['ell']} n={r['lwe_dimension']} "
              f"key switch logB={r['ks_log_basis']} ell={r['ks_ell']} batch={r['batch']}: handle == composition word for word: "
              f"{r['handle_equals_composition']}\n"
              f"  handle      {r['handle_per_s'] / 1e3:9.2f} k bootstraps/s ({r['handle_s'] * 1e3:8.2f} ms, spread "
              f"{100 * r['handle_spread']:.2f} %)\n"
              f"  composition {r['composition_per_s'] / 1e3:9.2f} k bootstraps/s ({r['composition_s'] * 1e3:8.2f} ms, spread "
              f"{100 * r['composition_spread']:.2f} %)\n"
              f"  rotation    {r['rotation_per_s'] / 1e3:9.2f} k rotations/s  ({r['rotation_s'] * 1e3:8.2f} ms, spread "
              f"{100 * r['rotation_spread']:.2f} %)\n"
              f"  handle / composition {r['handle_vs_composition']:.4f}, not below it by more than the spread: "
              f"{r['handle_within_spread']} | device time outside the rotation: {100 * r['outside_rotation']:.2f} % | handle "
              f"scratch {r['handle_scratch_bytes'] / 2**20:.1f} MiB", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
