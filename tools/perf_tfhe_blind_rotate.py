#!/usr/bin/env python3
"""Batched blind rotation over the TFHE product (pfhe_tfhe{,32}_blindrot_*): rotation steps per second of the whole-loop
kernel, of the forced per-step form (PFHE_DISABLE_FUSED_TFHE_BLINDROT), of the same loop built from public calls, and the
standalone product's rate at the same shape — device events after a warm-up.

    python tools/perf_tfhe_blind_rotate.py [--rounds 5] [--reps 2] [--shapes 0,1] [--batch 8192] [--json out.json]

The two forms of the handle are timed in alternation (round after round in one process), so their ratio can be set
against the run-to-run spread seen in the same run: `spread` is (max - min) / median of a form's rounds.  Step bytes are
computed from the shapes: the whole-loop form moves ACC once per rotation and one key per step; the per-step form adds
D written and read, E written and read, and ACC gathered, read and written per step.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import primus_fhe_amd as p  # noqa: E402

SWITCH = "PFHE_DISABLE_FUSED_TFHE_BLINDROT"
# (word bits, log_n, k, log_basis, ell, n_steps)
SHAPES = [
    (32, 10, 1, 7, 3, 64),
    (32, 11, 1, 10, 2, 64),
    (64, 11, 1, 15, 2, 64),
    (64, 12, 1, 15, 2, 16),   # a per-step shape: both handles take the same form
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


def run(bits, log_n, k, lb, ell, n_steps, batch, rounds, reps):
    n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    basis = p.ApproxSignedBasis(bits, lb, ell)
    loop = p.TfheBlindRotateContext(fft, basis, k)
    os.environ[SWITCH] = "1"
    try:
        steps = p.TfheBlindRotateContext(fft, basis, k)
    finally:
        os.environ.pop(SWITCH, None)
    prod = p.TfheFftContext(fft, basis, k)
    W, G = loop.glwe_len(), loop.key_len()
    acc = rand_words(bits, batch * W, 1)
    bsk = torch.empty(n_steps * G, dtype=torch.complex128, device="cuda")
    fft.forward_torus_dev(rand_words(bits, n_steps * G, 2), bsk)     # full-torus keys
    exps = torch.from_numpy(np.random.default_rng(3).integers(0, 2 * n, batch * n_steps).astype(np.int32)).cuda()
    forms = {"whole_loop": lambda: p.tfhe_blind_rotate_dev(acc, bsk, exps, loop),
             "per_step": lambda: p.tfhe_blind_rotate_dev(acc, bsk, exps, steps)}
    rot, e = torch.empty_like(acc), torch.empty_like(acc)
    ex_step = exps[:batch].contiguous()

    def public_loop():
        for i in range(n_steps):
            fft.mul_monomial_each_to_dev(acc, ex_step, rot, polys_per_exp=k + 1)
            rot.sub_(acc)
            p.tfhe_external_product_to_dev(rot, bsk[i * G:(i + 1) * G], e, prod)
            acc.add_(e)

    for fn in list(forms.values()) + [public_loop]:
        fn()  # warm-up
    total = batch * n_steps
    rates = {name: [] for name in forms}
    for _ in range(rounds):          # same-process alternation
        for name, fn in forms.items():
            rates[name].append(total / timed(fn, reps))
    key0 = bsk[:G]
    t_prod = timed(lambda: p.tfhe_external_product_to_dev(acc, key0, e, prod), reps * 8)
    t_pub = timed(public_loop, 1)
    w = bits // 8
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": basis.decompose_length(), "batch": batch,
           "n_steps": n_steps, "whole_loop_is_a_kernel": loop.scratch_bytes() == 0,
           "product_per_s": batch / t_prod, "public_loop_steps_per_s": total / t_pub,
           "step_bytes_whole_loop": G * 16 + 2 * batch * W * w / n_steps,
           "step_bytes_per_step": G * 16 + 7 * batch * W * w}
    for name, r in rates.items():
        med = statistics.median(r)
        res[name + "_steps_per_s"] = med
        res[name + "_rounds"] = r
        res[name + "_spread"] = (max(r) - min(r)) / med
    res["whole_loop_vs_per_step"] = res["whole_loop_steps_per_s"] / res["per_step_steps_per_s"]
    res["beats_spread"] = min(rates["whole_loop"]) > max(rates["per_step"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=0, help="override the steps of every shape")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    rows = []
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    for bits, log_n, k, lb, ell, n_steps in pick:
        r = run(bits, log_n, k, lb, ell, a.steps or n_steps, a.batch, a.rounds, a.reps)
        rows.append(r)
        form = "whole-loop kernel" if r["whole_loop_is_a_kernel"] else "per-step form (no whole-loop kernel on this shape)"
        print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={r['ell']} batch={a.batch} steps={r['n_steps']}: default handle = {form}\n"
              f"  default  {r['whole_loop_steps_per_s'] / 1e6:8.3f} M steps/s (spread {100 * r['whole_loop_spread']:.1f} %)"
              f" | forced per-step {r['per_step_steps_per_s'] / 1e6:8.3f} M steps/s (spread {100 * r['per_step_spread']:.1f} %)"
              f" | ratio {r['whole_loop_vs_per_step']:.3f}, every default round above every per-step round: {r['beats_spread']}\n"
              f"  public-call loop {r['public_loop_steps_per_s'] / 1e6:8.3f} M steps/s | standalone product "
              f"{r['product_per_s'] / 1e6:8.3f} M/s\n"
              f"  step bytes (computed from shapes): whole-loop {r['step_bytes_whole_loop'] / 2**20:.2f} MiB, per-step "
              f"{r['step_bytes_per_step'] / 2**20:.1f} MiB", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
