#!/usr/bin/env python3
"""Device key generation for the TFHE bootstrap (pfhe_tfhe{,32}_bsk_generate_dev, _ksk_generate_dev): seconds per key of
the bootstrapping key in the classic layout (g = 0) and the multi-bit layout at g = 2, and of the key-switch key, at the
two shapes of tools/perf_tfhe_bootstrap.py with n = 630 — device events after a warm-up, five rounds, median and spread.

    python tools/perf_tfhe_keygen.py [--rounds 5] [--shapes 0,1] [--lwe 630] [--json out.json] [--gaussian 256]

`spread` is (max - min) / median of a form's rounds in this run.  No threshold is judged: nothing was measured before.
A call generates in place and accumulates, so every round runs on the words the round before left: the cost does not
depend on the mask words, and the keys are binary throughout (a zero key coefficient is skipped by the whole workgroup).
`mac/s` counts k N^2 word multiply-adds per GLWE row, skipped ones included.  The split between
tfhe_glwe_body_mac_kernel and the forward transforms comes from one separate run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_tfhe_keygen.py --rounds 1 --no-ksk
    python tools/kernel_trace_summary.py DIR

--gaussian COUNT also runs each shape once the way a user would: keys with rounded Gaussian noise of the standard
deviations below, COUNT ciphertexts of every 2-bit message through the bootstrap handle, and prints the number of wrong
decodes.  That regime is statistical: the figure is reported, not judged.
"""
import argparse
import json
import math
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
GROUPINGS = (0, 2)
# standard deviations of the --gaussian run as fractions of the torus: the LWE side (inputs and key-switch key rows) and
# the GLWE side (bootstrapping key rows) per word width
LWE_STD = {32: 2.0 ** -15, 64: 2.0 ** -15}
GLWE_STD = {32: 2.0 ** -25, 64: 2.0 ** -45}
MESSAGE_BITS = 2


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def binary_key(bits, words, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 2, (words,), dtype=torch.int32 if bits == 32 else torch.int64, device="cuda", generator=g)


def summary(times):
    med = statistics.median(times)
    return {"s": med, "rounds_s": times, "spread": (max(times) - min(times)) / med}


def run(bits, log_n, k, lb, ell, ks_lb, ks_ell, n, rounds, with_ksk):
    big_n = 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, ks_lb, ks_ell)
    s, z = binary_key(bits, n, 1), binary_key(bits, k * big_n, 2)
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": basis.decompose_length(), "lwe_dimension": n,
           "ks_log_basis": ks_lb, "ks_ell": ks_basis.decompose_length(), "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={res['ell']} n={n} key switch logB={ks_lb} ell={res['ks_ell']}")
    for g in GROUPINGS:
        shape = p.TfheKeyShape(fft, basis, n, k, g)
        rand = p.torus_uniform(shape.bsk_len(), bits)
        out = torch.empty(shape.bsk_len(), dtype=torch.complex128, device="cuda")
        fn = lambda: p.tfhe_generate_bsk_dev(shape, s, z, rand, out)
        fn()  # warm-up
        f = summary([timed(fn) for _ in range(rounds)])
        rows = shape.bsk_len() // ((k + 1) * big_n)
        f.update(keys=shape.keys(), glwe_rows=rows, torus_MiB=rand.numel() * rand.element_size() / 2 ** 20,
                 fourier_MiB=out.numel() * 16 / 2 ** 20, mac_per_s=rows * k * big_n * big_n / f["s"])
        res["forms"][f"bsk g={g}"] = f
        print(f"  bsk g={g}  {f['s'] * 1e3:10.3f} ms/key  spread {100 * f['spread']:5.2f} %  {f['keys']} GGSWs, {rows} GLWE rows, "
              f"{f['mac_per_s'] / 1e12:.3f} T mac/s, torus {f['torus_MiB']:.0f} MiB + Fourier {f['fourier_MiB']:.0f} MiB", flush=True)
        del rand, out
    if with_ksk:
        rand = p.torus_uniform(k * big_n * ks_basis.decompose_length() * (n + 1), bits)
        fn = lambda: p.tfhe_generate_ksk_dev(z, s, ks_basis, rand)
        fn()
        f = summary([timed(fn) for _ in range(rounds)])
        f.update(rows=k * big_n * ks_basis.decompose_length(), MiB=rand.numel() * rand.element_size() / 2 ** 20)
        res["forms"]["ksk"] = f
        print(f"  ksk      {f['s'] * 1e3:10.3f} ms/key  spread {100 * f['spread']:5.2f} %  {f['rows']} rows, {f['MiB']:.0f} MiB",
              flush=True)
    return res


def gaussian(bits, log_n, k, lb, ell, ks_lb, ks_ell, n, count):
    """one bootstrap of `count` ciphertexts under generated keys with Gaussian noise; returns the number of wrong decodes"""
    big_n, pb = 1 << log_n, MESSAGE_BITS
    fft = p.FullComplex64FftTable(log_n)
    basis, ks_basis = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, ks_lb, ks_ell)
    ctx = p.TfheBootstrapContext(fft, basis, n, k, ks_basis)
    s, z = binary_key(bits, n, 11), binary_key(bits, k * big_n, 12)
    lwe_std, glwe_std = LWE_STD[bits] * 2.0 ** bits, GLWE_STD[bits] * 2.0 ** bits
    rand = p.torus_uniform(ctx.bsk_len(), bits).view(-1, k + 1, big_n)
    rand[:, k] = p.torus_noise(rand.shape[0] * big_n, bits, std=glwe_std).view(-1, big_n)
    bsk = p.tfhe_generate_bsk_dev(ctx, s, z, rand.view(-1))
    ksk = p.torus_uniform(ctx.ksk_len(), bits).view(-1, n + 1)
    ksk[:, n] = p.torus_noise(ksk.shape[0], bits, std=lwe_std)
    p.tfhe_generate_ksk_dev(z, s, ks_basis, ksk.view(-1))
    msgs = torch.arange(count, device="cuda") % (1 << pb)
    delta_shift = bits - pb - 1
    lwe = p.torus_uniform(count * (n + 1), bits).view(count, n + 1)
    lwe[:, n] = p.torus_noise(count, bits, std=lwe_std) + (msgs.to(lwe.dtype) << delta_shift)
    p.lwe_encrypt_dev(lwe.view(-1), s)
    # the half-box LUT of the identity: tv[j] = Delta * floor((j + N/2^(p+1)) 2^p / N), the last half box -Delta * 0 = 0
    box = big_n >> pb
    idx = (torch.arange(big_n, device="cuda") + box // 2) // box
    tv = torch.zeros((k + 1, big_n), dtype=lwe.dtype, device="cuda")
    tv[k] = torch.where(idx < (1 << pb), idx, torch.zeros_like(idx)).to(lwe.dtype) << delta_shift
    out = torch.empty(count * (n + 1), dtype=lwe.dtype, device="cuda")
    p.tfhe_bootstrap_dev(lwe.view(-1), bsk, tv.view(-1), ksk.view(-1), out, ctx)
    p.lwe_phase_dev(out, s)
    phases = out.view(count, n + 1)[:, n]
    decoded = ((phases + (1 << (delta_shift - 1))) >> delta_shift) & ((2 << pb) - 1)
    return int((decoded != msgs.to(decoded.dtype)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lwe", type=int, default=630, help="the LWE dimension n (even, for g = 2)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--no-ksk", action="store_true", help="bootstrapping keys only (a shorter trace)")
    ap.add_argument("--gaussian", type=int, default=0, metavar="COUNT", help="also bootstrap COUNT ciphertexts under Gaussian noise")
    a = ap.parse_args()
    rows = []
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    for shape in pick:
        r = run(*shape, a.lwe, a.rounds, not a.no_ksk)
        if a.gaussian:
            wrong = gaussian(*shape, a.lwe, a.gaussian)
            r["gaussian"] = {"ciphertexts": a.gaussian, "wrong_decodes": wrong, "lwe_std": LWE_STD[shape[0]],
                             "glwe_std": GLWE_STD[shape[0]], "message_bits": MESSAGE_BITS}
            print(f"  Gaussian noise (LWE std 2^{round(math.log2(LWE_STD[shape[0]]))}, GLWE std "
                  f"2^{round(math.log2(GLWE_STD[shape[0]]))} of the torus, {MESSAGE_BITS}-bit messages): "
                  f"{wrong} wrong decodes of {a.gaussian} (reported, not judged)", flush=True)
        rows.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
