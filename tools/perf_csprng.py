#!/usr/bin/env python3
"""The random layer (pfhe_rand{,32}_*): fill rates at 2^26 words beside a plain device copy of the same bytes and beside
torus_uniform, and fresh LWE encryptions at n = 630, batch 1, 64 and 8192, as three compositions — u32 and u64, device events
after a warm-up, five rounds, forms in alternation (odd rounds in reverse order), median and spread.

    python tools/perf_csprng.py [--rounds 5] [--bits 32,64] [--log-words 26] [--batches 1,64,8192] [--limit 600] [--json out.json]

Every word width runs in a process of its own under its own time limit (--limit seconds); the first one that fails ends the
run.  A timed window is `reps` calls between two device events (reps chosen so that a window is milliseconds, not one
launch); the figure is the window over reps.  `spread` is (max - min) / median of a form's rounds in this run.
  fill, at W = 2^log-words words:
    - uniform: torus_uniform_dev;  rows: tfhe_fill_rows_dev at (mask_len, body_len) = (630, 1) on floor(W / 631) rows;
    - copy: torch's device-to-device copy of as many bytes (read + write: the GB/s column counts the bytes WRITTEN, as for
      the fills, so the copy's traffic is twice that);  torus_uniform: the package's statistical filler (torch's Philox),
      which exists at the parent commit and allocates its result.
  encrypt, at n = 630 on `batch` ciphertexts with TUniform(b) / bound 2^b noise, b = BITS / 2:
    - parent: torus_uniform + torus_noise into the body slots + lwe_encrypt_dev (the parent commit's composition);
    - rows: tfhe_fill_rows_dev + lwe_encrypt_dev;
    - seeded: lwe_encrypt_seeded_dev (the mask never stored; batch words written instead of batch * 631).
Nothing is judged: the lines record what was measured, and `seeded/rows` says faster, same or slower beyond the spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIMENSION = 630


def summary(times):
    med = statistics.median(times)
    return {"s": med, "rounds_s": times, "spread": (max(times) - min(times)) / med}


def run(bits, rounds, log_words, batches):
    sys.path.insert(0, ROOT)
    import torch

    import primus_fhe_amd as p

    def timed(fn, reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3 / reps

    def measure(forms, reps):
        times = {name: [] for name in forms}
        for fn in forms.values():
            fn()  # warm-up
        for i in range(rounds):
            order = list(forms.items())
            for name, fn in (reversed(order) if i % 2 else order):
                times[name].append(timed(fn, reps))
        return {name: summary(t) for name, t in times.items()}

    dtype = torch.int32 if bits == 32 else torch.int64
    word, b = bits // 8, bits // 2
    mask, noise = p.RandSeed(bytes(range(32)), 1), p.RandSeed(bytes(range(1, 33)), 2)
    lines = []

    # ---- fill ----
    words = 1 << log_words
    row = DIMENSION + 1
    out, src = torch.empty(words, dtype=dtype, device="cuda"), torch.zeros(words, dtype=dtype, device="cuda")
    rows_out = out[:words // row * row]
    forms = {
        "uniform": lambda: p.torus_uniform_dev(mask, 0, out),
        "rows": lambda: p.tfhe_fill_rows_dev(mask, noise, 0, DIMENSION, 1, b, rows_out),
        "copy": lambda: out.copy_(src),
        "torus_uniform": lambda: p.torus_uniform(words, bits),
    }
    res = measure(forms, 8)
    text = f"u{bits} fill 2^{log_words} words"
    for name, r in res.items():
        written = (rows_out.numel() if name == "rows" else words) * word
        r["bytes_written"] = written
        text += f"  |  {name} {r['s'] * 1e6:9.1f} us ({100 * r['spread']:4.1f} %) {written / r['s'] / 1e9:7.1f} GB/s"
    text += (f"  |  uniform / torus_uniform x{res['torus_uniform']['s'] / res['uniform']['s']:5.2f}"
             f"  copy / uniform x{res['uniform']['s'] / res['copy']['s']:5.2f}")
    print(text, flush=True)
    lines.append({"word_bits": bits, "kind": "fill", "words": words, "forms": res})
    del out, src, rows_out

    # ---- fresh encryptions ----
    key = torch.empty(DIMENSION, dtype=dtype, device="cuda")
    p.torus_binary_dev(noise.with_nonce(3), 0, key)
    for batch in batches:
        lwe = torch.empty(batch * row, dtype=dtype, device="cuda")
        bodies = torch.zeros(batch, dtype=dtype, device="cuda")

        def parent():
            ct = p.torus_uniform(batch * row, bits)
            ct.view(batch, row)[:, DIMENSION] = p.torus_noise(batch, bits, bound=1 << b)
            p.lwe_encrypt_dev(ct, key)

        def by_rows():
            p.tfhe_fill_rows_dev(mask, noise, 0, DIMENSION, 1, b, lwe)
            p.lwe_encrypt_dev(lwe, key)

        forms = {"parent": parent, "rows": by_rows,
                 "seeded": lambda: p.lwe_encrypt_seeded_dev(mask, noise, 0, key, b, bodies)}
        res = measure(forms, 32 if batch <= 64 else 8)
        # the same ciphertexts: the seeded bodies of one call against the rows form's body slots
        bodies.zero_()
        p.lwe_encrypt_seeded_dev(mask, noise, 0, key, b, bodies)
        by_rows()
        same = bool(torch.equal(bodies, lwe.view(batch, row)[:, DIMENSION]))
        rw, sd = res["rows"], res["seeded"]
        gap = max(rw["spread"], sd["spread"]) * rw["s"]
        verdict = "faster" if rw["s"] - sd["s"] > gap else "slower" if sd["s"] - rw["s"] > gap else "same"
        text = f"u{bits} encrypt n {DIMENSION} batch {batch:5d}"
        for name, r in res.items():
            text += f"  |  {name} {r['s'] * 1e6:9.1f} us ({100 * r['spread']:4.1f} %) {batch / r['s'] / 1e6:8.3f} Mct/s"
        text += (f"  |  seeded/rows x{rw['s'] / sd['s']:5.2f} {verdict}  rows/parent x{res['parent']['s'] / rw['s']:5.2f}"
                 f"  |  bytes stored {batch * word} against {batch * row * word}  |  same words {same}")
        print(text, flush=True)
        lines.append({"word_bits": bits, "kind": "encrypt", "dimension": DIMENSION, "batch": batch, "same_words": same,
                      "seeded_against_rows": verdict, "forms": res})
        del lwe, bodies
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bits", default="32,64")
    ap.add_argument("--log-words", type=int, default=26)
    ap.add_argument("--batches", default="1,64,8192")
    ap.add_argument("--limit", type=int, default=600, help="seconds one word width may take")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)        # the word width: the child's work
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    if a.one:
        print("JSON " + json.dumps(run(int(a.one), a.rounds, a.log_words, batches)))
        return
    lines = []
    for bits in (int(v) for v in a.bits.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(bits), "--rounds", str(a.rounds), "--batches", a.batches,
               "--log-words", str(a.log_words)]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        limit = threading.Timer(a.limit, child.kill)
        limit.start()
        for line in child.stdout:      # passed on line by line, as the child prints
            if line.startswith("JSON "):
                lines += json.loads(line[5:])
            else:
                print(line, end="", flush=True)
        child.wait()
        limit.cancel()
        if child.returncode != 0:      # nothing more is started on the device after a failure or a time limit
            sys.exit(f"u{bits} ended with status {child.returncode}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
