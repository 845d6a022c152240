#!/usr/bin/env python3
"""The look-up table on encrypted bits (pfhe_tfhe{,32}_lut_eval_dev): time per call at the two shapes of
tools/perf_tfhe_bootstrap.py (k = 1: the fused form), one output, (tree depth, rotation bits) = (4, log N) and (0, log N), a
shared table, extract = 1 and batch 1, 64 and 1024 — device events after a warm-up, five rounds, median and spread.

    python tools/perf_tfhe_lut.py [--rounds 5] [--shapes 0,1] [--trees 4,0] [--batches 1,64,1024] [--limit 900] [--json out.json]

Every (shape, tree depth) runs in a process of its own under its own time limit (--limit seconds); the first one that fails
ends the run.  `spread` is (max - min) / median of a form's rounds in this run.  The forms are timed in turn within every
round, odd rounds in reverse order:
  - the handle: one tfhe_lut_eval_dev;
  - the composition of public calls: tfhe_cmux_tree_dev on the tree's keys, then per rotation step
    mul_monomial_each_to_dev and tfhe_cmux_dev on the step's keys, then glwe_sample_extract_dev.  The public calls take
    their keys end to end, so the keys of a level or step are gathered by stride in torch, inside the timing: that is what
    a caller holding the circuit bootstrap's output has to do.  JUDGED at batch 64 and 1024: the handle's median must be
    shorter than this form's by more than the larger of the two spreads (taken of the composition's median); the line ends
    in `ok` or `SLOWER` (batch 1 is reported only);
  - reported, not judged: the same composition on keys gathered before the clock starts.
All forms are checked to give the same words in the run."""
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


def summary(times):
    med = statistics.median(times)
    return {"s": med, "rounds_s": times, "spread": (max(times) - min(times)) / med}


def run(bits, log_n, k, lb, ell, t, rounds, batches):
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

    r, n = log_n, 1 << log_n
    pb = t + r
    fft, basis = p.FullComplex64FftTable(log_n), p.ApproxSignedBasis(bits, lb, ell)
    lut = p.TfheLutContext(fft, basis, k, t, r)
    cmux = p.TfheCmuxTreeContext(fft, basis, k, 1)
    tree = p.TfheCmuxTreeContext(fft, basis, k, t) if t else None
    glwe, key_len, lwe = lut.glwe_len(), lut.key_len(), k * n + 1
    word = bits // 8
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "tree_depth": t, "rot_bits": r, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={ell} (t, r) = ({t}, {r})  ciphertext {glwe * word / 1024:.0f} KiB  "
          f"key {key_len * 16 / 1024:.0f} KiB  nodes per input {(1 << t) - 1 + r} (a tree alone: {(1 << pb) - 1})", flush=True)
    table = p.torus_uniform(glwe << t, bits)                 # full-range words: the cost does not depend on them
    for batch in batches:
        selectors = torch.empty(batch * pb * key_len, dtype=torch.complex128, device="cuda")
        for e in range(0, batch, 16):                        # 16 inputs' keys per forward call bound the torus form
            c = min(16, batch - e)
            p.write_fourier_form(p.torus_uniform(c * pb * key_len, bits), selectors[e * pb * key_len:(e + c) * pb * key_len], fft)
        sel = selectors.view(batch, pb, key_len)
        exps = [torch.full((batch,), 2 * n - (1 << j), dtype=torch.int32, device="cuda") for j in range(r)]
        out, out_c, out_g = (torch.empty(batch * lwe, dtype=table.dtype, device="cuda") for _ in range(3))
        acc, rot = (torch.empty(batch * glwe, dtype=table.dtype, device="cuda") for _ in range(2))

        def composition(dst, keys_of):
            if t:
                p.tfhe_cmux_tree_dev(table, keys_of(None), acc, tree)
            else:
                acc.copy_(table.repeat(batch))
            for j in range(r):
                fft.mul_monomial_each_to_dev(acc, exps[j], rot, polys_per_exp=k + 1)
                p.tfhe_cmux_dev(acc, rot, keys_of(j), acc, cmux, 1)
            p.glwe_sample_extract_dev(acc, dst, fft, k, 0)

        gather = lambda j: (sel[:, r:] if j is None else sel[:, j]).contiguous().view(-1)
        ready = {j: gather(j) for j in ([None] if t else []) + list(range(r))}
        forms = {
            "handle": lambda: p.tfhe_lut_eval_dev(table, selectors, out, lut, 1),
            "composition": lambda: composition(out_c, gather),
            "gathered": lambda: composition(out_g, ready.__getitem__),
        }
        times = {name: [] for name in forms}
        for fn in forms.values():
            fn()  # warm-up
        same = bool(torch.equal(out, out_c)) and bool(torch.equal(out, out_g))
        for i in range(rounds):
            order = list(forms.items())
            for name, fn in (reversed(order) if i % 2 else order):
                times[name].append(timed(fn))
        h, c, g = (summary(times[name]) for name in ("handle", "composition", "gathered"))
        judged = batch > 1
        margin = max(h["spread"], c["spread"]) * c["s"]
        beats = c["s"] - h["s"] > margin
        h.update(batch=batch, composition=c, gathered=g, same_words=same, judged=judged, beats=beats,
                 key_bytes=batch * pb * key_len * 16)
        res["forms"][f"batch={batch}"] = h
        verdict = ("ok" if beats else "SLOWER") if judged else "-"
        print(f"  batch {batch:5d}  handle {h['s'] * 1e3:10.3f} ms/call  spread {100 * h['spread']:5.2f} %  |  composition "
              f"{c['s'] * 1e3:10.3f} ms ({100 * c['spread']:5.2f} %)  x{c['s'] / h['s']:6.2f}  {verdict}  |  keys gathered before "
              f"{g['s'] * 1e3:10.3f} ms ({100 * g['spread']:5.2f} %)  x{g['s'] / h['s']:6.2f}  |  same words {same}  keys "
              f"{batch * pb * key_len * 16 / 2 ** 20:8.1f} MiB", flush=True)
        del selectors, sel, ready, out, out_c, out_g, acc, rot
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trees", default="4,0")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--limit", type=int, default=900, help="seconds one (shape, tree depth) may take")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)        # "shape index,tree depth": the child's work
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    if a.one:
        shape, t = (int(v) for v in a.one.split(","))
        print("JSON " + json.dumps(run(*SHAPES[shape], t, a.rounds, batches)))
        return
    pick = [int(i) for i in a.shapes.split(",")] if a.shapes else range(len(SHAPES))
    rows = []
    for shape in pick:
        for t in (int(v) for v in a.trees.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{shape},{t}", "--rounds", str(a.rounds), "--batches",
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
                sys.exit(f"shape {shape} tree depth {t} ended with status {child.returncode}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
