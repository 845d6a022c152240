#!/usr/bin/env python3
"""The linear layer with clear weights (pfhe_lwe{,32}_linear*_dev): time per call at dimension 630, (in_features,
out_features) = (128, 128), (784, 128), (128, 10), (128, 1), batch 1 and 64, u32 and u64 — device events after a warm-up,
five rounds, forms in alternation (odd rounds in reverse order), median and spread.

    python tools/perf_lwe_linear.py [--rounds 5] [--bits 32,64] [--shapes 0,1,2,3] [--batches 1,64] [--limit 600] [--json out.json]

Every word width runs in a process of its own under its own time limit (--limit seconds); the first one that fails ends the
run.  `spread` is (max - min) / median of a form's rounds in this run.  The forms of one line:
  - word: lwe_linear_dev with weights of the words' dtype (the int8 weights, sign-extended);
  - i8: lwe_linear_dev with the int8 weights;
  - torch: the fastest of two compositions of existing public torch operations that give the same words, named on the line:
      `by input`:  out += w[:, i] (outer) x[:, i], one addcmul_ per input on (batch, out_features, row);
      `by output`: out[:, o] = (w[o][:, None] * x).sum(1), one product and one sum per output;
  - at batch 1, keyswitch: lwe_keyswitch_dev at batch = out_features, in_dimension * ell = in_features (log B 4, ell 4) and
    the same 631 columns: the same traffic plus the digit stage, on the key switch's fixed tile of eight rows per thread
    where the linear call picks its rows per thread by the grid (tools/microbench13_linear_tiles.hip compares those
    instances); recorded per multiply-add, not judged.
JUDGED on every line, for each of word and i8: the call's median must not be longer than the composition's by more than the
larger of the two spreads (taken of the composition's median), and the words must be the same; the line ends in `ok` or
`SLOWER`.  i8 against word is reported as a ratio with `faster`, `same` or `slower` beyond the spread.  Beside every form:
multiply-adds per second (batch * out_features * in_features * row) and the bytes per second of the traffic the rule needs
(inputs read once, outputs written once, weights once)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIMENSION = 630
SHAPES = [(128, 128), (784, 128), (128, 10), (128, 1)]         # (in_features, out_features)
KS_BASIS = (4, 4)


def summary(times):
    med = statistics.median(times)
    return {"s": med, "rounds_s": times, "spread": (max(times) - min(times)) / med}


def run(bits, rounds, shapes, batches):
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

    def measure(forms):
        times = {name: [] for name in forms}
        for fn in forms.values():
            fn()  # warm-up
        for i in range(rounds):
            order = list(forms.items())
            for name, fn in (reversed(order) if i % 2 else order):
                times[name].append(timed(fn))
        return {name: summary(t) for name, t in times.items()}

    row, word = DIMENSION + 1, bits // 8
    rows = []
    for in_f, out_f in shapes:
        w8 = torch.randint(-128, 128, (out_f, in_f), dtype=torch.int8, device="cuda")
        ww = w8.to(torch.int32 if bits == 32 else torch.int64)
        bias = p.torus_uniform(out_f, bits)
        for batch in batches:
            x = p.torus_uniform(batch * in_f * row, bits)
            out_w, out_8, out_t = (torch.empty(batch * out_f * row, dtype=x.dtype, device="cuda") for _ in range(3))
            xv, tv = x.view(batch, in_f, row), out_t.view(batch, out_f, row)

            def by_input():
                tv.zero_()
                tv[:, :, DIMENSION] = bias
                for i in range(in_f):
                    tv.addcmul_(ww[:, i].view(1, out_f, 1), xv[:, i].unsqueeze(1))

            def by_output():
                for o in range(out_f):
                    tv[:, o] = (ww[o].view(1, in_f, 1) * xv).sum(1)
                tv[:, :, DIMENSION] += bias

            # which composition is faster here: one timed call each after a warm-up
            by_input(), by_output()
            name_t, torch_form = min((("by input", by_input), ("by output", by_output)), key=lambda f: timed(f[1]))
            forms = {
                "word": lambda: p.lwe_linear_dev(x, ww, bias, out_w, DIMENSION, in_f, out_f),
                "i8": lambda: p.lwe_linear_dev(x, w8, bias, out_8, DIMENSION, in_f, out_f),
                "torch": torch_form,
            }
            ks_args = None
            if batch == 1 and in_f % KS_BASIS[1] == 0:
                in_dim = in_f // KS_BASIS[1]
                ks_basis = p.ApproxSignedBasis(bits, *KS_BASIS)
                ks_in = p.torus_uniform(out_f * (in_dim + 1), bits)
                ksk = p.torus_uniform(in_f * row, bits)
                ks_out = torch.empty(out_f * row, dtype=x.dtype, device="cuda")
                forms["keyswitch"] = lambda: p.lwe_keyswitch_dev(ks_in, ksk, ks_out, in_dim, DIMENSION, ks_basis)
                ks_args = (ks_in, ksk, ks_out)
            res = measure(forms)
            same = bool(torch.equal(out_w, out_t)) and bool(torch.equal(out_8, out_t))
            macs = batch * out_f * in_f * row
            traffic = (batch * (in_f + out_f) * row + out_f) * word
            t = res["torch"]
            line = {"word_bits": bits, "in_features": in_f, "out_features": out_f, "batch": batch, "composition": name_t,
                    "same_words": same, "macs": macs, "bytes": traffic, "forms": res}
            text = f"u{bits} in {in_f:4d} out {out_f:4d} batch {batch:3d}"
            for name in ("word", "i8"):
                r = res[name]
                r["holds"] = same and r["s"] - t["s"] <= max(r["spread"], t["spread"]) * t["s"]
                text += (f"  |  {name} {r['s'] * 1e6:9.1f} us ({100 * r['spread']:4.1f} %) {macs / r['s'] / 1e12:6.3f} TMAC/s "
                         f"{traffic / r['s'] / 1e9:7.1f} GB/s {'ok' if r['holds'] else 'SLOWER'}")
            wd, i8 = res["word"], res["i8"]
            gap = max(wd["spread"], i8["spread"]) * wd["s"]
            verdict = "faster" if wd["s"] - i8["s"] > gap else "slower" if i8["s"] - wd["s"] > gap else "same"
            line["i8_against_word"] = verdict
            text += (f"  |  i8/word x{wd['s'] / i8['s']:5.2f} {verdict}  |  torch {name_t} {t['s'] * 1e6:10.1f} us "
                     f"({100 * t['spread']:4.1f} %) x{t['s'] / wd['s']:7.1f}  |  same words {same}")
            if "keyswitch" in res:
                k = res["keyswitch"]
                text += (f"  |  keyswitch {k['s'] * 1e6:8.1f} us ({100 * k['spread']:4.1f} %): {k['s'] / macs * 1e12:6.3f} ps/MAC, "
                         f"word {wd['s'] / macs * 1e12:6.3f} ps/MAC")
            print(text, flush=True)
            rows.append(line)
            del x, out_w, out_8, out_t, ks_args
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bits", default="32,64")
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--limit", type=int, default=600, help="seconds one word width may take")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)        # the word width: the child's work
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    shapes = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    if a.one:
        print("JSON " + json.dumps(run(int(a.one), a.rounds, shapes, batches)))
        return
    rows = []
    for bits in (int(v) for v in a.bits.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(bits), "--rounds", str(a.rounds), "--batches", a.batches]
        if a.shapes:
            cmd += ["--shapes", a.shapes]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        limit = threading.Timer(a.limit, child.kill)
        limit.start()
        for line in child.stdout:      # passed on line by line, as the child prints
            if line.startswith("JSON "):
                rows += json.loads(line[5:])
            else:
                print(line, end="", flush=True)
        child.wait()
        limit.cancel()
        if child.returncode != 0:      # nothing more is started on the device after a failure or a time limit
            sys.exit(f"u{bits} ended with status {child.returncode}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
