#!/usr/bin/env python3
"""The CMUX tree (pfhe_tfhe{,32}_cmux_tree_dev): time per call and per CMUX node at the two shapes of
tools/perf_tfhe_bootstrap.py (k = 1: the fused form), depth 4 and 8, a shared table and batch 1, 64 and 1024 — device events
after a warm-up, five rounds, median and spread.

    python tools/perf_tfhe_cmux.py [--rounds 5] [--shapes 0,1] [--depths 4,8] [--batches 1,64,1024] [--json out.json]

`spread` is (max - min) / median of a form's rounds in this run.  The three forms are timed in turn within every round:
  - the handle;
  - the same tree from the calls there were before the handle: per input and level a wrapping subtraction,
    tfhe_external_product_to_dev on the level's nodes of that input with that input's key, a wrapping addition.  JUDGED at
    batch 64 and 1024: every round of the handle must beat every round of this composition; the line ends in `ok` or
    `SLOWER` (batch 1 is reported only);
  - as a yardstick (reported, not judged): tfhe_external_product_to_dev with ONE key on as many ciphertexts as the tree has
    nodes, batch * (2^depth - 1).  A CMUX moves three ciphertexts where the product moves two, and the tree reads
    batch * depth keys where the yardstick reads one: the line gives the ratio and both byte counts.
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


def composition(table, selectors, out, plan, depth, batch, scratch):
    """the tree as the calls of before: per input and level, subtraction, product with the input's key, addition"""
    glwe, key_len = plan.glwe_len(), plan.key_len()
    sel = selectors.view(batch, depth, key_len)
    for e in range(batch):
        nodes = table.view(-1, 2, glwe)
        for j in range(depth):
            count = 1 << (depth - 1 - j)
            diff = (nodes[:, 1] - nodes[:, 0]).view(-1)
            prod = scratch[:count * glwe]
            p.tfhe_external_product_to_dev(diff, sel[e, j], prod, plan)
            nxt = nodes[:, 0] + prod.view(count, glwe)
            nodes = nxt.view(-1, 2, glwe) if j + 1 < depth else nxt
        out[e * glwe:(e + 1) * glwe] = nodes.view(-1)


def run(bits, log_n, k, lb, ell, rounds, depths, batches):
    fft, basis = p.FullComplex64FftTable(log_n), p.ApproxSignedBasis(bits, lb, ell)
    plan = p.TfheFftContext(fft, basis, k)
    glwe, key_len = plan.glwe_len(), plan.key_len()
    word = bits // 8
    res = {"word_bits": bits, "log_n": log_n, "k": k, "log_basis": lb, "ell": ell, "forms": {}}
    print(f"u{bits} N=2^{log_n} k={k} logB={lb} ell={ell}  ciphertext {glwe * word / 1024:.0f} KiB  key {key_len * 16 / 1024:.0f} KiB")
    for depth in depths:
        ctx = p.TfheCmuxTreeContext(fft, basis, k, depth)
        table = p.torus_uniform(glwe << depth, bits)        # full-range words: the cost does not depend on them
        scratch = torch.empty((glwe << depth) // 2, dtype=table.dtype, device="cuda")
        for batch in batches:
            torus = p.torus_uniform(batch * depth * key_len, bits)
            selectors = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
            p.write_fourier_form(torus, selectors, fft)
            del torus
            nodes = batch * ((1 << depth) - 1)
            out, out_c = (torch.empty(batch * glwe, dtype=table.dtype, device="cuda") for _ in range(2))
            many, many_out = p.torus_uniform(nodes * glwe, bits), torch.empty(nodes * glwe, dtype=table.dtype, device="cuda")
            forms = {
                "handle": lambda: p.tfhe_cmux_tree_dev(table, selectors, out, ctx),
                "composition": lambda: composition(table, selectors, out_c, plan, depth, batch, scratch),
                "yardstick": lambda: p.tfhe_external_product_to_dev(many, selectors[:key_len], many_out, plan),
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
            beats = max(h["rounds_s"]) < min(c["rounds_s"])
            # bytes the tree and the yardstick must move at least: three and two ciphertexts per node, and the keys
            tree_bytes = nodes * 3 * glwe * word + batch * depth * key_len * 16
            yard_bytes = nodes * 2 * glwe * word + key_len * 16
            h.update(depth=depth, batch=batch, nodes=nodes, s_per_node=h["s"] / nodes, composition=c, yardstick=y,
                     same_words=same, judged=judged, beats_every_round=beats, ratio_to_yardstick=h["s"] / y["s"],
                     tree_bytes=tree_bytes, yardstick_bytes=yard_bytes)
            res["forms"][f"depth={depth} batch={batch}"] = h
            verdict = ("ok" if beats else "SLOWER") if judged else "-"
            print(f"  depth {depth} batch {batch:5d}  handle {h['s'] * 1e3:10.3f} ms/call  {h['s_per_node'] * 1e6:8.2f} us/node  "
                  f"spread {100 * h['spread']:5.2f} %  max {max(h['rounds_s']) * 1e3:10.3f}  |  composition {c['s'] * 1e3:10.3f} ms "
                  f"({100 * c['spread']:5.2f} %)  min {min(c['rounds_s']) * 1e3:10.3f}  x{c['s'] / h['s']:7.1f}  {verdict}  "
                  f"same words {same}  |  product x{nodes} one key {y['s'] * 1e3:9.3f} ms ({100 * y['spread']:5.2f} %)  "
                  f"handle / yardstick {h['ratio_to_yardstick']:5.2f}  bytes {tree_bytes / 2 ** 20:8.1f} / {yard_bytes / 2 ** 20:8.1f} MiB "
                  f"= {tree_bytes / yard_bytes:5.2f}", flush=True)
            del selectors, out, out_c, many, many_out
        del ctx, table, scratch
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depths", default="4,8")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    a = ap.parse_args()
    pick = [SHAPES[int(i)] for i in a.shapes.split(",")] if a.shapes else SHAPES
    depths, batches = ([int(v) for v in s.split(",")] for s in (a.depths, a.batches))
    rows = [run(*shape, a.rounds, depths, batches) for shape in pick]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
