#!/usr/bin/env python3
"""The circuit bootstrap handle beside the two calls whose work it queues, timed as ONE region: tools/perf_tfhe_cbs.py times
tfhe_bootstrap_dev and lwe_private_keyswitch_dev each in a loop of its own, where each finds its own key in the Infinity
Cache; here a bootstrap, the key switch right behind it (an event in between, nothing else), the key switch behind itself
and the handle alternate, five rounds, medians.  The two shapes of that tool, n = 630, k = 1, ell_cb 4, batch 1 and 1024.

    python tools/perf_tfhe_cbs_pair.py
"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import primus_fhe_amd as p

def ev():
    return torch.cuda.Event(enable_timing=True)

for bits, log_n, lb, ell in ((64, 11, 15, 2), (32, 10, 7, 3)):
    k, n, big_n = 1, 630, 1 << log_n
    fft = p.FullComplex64FftTable(log_n)
    basis, pf = p.ApproxSignedBasis(bits, lb, ell), p.ApproxSignedBasis(bits, 4, 3)
    glwe, ext = 2 * big_n, big_n + 1
    torus = p.torus_uniform(n * 2 * ell * glwe, bits)
    bsk = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, bsk, fft)
    del torus
    pfksk = p.torus_uniform(2 * ext * 3 * glwe, bits)
    tv = p.torus_uniform(glwe, bits)
    boot = p.TfheBootstrapContext(fft, basis, n, k)
    levels = 4
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, p.ApproxSignedBasis(bits, 4, levels), pf)
    for batch in (1, 1024):
        rows = batch * levels
        lwe = p.torus_uniform(batch * (n + 1), bits)
        many = p.torus_uniform(rows * (n + 1), bits)
        extracted = torch.empty(rows * ext, dtype=lwe.dtype, device="cuda")
        out = torch.empty(batch * ctx.ggsw_len(), dtype=lwe.dtype, device="cuda")
        bs = lambda: p.tfhe_bootstrap_dev(many, bsk, tv, None, extracted, boot)
        ks = lambda: p.lwe_private_keyswitch_dev(extracted, pfksk, out, big_n, levels, fft, pf, k)
        hd = lambda: p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx)
        bs(); ks(); hd()
        tb, tk_behind, tk_alone, th, tpair = [], [], [], [], []
        for _ in range(5):
            torch.cuda.synchronize()
            a, b, c = ev(), ev(), ev()
            a.record(); bs(); b.record(); ks(); c.record(); c.synchronize()
            tb.append(a.elapsed_time(b)); tk_behind.append(b.elapsed_time(c)); tpair.append(a.elapsed_time(c))
            a, b = ev(), ev()
            a.record(); ks(); b.record(); b.synchronize()
            tk_alone.append(a.elapsed_time(b))
            a, b = ev(), ev()
            a.record(); hd(); b.record(); b.synchronize()
            th.append(a.elapsed_time(b))
        med = statistics.median
        print(f"u{bits} N=2^{log_n} ell_cb {levels} batch {batch:5d}: bootstrap x{rows} {med(tb):9.3f} ms | key switch right behind it "
              f"{med(tk_behind):8.3f} ms | key switch behind itself {med(tk_alone):8.3f} ms | the pair as one region {med(tpair):9.3f} ms | "
              f"handle {med(th):9.3f} ms", flush=True)
