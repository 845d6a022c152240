"""Time of the base converter's kernels on wide 62-bit bases (device-table form, ConvWide<16> / <24> / <32>): fast
conversion, the pair form and the exact form on N = 2^20 coefficients (COEFFS).  PFHE_LIB_PATH selects another build of the
library, so the same script times two builds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import primus_fhe_amd as p
from primes import ntt_primes_below

P = ntt_primes_below(40, 62, 4)
n = int(os.environ.get("COEFFS", str(1 << 20)))
st = torch.cuda.current_stream()


def timed(fn, reps=200):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


print(f"library {os.path.basename(p.library_path())}, {n} coefficients")
rng = np.random.default_rng(1)
for lin, lout in ((16, 2), (16, 8), (24, 2), (24, 8), (32, 2), (32, 8)):
    mod_in, mod_out = P[:lin], P[32:32 + lout]
    x = torch.from_numpy(np.concatenate([rng.integers(0, q, n, dtype=np.uint64) for q in mod_in]).view(np.int64)).cuda()
    out = torch.empty(lout * n, dtype=torch.int64, device="cuda")
    one = torch.empty(n, dtype=torch.int64, device="cuda")
    conv = p.BaseConverter(p.RNSBase(mod_in), p.RNSBase(mod_out))
    exact = p.BaseConverter(p.RNSBase(mod_in), p.RNSBase(mod_out[:1]))
    line = f"{lin:2d} -> {lout}:  fast {timed(lambda: conv.fast_convert_array_dev(x, out, n)):7.3f} ms"
    if lout == 2:
        line += f"   pairs {timed(lambda: conv.fast_convert_array_to_pairs_dev(x, out, n)):7.3f} ms"
    line += f"   exact (-> 1) {timed(lambda: exact.exact_convert_array_dev(x, one, n)):7.3f} ms"
    print(line)
