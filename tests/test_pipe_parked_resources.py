"""Build-time check (no GPU): the parked forward pipelined kernel fits five workgroups per CU.

Five waves per SIMD leave 96 VGPRs (512 / 5, allocated in eights) and five workgroups per CU leave 31 744 bytes of LDS
(160 KiB in 1280-byte granules).  Read from the code-object metadata of the BUILT library; the dynamic LDS size of the
launch is PipeParked::kLdsBytes (csrc/pfhe_ntt_device.hpp), which a static_assert there holds below the same bound."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "ntt_pipe_fwd_kernel<PmArith, 12>"
LDS_PER_WG_AT_FIVE = 31744


def test_parked_forward_kernel_fits_five_workgroups():
    import primus_fhe_amd as p
    from primus_fhe_amd import _codeobj

    res = _codeobj.kernel_resources(p.build())
    assert KERNEL in res, sorted(k for k in res if "ntt_pipe" in k)
    r = res[KERNEL]
    assert r["vgpr"] + (r["agpr"] or 0) <= 96, r
    assert r["scratch"] == 0, r
    # dynamic LDS as launched: fifteen parked rows of 64 lanes per wave, four waves
    src = open(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_ntt_device.hpp")).read()
    rows = int(re.search(r"struct PipeParked \{\s*static constexpr int kRows = (\d+);", src).group(1))
    assert re.search(r"kLdsBytes = 4 \* kWaveWords \* \(u32\)sizeof\(u64\);", src) and "kWaveWords = kRows * 64;" in src
    assert re.search(r"static_assert\(kLdsBytes <= kLdsPerWgAtFive", src) and f"kLdsPerWgAtFive = {LDS_PER_WG_AT_FIVE};" in src
    src_ntt = open(os.path.join(ROOT, "primus-fhe_amd", "csrc", "pfhe_ntt.hip")).read()
    assert re.search(r"launch<ntt_pipe_fwd_kernel<A, LOGB>>\(grid, threads, \(size_t\)PipeParked::kLdsBytes,", src_ntt)
    dynamic = 4 * rows * 64 * 8
    assert r["lds"] + dynamic <= LDS_PER_WG_AT_FIVE, (r, dynamic)
