"""What the RNS side's two scratch-owning handles allocate: an external-product plan (csrc/pfhe_capi_rns.hip,
ExtprodPlanCore) and a blind-rotation handle (BlindRotCore), u64 and u32.  Per case: the pfhe_debug_alloc_count delta of
the create, the equal delta of the destroy, and scratch_bytes() against the buffer lists in the two structs' comments,
not against what the code gives.  The rings are the smallest the other RNS tests use, plus, per width, the smallest ring
at which the plan keeps compact signed digits."""
import pytest

from test_table_statuses_cpu import Q30, Q61

pytestmark = pytest.mark.gpu

K, L, ELL = 1, 3, 6     # Q61 at log B = 30 and Q30 at log B = 15: six levels each
# From the comments above the two structs, W = 8 or 4 bytes per word:
#   plan      the digit buffer, chunk * (k+1) * ell * L * N words, and, where one of the width's kernels wants them, the
#             compact signed digits, chunk * (k+1) * ell * N of 4 bytes (int32: log B <= 31 at u64, always at u32).  u64
#             keeps them for the small-ring kernel (N = 2^10, 2^11, k = 1) and for the lifting strided pass of the
#             two-pass rings; u32 for the fused kernels of N = 2^16, k = 1.  N = 2^5 has the digit buffer alone.
#   rotation  the plan's plus D, E and the second accumulator: three buffers of chunk * (k+1) * L * N words
#     u64, N = 2^5,  chunk 2: digits 2*2*6*3*32*8 = 18432, one buffer;  glue 3 * 2*2*3*32*8 = 9216
#     u64, N = 2^10, chunk 2: digits 2*2*6*3*1024*8 = 589824, compact 2*2*6*1024*4 = 98304, two;  glue 3 * 98304 = 294912
#     u32, N = 2^5,  chunk 2: digits 2*2*6*3*32*4 = 9216, one;  glue 3 * 2*2*3*32*4 = 4608
#     u32, N = 2^16, chunk 1: digits 2*6*3*65536*4 = 9437184, compact 2*6*65536*4 = 3145728, two;  glue 3 * 1572864 = 4718592
CASES = {
    "u64, N = 2^5": (True, 5, 2, 18432, 1, 9216),
    "u64, N = 2^10, compact digits": (True, 10, 2, 589824 + 98304, 2, 294912),
    "u32, N = 2^5": (False, 5, 2, 9216, 1, 4608),
    "u32, N = 2^16, compact digits": (False, 16, 1, 9437184 + 3145728, 2, 4718592),
}


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


@pytest.mark.parametrize("kind", ("plan", "rotation"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_rns_handle_scratch_and_allocations(p, case, kind):
    wide, log_n, chunk, plan_bytes, plan_allocs, glue_bytes = CASES[case]
    if wide:
        table, base = p.U64DcrtTable(log_n, list(Q61)), p.RNSBase(list(Q61))
        basis, plan, rotation = p.BigUintApproxSignedBasis(base, 30), p.DcrtGlevContext, p.BlindRotateContext
    else:
        table, base = p.U32DcrtTable(log_n, list(Q30)), p.RNSBase32(list(Q30))
        basis, plan, rotation = p.BigUintApproxSignedBasis32(base, 15), p.DcrtGlevContext32, p.BlindRotateContext32
    assert len(Q61) == len(Q30) == L and basis.decompose_length() == ELL
    scratch, allocs = (plan_bytes, plan_allocs) if kind == "plan" else (plan_bytes + glue_bytes, plan_allocs + 3)
    count = p.lib().pfhe_debug_alloc_count
    before = count()
    ctx = (plan if kind == "plan" else rotation)(table, base, basis, K, chunk)
    created = count()
    assert ctx.scratch_bytes() == scratch and created - before == allocs and not ctx.in_use()
    ctx.__del__()
    assert count() - created == allocs
