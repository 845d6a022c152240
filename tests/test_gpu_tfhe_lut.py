"""GPU tests of the look-up table on encrypted bits (include/pfhe.h, pfhe_tfhe{,32}_lut_*, _rotate_by_bits*, _lut_eval*;
DESIGN.md §23): rule 1 word for word against the composition of public calls (mul_monomial_each_to_dev, then tfhe_cmux_dev
with the step's keys gathered by stride) at the shapes where the fused loop kernel's slot loop and the general form take
their paths, with chunking, in place, the host form and first_key > 0; all 2^r patterns in the exact regime; rule 2 against
its composition (the CMUX tree or rule-1 calls of the CMUX handle, rule 1, sample extraction), with a repeat call and a graph
replay; what the table means behind a circuit bootstrap on noisy keys, all on the device; errors and the lease."""
import itertools
import threading

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_cmux_model as xm
import tfhe_fft_model as m
import tfhe_lut_model as lm
from test_gpu_tfhe_cbs import device_randomness, product_model_error
from test_gpu_tfhe_fft import TORCH_INT, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import primus_fhe_amd as p
    return p


_TABLES = {}


def table(p, log_n):
    if log_n not in _TABLES:
        _TABLES[log_n] = p.FullComplex64FftTable(log_n)
    return _TABLES[log_n]


def empty_words(size, bits):
    import torch
    return torch.full((size,), -1, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")


def fourier_keys(p, fft, torus):
    import torch
    out = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, out, fft)
    return out


def rotation_composition(p, fft, cmux, inp, keys, r, s, o, keys_per_input, first_key, k, bits):
    """rule 1 as public calls: per step mul_monomial_each_to_dev with exponent 2N - 2^(j+s), then tfhe_cmux_dev with d0 the
    accumulator, d1 the rotated one, per_key = o and the step's key of every input gathered by stride in torch"""
    import torch
    glwe, key_len, n = cmux.glwe_len(), cmux.key_len(), fft.poly_length()
    count = inp.numel() // glwe
    acc = inp.clone()
    for j in range(r):
        exps = torch.full((count,), 2 * n - (1 << (j + s)), dtype=torch.int32, device="cuda")
        rot = empty_words(acc.numel(), bits)
        fft.mul_monomial_each_to_dev(acc, exps, rot, polys_per_exp=k + 1)
        step_keys = keys.view(count // o, keys_per_input, key_len)[:, first_key + j].contiguous().view(-1)
        nxt = empty_words(acc.numel(), bits)
        p.tfhe_cmux_dev(acc, rot, step_keys, nxt, cmux, o)
        acc = nxt
    return acc


def rotate_run(p, ctx, inp, keys, bits, keys_per_input=None, first_key=0):
    out = empty_words(inp.numel(), bits)
    p.tfhe_rotate_by_bits_dev(inp, keys, out, ctx, keys_per_input, first_key)
    return out


# ---------------- rule 1 against the composition of public calls ----------------

# bits, log_n, k, log_basis, ell (None: the full length, drop_bits 0), r, s, o
RULE1_CASES = [
    (32, 1, 1, 8, None, 1, 0, 1),      # fused: N = 2, one step with exponent 3, 255 idle threads; drop_bits 0; r + s = log N
    (64, 9, 1, 15, 2, 3, 0, 3),        # fused: exactly one slot per thread; s = 0
    (32, 10, 1, 7, 3, 2, 8, 3),        # fused: two slots; r + s = log N
    (64, 11, 1, 20, 1, 2, 0, 1),       # fused: four slots; ell = 1
    (32, 11, 1, 16, None, 3, 8, 3),    # fused: four slots at u32, drop_bits 0; r + s = log N
    (64, 10, 1, 15, 2, 10, 0, 1),      # fused: every one of the log N steps
    (32, 5, 2, 7, 3, 2, 3, 3),         # general: k = 2; r + s = log N
    (64, 12, 1, 15, 2, 2, 0, 3),       # general: k = 1 above the fused N
    (32, 12, 1, 10, 1, 1, 11, 1),      # general, ell = 1; r + s = log N
]


@pytest.mark.parametrize("bits,log_n,k,lb,ell,r,s,o", RULE1_CASES, ids=lambda v: str(v))
def test_rotation_equals_the_composition_of_public_calls(p, bits, log_n, k, lb, ell, r, s, o):
    """batch 3 with r + 2 keys per input of which the rotation takes those from 1 on; a default handle (one launch), chunk 2
    (a chunk smaller than the batch) and chunk 1 (with o = 3 every launch is one input's three outputs); in place; the host
    form; one accumulator alone"""
    import torch
    batch, kpi, first = 3, r + 2, 1
    rng = np.random.default_rng(bits + 10 * log_n + k + r)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    cmux = p.TfheCmuxTreeContext(fft, basis, k, 1)
    wide, two, one = (p.TfheLutContext(fft, basis, k, 0, r, outputs=o, log_stride=s, chunk=c) for c in (0, 2, 1))
    assert wide.key_len() == cmux.key_len() and wide.bits() == r and not wide.in_use()
    glwe, key_len = wide.glwe_len(), wide.key_len()
    inp = dev_words(rand_words(rng, bits, batch * o * glwe), bits)
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * kpi * key_len), bits))
    want = rotation_composition(p, fft, cmux, inp, keys, r, s, o, kpi, first, k, bits)
    for ctx in (wide, two, one, one):
        assert torch.equal(rotate_run(p, ctx, inp, keys, bits, kpi, first), want), ctx.scratch_bytes()
    acc = inp.clone()
    p.tfhe_rotate_by_bits_dev(acc, keys, acc, two, kpi, first)                # out is inp
    assert torch.equal(acc, want)
    host = np.zeros(batch * o * glwe, m.UINT[bits])
    p.tfhe_rotate_by_bits(host_words(inp, bits), keys.cpu().numpy(), host, two, kpi, first)
    assert np.array_equal(host, host_words(want, bits))
    # the last accumulator alone with its input's own keys: the words depend on neither the batch nor the launch
    own = keys.view(batch, kpi, key_len)[batch - 1, first:first + r].contiguous().view(-1)
    alone = rotate_run(p, wide, inp[-o * glwe:].clone(), own, bits)
    assert torch.equal(alone, want[-o * glwe:])
    fused = k == 1 and log_n <= 11
    assert wide.scratch_bytes() > two.scratch_bytes() > one.scratch_bytes() >= o * glwe * bits // 8
    assert (one.scratch_bytes() == o * glwe * bits // 8) == fused           # the general form owns more than the accumulators


# ---------------- the exact regime ----------------

@pytest.mark.parametrize("log_n, r, s, o", [(6, 3, 1, 2), (9, 4, 0, 1), (5, 5, 0, 1)])
def test_every_bit_pattern_rotates_by_its_clear_exponent_u32_exactly(p, log_n, r, s, o):
    """u32, trivial GGSWs of the bits in a basis that drops no bit: a digit times a gadget word is below 2^31, the f64
    arithmetic is exact, and out[a] IS X^{-x 2^s} inp[a] word for word: mul_monomial_each_to_dev on the clear exponent; the
    all-zero pattern returns inp"""
    import torch
    bits, k = 32, 1
    n = 1 << log_n
    rng = np.random.default_rng(log_n + r)
    mb = m.ApproxSignedBasis(bits, 8, 4)
    fft = table(p, log_n)
    ctx = p.TfheLutContext(fft, p.ApproxSignedBasis(bits, 8, 4), k, 0, r, outputs=o, log_stride=s, chunk=3)
    patterns = list(itertools.product((0, 1), repeat=r))
    glwe = ctx.glwe_len()
    inp = dev_words(rand_words(rng, bits, len(patterns) * o * glwe), bits)
    msgs = [b for pat in patterns for b in pat]
    keys = fourier_keys(p, fft, dev_words(xm.bit_ggsws(msgs, None, mb, log_n, k, rng, trivial=True), bits))
    got = rotate_run(p, ctx, inp, keys, bits)
    clear = [(2 * n - (xm.leaf_index(pat) << s)) % (2 * n) for pat in patterns for _ in range(o)]
    want = empty_words(inp.numel(), bits)
    fft.mul_monomial_each_to_dev(inp, torch.tensor(clear, dtype=torch.int32, device="cuda"), want, polys_per_exp=k + 1)
    assert torch.equal(got, want)
    assert xm.leaf_index(patterns[0]) == 0 and torch.equal(got[:o * glwe], inp[:o * glwe])


# ---------------- rule 2 against its composition ----------------

def eval_composition(p, fft, lut, cmux, tree, tbl, sel, batch, extract, k, bits):
    """stage A as tfhe_cmux_tree_dev on the tree's keys (o = 1) or as rule-1 calls of the CMUX handle with per_key =
    o 2^(t-1-j) and the level's key of every input; stage B as tfhe_rotate_by_bits_dev on the selectors themselves; stage C as
    glwe_sample_extract_dev per index"""
    import torch
    t, r, o, pb = lut.tree_depth, lut.rot_bits, lut.outputs, lut.bits()
    glwe, key_len = lut.glwe_len(), lut.key_len()
    keys = sel.view(batch, pb, key_len)
    if t == 0:
        acc = tbl.repeat(batch) if tbl.numel() == o * glwe and batch > 1 else tbl.clone()
    elif o == 1:
        acc = empty_words(batch * glwe, bits)
        p.tfhe_cmux_tree_dev(tbl, keys[:, r:].contiguous().view(-1), acc, tree)
    else:
        nodes = tbl.view(-1, glwe)
        if nodes.shape[0] == o << t:
            nodes = nodes.repeat(batch, 1)
        for j in range(t):
            pairs = nodes.view(-1, 2, glwe)
            d0, d1 = pairs[:, 0].contiguous().view(-1), pairs[:, 1].contiguous().view(-1)
            out = empty_words(d0.numel(), bits)
            p.tfhe_cmux_dev(d0, d1, keys[:, r + j].contiguous().view(-1), out, cmux, o << (t - 1 - j))
            nodes = out.view(-1, glwe)
        acc = nodes.reshape(-1)
    res = empty_words(acc.numel(), bits)
    p.tfhe_rotate_by_bits_dev(acc, sel, res, lut, pb, 0)
    if not extract:
        return res
    n = fft.poly_length()
    rows = torch.empty((batch * o, extract, k * n + 1), dtype=res.dtype, device="cuda")
    for i in range(extract):
        lwe = empty_words(batch * o * (k * n + 1), bits)
        p.glwe_sample_extract_dev(res, lwe, fft, k, i)
        rows[:, i] = lwe.view(batch * o, -1)
    return rows.view(-1)


def eval_run(p, ctx, tbl, sel, batch, extract, bits, stream=None):
    n, k = ctx.fft.poly_length(), ctx.glwe_dimension
    per = extract * (k * n + 1) if extract else ctx.glwe_len()
    out = empty_words(batch * ctx.outputs * per, bits)
    p.tfhe_lut_eval_dev(tbl, sel, out, ctx, extract, stream)
    return out


@pytest.mark.parametrize("bits,log_n,k", [(32, 6, 1), (64, 9, 1), (64, 4, 2)])
@pytest.mark.parametrize("o", [1, 2])
@pytest.mark.parametrize("t, r", [(0, 2), (2, 0), (1, 1), (3, 2)])
def test_table_evaluation_equals_its_composition(p, bits, log_n, k, t, r, o):
    """shared and per-input tables, extract 0, 1 and 2, a default handle and one of chunk 2 under a batch of 3, a repeat call"""
    import torch
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    batch, s = 3, 1
    rng = np.random.default_rng(bits + log_n + 10 * t + r + o)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    big, two = (p.TfheLutContext(fft, basis, k, t, r, outputs=o, log_stride=s, chunk=c) for c in (0, 2))
    cmux = p.TfheCmuxTreeContext(fft, basis, k, 1)
    tree = p.TfheCmuxTreeContext(fft, basis, k, t) if t else None
    glwe, pb = big.glwe_len(), t + r
    sel = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * pb * big.key_len()), bits))
    own = dev_words(rand_words(rng, bits, batch * (o << t) * glwe), bits)
    for tbl in (own, own[:(o << t) * glwe].clone()):
        for extract in (0, 1, 2):
            want = eval_composition(p, fft, big, cmux, tree, tbl, sel, batch, extract, k, bits)
            for ctx in (big, two, two):
                assert torch.equal(eval_run(p, ctx, tbl, sel, batch, extract, bits), want), (extract, ctx.scratch_bytes())
    if (t, r, o) == (1, 1, 2):
        per = 2 * (k * fft.poly_length() + 1)
        host = np.zeros(batch * o * per, m.UINT[bits])
        p.tfhe_lut_eval(host_words(own, bits), sel.cpu().numpy(), host, two, 2)
        assert np.array_equal(host, host_words(eval_composition(p, fft, big, cmux, tree, own, sel, batch, 2, k, bits), bits))


def test_graph_capture_replays_the_eager_call(p):
    """a linear capture on one stream: two chunks, two tree levels, the rotation and the extraction in the graph, replayed
    twice on fresh tables"""
    import torch
    bits, log_n, k, t, r, o, batch = 32, 8, 1, 2, 2, 2, 3
    rng = np.random.default_rng(78)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, 7, 3)
    ctx = p.TfheLutContext(fft, basis, k, t, r, outputs=o, chunk=2)
    glwe = ctx.glwe_len()
    sel = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * (t + r) * ctx.key_len()), bits))
    fresh = dev_words(rand_words(rng, bits, batch * (o << t) * glwe), bits)
    eager = eval_run(p, ctx, fresh, sel, batch, 1, bits)
    torch.cuda.synchronize()
    tbl, out = fresh.clone(), torch.zeros_like(eager)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            p.tfhe_lut_eval_dev(tbl, sel, out, ctx, 1)
    torch.cuda.current_stream().wait_stream(st)
    for _ in range(2):
        tbl.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------- meaning on noisy keys, end to end on the device ----------------

@pytest.mark.parametrize("case, t, r", lm.NOISY_LUTS,
                         ids=lambda c: str(c) if isinstance(c, int) else "u%d-N%d-k%d-n%d" % (c[0], 1 << c[1], c[2], c[3]))
def test_noisy_circuit_bootstrap_drives_the_table(p, case, t, r):
    """Binary keys, torus_noise(bound=E) on every row of both generated keys.  tfhe_generate_bsk_dev and
    tfhe_generate_pfksk_dev, tfhe_circuit_bootstrap_dev on the batch x p bit ciphertexts of all 2^p patterns (input e, bit j
    at e p + j), write_fourier_form, tfhe_lut_eval_dev with extract = 1 over a shared tfhe_lut_table of random 1-bit entries
    under one padding bit, lwe_phase_dev under the flattened GLWE key.  Every pattern decodes to its entry and the error stays
    within tfhe_lut_model.lut_bound of the row allowance (tfhe_cbs_model.row_bound plus the rotation's f64 allowance, as
    tests/test_gpu_tfhe_cbs.py) plus (t + r) (1 + k N) (4 model_err + 2) for the table's own f64 arithmetic.
    Largest errors seen on the device are in DESIGN.md §23's table."""
    import torch
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, pbits = case
    big_n, pb = 1 << log_n, t + r
    c = cm.noisy_case(*case, seed=4000 + bits + log_n + k)
    rng = np.random.default_rng(bits + log_n + pb)
    gen = torch.Generator(device="cuda").manual_seed(6000 + bits + log_n + k)
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = (p.ApproxSignedBasis(bits, *b) for b in ((lb, ell), (cb_lb, cb_ell), (pf_lb, pf_ell)))
    cbs = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    lut = p.TfheLutContext(fft, cbs_basis, k, t, r)
    assert lut.key_len() == cbs.ggsw_len()
    s, z_flat = dev_words(c["s"], bits), dev_words(bs.flatten_key(c["z"]), bits)
    torus = device_randomness(p, bits, log_n, k, n * (k + 1) * ell, noise, gen)
    pfksk = device_randomness(p, bits, log_n, k, (k + 1) * (k * big_n + 1) * pf_ell, noise, gen)
    bsk = p.tfhe_generate_bsk_dev(p.TfheKeyShape(fft, basis, n, k), s, z_flat, torus)
    p.tfhe_generate_pfksk_dev(z_flat, z_flat, fft, pfks_basis, pfksk, k)
    patterns = list(itertools.product((0, 1), repeat=pb))
    batch = len(patterns)
    msgs = np.array([b for pat in patterns for b in pat], np.uint64)
    lwe = bs.lwe_encrypt(msgs << np.uint64(bits - 1), c["s"], bits, rng)
    ggsw = empty_words(batch * pb * cbs.ggsw_len(), bits)
    p.tfhe_circuit_bootstrap_dev(dev_words(lwe, bits), bsk, pfksk, ggsw, cbs)
    selectors = fourier_keys(p, fft, ggsw)
    data = rng.integers(0, 1 << pbits, (1, 1 << pb))
    values = (data.astype(np.uint64) << np.uint64(bits - pbits - 1)).astype(m.UINT[bits])
    tbl = p.tfhe_lut_table(dev_words(values, bits), log_n, k, t, r)
    assert np.array_equal(host_words(tbl, bits), lm.lut_table(values, log_n, k, t, r))
    out = eval_run(p, lut, tbl.view(-1), selectors, batch, 1, bits)
    p.lwe_phase_dev(out, z_flat)
    phases = host_words(out, bits).reshape(batch, k * big_n + 1)[:, k * big_n]
    rot_err = product_model_error(c["basis"], host_words(torus, bits).reshape(n, -1)[0], bits, log_n, k, rng)
    cb_err = product_model_error(c["cbs_basis"], host_words(ggsw[:cbs.ggsw_len()], bits), bits, log_n, k, rng)
    row_allowed = cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell) + n * (1 + k * big_n) * (4 * rot_err + 2)
    allowed = lm.lut_bound(t, r, bits, log_n, k, cb_lb, cb_ell, row_allowed) + pb * (1 + k * big_n) * (4 * cb_err + 2)
    worst = 0.0
    for e, pat in enumerate(patterns):
        x = xm.leaf_index(pat)
        worst = max(worst, float(m.centred_error(phases[e:e + 1], values[0, x:x + 1], bits).max()))
        assert bs.decode(phases[e:e + 1], pbits, bits) == [int(data[0, x])], pat
    print("bits %d log_n %d k %d n %d (t, r) = (%d, %d): look-up err 2^%.2f bound 2^%.2f allowed 2^%.2f (model_err rot %g cbs "
          "%g) Delta/2 2^%d" % (bits, log_n, k, n, t, r, np.log2(max(worst, 1)), np.log2(lm.noisy_lut_bound(case, t, r)),
                                np.log2(allowed), rot_err, cb_err, bits - pbits - 2))
    assert worst <= allowed, (worst, allowed)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    bits, log_n, k, t, r, o = 32, 5, 1, 2, 2, 2
    fft, basis = table(p, log_n), p.ApproxSignedBasis(32, 7, 3)
    ctx = p.TfheLutContext(fft, basis, k, t, r, outputs=o)
    glwe, key_len, lwe = ctx.glwe_len(), ctx.key_len(), k * 32 + 1
    assert glwe == 64 and key_len == 2 * 3 * 64 and not ctx.in_use()
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")
    f = lambda size: torch.zeros(size, dtype=torch.complex128, device="cuda")
    inp, out, keys = z(6 * glwe), z(6 * glwe), f(3 * 3 * key_len)
    p.tfhe_rotate_by_bits_dev(inp, keys[:3 * 2 * key_len], out, ctx)         # the lengths that fit: r keys per input
    p.tfhe_rotate_by_bits_dev(inp, keys, out, ctx, 3, 1)
    p.tfhe_rotate_by_bits_dev(z(0), f(0), z(0), ctx)                         # an empty batch is a no-op
    for args, kpi, first in (((inp[:-1], keys, out[:-1]), 3, 0),             # not a whole number of ciphertexts
                             ((inp, keys, out[:4 * glwe]), 3, 0),
                             ((inp[:5 * glwe], keys, out[:5 * glwe]), 3, 0), # count no multiple of the outputs
                             ((inp, keys[:-1], out), 3, 0),
                             ((inp, keys, out), 3, 2),                       # first_key + r above keys_per_input
                             ((inp, keys[:3 * key_len], out), 1, 0),
                             ((inp, keys, out), 2, 0)):                      # nine keys for three inputs of two
        with pytest.raises(p.PfheError) as e:
            p.tfhe_rotate_by_bits_dev(*args, ctx, kpi, first)
        assert e.value.kind == "BadLength", (kpi, first, e.value)
    both = z(7 * glwe)
    with pytest.raises(p.PfheError) as e:                                    # a ciphertext further on in the same buffer
        p.tfhe_rotate_by_bits_dev(both[:6 * glwe], keys, both[glwe:], ctx, 3, 0)
    assert e.value.kind == "BadArgument" and "exactly inp" in str(e.value)
    with pytest.raises(TypeError):                                           # words of another width
        p.tfhe_rotate_by_bits_dev(inp.long(), keys, out, ctx, 3, 0)
    with pytest.raises(TypeError):
        p.tfhe_lut_eval_dev(z(8 * glwe).long(), f(3 * 4 * key_len), z(6 * glwe), ctx)
    tbl, sel = z(o * 4 * glwe), f(3 * 4 * key_len)
    p.tfhe_lut_eval_dev(tbl, sel, z(3 * o * glwe), ctx)                      # a shared table, GLWE results
    p.tfhe_lut_eval_dev(z(3 * o * 4 * glwe), sel, z(3 * o * 2 * lwe), ctx, 2)   # a table per input, two extractions
    p.tfhe_lut_eval_dev(z(0), f(0), z(0), ctx, 1)                            # an empty batch is a no-op
    with pytest.raises(p.PfheError) as e:                                    # before the lengths
        p.tfhe_lut_eval_dev(tbl, sel[:-1], z(5), ctx, 33)
    assert e.value.kind == "BadArgument" and "extract must be at most N" in str(e.value)
    for args, extract in (((z(2 * o * 4 * glwe), sel, z(3 * o * glwe)), 0),  # neither one table nor batch tables
                          ((z(4 * glwe), sel, z(3 * o * glwe)), 0),          # the table of one output
                          ((tbl, sel[:-1], z(3 * o * glwe)), 0), ((tbl, sel[:3 * 2 * key_len], z(3 * o * glwe)), 0),
                          ((tbl, sel, z(3 * o * glwe - 1)), 0),
                          ((tbl, sel, z(3 * o * glwe)), 1),                  # GLWE words where LWE rows are asked for
                          ((tbl, sel, z(3 * o * 2 * lwe)), 3)):
        with pytest.raises(p.PfheError) as e:
            p.tfhe_lut_eval_dev(*args, ctx, extract)
        assert e.value.kind == "BadLength", (extract, e.value)
    both = z(o * 4 * glwe + 3 * o * glwe)
    with pytest.raises(p.PfheError) as e:                                    # the output inside the table
        p.tfhe_lut_eval_dev(both[:o * 4 * glwe], sel, both[glwe:glwe + 3 * o * glwe], ctx)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    for args, text in (((17, 0), "tree_depth"), ((0, 6), "rot_bits + log_stride"), ((0, 0), "at least 1")):
        with pytest.raises(p.PfheError) as e:
            p.TfheLutContext(fft, basis, k, *args)
        assert e.value.kind == "BadArgument" and text in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheLutContext(fft, basis, k, 1, 3, log_stride=3)
    assert e.value.kind == "BadArgument" and "rot_bits + log_stride" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheLutContext(fft, basis, k, 1, 1, outputs=0)
    assert e.value.kind == "BadArgument" and "outputs" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheLutContext(fft, basis, 65, 1, 1)
    assert e.value.kind == "Unsupported"
    torch.cuda.synchronize()


def test_second_thread_gets_busy(p):
    """Two threads call the host form of one handle over and over until one of them has been refused: a call that arrives
    while the other thread is inside gets Busy, and a call that arrives in between runs (neither is a failure, so the test
    waits for no timing).  Every refusal seen is Busy, and the handle still gives the right words afterwards."""
    bits, log_n, k, t, r, batch = 32, 10, 1, 2, 2, 16
    rng = np.random.default_rng(35)
    fft = table(p, log_n)
    ctx = p.TfheLutContext(fft, p.ApproxSignedBasis(bits, 8, 4), k, t, r)
    n, pb = 1 << log_n, t + r
    msgs = [int(b) for b in rng.integers(0, 2, batch * pb)]
    sel = xm.to_fourier(xm.bit_ggsws(msgs, None, m.ApproxSignedBasis(bits, 8, 4), log_n, k, rng, trivial=True), bits, log_n)
    values = rand_words(rng, bits, 1 << pb).reshape(1, -1)
    tbl = p.tfhe_lut_table(values, log_n, k, t, r).reshape(-1)
    outs = [np.zeros(batch * (k * n + 1), np.uint32) for _ in range(2)]
    refused, done = [], threading.Event()

    def caller(out):
        for _ in range(200):
            if done.is_set():
                return
            try:
                p.tfhe_lut_eval(tbl, sel, out, ctx, 1)
            except p.PfheError as e:
                refused.append(e.kind)
                done.set()

    th = threading.Thread(target=caller, args=(outs[1],))
    th.start()
    caller(outs[0])
    done.set()
    th.join()
    assert refused and set(refused) == {"Busy"}, refused
    assert not ctx.in_use()
    p.tfhe_lut_eval(tbl, sel, outs[0], ctx, 1)
    for e in range(batch):          # exact: trivial selectors and a trivial table in a basis that drops no bit
        x = xm.leaf_index(msgs[e * pb:(e + 1) * pb])
        assert outs[0].reshape(batch, -1)[e, k * n] == values[0, x] and not outs[0].reshape(batch, -1)[e, :k * n].any()
