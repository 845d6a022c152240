"""GPU tests of the batched CMUX and the CMUX tree (include/pfhe.h, pfhe_tfhe{,32}_cmux_tree_*, _cmux*): rule 1 word for word
against the composition of public calls on full-torus keys, at the shapes where the fused kernel's slot loop and the general
form take their paths; bit for bit against the integer schoolbook where the product is exact, the difference walking the
digit rule's edge words; in place; the tree against its d calls of rule 1, with chunking, repeat calls and graph replay;
noise-free bit selectors picking every leaf; the rotation by an encrypted bit; what the tree means behind a circuit
bootstrap on noisy keys, all on the device; errors and the lease."""
import itertools
import threading

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_cmux_model as xm
import tfhe_edge_words as ew
import tfhe_fft_model as m
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


def composition(p, plan, d0, d1, keys, per_key):
    """rule 1 as public calls: a wrapping subtraction, the product on each group of per_key differences with the group's
    key, a wrapping addition"""
    import torch
    glwe, key_len = plan.glwe_len(), plan.key_len()
    diff, prod = d1 - d0, torch.empty_like(d0)
    for g in range(d0.numel() // glwe // per_key):
        at = slice(g * per_key * glwe, (g + 1) * per_key * glwe)
        p.tfhe_external_product_to_dev(diff[at], keys[g * key_len:(g + 1) * key_len], prod[at], plan)
    return d0 + prod


def cmux_run(p, ctx, d0, d1, keys, per_key, bits):
    out = empty_words(d0.numel(), bits)
    p.tfhe_cmux_dev(d0, d1, keys, out, ctx, per_key)
    return out


# ---------------- rule 1 against the composition of public calls ----------------

# bits, log_n, k, log_basis, ell (None: the full length, drop_bits 0)
RULE1_CASES = [
    (32, 1, 1, 8, None),       # fused: one slot, 255 idle threads; drop_bits 0
    (64, 9, 1, 15, 2),         # fused: exactly one slot per thread
    (32, 10, 1, 7, 3),         # fused: two slots
    (64, 11, 1, 15, 2),        # fused: four slots
    (64, 10, 1, 20, 1),        # ell = 1
    (32, 11, 1, 16, None),     # four slots at u32, drop_bits 0
    (32, 5, 2, 7, 3),          # general
    (64, 3, 3, 16, None),      # general, drop_bits 0
    (64, 12, 1, 15, 2),        # general: k = 1 above the fused N
    (32, 12, 1, 10, 1),        # general, ell = 1
]


@pytest.mark.parametrize("bits,log_n,k,lb,ell", RULE1_CASES, ids=lambda v: str(v))
def test_cmux_equals_the_composition_of_public_calls(p, bits, log_n, k, lb, ell):
    """count 6 with per_key 1, 3 and 6, on a default handle (one launch) and on one of depth 1 and chunk 1, where every
    launch is one ciphertext and starts inside a key group"""
    import torch
    count = 6
    rng = np.random.default_rng(bits + 10 * log_n + k)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    plan = p.TfheFftContext(fft, basis, k)
    wide, narrow = p.TfheCmuxTreeContext(fft, basis, k, 2), p.TfheCmuxTreeContext(fft, basis, k, 1, chunk=1)
    assert wide.key_len() == plan.key_len() and not wide.in_use()
    glwe = plan.glwe_len()
    d0, d1 = (dev_words(rand_words(rng, bits, count * glwe), bits) for _ in range(2))
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, count * plan.key_len()), bits))
    for per_key in (1, 3, 6):
        ks = keys[:count // per_key * plan.key_len()]
        want = composition(p, plan, d0, d1, ks, per_key)
        for ctx in (wide, narrow):
            assert torch.equal(cmux_run(p, ctx, d0, d1, ks, per_key, bits), want), (per_key, ctx.depth)
    # the host form, and one ciphertext alone: the words depend on neither the batch nor the launch
    host = np.zeros(count * glwe, m.UINT[bits])
    p.tfhe_cmux(host_words(d0, bits), host_words(d1, bits), keys.cpu().numpy(), host, wide, 1)
    assert np.array_equal(host, host_words(composition(p, plan, d0, d1, keys, 1), bits))
    one = cmux_run(p, narrow, d0[4 * glwe:5 * glwe].clone(), d1[4 * glwe:5 * glwe].clone(),
                   keys[4 * plan.key_len():5 * plan.key_len()].clone(), 1, bits)
    assert np.array_equal(host_words(one, bits), host[4 * glwe:5 * glwe])
    # the general form owns a plan and the D / E buffers; the fused form of depth 1 owns nothing
    fused = k == 1 and log_n <= 11
    assert (narrow.scratch_bytes() == 0) == fused and wide.scratch_bytes() > narrow.scratch_bytes()


# ---------------- the exact regime against the integer schoolbook ----------------

@pytest.mark.parametrize("bits,log_n,lb,ell", [(32, 4, 7, 3), (64, 4, 15, 2), (32, 9, 7, 3), (64, 9, 15, 2), (32, 4, 8, None)])
def test_exact_regime_equals_the_integer_schoolbook(p, bits, log_n, lb, ell):
    """key words |g| <= 2^10 and (k+1) ell N 2^(logB-1) 2^10 <= 2^40: the f64 product is the integer one.  d1 = d0 + w for
    the digit rule's edge words w, so the difference that the row source forms walks every edge"""
    k, n = 1, 1 << log_n
    mb = m.ApproxSignedBasis(bits, lb, ell)
    assert (k + 1) * mb.decompose_length * n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    rng = np.random.default_rng(bits + log_n + lb)
    glwe = (k + 1) * n
    edges = ew.edge_words(bits, lb, ell)
    count = max(3, -(-edges.size // glwe))                          # every edge word is somewhere in the differences
    diff = rng.permutation(np.resize(edges, max(edges.size, count * glwe)))[:count * glwe].astype(m.UINT[bits])
    d0 = rand_words(rng, bits, count * glwe)
    with np.errstate(over="ignore"):
        d1 = (d0 + diff).astype(m.UINT[bits])
    keys = [rng.integers(-1024, 1025, (k + 1) * mb.decompose_length * glwe).astype(m.UINT[bits]) for _ in range(count)]
    fft = table(p, log_n)
    ctx = p.TfheCmuxTreeContext(fft, p.ApproxSignedBasis(bits, lb, ell), k, 1)
    got = cmux_run(p, ctx, dev_words(d0, bits), dev_words(d1, bits),
                   fourier_keys(p, fft, dev_words(np.concatenate(keys), bits)), 1, bits)
    want = xm.cmux(d0, d1, np.stack(keys), 1, xm.exact_product(mb, log_n, k), bits, log_n, k)
    assert np.array_equal(host_words(got, bits), want)


# ---------------- in place ----------------

@pytest.mark.parametrize("bits,log_n,k", [(32, 10, 1), (64, 6, 1), (64, 4, 2)])
def test_in_place_and_partial_overlap(p, bits, log_n, k):
    import torch
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    count, per_key = 4, 2
    rng = np.random.default_rng(bits + log_n)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    ctx = p.TfheCmuxTreeContext(fft, basis, k, 1)
    glwe = ctx.glwe_len()
    d0, d1 = (dev_words(rand_words(rng, bits, count * glwe), bits) for _ in range(2))
    keys = fourier_keys(p, fft, dev_words(rand_words(rng, bits, 2 * ctx.key_len()), bits))
    want = cmux_run(p, ctx, d0, d1, keys, per_key, bits)
    a = d0.clone()
    p.tfhe_cmux_dev(a, d1, keys, a, ctx, per_key)                           # out is d0
    assert torch.equal(a, want)
    b = d1.clone()
    p.tfhe_cmux_dev(d0, b, keys, b, ctx, per_key)                           # out is d1
    assert torch.equal(b, want)
    both = torch.cat([d0, d0[:glwe]])
    for args in ((both[:count * glwe], d1, both[glwe:]), (d1, both[:count * glwe], both[glwe:])):
        with pytest.raises(p.PfheError) as e:                               # a ciphertext further on in the same buffer
            p.tfhe_cmux_dev(args[0], args[1], keys, args[2], ctx, per_key)
        assert e.value.kind == "BadArgument" and "exactly d0" in str(e.value)


# ---------------- the tree against its d calls of rule 1 ----------------

def tree_by_rule_1(p, ctx, tbl, selectors, batch, bits):
    import torch
    d, glwe, key_len = ctx.depth, ctx.glwe_len(), ctx.key_len()
    nodes = tbl.view(-1, glwe)
    if nodes.shape[0] == 1 << d:
        nodes = nodes.repeat(batch, 1)
    sel = selectors.view(batch, d, key_len)
    for j in range(d):
        pairs = nodes.view(-1, 2, glwe)
        d0, d1 = pairs[:, 0].contiguous().view(-1), pairs[:, 1].contiguous().view(-1)
        nodes = cmux_run(p, ctx, d0, d1, sel[:, j].contiguous().view(-1), 1 << (d - 1 - j), bits).view(-1, glwe)
    return nodes.reshape(-1)


def tree_run(p, ctx, tbl, selectors, batch, bits, stream=None):
    out = empty_words(batch * ctx.glwe_len(), bits)
    p.tfhe_cmux_tree_dev(tbl, selectors, out, ctx, stream)
    return out


@pytest.mark.parametrize("bits,log_n,k", [(32, 6, 1), (64, 9, 1), (64, 4, 2)])
@pytest.mark.parametrize("depth", [1, 2, 3, 5])
def test_tree_equals_its_calls_of_rule_1(p, bits, log_n, k, depth):
    """shared and per-input tables, chunk 1 and a chunk that does not divide the batch, a repeat call, the host form"""
    import torch
    lb, ell = (7, 3) if bits == 32 else (15, 2)
    batch = 5
    rng = np.random.default_rng(bits + log_n + depth)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    big = p.TfheCmuxTreeContext(fft, basis, k, depth)
    one, two = (p.TfheCmuxTreeContext(fft, basis, k, depth, chunk=c) for c in (1, 2))
    if depth > 1:
        assert one.scratch_bytes() < two.scratch_bytes() < big.scratch_bytes()
    glwe = big.glwe_len()
    selectors = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * depth * big.key_len()), bits))
    own = dev_words(rand_words(rng, bits, batch * (glwe << depth)), bits)
    for tbl in (own, own[:glwe << depth].clone()):
        want = tree_by_rule_1(p, big, tbl, selectors, batch, bits)
        for ctx in (big, one, two, two):
            assert torch.equal(tree_run(p, ctx, tbl, selectors, batch, bits), want), ctx.scratch_bytes()
    alone = tree_run(p, two, own[3 * (glwe << depth):4 * (glwe << depth)].clone(),
                     selectors[3 * depth * big.key_len():4 * depth * big.key_len()].clone(), 1, bits)
    per_input = tree_by_rule_1(p, big, own, selectors, batch, bits)
    assert torch.equal(alone, per_input[3 * glwe:4 * glwe])
    if depth == 2:
        host = np.zeros(batch * glwe, m.UINT[bits])
        p.tfhe_cmux_tree(host_words(own, bits), selectors.cpu().numpy(), host, two)
        assert np.array_equal(host, host_words(per_input, bits))


def test_graph_capture_replays_the_eager_call(p):
    """a linear capture on one stream, two chunks and three levels in the graph, replayed twice on fresh tables"""
    import torch
    bits, log_n, k, depth, batch = 32, 8, 1, 3, 3
    rng = np.random.default_rng(77)
    fft, basis = table(p, log_n), p.ApproxSignedBasis(bits, 7, 3)
    ctx = p.TfheCmuxTreeContext(fft, basis, k, depth, chunk=2)
    glwe = ctx.glwe_len()
    selectors = fourier_keys(p, fft, dev_words(rand_words(rng, bits, batch * depth * ctx.key_len()), bits))
    fresh = dev_words(rand_words(rng, bits, batch * (glwe << depth)), bits)
    eager = tree_run(p, ctx, fresh, selectors, batch, bits)
    torch.cuda.synchronize()
    tbl, out = fresh.clone(), torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.tfhe_cmux_tree_dev(tbl, selectors, out, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        tbl.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------- noise-free bit selectors ----------------

PATTERNS = list(itertools.product((0, 1), repeat=3))


def test_every_selector_pattern_picks_its_leaf_u32_exactly(p):
    """batch 8 at depth 3, trivial GGSWs of the bits in a basis that drops no bit: a digit times a gadget word is below
    2^31, the f64 arithmetic is exact, and out[e] IS leaf sum_j m_j 2^j of e's table"""
    bits, log_n, k, depth = 32, 5, 1, 3
    rng = np.random.default_rng(8)
    mb = m.ApproxSignedBasis(bits, 8, 4)
    fft = table(p, log_n)
    ctx = p.TfheCmuxTreeContext(fft, p.ApproxSignedBasis(bits, 8, 4), k, depth, chunk=3)
    glwe = ctx.glwe_len()
    msgs = [b for pat in PATTERNS for b in pat]
    selectors = fourier_keys(p, fft, dev_words(xm.bit_ggsws(msgs, None, mb, log_n, k, rng, trivial=True), bits))
    tbl = rand_words(rng, bits, 8 * (glwe << depth))
    got = host_words(tree_run(p, ctx, dev_words(tbl, bits), selectors, 8, bits), bits).reshape(8, glwe)
    for e, pat in enumerate(PATTERNS):
        assert np.array_equal(got[e], tbl.reshape(8, -1, glwe)[e, xm.leaf_index(pat)]), pat


def test_every_selector_pattern_picks_its_leaf_u64(p):
    """u64 gadget words do not fit f64's 53 bits times a digit sum, so the leaf is met within the bound instead: a shared
    noise-free table of 1-bit messages under a binary key, trivial GGSWs of the bits in the circuit bootstrap's output
    basis (log B 4, ell 3, drop_bits 52).  Every level rounds its difference to 12 bits: tree_bound with noise-free rows,
    plus d (1 + k N) (4 model_err + 2) for the f64 arithmetic"""
    bits, log_n, k, depth, pbits = 64, 6, 1, 3, 1
    n = 1 << log_n
    rng = np.random.default_rng(9)
    mb = m.ApproxSignedBasis(bits, 4, 3)
    fft = table(p, log_n)
    ctx = p.TfheCmuxTreeContext(fft, p.ApproxSignedBasis(bits, 4, 3), k, depth)
    z = rng.integers(0, 2, (k, n)).astype(m.UINT[bits])
    tbl, data = xm.message_table(rng, 1 << depth, bits, log_n, k, pbits, z)
    msgs = [b for pat in PATTERNS for b in pat]
    torus = xm.bit_ggsws(msgs, None, mb, log_n, k, rng, trivial=True)
    got = host_words(tree_run(p, ctx, dev_words(tbl, bits), fourier_keys(p, fft, dev_words(torus, bits)), 8, bits), bits)
    model_err = product_model_error(mb, torus[-ctx.key_len():], bits, log_n, k, rng)
    allowed = xm.tree_bound(depth, bits, log_n, k, 4, 3, 0) + depth * (1 + k * n) * (4 * model_err + 2)
    assert allowed < 2.0 ** (bits - pbits - 2)
    worst = 0.0
    for e, pat in enumerate(PATTERNS):
        ph = bs.glwe_phase(got.reshape(8, -1)[e], z, bits, log_n, k)
        leaf = data[xm.leaf_index(pat)]
        assert bs.decode(ph, pbits, bits) == [int(v) for v in leaf], pat
        want = (leaf.astype(np.uint64) << np.uint64(bits - pbits - 1)).astype(m.UINT[bits])
        worst = max(worst, float(m.centred_error(ph, want, bits).max()))
    print("u64 noise-free selectors depth 3: err 2^%.1f allowed 2^%.1f (model_err %g)" % (np.log2(max(worst, 1)),
                                                                                      np.log2(allowed), model_err))
    assert worst <= allowed


def test_rotation_by_an_encrypted_bit(p):
    """the horizontal step: d1 = X^{-2^j} d0 through mul_monomial_each_to_dev, then rule 1 with a key of the bit m, gives
    X^{-m 2^j} d0: here exactly (u32, trivial GGSWs, no dropped bit), against mul_monomial_each_to_dev on the clear bit"""
    import torch
    bits, log_n, k, j = 32, 6, 1, 3
    n = 1 << log_n
    rng = np.random.default_rng(10)
    mb = m.ApproxSignedBasis(bits, 8, 4)
    fft = table(p, log_n)
    ctx = p.TfheCmuxTreeContext(fft, p.ApproxSignedBasis(bits, 8, 4), k, 1)
    glwe, msgs = ctx.glwe_len(), [0, 1, 1, 0]
    d0 = dev_words(rand_words(rng, bits, len(msgs) * glwe), bits)
    keys = fourier_keys(p, fft, dev_words(xm.bit_ggsws(msgs, None, mb, log_n, k, rng, trivial=True), bits))
    exps = torch.full((len(msgs),), 2 * n - (1 << j), dtype=torch.int32, device="cuda")
    d1 = empty_words(d0.numel(), bits)
    fft.mul_monomial_each_to_dev(d0, exps, d1, polys_per_exp=k + 1)
    got = cmux_run(p, ctx, d0, d1, keys, 1, bits)
    clear = torch.tensor([bit * (2 * n - (1 << j)) for bit in msgs], dtype=torch.int32, device="cuda")
    want = empty_words(d0.numel(), bits)
    fft.mul_monomial_each_to_dev(d0, clear, want, polys_per_exp=k + 1)
    assert torch.equal(got, want)


# ---------------- meaning on noisy keys, end to end on the device ----------------

@pytest.mark.parametrize("case, depth", xm.NOISY_TREES,
                         ids=lambda c: str(c) if isinstance(c, int) else "u%d-N%d-k%d-n%d" % (c[0], 1 << c[1], c[2], c[3]))
def test_noisy_circuit_bootstrap_drives_the_tree(p, case, depth):
    """Binary keys, torus_noise(bound=E) on every row of both generated keys.  tfhe_generate_bsk_dev and
    tfhe_generate_pfksk_dev, tfhe_circuit_bootstrap_dev on the batch x depth bit ciphertexts of all 2^depth selector
    patterns (input e, bit j at e depth + j), write_fourier_form, tfhe_cmux_tree_dev over a shared table of 2^depth noise-free
    GLWE ciphertexts of 1-bit messages, glwe_phase_dev.  The decode equals the chosen leaf at every coefficient and the error
    stays within tfhe_cmux_model.tree_bound of the row allowance (tfhe_cbs_model.row_bound plus the rotation's f64 allowance,
    as tests/test_gpu_tfhe_cbs.py) plus depth (1 + k N) (4 model_err + 2) for the tree's own f64 arithmetic.
    Largest errors seen on the device are in DESIGN.md §20's table."""
    import torch
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, pbits = case
    big_n = 1 << log_n
    c = cm.noisy_case(*case, seed=4000 + bits + log_n + k)
    rng = np.random.default_rng(bits + log_n + depth)
    gen = torch.Generator(device="cuda").manual_seed(5000 + bits + log_n + k)
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = (p.ApproxSignedBasis(bits, *b) for b in ((lb, ell), (cb_lb, cb_ell), (pf_lb, pf_ell)))
    cbs = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    tree = p.TfheCmuxTreeContext(fft, cbs_basis, k, depth)
    assert tree.key_len() == cbs.ggsw_len()
    s, z_flat = dev_words(c["s"], bits), dev_words(bs.flatten_key(c["z"]), bits)
    torus = device_randomness(p, bits, log_n, k, n * (k + 1) * ell, noise, gen)
    pfksk = device_randomness(p, bits, log_n, k, (k + 1) * (k * big_n + 1) * pf_ell, noise, gen)
    bsk = p.tfhe_generate_bsk_dev(p.TfheKeyShape(fft, basis, n, k), s, z_flat, torus)
    p.tfhe_generate_pfksk_dev(z_flat, z_flat, fft, pfks_basis, pfksk, k)
    patterns = list(itertools.product((0, 1), repeat=depth))
    batch = len(patterns)
    msgs = np.array([b for pat in patterns for b in pat], np.uint64)
    lwe = bs.lwe_encrypt(msgs << np.uint64(bits - 1), c["s"], bits, rng)
    ggsw = empty_words(batch * depth * cbs.ggsw_len(), bits)
    p.tfhe_circuit_bootstrap_dev(dev_words(lwe, bits), bsk, pfksk, ggsw, cbs)
    selectors = fourier_keys(p, fft, ggsw)
    tbl, data = xm.message_table(rng, 1 << depth, bits, log_n, k, pbits, c["z"])
    out = tree_run(p, tree, dev_words(tbl, bits), selectors, batch, bits)
    p.glwe_phase_dev(out, z_flat, fft, k)
    phases = host_words(out, bits).reshape(batch, k + 1, big_n)[:, k]
    rot_err = product_model_error(c["basis"], host_words(torus, bits).reshape(n, -1)[0], bits, log_n, k, rng)
    cb_err = product_model_error(c["cbs_basis"], host_words(ggsw[:cbs.ggsw_len()], bits), bits, log_n, k, rng)
    row_allowed = cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell) + n * (1 + k * big_n) * (4 * rot_err + 2)
    allowed = xm.tree_bound(depth, bits, log_n, k, cb_lb, cb_ell, row_allowed) + depth * (1 + k * big_n) * (4 * cb_err + 2)
    worst = 0.0
    for e, pat in enumerate(patterns):
        leaf = data[xm.leaf_index(pat)]
        want = (leaf.astype(np.uint64) << np.uint64(bits - pbits - 1)).astype(m.UINT[bits])
        worst = max(worst, float(m.centred_error(phases[e], want, bits).max()))
        assert bs.decode(phases[e], pbits, bits) == [int(v) for v in leaf], pat
    print("bits %d log_n %d k %d n %d depth %d: tree err 2^%.2f bound 2^%.2f allowed 2^%.2f (model_err rot %g cbs %g) "
          "Delta/2 2^%d" % (bits, log_n, k, n, depth, np.log2(max(worst, 1)), np.log2(xm.noisy_tree_bound(case, depth)),
                            np.log2(allowed), rot_err, cb_err, bits - pbits - 2))
    assert worst <= allowed, (worst, allowed)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    bits, log_n, k, depth = 32, 5, 1, 2
    fft, basis = table(p, log_n), p.ApproxSignedBasis(32, 7, 3)
    ctx = p.TfheCmuxTreeContext(fft, basis, k, depth)
    glwe, key_len = ctx.glwe_len(), ctx.key_len()
    assert glwe == 64 and key_len == 2 * 3 * 64 and not ctx.in_use()
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")
    f = lambda size: torch.zeros(size, dtype=torch.complex128, device="cuda")
    d0, d1, out, keys = z(6 * glwe), z(6 * glwe), z(6 * glwe), f(6 * key_len)
    p.tfhe_cmux_dev(d0, d1, keys, out, ctx, 1)                               # the lengths that fit
    p.tfhe_cmux_dev(d0, d1, keys[:2 * key_len], out, ctx, 3)
    p.tfhe_cmux_dev(z(0), z(0), f(0), z(0), ctx, 3)                          # an empty batch is a no-op
    for args, per_key in (((d0[:-1], d1[:-1], keys, out[:-1]), 1),           # not a whole number of ciphertexts
                          ((d0, d1[:5 * glwe], keys, out), 1),
                          ((d0, d1, keys, out[:5 * glwe]), 1),
                          ((d0, d1, keys[:-1], out), 1),
                          ((d0, d1, keys[:key_len], out), 4),                # count % per_key
                          ((d0, d1, keys, out), 0),
                          ((d0, d1, keys[:3 * key_len], out), 3)):           # three keys for two groups
        with pytest.raises(p.PfheError) as e:
            p.tfhe_cmux_dev(*args, ctx, per_key)
        assert e.value.kind == "BadLength", (per_key, e.value)
    with pytest.raises(TypeError):                                           # words of another width
        p.tfhe_cmux_dev(d0.long(), d1, keys, out, ctx, 1)
    with pytest.raises(TypeError):
        p.tfhe_cmux_tree_dev(z(4 * glwe).long(), f(2 * key_len), z(glwe), ctx)
    tbl, sel, res = z(4 * glwe), f(3 * depth * key_len), z(3 * glwe)
    p.tfhe_cmux_tree_dev(tbl, sel, res, ctx)                                 # a shared table
    p.tfhe_cmux_tree_dev(z(3 * 4 * glwe), sel, res, ctx)                     # a table per input
    p.tfhe_cmux_tree_dev(z(0), f(0), z(0), ctx)                              # an empty batch is a no-op
    for args in ((z(2 * 4 * glwe), sel, res),                                # neither one table nor batch tables
                 (z(2 * glwe), sel, res),                                    # a table of another depth
                 (tbl, sel[:-1], res), (tbl, sel[:3 * key_len], res),        # not batch x depth keys
                 (tbl, sel, res[:-1])):
        with pytest.raises(p.PfheError) as e:
            p.tfhe_cmux_tree_dev(*args, ctx)
        assert e.value.kind == "BadLength"
    both = z(4 * glwe + 3 * glwe)
    with pytest.raises(p.PfheError) as e:                                    # the output inside the table
        p.tfhe_cmux_tree_dev(both[:4 * glwe], sel, both[glwe:4 * glwe], ctx)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    for bad_depth in (0, 17):
        with pytest.raises(p.PfheError) as e:
            p.TfheCmuxTreeContext(fft, basis, k, bad_depth)
        assert e.value.kind == "BadArgument" and "depth" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.TfheCmuxTreeContext(fft, basis, 65, depth)
    assert e.value.kind == "Unsupported"
    torch.cuda.synchronize()


def test_second_thread_gets_busy(p):
    """Two threads call the host form of one handle over and over until one of them has been refused: a call that arrives
    while the other thread is inside gets Busy, and a call that arrives in between runs (neither is a failure, so the test
    waits for no timing).  Every refusal seen is Busy, and the handle still gives the right words afterwards."""
    bits, log_n, k, depth, batch = 32, 10, 1, 3, 16
    rng = np.random.default_rng(34)
    fft = table(p, log_n)
    ctx = p.TfheCmuxTreeContext(fft, p.ApproxSignedBasis(bits, 8, 4), k, depth)
    glwe = ctx.glwe_len()
    msgs = [int(b) for b in rng.integers(0, 2, batch * depth)]
    sel = xm.to_fourier(xm.bit_ggsws(msgs, None, m.ApproxSignedBasis(bits, 8, 4), log_n, k, rng, trivial=True), bits, log_n)
    tbl = rand_words(rng, bits, glwe << depth)
    outs = [np.zeros(batch * glwe, np.uint32) for _ in range(2)]
    refused, done = [], threading.Event()

    def caller(out):
        for _ in range(200):
            if done.is_set():
                return
            try:
                p.tfhe_cmux_tree(tbl, sel, out, ctx)
            except p.PfheError as e:
                refused.append(e.kind)
                done.set()

    t = threading.Thread(target=caller, args=(outs[1],))
    t.start()
    caller(outs[0])
    done.set()
    t.join()
    assert refused and set(refused) == {"Busy"}, refused
    assert not ctx.in_use()
    p.tfhe_cmux_tree(tbl, sel, outs[0], ctx)
    for e in range(batch):          # exact: trivial selectors in a basis that drops no bit
        leaf = xm.leaf_index(msgs[e * depth:(e + 1) * depth])
        assert np.array_equal(outs[0][e * glwe:(e + 1) * glwe], tbl[leaf * glwe:(leaf + 1) * glwe])
