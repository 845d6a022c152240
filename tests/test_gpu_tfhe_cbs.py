"""GPU parity of the circuit bootstrap (include/pfhe.h, pfhe_tfhe{,32}_private_keyswitch*, _pfksk_generate_dev, _cbs_*): the
private functional key switch and its key bit for bit against the integer model (tests/tfhe_cbs_model.py) at the shapes
where the kernel's tiling takes its other paths (tfhe_cbs_model.PFKS_EDGE_SHAPES, which tests/test_tfhe_cbs_model.py proves
to hold them), the handle word for word against the same stages run as public calls and, where the rotation is exact,
against the model; then what the output means on noisy keys, all on the device; then chunking, graph replay, errors and
the lease."""
import threading

import numpy as np
import pytest

import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_keygen_model as kg
from test_gpu_tfhe_fft import TORCH_INT, dev_words, host_words, rand_words

pytestmark = pytest.mark.gpu

BASES = {32: (7, 3), 64: (15, 2)}      # the rotation's (log B, ell) per width
CBS_BASIS = (4, 3)                     # the output basis: drop_bits 20 and 52
PFKS_BASIS = (5, 4)                    # the key switch's


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
    return torch.empty(size, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")


def signed(value: int, bits: int) -> int:
    """a torus word as the two's-complement integer torch takes"""
    value %= 1 << bits
    return value - (1 << bits) if value >> (bits - 1) else value


# ---------------- rule 1: the private functional key switch ----------------

def pfks_inputs(rng, bits, in_dim, log_n, k, lb, ell, levels, batch):
    """full-range random key words; random ciphertexts with the basis's digit edge words spread over mask and body
    positions, and down the body column"""
    basis = m.ApproxSignedBasis(bits, lb, ell)
    pfksk = rand_words(rng, bits, (k + 1) * (in_dim + 1) * ell * ((k + 1) << log_n))
    rows = batch * levels
    lwe = rand_words(rng, bits, rows * (in_dim + 1)).reshape(rows, in_dim + 1)
    edges = ew.edge_words(bits, lb, ell)
    at = rng.permutation(lwe.size)[:min(lwe.size, 2 * edges.size)]
    lwe.reshape(-1)[at] = rng.permutation(np.tile(edges, 2))[:at.size]
    body = rng.permutation(rows)[:max(1, rows // 2)]
    lwe[body, in_dim] = rng.permutation(np.resize(edges, max(body.size, edges.size)))[:body.size]
    return basis, pfksk, lwe.reshape(-1)


def device_pfks(p, lwe, pfksk, bits, in_dim, log_n, k, levels, basis, stream=None):
    import torch
    rows = lwe.size // (in_dim + 1)
    out = torch.full((rows * (k + 1) * ((k + 1) << log_n),), -1, dtype=getattr(torch, TORCH_INT[bits]), device="cuda")
    p.lwe_private_keyswitch_dev(dev_words(lwe, bits), dev_words(pfksk, bits), out, in_dim, levels, table(p, log_n),
                                p.ApproxSignedBasis(bits, basis.log_basis, basis.decompose_length), k, stream=stream)
    return out


@pytest.mark.parametrize("case", cm.PFKS_EDGE_SHAPES, ids=lambda c: "u%d-n%d-N%d-k%d-B%d-l%d-L%d-b%d" % c)
def test_private_key_switch_matches_the_model(p, case):
    bits, in_dim, log_n, k, lb, ell, levels, batch = case
    rng = np.random.default_rng(sum(case))
    basis, pfksk, lwe = pfks_inputs(rng, bits, in_dim, log_n, k, lb, ell, levels, batch)
    want = cm.private_keyswitch(lwe, pfksk, in_dim, levels, basis, log_n, k)
    got = host_words(device_pfks(p, lwe, pfksk, bits, in_dim, log_n, k, levels, basis), bits)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


@pytest.mark.parametrize("bits", [32, 64])
def test_private_key_switch_host_form_repeat_and_batch_independence(p, bits):
    """the host form equals the device form; a second call into the same output repeats it; a ciphertext gives the same rows
    alone (levels = 1) as inside a batch"""
    import torch
    in_dim, log_n, k, lb, ell, levels, batch = 9, 4, 2, 6, 4, 3, 5
    rng = np.random.default_rng(bits + 7)
    basis, pfksk, lwe = pfks_inputs(rng, bits, in_dim, log_n, k, lb, ell, levels, batch)
    want = cm.private_keyswitch(lwe, pfksk, in_dim, levels, basis, log_n, k)
    fft, dev_basis = table(p, log_n), p.ApproxSignedBasis(bits, lb, ell)
    out = np.zeros(want.size, m.UINT[bits])
    p.lwe_private_keyswitch(lwe, pfksk, out, in_dim, levels, fft, dev_basis, k)
    assert np.array_equal(out, want)
    d_in, d_key, d_out = dev_words(lwe, bits), dev_words(pfksk, bits), empty_words(want.size, bits)
    for _ in range(2):
        p.lwe_private_keyswitch_dev(d_in, d_key, d_out, in_dim, levels, fft, dev_basis, k)
        assert np.array_equal(host_words(d_out, bits), want)
    cols = (k + 1) << log_n
    one = empty_words((k + 1) * cols, bits)
    e, l = 3, 1
    at = (e * levels + l) * (in_dim + 1)
    p.lwe_private_keyswitch_dev(d_in[at:at + in_dim + 1].clone(), d_key, one, in_dim, 1, fft, dev_basis, k)
    assert torch.equal(one.view(k + 1, cols), d_out.view(batch, k + 1, levels, cols)[e, :, l])


def test_private_key_switch_across_the_grid_boundary(p):
    """65535 x 32 + 33 input ciphertexts at N = 2 are two launches (grid.y holds 65535 tiles); the second starts inside
    input e = 699040, whose three levels it places behind the first launch's"""
    bits, in_dim, log_n, k, lb, ell, levels = 32, 1, 1, 1, 8, 2, 3
    batch = (65535 * 32 + 33) // levels
    assert batch * levels == 65535 * 32 + 33
    rng = np.random.default_rng(65535)
    basis = m.ApproxSignedBasis(bits, lb, ell)
    pfksk = rand_words(rng, bits, (k + 1) * (in_dim + 1) * ell * ((k + 1) << log_n))
    lwe = rand_words(rng, bits, batch * levels * (in_dim + 1))
    want = cm.private_keyswitch(lwe, pfksk, in_dim, levels, basis, log_n, k)
    got = host_words(device_pfks(p, lwe, pfksk, bits, in_dim, log_n, k, levels, basis), bits)
    assert np.array_equal(got, want)


# ---------------- rule 2: its key ----------------

@pytest.mark.parametrize("bits, log_n, k, in_dim, lb, ell", [(32, 3, 1, 5, 4, 3), (64, 4, 2, 7, 9, 7), (32, 1, 3, 2, 8, None),
                                                             (64, 6, 1, 64, 15, 2)])
def test_key_generation_matches_the_model(p, bits, log_n, k, in_dim, lb, ell):
    """full-range keys and randomness; in_dimension below, at and above N; drop_bits 0 (ell None)"""
    rng = np.random.default_rng(bits + log_n + k + in_dim)
    basis = m.ApproxSignedBasis(bits, lb, ell)
    rows = (k + 1) * (in_dim + 1) * basis.decompose_length
    rand = kg.glwe_randomness(rng, bits, log_n, k, rows, 2 ** (bits // 2))
    s, z = rand_words(rng, bits, in_dim), rand_words(rng, bits, k << log_n)
    want = cm.generate_pfksk(rand, s, z.reshape(k, -1), basis, log_n, k)
    key = dev_words(rand, bits)
    p.tfhe_generate_pfksk_dev(dev_words(s, bits), dev_words(z, bits), table(p, log_n),
                              p.ApproxSignedBasis(bits, lb, basis.decompose_length), key, k)
    got = host_words(key, bits)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


# ---------------- rule 3: the handle against the same stages as public calls ----------------

def composition(p, fft, rot, lwe, bsk, pfksk, bits, log_n, k, n, cbs_basis, pfks_basis):
    """the circuit bootstrap as public calls on device tensors:
         b += 2^(BITS-2)                                       (torch)
         lwe_modulus_switch_dev                                -> exps, neg_b
         every exponent row and neg_b once per level           (torch)
         mul_monomial_each_to_dev on TV_l = (0, .., 0, -g_l/2) -> ACC_{e,l}
         tfhe_blind_rotate_dev
         glwe_sample_extract_dev at index 0
         body += g_l/2                                         (torch)
         lwe_private_keyswitch_dev with levels = ell_cb, in_dimension = k N"""
    import torch
    big_n = 1 << log_n
    glwe, ext = (k + 1) * big_n, k * big_n + 1
    batch, levels = lwe.numel() // (n + 1), cbs_basis.decompose_length()
    shifted = lwe.clone()
    shifted.view(batch, n + 1)[:, n] += signed(1 << (bits - 2), bits)
    exps = torch.empty(batch * n, dtype=torch.int32, device="cuda")
    neg_b = torch.empty(batch, dtype=torch.int32, device="cuda")
    p.lwe_modulus_switch_dev(shifted, n, log_n, exps, neg_b)
    exps = exps.view(batch, n).repeat_interleave(levels, dim=0).contiguous().view(-1)
    neg_b = neg_b.repeat_interleave(levels).contiguous()
    half = [1 << (cbs_basis.drop_bits() + l * cbs_basis.log_basis() - 1) for l in range(levels)]
    tv = torch.zeros((batch, levels, k + 1, big_n), dtype=lwe.dtype, device="cuda")
    for l in range(levels):
        tv[:, l, k, :] = signed(-half[l], bits)
    acc = empty_words(batch * levels * glwe, bits)
    fft.mul_monomial_each_to_dev(tv.view(-1), neg_b, acc, polys_per_exp=k + 1)
    p.tfhe_blind_rotate_dev(acc, bsk, exps, rot)
    lwe_ext = empty_words(batch * levels * ext, bits)
    p.glwe_sample_extract_dev(acc, lwe_ext, fft, k, 0)
    for l in range(levels):
        lwe_ext.view(batch, levels, ext)[:, l, ext - 1] += signed(half[l], bits)
    out = empty_words(batch * (k + 1) * levels * glwe, bits)
    p.lwe_private_keyswitch_dev(lwe_ext, pfksk, out, k * big_n, levels, fft, pfks_basis, k)
    return out


def handle_run(p, ctx, lwe, bsk, pfksk, bits, stream=None):
    import torch
    batch = lwe.numel() // (ctx.lwe_dimension + 1)
    out = torch.full((batch * ctx.ggsw_len(),), -1, dtype=lwe.dtype, device="cuda")       # uninitialised
    p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx, stream)
    return out


def random_case(p, rng, bits, log_n, k, n, batch):
    """full-torus keys and random everything: (fft, the three bases, bsk, pfksk, lwe)"""
    import torch
    lb, ell = BASES[bits]
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = (p.ApproxSignedBasis(bits, *b) for b in ((lb, ell), CBS_BASIS, PFKS_BASIS))
    glwe = (k + 1) << log_n
    torus = dev_words(rand_words(rng, bits, n * (k + 1) * ell * glwe), bits)
    bsk = torch.empty(torus.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(torus, bsk, fft)
    pfksk = dev_words(rand_words(rng, bits, (k + 1) * ((k << log_n) + 1) * PFKS_BASIS[1] * glwe), bits)
    lwe = dev_words(rand_words(rng, bits, batch * (n + 1)), bits)
    return fft, basis, cbs_basis, pfks_basis, bsk, pfksk, lwe


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k", [(6, 1), (5, 2)])
def test_handle_equals_the_composition_of_public_calls(p, bits, log_n, k):
    """one differing word anywhere in the rotation would spread over the whole output; both forms of the handle"""
    import torch
    n, batch = 5, 3
    rng = np.random.default_rng(bits + log_n + k)
    fft, basis, cbs_basis, pfks_basis, bsk, pfksk, lwe = random_case(p, rng, bits, log_n, k, n, batch)
    rot = p.TfheBlindRotateContext(fft, basis, k)
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    assert ctx.bsk_len() == bsk.numel() and ctx.pfksk_len() == pfksk.numel()
    assert ctx.ggsw_len() == (k + 1) * CBS_BASIS[1] * ((k + 1) << log_n) and ctx.scratch_bytes() > rot.scratch_bytes()
    want = composition(p, fft, rot, lwe, bsk, pfksk, bits, log_n, k, n, cbs_basis, pfks_basis)
    got = handle_run(p, ctx, lwe, bsk, pfksk, bits)
    assert torch.equal(got, want)
    host_out = np.zeros(batch * ctx.ggsw_len(), m.UINT[bits])
    p.tfhe_circuit_bootstrap(host_words(lwe, bits), bsk.cpu().numpy(), host_words(pfksk, bits), host_out, ctx)
    assert np.array_equal(host_out, host_words(want, bits))
    assert not ctx.in_use()


# bits, log_n, k, lb, ell: key words |g| <= 2^10 and (k+1) ell N 2^(logB-1) 2^10 <= 2^40, as test_gpu_tfhe_blind_rotate's
EXACT_CASES = [(32, 6, 1, 7, 3), (64, 6, 1, 15, 2), (32, 5, 2, 7, 3), (64, 5, 2, 15, 2), (32, 6, 1, 8, None)]


@pytest.mark.parametrize("bits,log_n,k,lb,ell", EXACT_CASES)
def test_exact_regime_equals_the_integer_model(p, bits, log_n, k, lb, ell):
    """every product of the rotation is the integer schoolbook, and every other stage is integer arithmetic anyway"""
    import torch
    n, batch, big_n = 3, 2, 1 << log_n
    basis, mb = p.ApproxSignedBasis(bits, lb, ell), m.ApproxSignedBasis(bits, lb, ell)
    L = basis.decompose_length()
    assert (k + 1) * L * big_n * 2 ** (lb - 1) * 2 ** 10 <= 2 ** 40
    cbs_basis, pfks_basis = p.ApproxSignedBasis(bits, *CBS_BASIS), p.ApproxSignedBasis(bits, *PFKS_BASIS)
    cbs_mb, pfks_mb = m.ApproxSignedBasis(bits, *CBS_BASIS), m.ApproxSignedBasis(bits, *PFKS_BASIS)
    rng = np.random.default_rng(log_n * 100 + lb + k + bits)
    fft = table(p, log_n)
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    keys = [rng.integers(-1024, 1025, (k + 1) * L * (k + 1) * big_n).astype(m.UINT[bits]) for _ in range(n)]
    bsk = torch.empty(ctx.bsk_len(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(dev_words(np.concatenate(keys), bits), bsk, fft)
    lwe = rand_words(rng, bits, batch * (n + 1))
    pfksk = rand_words(rng, bits, ctx.pfksk_len())
    got = handle_run(p, ctx, dev_words(lwe, bits), bsk, dev_words(pfksk, bits), bits)
    want = cm.circuit_bootstrap(lwe, keys, pfksk, mb, cbs_mb, pfks_mb, log_n, k, n)
    assert np.array_equal(host_words(got, bits), want)


# ---------------- meaning on noisy keys, all on the device ----------------

def product_model_error(basis, key_torus, bits, log_n, k, rng) -> float:
    """the f64 numpy product's error against the schoolbook on one key of the shape, on a full-range input"""
    n = 1 << log_n
    acc = rand_words(rng, bits, (k + 1) * n)
    fourier = m.FullComplex64FftTable(log_n).forward(key_torus.reshape(-1, n), bits).reshape(-1)
    model, _ = m.external_product(acc, fourier, basis, log_n, k)
    return float(m.centred_error(model, m.schoolbook(acc, key_torus, basis, log_n, k), bits).max())


def device_randomness(p, bits, log_n, k, rows, noise, gen):
    """`rows` GLWE rows drawn on the device: torus_uniform masks, torus_noise(bound=noise) bodies"""
    n = 1 << log_n
    rand = p.torus_uniform(rows * (k + 1) * n, bits, generator=gen).view(rows, k + 1, n)
    rand[:, k] = p.torus_noise(rows * n, bits, bound=noise, generator=gen).view(rows, n)
    return rand.view(-1)


@pytest.mark.parametrize("case", cm.NOISY_CASES, ids=lambda c: "u%d-N%d-k%d-n%d" % (c[0], 1 << c[1], c[2], c[3]))
def test_noisy_circuit_bootstrap_gives_a_usable_ggsw_on_the_device(p, case):
    """Binary LWE and GLWE keys, torus_noise(bound=E) on every row of both generated keys (the randomness is drawn on the
    device and copied out, so that the generated keys can also be compared with the model word for word), both bits twice.
    Both keys are generated by the device, consumed by tfhe_circuit_bootstrap_dev, and the output is read with glwe_phase_dev.
      (i)  every coefficient of every row's phase is within row of f_r(m g_l), row = tfhe_cbs_model.row_bound's worst case
           plus the rotation's f64 allowance n (1 + k N) (4 model_err + 2) of tests/test_gpu_tfhe_keygen.py's (d);
      (ii) after write_fourier_form, d0 + (d1 - d0) (x) GGSW through tfhe_external_product_to_dev on two noise-free GLWE
           ciphertexts of p-bit messages decodes to d_m at every coefficient, within tfhe_cbs_model.product_bound of the row
           allowance plus (1 + k N) (4 model_err + 2) for the product's own f64 arithmetic.
    Largest errors seen on the device are in DESIGN.md §19's table."""
    import torch
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, pbits = case
    big_n = 1 << log_n
    c = cm.noisy_case(*case, seed=2000 + bits + log_n + k)
    rng = np.random.default_rng(bits + log_n)
    gen = torch.Generator(device="cuda").manual_seed(3000 + bits + log_n + k)
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = (p.ApproxSignedBasis(bits, *b) for b in ((lb, ell), (cb_lb, cb_ell), (pf_lb, pf_ell)))
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    row = cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell)
    assert (n + 1) / 2 < big_n / 2
    assert cm.product_bound(bits, log_n, k, cb_lb, cb_ell, row) < 2.0 ** (bits - pbits - 2)
    s, z_flat = dev_words(c["s"], bits), dev_words(bs.flatten_key(c["z"]), bits)
    torus = device_randomness(p, bits, log_n, k, n * (k + 1) * ell, noise, gen)
    pfksk = device_randomness(p, bits, log_n, k, (k + 1) * (k * big_n + 1) * pf_ell, noise, gen)
    c["rand_bsk"], c["rand_pfksk"] = host_words(torus, bits).copy(), host_words(pfksk, bits).copy()
    bsk = p.tfhe_generate_bsk_dev(p.TfheKeyShape(fft, basis, n, k), s, z_flat, torus)
    p.tfhe_generate_pfksk_dev(z_flat, z_flat, fft, pfks_basis, pfksk, k)
    assert bsk.numel() == ctx.bsk_len() and pfksk.numel() == ctx.pfksk_len()
    keys_torus = host_words(torus, bits).reshape(n, -1)
    assert np.array_equal(keys_torus.reshape(-1), kg.bsk(c["rand_bsk"], c["s"], c["z"], c["basis"], log_n, k))
    assert np.array_equal(host_words(pfksk, bits),
                          cm.generate_pfksk(c["rand_pfksk"], bs.flatten_key(c["z"]), c["z"], c["pfks_basis"], log_n, k))
    ggsw = handle_run(p, ctx, dev_words(c["lwe"], bits), bsk, pfksk, bits)
    # (i)
    phases = ggsw.clone()
    p.glwe_phase_dev(phases, z_flat, fft, k)
    got = host_words(phases, bits).reshape(-1, k + 1, big_n)[:, k]
    err = float(m.centred_error(got, cm.expected_row_phases(c["msgs"], c["z"], c["cbs_basis"], log_n, k), bits).max())
    rot_err = product_model_error(c["basis"], keys_torus[0], bits, log_n, k, rng)
    row_allowed = row + n * (1 + k * big_n) * (4 * rot_err + 2)
    # (ii)
    fourier = torch.empty(ggsw.numel(), dtype=torch.complex128, device="cuda")
    p.write_fourier_form(ggsw, fourier, fft)
    plan = p.TfheFftContext(fft, cbs_basis, k)
    d = dev_words(c["glwe_rand"], bits)
    p.glwe_encrypt_dev(d, z_flat, fft, k)
    glwe = (k + 1) * big_n
    d0, d1 = d[:glwe], d[glwe:]
    diff, prod = d1 - d0, empty_words(glwe, bits)
    cb_err = product_model_error(c["cbs_basis"], host_words(ggsw[:ctx.ggsw_len()], bits), bits, log_n, k, rng)
    allowed = cm.product_bound(bits, log_n, k, cb_lb, cb_ell, row_allowed) + (1 + k * big_n) * (4 * cb_err + 2)
    worst = 0.0
    for e, msg in enumerate(c["msgs"]):
        p.tfhe_external_product_to_dev(diff, fourier[e * ctx.ggsw_len():(e + 1) * ctx.ggsw_len()], prod, plan)
        sel = d0 + prod
        p.glwe_phase_dev(sel, z_flat, fft, k)
        ph = host_words(sel, bits)[k * big_n:]
        want = (c["data"][int(msg)].astype(np.uint64) * np.uint64(c["delta"])).astype(m.UINT[bits])
        worst = max(worst, float(m.centred_error(ph, want, bits).max()))
        assert bs.decode(ph, pbits, bits) == [int(v) for v in c["data"][int(msg)]], (e, msg)
    print("bits %d log_n %d k %d n %d: rows err 2^%.1f bound 2^%.1f allowed 2^%.1f (rotation model_err %g); product err 2^%.1f "
          "allowed 2^%.1f (model_err %g) Delta/2 2^%d" % (bits, log_n, k, n, np.log2(max(err, 1)), np.log2(row),
                                                        np.log2(row_allowed), rot_err, np.log2(max(worst, 1)),
                                                        np.log2(allowed), cb_err, bits - pbits - 2))
    assert err <= row_allowed, (err, row_allowed)
    assert worst <= allowed, (worst, allowed)


# ---------------- chunking, determinism, graphs ----------------

@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("log_n,k", [(6, 1), (5, 2)])
def test_chunking_and_repeat_calls(p, bits, log_n, k):
    import torch
    n, batch = 4, 5
    rng = np.random.default_rng(31 + bits + log_n)
    fft, basis, cbs_basis, pfks_basis, bsk, pfksk, lwe = random_case(p, rng, bits, log_n, k, n, batch)
    big = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    one = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, chunk=1)
    two = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, chunk=2)
    assert one.scratch_bytes() < two.scratch_bytes() < big.scratch_bytes()
    want = handle_run(p, big, lwe, bsk, pfksk, bits)
    for ctx in (one, two, two, big):
        assert torch.equal(handle_run(p, ctx, lwe, bsk, pfksk, bits), want)
    alone = handle_run(p, two, lwe[2 * (n + 1):3 * (n + 1)].clone(), bsk, pfksk, bits)
    assert torch.equal(alone, want[2 * big.ggsw_len():3 * big.ggsw_len()])


def test_graph_capture_replays_the_eager_call(p):
    """a linear capture on one stream, replayed twice on fresh inputs"""
    import torch
    bits, log_n, k, n, batch = 32, 6, 1, 3, 3
    rng = np.random.default_rng(32)
    fft, basis, cbs_basis, pfks_basis, bsk, pfksk, fresh = random_case(p, rng, bits, log_n, k, n, batch)
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis, chunk=2)      # two chunks in the graph
    eager = handle_run(p, ctx, fresh, bsk, pfksk, bits)
    torch.cuda.synchronize()
    lwe, out = fresh.clone(), torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        lwe.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------- errors and the lease ----------------

def test_length_and_argument_errors(p):
    import torch
    bits, log_n, k, n, big_n = 32, 5, 1, 4, 32
    fft = table(p, log_n)
    basis, cbs_basis, pfks_basis = p.ApproxSignedBasis(32, 7, 3), p.ApproxSignedBasis(32, 4, 3), p.ApproxSignedBasis(32, 5, 4)
    ctx = p.TfheCircuitBootstrapContext(fft, basis, n, k, cbs_basis, pfks_basis)
    assert ctx.key_len() == 12 * big_n and ctx.pfksk_len() == 2 * (big_n + 1) * 4 * 2 * big_n and ctx.ggsw_len() == 12 * big_n
    assert not ctx.in_use()
    z = lambda size: torch.zeros(size, dtype=torch.int32, device="cuda")
    lwe, pfksk, out = z(2 * (n + 1)), z(ctx.pfksk_len()), z(2 * ctx.ggsw_len())
    bsk = torch.zeros(ctx.bsk_len(), dtype=torch.complex128, device="cuda")
    p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, out, ctx)                  # the lengths that fit
    p.tfhe_circuit_bootstrap_dev(z(0), bsk, pfksk, z(0), ctx)                # an empty batch is a no-op
    for args in ((z(2 * (n + 1) + 1), bsk, pfksk, out),                      # not a whole number of ciphertexts
                 (lwe, bsk[:-1], pfksk, out),                                # not n keys
                 (lwe, bsk, pfksk[:-1], out),                                # a key of another shape
                 (lwe, bsk, z(big_n * 4 * 2 * big_n), out),                  # a packing key
                 (lwe, bsk, pfksk, out[:-1]),
                 (lwe, bsk, pfksk, z(ctx.ggsw_len()))):                      # one GGSW for two inputs
        with pytest.raises(p.PfheError) as e:
            p.tfhe_circuit_bootstrap_dev(*args, ctx)
        assert e.value.kind == "BadLength"
    both = z(2 * ctx.ggsw_len() + 2 * (n + 1))
    with pytest.raises(p.PfheError) as e:                                    # the output overlapping an input
        p.tfhe_circuit_bootstrap_dev(both[:2 * (n + 1)], bsk, pfksk, both[n + 1:n + 1 + 2 * ctx.ggsw_len()], ctx)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.tfhe_circuit_bootstrap_dev(lwe, bsk, pfksk, pfksk[8:8 + 2 * ctx.ggsw_len()], ctx)
    assert e.value.kind == "BadArgument"
    with pytest.raises(TypeError):                                           # words of another width
        p.tfhe_circuit_bootstrap_dev(lwe.long(), bsk, pfksk, out, ctx)
    # the stateless call behind the same checks
    ext = z(2 * 3 * (big_n + 1))
    with pytest.raises(p.PfheError) as e:
        p.lwe_private_keyswitch_dev(ext, pfksk, out, big_n, 3, fft, pfks_basis, k + 1)
    assert e.value.kind == "BadLength"
    with pytest.raises(p.PfheError) as e:
        p.lwe_private_keyswitch_dev(ext, pfksk, out, big_n, 0, fft, pfks_basis, k)
    assert e.value.kind == "BadArgument" and "levels" in str(e.value)
    with pytest.raises(p.PfheError) as e:
        p.lwe_private_keyswitch_dev(pfksk[:ext.numel()], pfksk, pfksk[8:8 + out.numel()], big_n, 3, fft, pfks_basis, k)
    assert e.value.kind == "BadArgument" and "overlap" in str(e.value)
    p.lwe_private_keyswitch_dev(ext, pfksk, out, big_n, 3, fft, pfks_basis, k)
    # create: the rotation's statuses first, then the handle's own
    with pytest.raises(p.PfheError) as e:
        p.TfheCircuitBootstrapContext(fft, basis, n, 65, cbs_basis, pfks_basis)
    assert e.value.kind == "Unsupported"
    for args in ((fft, basis, 0, 1, cbs_basis, pfks_basis), (fft, basis, n, 0, cbs_basis, pfks_basis),
                 (fft, basis, n, 1, p.ApproxSignedBasis(32, 4), pfks_basis)):    # the full length: drop_bits 0
        with pytest.raises(p.PfheError) as e:
            p.TfheCircuitBootstrapContext(*args)
        assert e.value.kind == "BadArgument"
    torch.cuda.synchronize()


def test_second_thread_gets_busy(p):
    """Two threads call the host form of one handle over and over until one of them has been refused: a call that arrives
    while the other thread is inside gets Busy, and a call that arrives in between runs (neither is a failure, so the test
    waits for no timing).  Every refusal seen is Busy, and the handle still gives the right words afterwards."""
    bits, log_n, k, n, batch = 32, 10, 1, 2, 256
    rng = np.random.default_rng(34)
    fft = table(p, log_n)
    ctx = p.TfheCircuitBootstrapContext(fft, p.ApproxSignedBasis(bits, 7, 3), n, k, p.ApproxSignedBasis(bits, 8, 2),
                                        p.ApproxSignedBasis(bits, 16, 1))
    bsk = np.zeros(ctx.bsk_len(), np.complex128)
    lwe = rand_words(rng, bits, batch * (n + 1))
    pfksk = rand_words(rng, bits, ctx.pfksk_len())
    outs = [np.zeros(batch * ctx.ggsw_len(), np.uint32) for _ in range(2)]
    refused, done = [], threading.Event()

    def caller(out):
        for _ in range(200):
            if done.is_set():
                return
            try:
                p.tfhe_circuit_bootstrap(lwe, bsk, pfksk, out, ctx)
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
    # zero keys: the rotation adds nothing, so every input gives the key switch of the extraction of X^{neg_b} TV_l + g_l/2
    p.tfhe_circuit_bootstrap(lwe, bsk, pfksk, outs[0], ctx)
    mb, cbs_mb, pfks_mb = m.ApproxSignedBasis(bits, 7, 3), m.ApproxSignedBasis(bits, 8, 2), m.ApproxSignedBasis(bits, 16, 1)
    zero_keys = [np.zeros(ctx.key_len(), np.uint32)] * n
    want = cm.circuit_bootstrap(lwe[:3 * (n + 1)], zero_keys, pfksk, mb, cbs_mb, pfks_mb, log_n, k, n)
    assert np.array_equal(outs[0][:3 * ctx.ggsw_len()], want)
