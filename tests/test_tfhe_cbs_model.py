"""CPU checks of the circuit bootstrap's model (tests/tfhe_cbs_model.py): (a) on a noise-free key the private functional key
switch puts f_u of the rounded phase into row u, word for word; (b) with trivial bootstrapping keys and a noise-free key
switch whose rounding is exact the model's circuit bootstrap of m has the row phases f_r(m g_l) exactly; (c) the derived
bounds stay below Delta / 2 at every noisy shape of the GPU file; (d) the edge-shape table of the GPU file reaches the paths
of the kernel's tiling that it claims.  Nothing here imports the library, and nothing needs a GPU."""
import numpy as np
import pytest

import tfhe_blindrot_model as bm
import tfhe_bootstrap_model as bs
import tfhe_cbs_model as cm
import tfhe_edge_words as ew
import tfhe_fft_model as m
import tfhe_keygen_model as kg


def rand_words(rng, bits, size):
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(m.UINT[bits])


# ---------------- (a) rule 1 and rule 2 on a noise-free key ----------------

@pytest.mark.parametrize("bits, log_n, k, in_dim, lb, ell, levels", [(32, 3, 1, 5, 4, 3, 1), (32, 2, 2, 3, 7, 4, 2),
                                                                    (64, 3, 1, 4, 9, 7, 3), (64, 2, 3, 2, 16, 4, 2),
                                                                    (32, 3, 1, 3, 1, 9, 2)])
def test_row_u_of_the_key_switch_holds_f_u_of_the_rounded_phase(bits, log_n, k, in_dim, lb, ell, levels):
    """full-range inputs and keys (the identity is one of wrapping words, it needs no small key); the key from
    generate_pfksk with noise-free bodies"""
    rng = np.random.default_rng(bits + log_n + k + lb)
    basis = m.ApproxSignedBasis(bits, lb, ell)
    s, z = rand_words(rng, bits, in_dim), rand_words(rng, bits, k << log_n).reshape(k, -1)
    pfksk = cm.noise_free_pfksk(s, z, basis, log_n, k, rng)
    batch = 3
    lwe = rand_words(rng, bits, batch * levels * (in_dim + 1))
    edges = ew.edge_words(bits, lb, ell)
    lwe[:min(lwe.size, edges.size)] = rng.permutation(edges)[:lwe.size]       # mask and body positions alike
    out = cm.private_keyswitch(lwe, pfksk, in_dim, levels, basis, log_n, k).reshape(batch, k + 1, levels, -1)
    phi = cm.rounded_phase(lwe, s, basis).reshape(batch, levels)
    for e in range(batch):
        for u in range(k + 1):
            for l in range(levels):
                got = bs.glwe_phase(out[e, u, l], z, bits, log_n, k)
                assert np.array_equal(got, cm.f_row(u, int(phi[e, l]), z, bits, log_n, k)), (e, u, l)


def test_key_rows_encrypt_their_messages():
    """the phase of row (u, j, t) of a noise-free key is f_u(s'_j g_t), and of a noisy one that plus the body's noise"""
    bits, log_n, k, in_dim, lb, ell = 32, 2, 2, 3, 5, 4
    rng = np.random.default_rng(3)
    basis = m.ApproxSignedBasis(bits, lb, ell)
    s, z = rand_words(rng, bits, in_dim), rand_words(rng, bits, k << log_n).reshape(k, -1)
    rows = (k + 1) * (in_dim + 1) * ell
    rand = kg.glwe_randomness(rng, bits, log_n, k, rows, 7)
    noise = rand.reshape(rows, k + 1, -1)[:, k].copy()
    key = cm.generate_pfksk(rand, s, z, basis, log_n, k).reshape(k + 1, in_dim + 1, ell, -1)
    sp = [int(v) for v in s] + [-1]
    g = cm.gadget(basis)
    row = 0
    for u in range(k + 1):
        for j in range(in_dim + 1):
            for t in range(ell):
                want = cm.f_row(u, sp[j] * int(g[t]), z, bits, log_n, k)
                with np.errstate(over="ignore"):
                    want = (want + noise[row]).astype(m.UINT[bits])
                assert np.array_equal(bs.glwe_phase(key[u, j, t], z, bits, log_n, k), want), (u, j, t)
                row += 1


def test_levels_and_batch_only_place_the_rows():
    """ciphertext (e, l) alone, through the plain form levels = 1, gives the same k + 1 rows: out[e][u][l]"""
    bits, log_n, k, in_dim, lb, ell, levels, batch = 64, 2, 2, 4, 6, 5, 3, 2
    rng = np.random.default_rng(11)
    basis = m.ApproxSignedBasis(bits, lb, ell)
    pfksk = rand_words(rng, bits, (k + 1) * (in_dim + 1) * ell * ((k + 1) << log_n))
    lwe = rand_words(rng, bits, batch * levels * (in_dim + 1)).reshape(batch, levels, -1)
    out = cm.private_keyswitch(lwe, pfksk, in_dim, levels, basis, log_n, k).reshape(batch, k + 1, levels, -1)
    for e in range(batch):
        for l in range(levels):
            one = cm.private_keyswitch(lwe[e, l], pfksk, in_dim, 1, basis, log_n, k).reshape(k + 1, -1)
            assert np.array_equal(out[e, :, l], one)


# ---------------- (b) the circuit bootstrap in the exact regime ----------------

# bits, log_n, k, n, rotation basis (drop 0), pfks basis, cbs basis: 2^drop_pf divides every g_l / 2
EXACT_CASES = [(32, 4, 1, 3, (8, 4), (4, 5), (5, 2)), (32, 3, 2, 2, (8, 4), (6, 3), (4, 3)),
               (64, 4, 1, 3, (16, 4), (8, 6), (9, 2)), (64, 3, 2, 2, (16, 4), (7, 5), (6, 4))]


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "u%d-N%d-k%d" % (c[0], 1 << c[1], c[2]))
def test_circuit_bootstrap_of_a_bit_is_a_ggsw_of_the_bit(case):
    bits, log_n, k, n, rot, pf, cb = case
    big_n = 1 << log_n
    basis, pfks_basis, cbs_basis = (m.ApproxSignedBasis(bits, *b) for b in (rot, pf, cb))
    assert basis.drop_bits == 0 and 1 <= pfks_basis.drop_bits <= cbs_basis.drop_bits - 1
    assert (n + 1) / 2 < big_n / 2            # the switched phase stays a quarter turn's worth away from the sign changes
    rng = np.random.default_rng(bits + log_n + k)
    s = rng.integers(0, 2, n)
    s[0] = 1
    z = rng.integers(0, 2, (k, big_n)).astype(m.UINT[bits])
    keys = [bm.trivial_ggsw(basis, log_n, k, int(si)) for si in s]
    pfksk = cm.noise_free_pfksk(bs.flatten_key(z), z, pfks_basis, log_n, k, rng)
    msgs = np.array([0, 1, 1, 0])
    lwe = bs.lwe_encrypt(msgs.astype(np.uint64) << np.uint64(bits - 1), s, bits, rng)
    ext = cm.extracted(lwe, keys, basis, cbs_basis, log_n, k, n).reshape(len(msgs), cbs_basis.decompose_length, -1)
    for e, msg in enumerate(msgs):            # trivial keys: the masks stay zero and the body is m g_l exactly
        assert not ext[e, :, :k * big_n].any()
        assert [int(v) for v in ext[e, :, k * big_n]] == [int(msg) * int(g) for g in cm.gadget(cbs_basis)]
    ggsw = cm.circuit_bootstrap(lwe, keys, pfksk, basis, cbs_basis, pfks_basis, log_n, k, n)
    assert ggsw.size == len(msgs) * (k + 1) * cbs_basis.decompose_length * (k + 1) * big_n
    got = cm.ggsw_row_phases(ggsw, z, bits, log_n, k)
    assert np.array_equal(got, cm.expected_row_phases(msgs, z, cbs_basis, log_n, k))
    # and the rows are those of a GGSW encryption of m: the gadget call's layout, phase for phase
    zero = np.zeros((k + 1) * cbs_basis.decompose_length * (k + 1) * big_n, m.UINT[bits])
    for e, msg in enumerate(msgs):
        ref = kg.ggsw_add_gadget(zero, [int(msg)], cbs_basis, log_n, k)
        assert np.array_equal(cm.ggsw_row_phases(ref, z, bits, log_n, k),
                              got[e * (k + 1) * cbs_basis.decompose_length:(e + 1) * (k + 1) * cbs_basis.decompose_length])


# ---------------- (c) the bounds ----------------

def test_bounds_are_below_half_a_step_at_every_noisy_shape():
    assert {c[0] for c in cm.NOISY_CASES} == {32, 64} and any(c[2] == 2 for c in cm.NOISY_CASES)
    for bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, p in cm.NOISY_CASES:
        cbs_basis = m.ApproxSignedBasis(bits, cb_lb, cb_ell)
        assert cbs_basis.drop_bits >= 1
        assert (n + 1) / 2 < (1 << log_n) / 2
        rows = cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell)
        assert rows < 2.0 ** (cbs_basis.drop_bits - 1)                  # below g_0 / 2: every row still reads as m g_l
        assert cm.product_bound(bits, log_n, k, cb_lb, cb_ell, rows) < 2.0 ** (bits - p - 2), (bits, log_n, k)
    # the two shapes worked out by hand when the bound was written
    assert abs(np.log2(cm.product_bound(32, 4, 1, 4, 2, cm.row_bound(32, 4, 1, 4, 8, 4, 4, 4, 8))) - 28.1) < 0.1
    assert abs(np.log2(cm.product_bound(64, 6, 1, 4, 3, cm.row_bound(64, 6, 1, 8, 15, 2, 2 ** 20, 8, 5))) - 58) < 0.2


def test_row_bound_holds_on_the_model_and_is_not_vacuous():
    """the exact model on a noisy case: every row coefficient within the bound, and not by orders of magnitude"""
    case = (32, 3, 1, 3, 8, 4, 4, 4, 8, 4, 2, 1)
    bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell, cb_lb, cb_ell, _ = case
    c = cm.noisy_case(*case, seed=5)
    keys = kg.bsk(c["rand_bsk"], c["s"], c["z"], c["basis"], log_n, k).reshape(n, -1)
    pfksk = cm.generate_pfksk(c["rand_pfksk"], bs.flatten_key(c["z"]), c["z"], c["pfks_basis"], log_n, k)
    ggsw = cm.circuit_bootstrap(c["lwe"], list(keys), pfksk, c["basis"], c["cbs_basis"], c["pfks_basis"], log_n, k, n)
    err = m.centred_error(cm.ggsw_row_phases(ggsw, c["z"], bits, log_n, k),
                          cm.expected_row_phases(c["msgs"], c["z"], c["cbs_basis"], log_n, k), bits).max()
    bound = cm.row_bound(bits, log_n, k, n, lb, ell, noise, pf_lb, pf_ell)
    assert 0 < err <= bound and err > bound / 2 ** 8, (err, bound)


# ---------------- (d) the edge-shape table ----------------

# ki and the key rows of every group as they were worked out by hand when the table was written, entry by entry
EXPECTED = [(8, [24, 15]), (8, [15]), (8, [2]), (8, [40, 40, 5]), (8, [56, 56, 21]), (7, [63, 36]), (1, [33] * 5),
            (3, [51, 51, 17])]


def test_table_entries_are_valid_and_as_worked_out():
    assert len(EXPECTED) == len(cm.PFKS_EDGE_SHAPES)
    for (bits, in_dim, log_n, k, lb, ell, levels, batch), (ki, rows) in zip(cm.PFKS_EDGE_SHAPES, EXPECTED):
        assert bits in (32, 64) and 0 < lb < bits and 0 < ell <= bits // lb       # ApproxSignedBasis::new accepts it
        assert 1 <= log_n <= 14 and 1 <= k <= 64 and in_dim > 0 and 1 <= levels <= 64 and batch > 0
        assert cm.group_words(ell) == ki and cm.group_rows(in_dim, ell) == rows, (bits, in_dim, lb, ell)
        assert sum(rows) == (in_dim + 1) * ell


def test_table_holds_every_path_of_the_tiling():
    shapes = [dict(bits=bits, k=k, levels=levels, batch=batch, m=batch * levels, cols=(k + 1) << log_n,
                   ki=cm.group_words(ell), rows=cm.group_rows(in_dim, ell), words=in_dim + 1)
              for bits, in_dim, log_n, k, _, ell, levels, batch in cm.PFKS_EDGE_SHAPES]
    groups = [r for s in shapes for r in s["rows"]]
    # the remainder loop behind the unrolled one with every count of left-over rows, and alone
    assert {r % cm.PF_UNROLL for r in groups} == {0, 1, 2, 3}
    for rem in (1, 3):
        assert any(r > cm.PF_UNROLL and r % cm.PF_UNROLL == rem for r in groups), rem
    assert any(r < cm.PF_UNROLL for r in groups)
    # group sizes 1, a non-power of two, 8; a partial last group behind a full one; fewer words than one group
    assert {s["ki"] for s in shapes} >= {1, 3, 7, 8}
    for ki in (3, 7, 8):
        assert any(s["ki"] == ki and len(s["rows"]) >= 2 and s["rows"][-1] < s["rows"][0] for s in shapes), ki
    assert any(s["words"] < s["ki"] for s in shapes)
    # the columns: far below a tile (the clamp), exactly one tile, a partial second tile, and no multiple of 64 lanes
    cols = {s["cols"] for s in shapes}
    assert cm.PF_TILE_COLS in cols and min(cols) == 4
    assert any(cm.PF_TILE_COLS < c < 2 * cm.PF_TILE_COLS for c in cols) and any(64 < c < cm.PF_TILE_COLS for c in cols)
    assert any(c > 2 * cm.PF_TILE_COLS for c in cols)
    # the rows of input ciphertexts: one short of a tile, a tile, one more; both through the batch and through the levels
    ms = {s["m"] for s in shapes}
    assert ms >= {cm.PF_TILE_ROWS - 1, cm.PF_TILE_ROWS, cm.PF_TILE_ROWS + 1}
    assert any(s["m"] == cm.PF_TILE_ROWS + 1 and s["levels"] == 1 for s in shapes)
    assert any(s["m"] == cm.PF_TILE_ROWS + 1 and s["levels"] > 1 for s in shapes)      # an e split across two tiles
    assert any(s["m"] == 1 for s in shapes)
    # levels 1 and above, k = 1, 2 and 3 (two, three and four key blocks), both widths
    assert {s["levels"] for s in shapes} >= {1, 2, 3, 4}
    assert {s["k"] for s in shapes} == {1, 2, 3} and {s["bits"] for s in shapes} == {32, 64}
