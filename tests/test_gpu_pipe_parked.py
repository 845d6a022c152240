"""The parked form of the pipelined forward 2^16 transform (ntt_pipe_fwd_kernel<PmArith, 12>: chunk rows parked in LDS by
LDS-DMA, exchanges in halves, five workgroups per CU) at batches small enough for a test: PFHE_PIPELINED_MIN_MB = 1 sends
a handful of RNS polynomials through it.  Every case is compared word for word with the two plain launches
(PFHE_DISABLE_PIPELINED) and, for one RNS polynomial, with the oracle."""
import numpy as np
import pytest

from gpu_util import to_dev, to_host
from pyref import Q61

pytestmark = pytest.mark.gpu

LOG_N = 16
N = 1 << LOG_N


@pytest.fixture(scope="module")
def pf():
    import primus_fhe_amd as p
    return p


def _tables(pf, monkeypatch, moduli, tiles):
    """(pipelined table, plain table): the switches are read when a table is created"""
    monkeypatch.setenv("PFHE_PIPELINED_MIN_MB", "1")
    monkeypatch.setenv("PFHE_PIPE_TILES", str(tiles))
    monkeypatch.delenv("PFHE_DISABLE_PIPELINED", raising=False)
    piped = pf.U64DcrtTable(LOG_N, moduli)
    monkeypatch.setenv("PFHE_DISABLE_PIPELINED", "1")
    plain = pf.U64DcrtTable(LOG_N, moduli)
    monkeypatch.delenv("PFHE_DISABLE_PIPELINED")
    return piped, plain


def _check(orc, piped, plain, moduli, tiles, host, oracle_at):
    """canonical and lazy output of `piped` on `host` against `plain` (all words) and the oracle (RNS polynomial oracle_at)"""
    import torch
    L = len(moduli)
    batch = host.size // (L * N)
    name, launches = piped.transform_form(host.size)
    assert name == "ntt_pipe_fwd_kernel" and launches == min(tiles, batch) + 1
    assert plain.transform_form(host.size)[1] == 2
    x, y = to_dev(host), to_dev(host)
    piped.transform_dev(x)
    plain.transform_dev(y)
    assert torch.equal(x, y)
    W = L * N
    exp = host[oracle_at * W:(oracle_at + 1) * W].copy()
    orc.U64DcrtTable(LOG_N, moduli).transform_slice(exp)
    assert np.array_equal(to_host(x)[oracle_at * W:(oracle_at + 1) * W], exp)
    lz = to_dev(host)
    piped.transform_dev(lz, lazy=True)
    lz = to_host(lz)
    qs = np.tile(np.repeat(np.array(moduli, np.uint64), N), batch)
    assert np.all(lz < 4 * qs) and np.array_equal(lz % qs, to_host(x))


@pytest.mark.parametrize("tiles", [2, 3])
@pytest.mark.parametrize("batch", [2, 3, 5])
@pytest.mark.parametrize("L", [1, 3])
def test_parked_form_equals_plain_launches(pf, orc, monkeypatch, L, batch, tiles):
    """Ragged tiles (3 and 5 polynomials over 2 and 3 tiles), a first launch that is strided-only and a last one that is
    block-only; L = 1 and L = 3: block i and chunk i of a launch belong to the same limb."""
    moduli = Q61[:L]
    piped, plain = _tables(pf, monkeypatch, moduli, tiles)
    rng = np.random.default_rng(100 * L + 10 * batch + tiles)
    host = np.concatenate([rng.integers(0, q, N, dtype=np.uint64) for _ in range(batch) for q in moduli])
    _check(orc, piped, plain, moduli, tiles, host, oracle_at=batch - 1)


@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_parked_form_at_the_edges_of_the_lazy_range(pf, orc, monkeypatch, fill):
    """Every word q - 1 (the widest lazy values through the parked rows and the row kept in registers) and every word 0."""
    moduli, batch = Q61, 3
    piped, plain = _tables(pf, monkeypatch, moduli, 2)
    qs = np.tile(np.repeat(np.array(moduli, np.uint64), N), batch)
    host = qs - np.uint64(1) if fill == "q-1" else np.zeros_like(qs)
    _check(orc, piped, plain, moduli, 2, host, oracle_at=1)


def test_generic_prime_table_on_a_small_pipelined_batch(pf, orc, monkeypatch):
    """PFHE_DISABLE_PM: the same batch through the generic-prime table's forward pipelined kernel."""
    monkeypatch.setenv("PFHE_DISABLE_PM", "1")
    moduli, batch = Q61, 5
    piped, plain = _tables(pf, monkeypatch, moduli, 3)
    rng = np.random.default_rng(7)
    host = np.concatenate([rng.integers(0, q, N, dtype=np.uint64) for _ in range(batch) for q in moduli])
    _check(orc, piped, plain, moduli, 3, host, oracle_at=2)
