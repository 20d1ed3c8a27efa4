"""The truncated selection kernel on its own (C-ABI aa_sample_select) on hand-built logits, against
tests/sample_trunc_oracle.py ``select`` on the same arrays.

The rows of tests/sample_trunc_cases.py have large margins by construction (value gaps >= 0.1, masses at
least 1 % from a threshold; each case asserts the oracle's inner and outer sets equal), so kept, theta
and the token must be equal; logp within 5e-5 (a log-sum-exp in fp32 against float64).  Every case is at
most 8 rows."""
import numpy as np
import pytest
import torch

from adaptive_amd import _lib, synth
import sample_trunc_cases as cases
from sample_trunc_oracle import select

pytestmark = pytest.mark.gpu

LOGP_TOL = 5e-5
KEY = synth.stream_key(3, "sample")


def gpu_select(dev, logits, V, T=4, t=1, tau=1.0, row0=0, top_k=0, top_p=1.0, want=True):
    """logits [R, Vp] fp32 (numpy) -> tok, logp, kept, theta of column t (numpy), and the untouched columns."""
    lib = _lib.load()
    R, Vp = logits.shape
    x = torch.from_numpy(np.ascontiguousarray(logits)).to(dev)
    tok = torch.full((R,), -7, dtype=torch.int64, device=dev)
    ids = torch.full((R, T), -7, dtype=torch.int64, device=dev)
    logp = torch.full((R, T), 123.0, dtype=torch.float32, device=dev)
    kept = torch.full((R, T), -7, dtype=torch.int32, device=dev)
    theta = torch.full((R, T), 123.0, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.aa_sample_select(x.data_ptr(), R, V, Vp, T, t, tau, KEY, row0, top_k, top_p, tok.data_ptr(),
                                        ids.data_ptr(), logp.data_ptr(), kept.data_ptr() if want else None,
                                        theta.data_ptr() if want else None, _lib.stream_handle()), "sample_select")
    torch.cuda.synchronize()
    others = [c for c in range(T) if c != t]
    assert bool((ids[:, others] == -7).all()) and bool((logp[:, others] == 123.0).all())  # only column t is written
    assert bool((kept[:, others] == -7).all()) and bool((theta[:, others] == 123.0).all())
    assert torch.equal(tok, ids[:, t])
    return tok.cpu().numpy(), logp[:, t].cpu().numpy(), kept[:, t].cpu().numpy(), theta[:, t].cpu().numpy()


def oracle_rows(rows, T=4, t=1, tau=1.0, row0=0, top_k=0, top_p=1.0, ties=False):
    """ties: the rows hold exactly equal values (equal on both sides: no tolerance applies to them), which the
    inner set -- every other value within 2 delta counted as better -- would throw out."""
    R, V = rows.shape
    out = []
    for r in range(R):
        g = synth.gumbel_f32(KEY, ((row0 + r) * T + t) * V, V)
        y = rows[r] / np.float32(tau)
        s = select(y, g, top_k, top_p, delta=LOGP_TOL)
        assert s["kept"] == s["kept_out"] and s["lead"] > 4 * LOGP_TOL, "case meant to have large margins"
        assert ties or (s["kept_in"] == s["kept"] and s["robust"]), "case meant to have large margins"
        out.append(s)
    return out


def check(dev, rows, Vp, ties=False, **kw):
    R, V = rows.shape
    ref = oracle_rows(rows, ties=ties, **kw)
    tok, logp, kept, theta = gpu_select(dev, cases.padded(rows, Vp), V, **kw)
    assert kept.tolist() == [s["kept"] for s in ref]
    assert theta.tolist() == [float(s["theta"]) for s in ref]
    assert tok.tolist() == [s["token"] for s in ref]
    np.testing.assert_allclose(logp, np.array([s["logp"] for s in ref]), atol=LOGP_TOL, rtol=0)
    return tok, logp, kept, theta


@pytest.mark.parametrize("top_k,top_p", list(cases.GEOMETRIC_KEPT))
def test_geometric(top_k, top_p, gpu_device):
    """V = 300 in a pitch of 320 with poisoned padding."""
    _, _, kept, _ = check(gpu_device, cases.geometric(R=4), 320, top_k=top_k, top_p=top_p)
    assert (kept == cases.GEOMETRIC_KEPT[(top_k, top_p)]).all()


@pytest.mark.parametrize("top_k,top_p", list(cases.TIES_KEPT))
def test_ties_are_kept_whole(top_k, top_p, gpu_device):
    _, _, kept, _ = check(gpu_device, cases.ties(R=4), 320, ties=True, top_k=top_k, top_p=top_p)
    assert (kept == cases.TIES_KEPT[(top_k, top_p)]).all()


def test_all_equal_row_is_one_tie_group(gpu_device):
    rows = np.zeros((2, 300), np.float32)
    for k, p in ((1, 1.0), (0, 0.01), (3, 0.5)):
        _, _, kept, theta = check(gpu_device, rows, 320, ties=True, top_k=k, top_p=p)
        assert (kept == 300).all() and (theta == 0).all()


def test_the_truncation_bites(gpu_device):
    rows = cases.bites(R=8)
    plain = gpu_select(gpu_device, cases.padded(rows, 10240), 10123)[0]
    assert not np.isin(plain, cases.BITES_HIGH).any()  # the untruncated draw lands among the zeros
    tok, _, kept, _ = check(gpu_device, rows, 10240, ties=True, top_p=cases.BITES_P)
    assert np.isin(tok, cases.BITES_HIGH).all() and (kept == 3).all()
    # top_p = 0.5 keeps the zeros' tie group (0.5 % above it): every column, and the untruncated token
    tok, _, kept, _ = check(gpu_device, rows, 10240, ties=True, top_p=0.5)
    assert (kept == 10123).all() and np.array_equal(tok, plain)


@pytest.mark.parametrize("V,Vp", [(150, 256), (16384, 16384), (10123, 10240)])
def test_vocabulary_sizes(V, Vp, gpu_device):
    """V = 150: two waves of the workgroup hold no column; V = 16,384: the limit (every column of the LDS
    row); truncations that are off by rule are bitwise the untruncated kernel; top_k = 1 gives logp 0."""
    rows = cases.spread(4, V, seed=V)
    # y = -0.2 rank: the mass above rank j is 1 - e^(-0.2 j): 0.699 / 0.753 around 0.72, 0.889 / 0.909 around 0.9
    for k, p in ((7, 1.0), (0, 0.72), (40, 0.9), (1, 1.0)):
        _, logp, kept, _ = check(gpu_device, rows, Vp, top_k=k, top_p=p, tau=0.5)
        if k == 1:
            assert (logp == 0).all() and (kept == 1).all()
    x = cases.padded(rows, Vp)
    plain = gpu_select(gpu_device, x, V, want=False)
    for k, p in ((V, 1.0), (V + 5, 1.0), (0, 1.0)):
        off = gpu_select(gpu_device, x, V, top_k=k, top_p=p)
        assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])  # bitwise
        assert (off[2] == V).all() and np.array_equal(off[3], rows.min(axis=1))


@pytest.mark.parametrize("V,Vp", [(10123, 10240), (16384, 16384)])
def test_row_independence_and_determinism(V, Vp, gpu_device):
    """Random rows (no margins by construction: kept is compared within the oracle's band for the mass
    rounding alone, y being the same fp32 values on both sides).  top_p = 0.99 keeps about four columns in
    five: at V = 16,384 more than the compacted list holds (5,120 columns; at V = 10,123 the list has room for
    every column), so there the final pass is the dense one."""
    rng = np.random.default_rng(5)
    rows = rng.normal(0, 1.5, (8, V)).astype(np.float32)
    x = cases.padded(rows, Vp)
    for k, p in ((50, 1.0), (0, 0.9), (200, 0.5), (0, 0.99)):
        a = gpu_select(gpu_device, x, V, top_k=k, top_p=p)
        b = gpu_select(gpu_device, x, V, top_k=k, top_p=p)
        part = gpu_select(gpu_device, x[2:6], V, top_k=k, top_p=p, row0=2)
        for u, v, w in zip(a, b, part):
            assert np.array_equal(u, v)            # two runs: the same bits
            assert np.array_equal(u[2:6], w)       # rows 2..5 of 8 == the 4-row call with row0 = 2
        assert (a[2] >= 1).all() and (a[1] <= 0).all()
        # the kept set is what the oracle keeps, up to the fp32 mass rounding at the nucleus's edge
        for r in range(8):
            g = synth.gumbel_f32(KEY, (r * 4 + 1) * V, V)
            s = select(rows[r], g, k, p, delta=1e-5)  # the noise's two logf: within 1e-5 (test_gpu_sample.py)
            assert s["kept_in"] <= a[2][r] <= s["kept_out"]
            assert not s["robust"] or a[0][r] == s["token"]
            assert abs(a[1][r] - s["logp"]) <= LOGP_TOL or a[2][r] != s["kept"] or a[0][r] != s["token"]
            assert p != 0.99 or a[2][r] > 0.7 * V
