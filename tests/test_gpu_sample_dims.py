"""The sampling decode (aa_sample_decode / aa_sample_decode_ex, through ``Encoder2Decoder.sample``) at
hidden 256, 768 and 1024 against ``SampleOracle`` and ``SampleTruncOracle`` (tests/decode_cases.py: the
case table and its oracles; its conditions are asserted on the CPU in tests/test_decode_cases_cpu.py).

What the cases reach that no other test compares with an oracle: the plain k_lstm<256 | 768 | 1024>
step of the sampling loop with its k_atten<1> / k_atten<3> / k_atten5<1024> (h256_ragged, h768_tau,
h1024, h1024_v300), those attention kernels with kdiv = num_samples = 3 (h256_n3, h768_n3, h1024_n3:
the oracle decodes the features repeated three times from global row ``row0 * 3``, as ``sample()``
documents), and the truncated selection at 768 and, with three draws per image, at 1024.

Bounds: the project's own, from tests/test_gpu_sample.py and tests/test_gpu_sample_trunc.py -- ids equal
to the oracle's (its selection margin is asserted above 4 x the logit tolerance first), ``logp`` within
SCORE_TOL x max(1, 1/tau) of the float64 oracle, alpha / beta within ATT_TOL = 2e-5; a truncated case
is banded exactly as in tests/test_gpu_sample_trunc.py, the band taken from the float64 oracle.

Measured on an MI355X: profiles/decode_dims_errors.txt (the lines this module prints).
"""
import numpy as np
import pytest
import torch

import decode_cases as dc
from sample_trunc_oracle import logp_for_kept
from test_gpu_beam_dims import model_for
from test_gpu_sample import ATT_TOL, SCORE_TOL

pytestmark = pytest.mark.gpu

assert (SCORE_TOL, ATT_TOL) == (dc.SCORE_TOL, dc.ATT_TOL) == (5e-5, 2e-5)


@pytest.mark.parametrize("name", [k for k, c in dc.SAMPLE.items() if not c.truncated])
def test_sample_vs_oracle(name, gpu_device):
    case = dc.SAMPLE[name]
    tol = dc.sample_tol(case)
    o_ids, _, _, _, margin = dc.sample_oracle(name)
    assert margin > 4 * tol, f"oracle case too close to call: margin {margin}"
    d_ids, d_logp, d_al, d_be, _ = dc.sample_oracle(name, torch.float64)
    assert torch.equal(o_ids, d_ids)
    m = model_for(case, gpu_device)
    feats = torch.from_numpy(dc.features(case)).to(gpu_device)
    ids, logp, al, be = m.sample(feats, case.T, temperature=case.tau, seed=case.seed, row0=case.row0,
                                 num_samples=case.N)
    R = case.B * case.N
    assert ids.shape == (R, case.T) and logp.shape == (R, case.T) and al.shape == (R, case.T, 49)
    e_lp = float((logp.cpu().double() - d_logp.double()).abs().max())
    e_al = float((al.cpu().double() - d_al).abs().max())
    e_be = float((be.cpu().double() - d_be).abs().max())
    print(f"sample {name} H={case.H} E={case.E} V={case.V} B={case.B} T={case.T} tau={case.tau} N={case.N}: "
          f"margin {margin:.3e}, rows equal {float((ids.cpu() == o_ids).all(1).float().mean()):.3f}, "
          f"max |logp - float64| {e_lp:.3e} (tol {tol:.1e}), alpha {e_al:.2e}, beta {e_be:.2e} (tol {ATT_TOL:.0e})")
    assert torch.equal(ids.cpu(), o_ids)
    assert e_lp <= tol
    assert e_al <= ATT_TOL and e_be <= ATT_TOL


@pytest.mark.parametrize("name", [k for k, c in dc.SAMPLE.items() if c.truncated])
def test_truncated_sample_vs_oracle(name, gpu_device):
    case = dc.SAMPLE[name]
    delta = dc.sample_tol(case)
    o = dc.sample_oracle(name, torch.float64)
    assert o["robust"].all() and dc.sample_oracle(name)["robust"].all(), "case not robust: pick another seed"
    m = model_for(case, gpu_device)
    feats = torch.from_numpy(dc.features(case)).to(gpu_device)
    ids, logp, al, be, kept, theta = m.sample(feats, case.T, temperature=case.tau, seed=case.seed, row0=case.row0,
                                              top_k=case.top_k, top_p=case.top_p, num_samples=case.N, return_kept=True)
    R, T = case.B * case.N, case.T
    assert ids.shape == (R, T) and kept.shape == (R, T) and theta.shape == (R, T)
    ids, logp, kept, theta = ids.cpu(), logp.cpu().numpy(), kept.cpu().numpy(), theta.cpu().numpy()
    ref = np.array([[logp_for_kept(o["y"][r, t], int(o["ids"][r, t]), int(kept[r, t])) for t in range(T)]
                    for r in range(R)])
    e_al = float((al.cpu().double() - o["alpha"]).abs().max())
    e_be = float((be.cpu().double() - o["beta"]).abs().max())
    print(f"sample {name} H={case.H} V={case.V} B={case.B} T={T} tau={case.tau} N={case.N} k={case.top_k} p={case.top_p}: "
          f"kept {kept.min()}..{kept.max()} (oracle {o['kept'].min()}..{o['kept'].max()}, band <= "
          f"{(o['kept_out'] - o['kept_in']).max()}), max |logp - float64(kept)| {np.abs(logp - ref).max():.3e} "
          f"(tol {delta:.1e}), alpha {e_al:.2e}, beta {e_be:.2e}")
    assert torch.equal(ids, o["ids"])
    assert (o["kept_in"] <= kept).all() and (kept <= o["kept_out"]).all()
    assert (theta >= o["theta_out"] - 2 * delta).all() and (theta <= o["theta_in"] + 2 * delta).all()
    np.testing.assert_allclose(logp, ref, atol=delta, rtol=0)
    assert e_al <= ATT_TOL and e_be <= ATT_TOL
