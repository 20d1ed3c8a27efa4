"""CPU: the case table of tests/decode_cases.py and the conditions its GPU tests
(tests/test_gpu_beam_dims.py, tests/test_gpu_sample_dims.py) rest on.

* Every case is admissible: the fp32 oracle's selection margin exceeds 4 x SCORE_TOL (beam), 4 x
  SCORE_TOL x max(1, 1/tau) (sampling); a truncated sampling case is robust at every (row, step).
* The float64 oracle (the same program text in double) selects the same sequences / tokens, and its
  scores lie within a quarter of SCORE_TOL of the fp32 oracle's, so it can stand in as the reference
  of the GPU comparison (measured: beam scores 8.1e-7 .. 7.7e-6, logp 4.8e-7 .. 1.4e-6).
* A case has the properties it is listed for: beams finish, fewer non-empty granules than K, and the
  table covers the kernel forms the GPU tests are there for.
"""
import numpy as np
import pytest
import torch

import decode_cases as dc

QUARTER = dc.SCORE_TOL / 4


@pytest.mark.parametrize("name", list(dc.BEAM))
def test_beam_case_is_admissible_and_float64_agrees(name):
    case = dc.BEAM[name]
    ids, al, be, seqs, sc, margin = dc.beam_oracle(name)
    d_ids, d_al, d_be, d_seqs, d_sc, d_margin = dc.beam_oracle(name, torch.float64)
    assert sc.dtype == torch.float32 and d_sc.dtype == torch.float64 and d_al.dtype == torch.float64
    assert seqs.shape == (case.B, case.K, case.T)
    err = float((sc.double() - d_sc).abs().max())
    print(f"{name}: margin {margin:.3e} (float64 {d_margin:.3e}), max |fp32 - float64| score {err:.2e}, "
          f"alpha {float((al.double() - d_al).abs().max()):.1e}, beta {float((be.double() - d_be).abs().max()):.1e}, "
          f"beams with <end>: {float((seqs == 2).any(2).float().mean()):.2f}")
    assert margin > 4 * dc.SCORE_TOL, f"case too close to call: margin {margin}"
    assert torch.equal(seqs, d_seqs) and torch.equal(ids, d_ids)
    assert err < QUARTER
    assert bool((seqs == 2).any()) == case.finishes
    assert bool(((seqs >= 0) & (seqs < case.V)).all()) and bool(torch.isfinite(d_sc).all())


@pytest.mark.parametrize("name", [k for k, c in dc.SAMPLE.items() if not c.truncated])
def test_sample_case_is_admissible_and_float64_agrees(name):
    case = dc.SAMPLE[name]
    ids, logp, al, be, margin = dc.sample_oracle(name)
    d_ids, d_logp, d_al, d_be, d_margin = dc.sample_oracle(name, torch.float64)
    assert ids.shape == (case.B * case.N, case.T) and d_al.dtype == torch.float64
    err = float((logp - d_logp).abs().max())
    print(f"{name}: margin {margin:.3e} (float64 {d_margin:.3e}), max |fp32 - float64| logp {err:.2e}")
    assert margin > 4 * dc.sample_tol(case), f"case too close to call: margin {margin}"
    assert torch.equal(ids, d_ids)
    assert err < QUARTER
    if case.N > 1:  # an image's rows draw with their own noise
        rows = ids.view(case.B, case.N, case.T)
        assert not torch.equal(rows[:, 0], rows[:, 1])


@pytest.mark.parametrize("name", [k for k, c in dc.SAMPLE.items() if c.truncated])
def test_truncated_sample_case_is_robust_and_float64_agrees(name):
    case = dc.SAMPLE[name]
    o, d = dc.sample_oracle(name), dc.sample_oracle(name, torch.float64)
    print(f"{name}: kept {o['kept'].min()}..{o['kept'].max()}, smallest lead {o['lead'].min():.3e} "
          f"(float64 {d['lead'].min():.3e}), band <= {(d['kept_out'] - d['kept_in']).max()}")
    assert o["robust"].all() and d["robust"].all(), "case not robust: pick another seed"
    assert torch.equal(o["ids"], d["ids"])
    assert (d["kept_in"] <= o["kept"]).all() and (o["kept"] <= d["kept_out"]).all()
    assert (o["kept"] < case.V).all(), "the truncation must bite"
    assert np.abs(o["y"] - d["y"]).max() < dc.sample_tol(case) / 4


def test_small_vocabulary_cases_have_fewer_granules_than_beams():
    assert dc.SMALL_VOCAB == ("h256_v37", "h768_v100", "h1024_v65", "h512_v37")
    got = {(c.H, c.V, c.K) for c in (dc.BEAM[k] for k in dc.SMALL_VOCAB)}
    assert got == {(256, 37, 3), (768, 100, 8), (1024, 65, 4), (512, 37, 3)}
    for k in dc.SMALL_VOCAB:
        c = dc.BEAM[k]
        assert -(-c.V // 32) < c.K <= c.V


def test_table_covers_what_it_is_there_for():
    beam = list(dc.BEAM.values())
    for H in (256, 768, 1024):
        mine = [c for c in beam if c.H == H and not c.few_granules]
        assert {c.tile for c in mine} == {128, 256}, H
        assert {2, 3, 5, 8} <= {c.K for c in mine}, H
        assert any(c.E != 256 for c in mine) and any(c.finishes for c in mine), H
        assert any(c.few_granules and c.tile == 128 for c in beam if c.H == H), H
    assert any(c.B * c.K == 201 and c.H != 512 for c in beam)          # a tail in the 64- and 128-row tiles
    assert {c.K for c in beam if c.H == 512 and c.V == 10123} == {2, 4, 6, 7}
    assert all(c.B <= 67 and c.T <= 10 and 1 <= c.K <= 8 for c in beam)
    sample = list(dc.SAMPLE.values())
    for H in (256, 768, 1024):
        mine = [c for c in sample if c.H == H]
        assert any(c.N == 3 and not c.truncated for c in mine), H
        assert any(c.N == 1 and not c.truncated for c in mine), H
    assert any(c.B == 67 for c in sample) and any(c.tau != 1.0 for c in sample)
    assert any(c.truncated and c.H in (768, 1024) for c in sample)
    assert all(c.B <= 67 and c.T <= 10 and c.H != 512 for c in sample)
