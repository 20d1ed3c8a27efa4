"""CPU: the case table of tests/decode_cases.py and the conditions its GPU tests
(tests/test_gpu_beam_dims.py, tests/test_gpu_sample_dims.py, tests/test_gpu_greedy_dims.py) rest on.

* Every case is admissible: the fp32 oracle's selection margin exceeds 4 x SCORE_TOL (beam), 4 x
  SCORE_TOL x max(1, 1/tau) (sampling); a truncated sampling case is robust at every (row, step).
* The float64 oracle (the same program text in double) selects the same sequences / tokens, and its
  scores lie within a quarter of SCORE_TOL of the fp32 oracle's, so it can stand in as the reference
  of the GPU comparison (measured: beam scores 8.1e-7 .. 7.7e-6, logp 4.8e-7 .. 1.4e-6).
* A case has the properties it is listed for: beams finish, fewer non-empty granules than K, and the
  table covers the kernel forms the GPU tests are there for.
* Greedy cases: the fp32 oracle's smallest top-1 / top-2 logit gap exceeds 4 x SCORE_TOL and the float64
  oracle picks the same ids; a negative case has no logit >= 0 at the top of any (row, step).
* Adversarial greedy cases, every designed row, none left out: the float64 argmax is the designed
  winner and the fp32 oracle's token; the bf16 products' argmax is a designed decoy whose lead is at
  least 0.6 of 2 ||u|| ||w - bf16(w)|| (the larger of the pair's two norms: what the screen's bound
  charges the pair when they lead their granules); the numpy emulation of the screen keeps the winner
  with the kernel's bound and rejects it with the ||u|| D_g term left out; a triple's winner ranks third
  in its granule in bf16.  Measured shares: 0.76 .. 0.92; with the whole bound halved the emulation still
  rejects the winner of 35 of the 42 designed rows (printed, not asserted).
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


# ---- greedy ----------------------------------------------------------------------------------------

ADVERSARIAL = [k for k, c in dc.GREEDY.items() if c.adversarial]


@pytest.mark.parametrize("name", list(dc.GREEDY))
def test_greedy_case_is_admissible_and_float64_agrees(name):
    case = dc.GREEDY[name]
    o, d = dc.greedy_oracle(name), dc.greedy_oracle(name, torch.float64)
    assert o["ids"].shape == (case.B, case.T) and d["alpha"].dtype == torch.float64 and o["alpha"].dtype == torch.float32
    gap = float(o["gap"].min())
    print(f"{name}: smallest gap {gap:.3e} (float64 {float(d['gap'].min()):.3e}), largest logit "
          f"{float(o['top'].min()):.3f} .. {float(o['top'].max()):.3f}, max |fp32 - float64| alpha "
          f"{float((o['alpha'].double() - d['alpha']).abs().max()):.1e}, beta {float((o['beta'].double() - d['beta']).abs().max()):.1e}")
    assert gap > 4 * dc.SCORE_TOL, f"case too close to call: gap {gap}"
    assert torch.equal(o["ids"], d["ids"])
    assert bool(((o["ids"] >= 0) & (o["ids"] < case.V)).all())
    if case.negative:
        assert float(o["top"].max()) < 0 and float(d["top"].max()) < 0


@pytest.mark.parametrize("name", [k for k, c in {**dc.BEAM, **dc.SAMPLE}.items() if c.bias_shift])
def test_shifted_beam_and_sample_weights_give_negative_logits(name):
    """The largest logit of the case's weights on its features' greedy rows is below 0 with room to
    spare (the beam's / sampler's own rows see other tokens, whose logits differ by a few units)."""
    case = dc.BEAM.get(name) or dc.SAMPLE[name]
    o = dc._greedy_run(dc.state(case), dc.features(case), case.T, torch.float32)
    print(f"{name}: largest logit {float(o['top'].max()):.3f}")
    assert case.V % 128 and float(o["top"].max()) < -8


@pytest.mark.parametrize("name", ADVERSARIAL)
def test_adversarial_case_conditions(name):
    case = dc.GREEDY[name]
    o, d = dc.greedy_oracle(name), dc.greedy_oracle(name, torch.float64)
    sd = dc.state(case)
    W, b = sd[dc.MLP_W], sd[dc.MLP_B]
    u64 = d["u"][:, 0].numpy()
    u32 = u64.astype(np.float32)
    wb = dc.bf16(W).astype(np.float64)
    L = u64 @ W.astype(np.float64).T + b                       # float64 logits of the float64 u0
    A = dc.bf16(u32).astype(np.float64) @ wb.T + b             # what the screen ranks by
    dw = np.linalg.norm(W - wb, axis=1)
    keep = dc.screen_candidates(u32, W, b)
    keep_no_d = dc.screen_candidates(u32, W, b, with_D=False)
    keep_half = dc.screen_candidates(u32, W, b, scale=0.5)
    rows = dc.designed(case)
    assert len(rows) == case.B, "every row of an adversarial case is designed"
    shares, halves = [], 0
    for r, win, decoys in rows:
        top = int(A[r].argmax())
        assert int(L[r].argmax()) == win == int(o["ids"][r, 0]) == int(d["ids"][r, 0]), (r, win)    # (a)
        assert top in decoys, (r, top, decoys)                                                       # (b)
        share = (A[r, top] - A[r, win]) / (2 * np.linalg.norm(u64[r]) * max(dw[top], dw[win]))
        shares.append(share)
        assert share >= 0.6, (r, share)                                                              # (c)
        assert keep[r, win], f"row {r}: the kernel's bound drops the winner {win}"                   # (d)
        assert not keep_no_d[r, win], f"row {r}: the bound without ||u|| D_g still keeps {win}"
        halves += not keep_half[r, win]
        if len(decoys) == 2:                                                                         # (e)
            g = win // 32 * 32
            assert {n // 32 * 32 for n in decoys} == {g}
            order = g + np.argsort(-A[r, g:min(g + 32, case.V)])[:3]
            assert int(order[2]) == win and set(order[:2].tolist()) == set(decoys), (r, order)
    print(f"{name}: decoy's bf16 lead / (2 |u| |w - bf16(w)|) {min(shares):.3f} .. {max(shares):.3f}; candidates per row "
          f"{keep.sum(1).min()} .. {keep.sum(1).max()}; with the bound halved {halves} of {len(rows)} winners are rejected")


def test_greedy_table_covers_what_it_is_there_for():
    greedy = list(dc.GREEDY.values())
    plain = [c for c in greedy if not c.adversarial]
    adv = [c for c in greedy if c.adversarial]
    assert all(c.B <= 131 and c.T <= 4 for c in greedy)
    assert all(c.B <= 16 and c.T in (1, 2) for c in adv) and {c.T for c in adv} == {1, 2}
    assert {c.wide for c in plain if c.H == 256} == {c.wide for c in adv if c.H == 256} == {True, False}
    assert any(c.H == 512 and c.V == 10123 and c.wide for c in adv) and any(c.H == 512 and not c.wide for c in plain)
    assert any(c.B == 131 and c.wide for c in plain)            # a full 128-row screen tile and a tail
    for H in (256, 768, 1024):
        assert any(c.E != 256 for c in greedy if c.H == H), H
        assert any(c.B % 64 and c.B > 64 for c in plain if c.H == H), H   # a tail behind a full 64-row tile
    for H in (256, 512, 768, 1024):
        groups = [(c, g) for c in adv if c.H == H for g in c.adversarial.groups]
        assert any(len(g) == 2 and g[0] // 32 == g[1] // 32 for c, g in groups), H                 # one granule
        assert any(len(g) == 2 and g[0] // c.tile != g[1] // c.tile for c, g in groups), H         # two tiles
        assert any(len(g) == 2 and g[0] // c.tile == g[1] // c.tile and g[0] // 32 != g[1] // 32 for c, g in groups), H
        assert any(len(g) == 3 and len({n // 32 for n in g}) == 1 for c, g in groups), H           # a triple
    for c in adv:
        pairs = [g for g in c.adversarial.groups if len(g) == 2]
        assert sum(g[1] < g[0] for g in pairs) * 2 == len(pairs)   # decoy below the winner in half of them
        assert any(g[0] == 0 for g in pairs) and any(g[0] == c.V - 1 for g in pairs)
    assert any(c.V % 32 for c in adv)                            # a winner beside padding columns
    assert any(c.negative and c.V % 128 for c in adv) and any(c.negative and c.V % 128 for c in plain)
