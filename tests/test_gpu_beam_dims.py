"""Beam search (aa_beam_decode, through ``Encoder2Decoder.beam_search``) at hidden 256, 768 and 1024, at
the beam widths of hidden 512 no other test runs, and at vocabularies with fewer non-empty 32-column
granules than beams, against ``BeamOracle`` (tests/decode_cases.py: the case table and its oracles;
its conditions are asserted on the CPU in tests/test_decode_cases_cpu.py).

Every case runs the three vocabulary stages: the default (k_vexact), ``exact_vocab=True`` (k_vocab +
k_gsumm) and ``fast=True`` (bf16x3: k_vbeam5 on a vocabulary padded to whole 256-column tiles, else
k_vbeam4).  What each reaches that no other test does:

    k_lstm<256 | 768 | 1024, gather>     every h256_* / h768_* / h1024_* case from step 1 on
    k_atten<1>, kdiv = K                 h256_*  (K = 2, 3, 5, 8)
    k_atten<3>, kdiv = K                 h768_*  (K = 2, 3, 5, 8)
    k_atten5<1024>, kdiv = K             h1024_* (K = 2, 3, 4, 5, 8)
    k_atten5b<512, 2> / <512, 4>         h512_k2 / h512_k4
    k_atten5<512>, kdiv = 6, 7           h512_k6 / h512_k7
    k_vbeam5<H> (fast)                   h256_k8, h256_k2; h768_k5, h768_k8; h1024_k3, h1024_k8
    k_vbeam4<H> (fast)                   h256_k3, h256_ragged, h256_k5, h256_v37; h768_k3, h768_k2,
                                         h768_v100; h1024_k2, h1024_k5, h1024_v65; h512_v37 (<512>)
    ub3 written by k_atten<1>, <3>, k_atten5<1024>    every fast run off 512
    k_beam_select3, granules < K         h256_v37, h512_v37 (2 < 3), h1024_v65 (3 < 4), h768_v100 (4 < 8)

Bounds: the project's own, from tests/test_gpu_beam.py -- sequences and ids equal to the oracle's (the
fp32 oracle's selection margin is asserted above 4 x SCORE_TOL first), scores within SCORE_TOL = 5e-5
of the float64 oracle, alpha / beta within ATT_TOL = 2e-5; the default and ``exact_vocab=True`` agree
bit for bit.  The fast mode is held to the same bounds here, equality of the sequences included: with
margins of 4e-4 and more its bf16x3 logits (fp32-accurate) cannot move a selection.

Measured on an MI355X: profiles/decode_dims_errors.txt (the lines this module prints).

k_beam_select3 with fewer non-empty granules than K: before its fix the rounds that look for the K-th
largest granule maximum ran out of granules, the threshold became the NaN that key 0 decodes to, no
candidate was read, and the merge built its keys from empty slots (token -1, NaN scores); the four
small-vocabulary cases are the regression test (tokens in [0, V), finite scores, and the oracle's beams).
"""
import numpy as np
import pytest
import torch

import decode_cases as dc
from test_gpu_beam import ATT_TOL, SCORE_TOL

from adaptive_amd import Config, Encoder2Decoder

pytestmark = pytest.mark.gpu

assert (SCORE_TOL, ATT_TOL) == (dc.SCORE_TOL, dc.ATT_TOL) == (5e-5, 2e-5)

MODES = (("default", {}), ("exact_vocab", {"exact_vocab": True}), ("fast", {"fast": True}))


def model_for(case, dev):
    cf = Config(adaptive_word_embed_size=case.E, adaptive_lstm_hidden_size=case.H, vocab_length=case.V)
    m = Encoder2Decoder(cf).to(dev)
    m.load_state_dict({k: torch.from_numpy(v).to(dev) for k, v in dc.state(case).items()})
    return m


@pytest.mark.parametrize("name", list(dc.BEAM))
def test_beam_vs_oracle(name, gpu_device):
    case = dc.BEAM[name]
    o_ids, _, _, o_seqs, _, margin = dc.beam_oracle(name)
    assert margin > 4 * SCORE_TOL, f"oracle case too close to call: margin {margin}"
    d_ids, d_al, d_be, d_seqs, d_sc, _ = dc.beam_oracle(name, torch.float64)
    assert torch.equal(o_seqs, d_seqs) and torch.equal(o_ids, d_ids)
    if case.finishes:
        assert (o_seqs == 2).any(), "case meant to exercise finished beams has none"
    m = model_for(case, gpu_device)
    feats = torch.from_numpy(dc.features(case)).to(gpu_device)
    out = {}
    for mode, kw in MODES:
        out[mode] = [x.cpu() for x in m.beam_search(feats, case.T, case.K, **kw)]
    failures = []
    for mode, (ids, al, be, seqs, sc) in out.items():
        assert seqs.shape == (case.B, case.K, case.T) and sc.shape == (case.B, case.K)
        same = float((seqs == o_seqs).flatten(1).all(1).float().mean())
        e_sc = float((sc.double() - d_sc).abs().max())
        e_al = float((al.double() - d_al).abs().max())
        e_be = float((be.double() - d_be).abs().max())
        print(f"beam {name} H={case.H} E={case.E} V={case.V} B={case.B} T={case.T} K={case.K} {mode}: "
              f"margin {margin:.3e}, images equal {same:.3f}, max |score - float64| {e_sc:.3e} (tol {SCORE_TOL:.0e}), "
              f"alpha {e_al:.2e}, beta {e_be:.2e} (tol {ATT_TOL:.0e})")
        if case.few_granules:
            if not bool(((seqs >= 0) & (seqs < case.V)).all()):
                failures.append(f"{mode}: token outside [0, {case.V})")
            if not bool(torch.isfinite(sc).all()):
                failures.append(f"{mode}: score not finite")
        if not torch.equal(seqs, o_seqs):
            failures.append(f"{mode}: seqs differ from the oracle's on {1 - same:.1%} of the images")
        if not torch.equal(ids, o_ids):
            failures.append(f"{mode}: ids differ from the oracle's")
        if not e_sc <= SCORE_TOL:
            failures.append(f"{mode}: score error {e_sc:.3e}")
        if not (e_al <= ATT_TOL and e_be <= ATT_TOL):
            failures.append(f"{mode}: alpha / beta error {e_al:.3e} / {e_be:.3e}")
    for n, x, y in zip(("ids", "alpha", "beta", "seqs", "scores"), out["default"], out["exact_vocab"]):
        if not torch.equal(x, y):
            failures.append(f"default and exact_vocab differ bitwise in {n}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("mode,kw", MODES)
def test_beam_batch_invariance_hidden_256(mode, kw, gpu_device):
    """An image's beams do not depend on the rest of the batch (bit-exact): images 62..66 of the 67 of
    h256_ragged (rows 186..200: across the last 64-row boundary, 192, into the ragged tail) alone."""
    case = dc.BEAM["h256_ragged"]
    m = model_for(case, gpu_device)
    feats = torch.from_numpy(dc.features(case)).to(gpu_device)
    big = m.beam_search(feats, case.T, case.K, **kw)
    small = m.beam_search(feats[62:67].contiguous(), case.T, case.K, **kw)
    for n, a, b in zip(("ids", "alpha", "beta", "seqs", "scores"), big, small):
        assert torch.equal(a[62:67], b), n
