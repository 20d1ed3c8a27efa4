"""Diverse beam groups and the length-normalised final ranking (aa_beam_decode_ex, through
``Encoder2Decoder.beam_search(groups=, diversity=, length_penalty=, return_details=)``) against
``BeamDivOracle`` (tests/beam_div_oracle.py) on the cases of tests/beam_div_cases.py, whose admissibility
is asserted on the CPU in tests/test_beam_div_cpu.py, and against oracle-free bitwise identities.

Every oracle case runs the three vocabulary stages: the default (k_vexact), ``exact_vocab=True`` (k_vocab +
k_gsumm) and ``fast=True`` (k_vbeam4 / k_vbeam5); all feed k_beam_select3<true> and k_beam_final_ex.

Bounds: seqs, ids, lengths and group equal the oracle's (both fp32 margins exceed 4 x SCORE_TOL); scores
within SCORE_TOL = 5e-5 and alpha / beta within ATT_TOL = 2e-5 of the float64 oracle -- the project's beam
bounds, from tests/test_gpu_beam.py; rank_scores within SCORE_TOL + 1e-6 |rank| (the division and the power
add a few fp32 ulps to the error of cum; 1e-6 is about 16 ulps); the default and ``exact_vocab=True`` agree
bit for bit.

Identities, all bitwise: with diversity 0 and no length penalty the beams of group g, in rank order, are
``beam_search(beam_size=K/G)``'s; the ex path at G = 1, 0, 0 equals the plain call with
``rank_scores == scores``; ``length_penalty`` alone permutes the plain call's beams and ``lengths`` is the
position of the first ``<end>`` + 1; an image's result does not depend on the rest of the batch.  With a
penalty of 1e4 the first tokens of the groups' leading beams are pairwise distinct.

Measured on an MI355X: profiles/beam_div_errors.txt (the lines this module prints).
"""
import pytest
import torch

import beam_div_cases as cases
import decode_cases as dc
from test_gpu_beam import ATT_TOL, SCORE_TOL
from test_gpu_beam_dims import MODES, model_for

pytestmark = pytest.mark.gpu

assert (SCORE_TOL, ATT_TOL) == (dc.SCORE_TOL, dc.ATT_TOL) == (5e-5, 2e-5)
RANK_REL = 1e-6
NAMES = ("ids", "alpha", "beta", "seqs", "scores", "lengths", "rank_scores", "group")


def _first_end(seqs, T):
    is_end = seqs == 2
    return torch.where(is_end.any(2), is_end.long().argmax(2) + 1, torch.full(seqs.shape[:2], T)).int()


@pytest.mark.parametrize("name", list(cases.DIV))
def test_beam_div_vs_oracle(name, gpu_device):
    case = cases.DIV[name]
    b = case.beam
    o, d = cases.oracle(name), cases.oracle(name, torch.float64)
    assert o["sel_margin"] > 4 * SCORE_TOL and o["rank_margin"] > 4 * SCORE_TOL, "oracle case too close to call"
    for k in ("seqs", "lengths", "group", "ids"):
        assert torch.equal(o[k], d[k]), k
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    out = {}
    for mode, kw in MODES:
        out[mode] = [x.cpu() for x in m.beam_search(feats, b.T, b.K, **kw, **cases.kwargs(case), return_details=True)]
    failures = []
    for mode, (ids, al, be, seqs, sc, lengths, rank, group) in out.items():
        assert seqs.shape == (b.B, b.K, b.T) and sc.shape == lengths.shape == rank.shape == group.shape == (b.B, b.K)
        assert lengths.dtype == group.dtype == torch.int32 and rank.dtype == torch.float32
        same = float((seqs == o["seqs"]).flatten(1).all(1).float().mean())
        e_sc = float((sc.double() - d["scores"]).abs().max())
        e_al = float((al.double() - d["alpha"]).abs().max())
        e_be = float((be.double() - d["beta"]).abs().max())
        r_err = (rank.double() - d["rank_scores"]).abs()
        r_tol = SCORE_TOL + RANK_REL * d["rank_scores"].abs()
        print(f"beam_div {name} H={b.H} V={b.V} B={b.B} T={b.T} K={b.K} G={case.G} diversity={case.diversity} "
              f"length_penalty={case.length_penalty} {mode}: margins {o['sel_margin']:.3e} / {o['rank_margin']:.3e}, "
              f"images equal {same:.3f}, max |score - float64| {e_sc:.3e} (tol {SCORE_TOL:.0e}), "
              f"|rank - float64| {float(r_err.max()):.3e} (tol {float(r_tol.min()):.3e}), "
              f"alpha {e_al:.2e}, beta {e_be:.2e} (tol {ATT_TOL:.0e})")
        if not bool(((seqs >= 0) & (seqs < b.V)).all()):
            failures.append(f"{mode}: token outside [0, {b.V})")
        if not torch.equal(seqs, o["seqs"]):
            failures.append(f"{mode}: seqs differ from the oracle's on {1 - same:.1%} of the images")
        for k, x in (("ids", ids), ("lengths", lengths), ("group", group)):
            if not torch.equal(x, o[k]):
                failures.append(f"{mode}: {k} differ from the oracle's")
        if not e_sc <= SCORE_TOL:
            failures.append(f"{mode}: score error {e_sc:.3e}")
        if not bool((r_err <= r_tol).all()):
            failures.append(f"{mode}: rank score error {float(r_err.max()):.3e}")
        if not (e_al <= ATT_TOL and e_be <= ATT_TOL):
            failures.append(f"{mode}: alpha / beta error {e_al:.3e} / {e_be:.3e}")
    for n, x, y in zip(NAMES, out["default"], out["exact_vocab"]):
        if not torch.equal(x, y):
            failures.append(f"default and exact_vocab differ bitwise in {n}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("name,G", [("h256_k8", 4), ("h256_k8", 8), ("h768_k8", 2), ("h1024_k8", 2), ("h512_k6", 3),
                                    ("h512_k6", 2), ("h256_ragged", 3), ("h768_v100", 4)])
def test_zero_diversity_groups_equal_the_narrow_search(name, G, gpu_device):
    """diversity = 0, length_penalty = 0: the beams with group == g, in rank order, equal
    ``beam_search(beam_size=K/G)``'s seqs and scores bit for bit, for every g."""
    b = dc.BEAM[name]
    Kg = b.K // G
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    for mode, kw in MODES:
        _, _, _, seqs, sc = m.beam_search(feats, b.T, Kg, **kw)
        r = dict(zip(NAMES, m.beam_search(feats, b.T, b.K, **kw, groups=G, return_details=True)))
        assert torch.equal(r["rank_scores"], r["scores"]), mode
        for g in range(G):
            pick = r["group"] == g
            assert bool((pick.sum(1) == Kg).all()), (mode, g)
            assert torch.equal(r["seqs"][pick].view(b.B, Kg, b.T), seqs), (mode, g)
            assert torch.equal(r["scores"][pick].view(b.B, Kg), sc), (mode, g)


@pytest.mark.parametrize("name", ["h256_k3", "h768_v100", "h1024_v65", "h512_k7"])
def test_ex_path_at_defaults_equals_the_plain_call(name, gpu_device):
    """G = 1, diversity = 0, length_penalty = 0 through aa_beam_decode_ex (forced by return_details) is the
    plain call bit for bit, with rank_scores == scores, group 0 and lengths at the first <end>."""
    b = dc.BEAM[name]
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    for mode, kw in MODES:
        plain = m.beam_search(feats, b.T, b.K, **kw)
        assert len(plain) == 5
        ex = m.beam_search(feats, b.T, b.K, **kw, return_details=True)
        assert len(ex) == 8
        for n, x, y in zip(NAMES, plain, ex):
            assert torch.equal(x, y), (mode, n)
        r = dict(zip(NAMES, ex))
        assert torch.equal(r["rank_scores"], r["scores"]) and bool((r["group"] == 0).all()), mode
        assert torch.equal(r["lengths"].cpu(), _first_end(r["seqs"].cpu(), b.T)), mode
        if not b.finishes:
            assert bool((r["lengths"] == b.T).all())
        # end_id = -1: nothing finishes, every length is T
        off = dict(zip(NAMES, m.beam_search(feats, b.T, b.K, end_id=-1, **kw, length_penalty=0.7, return_details=True)))
        assert bool((off["lengths"] == b.T).all()), mode
        for n, x, y in zip(NAMES[:5], m.beam_search(feats, b.T, b.K, end_id=-1, **kw), [off[n] for n in NAMES[:5]]):
            assert torch.equal(x, y), (mode, n)   # equal lengths: the order of the raw scores


@pytest.mark.parametrize("name,lp", [("h256_k8", 0.7), ("h768_k5", 1.0), ("h1024_k5", 0.7), ("h512_k4", 2.0)])
def test_length_penalty_alone_permutes_the_plain_beams(name, lp, gpu_device):
    b = dc.BEAM[name]
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    _, _, _, seqs, sc = (x.cpu() for x in m.beam_search(feats, b.T, b.K))
    r = {n: x.cpu() for n, x in zip(NAMES, m.beam_search(feats, b.T, b.K, length_penalty=lp, return_details=True))}
    assert torch.equal(r["lengths"], _first_end(r["seqs"], b.T))
    assert bool((r["rank_scores"][:, :-1] >= r["rank_scores"][:, 1:]).all())
    assert torch.equal(r["ids"], r["seqs"][:, 0]) and bool((r["group"] == 0).all())
    for i in range(b.B):
        plain = sorted((tuple(s.tolist()), float(x)) for s, x in zip(seqs[i], sc[i]))
        assert sorted((tuple(s.tolist()), float(x)) for s, x in zip(r["seqs"][i], r["scores"][i])) == plain, i
    # rank = cum / len^lp in fp32, recomputed from the outputs (torch's pow and the device's may differ by an ulp or two)
    want = r["scores"].double() / r["lengths"].double() ** lp
    assert bool(((r["rank_scores"].double() - want).abs() <= RANK_REL * want.abs()).all())


@pytest.mark.parametrize("mode,kw", MODES)
def test_batch_invariance(mode, kw, gpu_device):
    """Images 62..66 of the 67 of h256_ragged (rows 186..200: across the last 64-row boundary) alone equal
    the same images in the full batch, bit for bit."""
    case = cases.DIV["h256_ragged"]
    b = case.beam
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    big = m.beam_search(feats, b.T, b.K, **kw, **cases.kwargs(case), return_details=True)
    small = m.beam_search(feats[62:67].contiguous(), b.T, b.K, **kw, **cases.kwargs(case), return_details=True)
    for n, x, y in zip(NAMES, big, small):
        assert torch.equal(x[62:67], y), n


@pytest.mark.parametrize("name,G", [("h256_k8", 4), ("h768_v100", 8), ("h512_k6", 3), ("h1024_k8", 2)])
def test_huge_penalty_makes_the_groups_first_tokens_distinct(name, G, gpu_device):
    b = dc.BEAM[name]
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    r = {n: x.cpu() for n, x in zip(NAMES, m.beam_search(feats, b.T, b.K, groups=G, diversity=1e4, return_details=True))}
    Kg = b.K // G
    for i in range(b.B):
        first = [r["seqs"][i][r["group"][i] == g][:, 0].tolist() for g in range(G)]
        assert all(len(f) == Kg for f in first)
        lead = [f[0] for f in first]
        assert len(set(lead)) == G, (i, lead)
    # the penalty steers the selection only: scores are raw log-probabilities
    assert bool(torch.isfinite(r["scores"]).all()) and bool((r["scores"] > -1e3).all())
