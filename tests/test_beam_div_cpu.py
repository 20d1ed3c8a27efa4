"""CPU: diverse beam groups and the length-normalised final ranking, without a GPU.

* the case table of tests/beam_div_cases.py and the conditions tests/test_gpu_beam_div.py rests on: every
  case is admissible -- both margins of the fp32 ``BeamDivOracle`` (selection and rank) exceed
  4 x SCORE_TOL = 2e-4, the float64 oracle gives the same seqs, lengths and group, ``<end>`` occurs exactly
  where the base case says beams finish -- and the two excluded configurations really fail the rule.
  These are conditions on the cases, not tolerances on the code;
* the oracle itself: G = 1, diversity = 0, length_penalty = 0 is ``BeamOracle.beam_search``; with
  diversity = 0 the beams of each group are those of a K / G-beam search; a huge penalty makes the groups'
  first tokens pairwise distinct; length_penalty alone permutes the plain beams;
* ``Encoder2Decoder.beam_search``'s new argument errors, raised before the library is touched, the
  baseline model's refusal, and the C ABI's argument checks (no device work: fake aligned pointers).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import beam_div_cases as cases
import decode_cases as dc
from beam_div_oracle import BeamDivOracle


@pytest.mark.parametrize("name", list(cases.DIV))
def test_case_is_admissible_and_float64_agrees(name):
    case = cases.DIV[name]
    b = case.beam
    o, d = cases.oracle(name), cases.oracle(name, torch.float64)
    err = float((o["scores"].double() - d["scores"]).abs().max())
    print(f"{name}: G={case.G} diversity={case.diversity} length_penalty={case.length_penalty}: selection margin "
          f"{o['sel_margin']:.3e} (float64 {d['sel_margin']:.3e}), rank margin {o['rank_margin']:.3e} "
          f"(float64 {d['rank_margin']:.3e}), penalised picks {o['penalised']}, max |fp32 - float64| score {err:.2e}")
    assert b.K % case.G == 0 and o["seqs"].shape == (b.B, b.K, b.T)
    assert o["scores"].dtype == torch.float32 and d["scores"].dtype == torch.float64
    assert o["sel_margin"] > cases.MARGIN, f"selection too close to call: {o['sel_margin']}"
    assert o["rank_margin"] > cases.MARGIN, f"final ranking too close to call: {o['rank_margin']}"
    for k in ("seqs", "lengths", "group", "ids"):
        assert torch.equal(o[k], d[k]), k
    assert err < dc.SCORE_TOL / 4
    assert bool((o["seqs"] == 2).any()) == b.finishes
    assert o["penalised"] == d["penalised"] == case.penalised
    # the outputs are what they say they are
    seqs, lengths = o["seqs"], o["lengths"].long()
    is_end = seqs == 2
    first = torch.where(is_end.any(2), is_end.long().argmax(2) + 1, torch.full_like(lengths, b.T))
    assert torch.equal(lengths, first)
    if not b.finishes:
        assert bool((lengths == b.T).all())
    assert bool((o["rank_scores"][:, :-1] > o["rank_scores"][:, 1:]).all())
    assert torch.equal(o["group"].sort(1).values, (torch.arange(b.K) // case.Kg).int().expand(b.B, b.K))
    assert torch.equal(o["ids"], seqs[:, 0])
    assert bool(((seqs >= 0) & (seqs < b.V)).all()) and bool(torch.isfinite(d["scores"]).all())


def test_table_covers_what_it_is_there_for():
    t = cases.DIV
    assert {c.beam.H for c in t.values()} == {256, 512, 768, 1024}
    assert {c.Kg for c in t.values()} >= {1, 2, 4}
    assert any(c.G == c.beam.K == 8 for c in t.values())
    assert any(c.beam.few_granules for c in t.values()) and any(not c.beam.finishes for c in t.values())
    assert any(c.length_penalty == 0.0 for c in t.values()) and any(c.beam.bias_shift < 0 for c in t.values())
    # both kinds of diversity: the penalty only excludes / a penalised candidate still wins
    assert all(c.penalised == 0 for c in t.values() if c.diversity == 2.0)
    assert sum(c.penalised > 0 for c in t.values() if c.diversity == 0.5) >= 4
    assert t["h256_ragged"].beam.B == 67 and t["h256_ragged"].Kg == 1


@pytest.mark.parametrize("name", list(cases.INADMISSIBLE))
def test_excluded_configurations_fail_the_rule(name):
    o = cases.run(cases.INADMISSIBLE[name], torch.float32)
    print(f"{name}: selection margin {o['sel_margin']:.3e}, rank margin {o['rank_margin']:.3e}")
    assert not (o["sel_margin"] > cases.MARGIN and o["rank_margin"] > cases.MARGIN)


@pytest.fixture(scope="module")
def small():
    case = dc.BEAM["h768_v100"]   # K = 8, V = 100: cheap on the CPU
    feats = torch.from_numpy(dc.features(case))
    return case, feats, BeamDivOracle(dc.state(case))


@pytest.fixture(scope="module")
def small64(small):
    """float64: the CPU's GEMM rounds a row differently with the number of rows beside it, which moves an
    fp32 score by a few 1e-6 between a K-row and a K / G-row search; in double that is below 1e-12."""
    case, feats, _ = small
    return case, feats.double(), BeamDivOracle(dc.state(case), dtype=torch.float64)


def test_defaults_equal_the_plain_oracle(small):
    case, feats, orc = small
    ids, al, be, seqs, sc = orc.beam_search(feats, case.T, case.K)
    r = orc.beam_search_div(feats, case.T, case.K)
    for k, x in (("ids", ids), ("alpha", al), ("beta", be), ("seqs", seqs), ("scores", sc)):
        assert torch.equal(r[k], x), k
    assert torch.equal(r["rank_scores"], sc) and bool((r["group"] == 0).all()) and r["penalised"] == 0


@pytest.mark.parametrize("G", (2, 4, 8))
def test_zero_diversity_groups_equal_the_narrow_search(small64, G):
    case, feats, orc = small64
    Kg = case.K // G
    _, _, _, seqs, sc = orc.beam_search(feats, case.T, Kg)
    r = orc.beam_search_div(feats, case.T, case.K, groups=G)
    for g in range(G):
        pick = r["group"] == g
        assert bool((pick.sum(1) == Kg).all())
        assert torch.equal(r["seqs"][pick].view(case.B, Kg, case.T), seqs)
        assert float((r["scores"][pick].view(case.B, Kg) - sc).abs().max()) < 1e-10


def test_huge_penalty_makes_first_tokens_distinct_and_length_penalty_permutes(small):
    case, feats, orc = small
    G = 4
    r = orc.beam_search_div(feats, case.T, case.K, groups=G, diversity=1e4)
    for b in range(case.B):
        lead = [int(r["seqs"][b][r["group"][b] == g][0, 0]) for g in range(G)]
        assert len(set(lead)) == G, lead
    _, _, _, seqs, sc = orc.beam_search(feats, case.T, case.K)
    p = orc.beam_search_div(feats, case.T, case.K, length_penalty=0.7)
    assert bool((p["rank_scores"][:, :-1] >= p["rank_scores"][:, 1:]).all())
    for b in range(case.B):
        plain = sorted((tuple(s.tolist()), float(x)) for s, x in zip(seqs[b], sc[b]))
        assert sorted((tuple(s.tolist()), float(x)) for s, x in zip(p["seqs"][b], p["scores"][b])) == plain
    want = (p["scores"] / p["lengths"].float() ** 0.7)
    assert torch.allclose(p["rank_scores"], want, rtol=1e-6, atol=0)


def _no_library():
    raise AssertionError("the library must not be touched")


def test_python_argument_errors_before_the_library(monkeypatch):
    from adaptive_amd import Config, Encoder2Decoder, _lib
    m = Encoder2Decoder(Config())
    monkeypatch.setattr(_lib, "load", _no_library)
    x = torch.zeros(2, 2048, 7, 7)
    for g in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="groups"):
            m.beam_search(x, 5, 6, groups=g)
    for K, g in ((6, 4), (3, 2), (8, 3), (2, 4)):
        with pytest.raises(ValueError, match="groups must divide"):
            m.beam_search(x, 5, K, groups=g)
    for v in (-0.1, float("nan"), float("inf"), -float("inf"), 1e60, "x", None, True):
        with pytest.raises(ValueError, match="diversity"):
            m.beam_search(x, 5, 6, groups=3, diversity=v)
        with pytest.raises(ValueError, match="length_penalty"):
            m.beam_search(x, 5, 6, length_penalty=v)
    with pytest.raises(TypeError):  # keyword-only
        m.beam_search(x, 5, 6, 2, None, False, None, 3)
    with pytest.raises(RuntimeError, match="GPU|CUDA"):  # valid arguments, CPU tensor: no CPU path
        m.beam_search(x, 5, 6, groups=3, diversity=0.5, length_penalty=0.7, return_details=True)


def test_baseline_model_still_refuses_beam_search(monkeypatch):
    from adaptive_amd import _lib
    from adaptive_amd.baseline_attention import Config, Encoder2Decoder
    m = Encoder2Decoder(Config())
    monkeypatch.setattr(_lib, "load", _no_library)
    with pytest.raises(NotImplementedError, match="baseline.*beam_search"):
        m.beam_search(torch.zeros(2, 2048, 7, 7), 5, 6, groups=3, diversity=0.5, return_details=True)


# ---- C-ABI, no device work --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from adaptive_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "adaptive_amd", "csrc")], check=True)
    return _lib.load()


def test_decode_ex_argument_errors_without_device_work(lib):
    from adaptive_amd import _lib
    p, big = 256, 10 ** 9  # fake aligned pointer
    dims = _lib.Dims(256, 512, 10123, 2048, 49)

    def model(vocab=10123, nbytes=big):
        return _lib.Model(_lib.Dims(256, 512, vocab, 2048, 49), p, nbytes)

    def call(m, B=4, T=20, K=6, end_id=2, feats=p, ws=p, ws_bytes=big, flags=0, G=3, lam=0.5, lp=0.7, opts=True):
        o = ctypes.byref(_lib.BeamOpts(G, lam, lp, None, None, None)) if opts else None
        return lib.aa_beam_decode_ex(m, feats, B, T, K, end_id, None, None, None, None, None, ws, ws_bytes, flags, None,
                                     None, o)

    m = model()
    need = lib.aa_beam_workspace_bytes(dims, 4, 20, 6)
    assert need > 0
    # the plain call's checks, in its order
    assert call(None) == -1 and call(model(nbytes=10)) == -4 and call(model(vocab=256 * 64 + 1)) == -2
    assert call(m, K=0) == -3 and call(m, K=9, G=3) == -3 and call(m, B=-1) == -3 and call(m, end_id=10123) == -3
    # the options: AA_ERR_SHAPE, for either vocabulary stage flag too
    for G in (0, -1, 4, 5, 12):
        assert call(m, G=G) == -3, G
    for v in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert call(m, lam=v) == -3 and call(m, lp=v) == -3, v
        assert call(m, lam=v, flags=_lib.BEAM_FAST) == -3 and call(m, lp=v, flags=_lib.DECODE_EXACT_VOCAB) == -3
    # ... before the empty-batch return, the pointer checks after it
    for B, T in ((0, 20), (4, 0)):
        assert call(m, B=B, T=T, feats=None, ws=None, ws_bytes=0) == 0
        assert call(m, B=B, T=T, G=4) == -3 and call(m, B=B, T=T, lam=-1.0) == -3 and call(m, B=B, T=T, lp=-1.0) == -3
    assert call(m, feats=None) == -1 and call(m, ws=None) == -1 and call(m, ws=p + 4) == -5
    # valid options pass every check up to the workspace size: the workspace is aa_beam_workspace_bytes
    for G in (1, 2, 3, 6):
        assert call(m, G=G, ws_bytes=need - 1) == -4
    assert call(m, G=1, lam=0.0, lp=0.0, ws_bytes=need - 1) == -4
    # opts == NULL: aa_beam_decode
    assert call(m, opts=False, ws_bytes=need - 1) == -4
    assert lib.aa_beam_decode(m, p, 4, 20, 6, 2, None, None, None, None, None, p, need - 1, 0, None, None) == -4
