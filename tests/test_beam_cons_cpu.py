"""CPU: the constrained beam search (suppressed tokens, minimum length, no repeated n-grams, no ``<end>``
after given tokens), without a GPU.

* the case table of tests/beam_cons_cases.py and the conditions tests/test_gpu_beam_cons.py rests on: every
  case is admissible -- both margins of the fp32 ``BeamConsOracle`` (selection and rank) exceed
  4 x SCORE_TOL = 2e-4 and the float64 oracle gives the same seqs, lengths and group -- each constraint
  blocks what the table says it blocks, and the two excluded configurations really fail the rule.  These are
  conditions on the cases, not tolerances on the code;
* the oracle itself: its results obey the four rules, and with everything off it is ``BeamDivOracle``;
* ``Encoder2Decoder.beam_search``'s new argument errors, raised before the library is touched, the baseline
  model's refusal, and the C ABI's argument checks (no device work: fake aligned pointers).
"""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import ROOT

import beam_cons_cases as cases
import decode_cases as dc
from beam_cons_oracle import KINDS, BeamConsOracle
from beam_div_oracle import BeamDivOracle

END = 2


@pytest.mark.parametrize("name", list(cases.CONS))
def test_case_is_admissible_and_float64_agrees(name):
    case = cases.CONS[name]
    b = case.beam
    o, d = cases.oracle(name), cases.oracle(name, torch.float64)
    err = float((o["scores"].double() - d["scores"]).abs().max())
    print(f"{name}: G={case.G} diversity={case.diversity} length_penalty={case.length_penalty} min_length="
          f"{case.min_length} n={case.ngram} suppress={case.suppress} no_end_after={case.no_end_after}: selection margin "
          f"{o['sel_margin']:.3e} (float64 {d['sel_margin']:.3e}), rank margin {o['rank_margin']:.3e} (float64 "
          f"{d['rank_margin']:.3e}), blocked {cases.blocked(o)}, max |fp32 - float64| score {err:.2e}")
    assert b.K % case.G == 0 and o["seqs"].shape == (b.B, b.K, b.T)
    assert o["scores"].dtype == torch.float32 and d["scores"].dtype == torch.float64
    assert o["sel_margin"] > cases.MARGIN, f"selection too close to call: {o['sel_margin']}"
    assert o["rank_margin"] > cases.MARGIN, f"final ranking too close to call: {o['rank_margin']}"
    for k in ("seqs", "lengths", "group", "ids"):
        assert torch.equal(o[k], d[k]), k
    assert err < dc.SCORE_TOL / 4
    assert cases.blocked(o) == cases.blocked(d) == case.blocked
    assert torch.equal(o["ids"], o["seqs"][:, 0])
    assert bool(((o["seqs"] >= 0) & (o["seqs"] < b.V)).all()) and bool(torch.isfinite(d["scores"]).all())


@pytest.mark.parametrize("name", list(cases.CONS))
def test_oracle_result_obeys_the_rules(name):
    case = cases.CONS[name]
    b = case.beam
    seqs = cases.oracle(name)["seqs"]
    n = case.ngram
    for v in case.suppress:
        assert not bool((seqs == v).any()), f"suppressed token {v} emitted"
    for s in seqs.reshape(-1, b.T).tolist():
        L = s.index(END) if END in s else b.T          # the tokens before the first <end>
        assert L >= case.min_length or L == b.T, s
        if L < b.T:
            assert (s[L - 1] if L else 1) not in case.no_end_after, s
            assert all(v == END for v in s[L:]), s       # a finished beam is carried as <end>
        if n:
            grams = [tuple(s[i:i + n]) for i in range(L - n + 1)]
            assert len(set(grams)) == len(grams), (n, s)
    if case.min_length >= b.T:
        assert not bool((seqs == END).any())


def test_table_covers_what_it_is_there_for():
    t = cases.CONS
    assert {c.beam.H for c in t.values()} == {256, 512, 768, 1024}
    assert {c.beam.V for c in t.values()} >= {37, 65} and any(c.beam.few_granules for c in t.values())
    assert t["h256_ragged"].beam.B == 67
    assert any(c.G > 1 and c.diversity > 0 for c in t.values()) and any(c.length_penalty > 0 for c in t.values())
    assert {c.ngram for c in t.values()} >= {1, 2, 3}
    assert any(c.min_length == c.beam.T for c in t.values()) and any(c.beam.bias_shift < 0 for c in t.values())
    for i, kind in enumerate(KINDS):
        assert any(c.blocked[i] > 0 for c in t.values()), kind
    assert any(1 in c.no_end_after for c in t.values())   # <start>: rule 3 at step 0


@pytest.mark.parametrize("name", list(cases.INADMISSIBLE))
def test_excluded_configurations_fail_the_rule(name):
    o = cases.run(cases.INADMISSIBLE[name], torch.float32)
    print(f"{name}: selection margin {o['sel_margin']:.3e}, rank margin {o['rank_margin']:.3e}")
    assert not (o["sel_margin"] > cases.MARGIN and o["rank_margin"] > cases.MARGIN)


@pytest.mark.parametrize("G,diversity,lp", [(1, 0.0, 0.0), (4, 0.5, 0.7)])
def test_everything_off_equals_the_div_oracle(G, diversity, lp):
    case = dc.BEAM["h768_v100"]   # K = 8, V = 100: cheap on the CPU
    feats = torch.from_numpy(dc.features(case))
    want = BeamDivOracle(dc.state(case)).beam_search_div(feats, case.T, case.K, groups=G, diversity=diversity,
                                                         length_penalty=lp)
    got = BeamConsOracle(dc.state(case)).beam_search_cons(feats, case.T, case.K, groups=G, diversity=diversity,
                                                          length_penalty=lp)
    assert got.pop("blocked") == {k: 0 for k in KINDS}
    assert got.keys() == want.keys()
    for k, x in want.items():
        assert torch.equal(got[k], x) if isinstance(x, torch.Tensor) else got[k] == x, k


def test_forbidden_mask_on_hand_built_histories():
    """Rule 4 restated on tiny histories: n = 2 after 'a b a' forbids b; n = 3 after 'a b c a b' forbids c;
    n = 1 forbids every emitted token; fewer than n - 1 tokens forbid nothing."""
    f = BeamConsOracle.forbidden

    def ngram(hist, n):
        h = torch.tensor(hist).view(1, 1, -1)
        return f(h, h.size(2), 10, END, (), 0, n, ())["ngram"][0, 0].nonzero().flatten().tolist()
    assert ngram([5, 6, 5], 2) == [6]
    assert ngram([5, 6, 7, 5, 6], 3) == [7]
    assert ngram([5, 6, 7, 5], 3) == []
    assert ngram([5, 6, 5], 1) == [5, 6]
    assert ngram([5], 3) == [] and ngram([], 2) == [] and ngram([5, 5], 2) == [5]
    m = f(torch.tensor([[[4]]]), 1, 10, END, (3, 3, 9), 2, 0, (4,))
    assert m["suppress"][0, 0].nonzero().flatten().tolist() == [3, 9]
    assert m["min_length"][0, 0].nonzero().flatten().tolist() == [END]
    assert m["no_end_after"][0, 0].nonzero().flatten().tolist() == [END]
    # y_{-1} = <start> = 1
    assert f(torch.zeros(1, 1, 0, dtype=torch.long), 0, 10, END, (), 0, 0, (1,))["no_end_after"][0, 0, END]


def _no_library():
    raise AssertionError("the library must not be touched")


def test_python_argument_errors_before_the_library(monkeypatch):
    from adaptive_amd import Config, Encoder2Decoder, _lib
    m = Encoder2Decoder(Config(vocab_length=100))
    monkeypatch.setattr(_lib, "load", _no_library)
    x = torch.zeros(2, 2048, 7, 7)
    for name in ("suppress_ids", "no_end_after"):
        for ids in ((100,), (-1,), (5, 1000), (1.5,), ("a",), (True,), 7, None):
            with pytest.raises(ValueError, match=name):
                m.beam_search(x, 5, 3, **{name: ids})
        with pytest.raises(ValueError, match="at most 64"):
            m.beam_search(x, 5, 3, **{name: tuple(range(3, 68))})
    with pytest.raises(ValueError, match="end_id"):
        m.beam_search(x, 5, 3, suppress_ids=(4, 2))
    with pytest.raises(ValueError, match="end_id"):
        m.beam_search(x, 5, 3, end_id=7, suppress_ids=(7,))
    for name in ("min_length", "no_repeat_ngram"):
        for v in (-1, 1.5, "2", None, True):
            with pytest.raises(ValueError, match=name):
                m.beam_search(x, 5, 3, **{name: v})
    with pytest.raises(ValueError, match="end_id >= 0"):
        m.beam_search(x, 5, 3, end_id=-1, min_length=2)
    with pytest.raises(ValueError, match="end_id >= 0"):
        m.beam_search(x, 5, 3, end_id=-1, no_end_after=(4,))
    # every hypothesis keeps beam_size allowed tokens: 100 - 64 - 1 - 30 = 5 < 6
    with pytest.raises(ValueError, match="fewer than beam_size"):
        m.beam_search(x, 30, 6, suppress_ids=tuple(range(3, 67)), no_repeat_ngram=2)
    with pytest.raises(ValueError, match="max_len <= 256"):
        Encoder2Decoder(Config()).beam_search(x, 257, 3, no_repeat_ngram=2)
    with pytest.raises(TypeError):  # keyword-only
        m.beam_search(x, 5, 6, 2, None, False, None, 1, 0.0, 0.0, False, (4,))
    # valid constraints (duplicates allowed, 64 ids, suppression without an end_id), CPU tensor: no CPU path
    for kw in ({"suppress_ids": (4, 4, 5), "min_length": 3, "no_repeat_ngram": 2, "no_end_after": [6, 6]},
               {"suppress_ids": tuple(range(3, 67))}, {"end_id": -1, "suppress_ids": (2,), "no_repeat_ngram": 1},
               {"suppress_ids": torch.tensor([4, 5])}):
        with pytest.raises(RuntimeError, match="GPU|CUDA"):
            m.beam_search(x, 5, 3, **kw)


def test_baseline_model_still_refuses_beam_search(monkeypatch):
    from adaptive_amd import _lib
    from adaptive_amd.baseline_attention import Config, Encoder2Decoder
    m = Encoder2Decoder(Config())
    monkeypatch.setattr(_lib, "load", _no_library)
    with pytest.raises(NotImplementedError, match="baseline.*beam_search"):
        m.beam_search(torch.zeros(2, 2048, 7, 7), 5, 6, suppress_ids=(3,), min_length=2, no_repeat_ngram=2)


# ---- C-ABI, no device work --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from adaptive_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "adaptive_amd", "csrc")], check=True)
    return _lib.load()


def test_abi_version_is_unchanged(lib):
    from adaptive_amd import _lib
    assert lib.aa_abi_version() == _lib.ABI_VERSION == 17
    assert (_lib.MAX_BEAM_SUPPRESS, _lib.MAX_BEAM_NGRAM_T) == (64, 256)
    # pointer, 3 x int32, (pad), pointer, int32, (pad)
    assert ctypes.sizeof(_lib.BeamConstraints) == 40 and _lib.BeamConstraints.no_end_after.offset == 24


def _cons(nsup=1, nmin=2, n=2, nnea=1, sup=256, nea=256):
    from adaptive_amd import _lib
    return ctypes.byref(_lib.BeamConstraints(sup, nsup, nmin, n, nea, nnea))


def test_decode_cx_argument_errors_without_device_work(lib):
    from adaptive_amd import _lib
    p, big = 256, 10 ** 9  # fake aligned pointer
    dims = _lib.Dims(256, 512, 10123, 2048, 49)

    def model(vocab=10123, nbytes=big):
        return _lib.Model(_lib.Dims(256, 512, vocab, 2048, 49), p, nbytes)

    def call(m, B=4, T=20, K=6, end_id=2, feats=p, ws=p, ws_bytes=big, flags=0, G=3, opts=True, cons=None):
        o = ctypes.byref(_lib.BeamOpts(G, 0.5, 0.7, None, None, None)) if opts else None
        return lib.aa_beam_decode_cx(m, feats, B, T, K, end_id, None, None, None, None, None, ws, ws_bytes, flags, None,
                                     None, o, cons if cons is not None else _cons())

    m = model()
    need = lib.aa_beam_workspace_bytes(dims, 4, 20, 6)
    assert need > 0
    # the plain call's and the options' checks, in their order, come first
    assert call(None) == -1 and call(model(nbytes=10)) == -4 and call(model(vocab=256 * 64 + 1)) == -2
    assert call(m, K=0) == -3 and call(m, B=-1) == -3 and call(m, end_id=10123) == -3 and call(m, G=4) == -3
    # the constraints: AA_ERR_SHAPE, for any vocabulary stage
    bad = (_cons(nsup=-1), _cons(nsup=65), _cons(nnea=-1), _cons(nnea=65), _cons(nmin=-1), _cons(n=-1))
    for c in bad:
        for flags in (0, _lib.BEAM_FAST, _lib.DECODE_EXACT_VOCAB):
            assert call(m, cons=c, flags=flags) == -3
        assert call(m, cons=c, opts=False) == -3
    assert call(m, end_id=-1, cons=_cons(nsup=0, nmin=1, n=0, nnea=0)) == -3
    assert call(m, end_id=-1, cons=_cons(nsup=0, nmin=0, n=0, nnea=1)) == -3
    assert call(m, end_id=-1, cons=_cons(nsup=3, nmin=0, n=2, nnea=0), ws_bytes=need - 1) == -4   # fine without <end>
    assert call(m, T=257, cons=_cons(n=1)) == -3 and call(m, T=257, cons=_cons(n=0), ws_bytes=0) == -4
    # every live row keeps K allowed candidates: V - n_suppress - 1 - (n ? T : 0) >= K
    small = model(vocab=100)
    assert call(small, T=30, cons=_cons(nsup=64, n=2)) == -3            # 100 - 64 - 1 - 30 = 5 < 6
    assert call(small, T=29, cons=_cons(nsup=64, n=2), ws_bytes=0) == -4  # 6 >= 6
    assert call(small, T=30, cons=_cons(nsup=64, n=0), ws_bytes=0) == -4
    # ... before the empty-batch return, the pointer checks after it
    for B, T in ((0, 20), (4, 0)):
        assert call(m, B=B, T=T, feats=None, ws=None, ws_bytes=0, cons=_cons(sup=None, nea=None)) == 0
        for c in bad:
            assert call(m, B=B, T=T, cons=c) == -3
    assert call(m, feats=None) == -1 and call(m, ws=None) == -1
    assert call(m, cons=_cons(sup=None)) == -1 and call(m, cons=_cons(nea=None)) == -1
    assert call(m, cons=_cons(nsup=0, sup=None, nnea=0, nea=None), ws_bytes=need - 1) == -4   # empty lists may be NULL
    assert call(m, ws=p + 4) == -5
    # valid constraints pass every check up to the workspace size: the workspace is aa_beam_workspace_bytes
    assert call(m, ws_bytes=need - 1) == -4 and call(m, opts=False, ws_bytes=need - 1) == -4
    assert call(m, cons=_cons(nsup=64, nnea=64, nmin=50, n=7), ws_bytes=need - 1) == -4
    # all four off, or cons == NULL: aa_beam_decode_ex / aa_beam_decode
    assert call(m, cons=_cons(0, 0, 0, 0, None, None), ws_bytes=need - 1) == -4
    assert lib.aa_beam_decode_cx(m, p, 4, 20, 6, 2, None, None, None, None, None, p, need - 1, 0, None, None, None,
                                 None) == -4


def test_select_step_argument_errors_without_device_work(lib):
    from adaptive_amd import _lib
    p, big = 256, 10 ** 9

    def call(B=4, K=3, V=3001, Vp=3072, t=5, end_id=2, logits=p, cum=p, fin=p, ht=p, hp=p, G=None, lam=0.5, cons=None,
             tok=p, par=p, cum_out=p, fin_out=p, ws=p, ws_bytes=big):
        o = ctypes.byref(_lib.BeamOpts(G, lam, 0.0, None, None, None)) if G is not None else None
        return lib.aa_beam_select_step(B, K, V, Vp, t, end_id, logits, cum, fin, ht, hp, o, cons, tok, par, cum_out,
                                       fin_out, ws, ws_bytes, None)

    size = lib.aa_beam_select_step_workspace_bytes
    need = size(4, 3, 3001, 3072, 5)
    assert need >= 12 * 96 * 8 + 2 * 6 * 12 * 4
    # shape
    for kw in ({"B": -1}, {"K": 0}, {"K": 9}, {"B": 1 << 23, "K": 3}, {"V": 0}, {"V": 16385, "Vp": 16416}, {"K": 3, "V": 2,
               "Vp": 32}, {"Vp": 3000}, {"Vp": 3073}, {"t": -1}, {"end_id": 3001}):
        assert call(**kw) == -3, kw
        a = {"B": 4, "K": 3, "V": 3001, "Vp": 3072, "t": 5, **{k: v for k, v in kw.items() if k != "end_id"}}
        if "end_id" not in kw:
            assert size(a["B"], a["K"], a["V"], a["Vp"], a["t"]) == 0, kw
    assert call(G=2) == -3 and call(K=6, G=4) == -3 and call(G=1, lam=-1.0) == -3 and call(G=1, lam=float("nan")) == -3
    for c in (_cons(nsup=65), _cons(nnea=-1), _cons(nmin=-1), _cons(n=-1)):
        assert call(cons=c) == -3
    assert call(end_id=-1, cons=_cons(nsup=0, nmin=1, n=0, nnea=0)) == -3
    assert call(t=257, cons=_cons(n=2)) == -3
    assert call(V=40, Vp=64, t=5, cons=_cons(nsup=32, n=1)) == -3     # 40 - 32 - 1 - 5 = 2 < 3
    assert call(V=40, Vp=64, t=5, cons=_cons(nsup=31, n=1), ws_bytes=0) == -4
    # ... before the empty-batch return, the pointer checks after it
    assert call(B=0, logits=None, ws=None, ws_bytes=0) == 0 and call(B=0, cons=_cons(n=-1)) == -3
    for name in ("logits", "cum", "fin", "ht", "hp", "tok", "par", "cum_out", "fin_out", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(t=0, ht=None, hp=None, ws_bytes=0) == -4                # no history at step 0
    assert call(cons=_cons(sup=None)) == -1 and call(cons=_cons(nea=None)) == -1
    assert call(logits=p + 4) == -5 and call(ws=p + 8) == -5
    assert call(ws_bytes=need - 1) == -4 and call(cons=_cons(), ws_bytes=need - 1) == -4
    assert call(K=6, G=3, cons=_cons(), ws_bytes=0) == -4
