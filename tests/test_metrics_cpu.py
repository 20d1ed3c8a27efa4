"""CPU: the BLEU / ROUGE-L oracle against the reference's recorded scores, its two LCS forms against each
other, the host corpus builder against the oracle, the constructors' errors, and the argument codes of
aa_metrics_score / aa_bleu_corpus (no device work).

Bounds: integers are exact; the oracle's floats are within 1e-12 of the golden, both sides being libm float64
on the same expression."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from cider_oracle import ngram_counts
from metrics_cases import BAD_EDGE_ROWS, edge_cases, golden_cases
from metrics_oracle import MetricsOracle, bleu_of, lcs_bits, lcs_dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return golden_cases()


def test_golden_covers_what_it_should(golden):
    refs, hyps, end, z = golden
    o = MetricsOracle(refs, end_id=end)
    st = o.stats(hyps)
    L, reflen = st[:, 8], st[:, 9]
    assert len(refs) >= 16 and set(len(r) for r in refs) == {1, 2, 3, 4, 5, 6, 7}
    assert {0, 1, 2, 3, 20} <= set(L.tolist())
    assert (st[L == 1][:, 5:8] == 0).all() and (st[L == 3][:, 7] == 0).all()   # guess_n = 0 above the length
    six = [i for i, row in enumerate(hyps) if L[i] == 6 and len(set(row[:6].tolist())) == 1]
    assert six and st[six[0], 0] == 3                                           # six of a token, clipped at 3
    assert any(L[i] > max(o.lengths[i]) for i in range(len(refs)))              # no brevity penalty
    assert any(0 < L[i] < min(o.lengths[i]) for i in range(len(refs)))          # brevity penalty
    assert any(len(o.lengths[i]) == 1 and o.tokens[i][0] == hyps[i][:L[i]].tolist() and L[i] > 4
               for i in range(len(refs)))                                       # its only reference
    tie = [i for i in range(len(refs)) if {L[i] - 2, L[i] + 2} <= set(o.lengths[i])
           and min(abs(l - L[i]) for l in o.lengths[i]) == 2]
    assert tie and all(reflen[i] == L[i] - 2 for i in tie)                      # a tie goes to the shorter
    assert any(hyps[i][:L[i]].tolist() in [r[::-1] for r in o.tokens[i] if len(r) > 4] for i in range(len(refs)))
    assert any(0 in o.lengths[i] and len(o.lengths[i]) > 1 for i in range(len(refs)))
    quirk = [i for i in range(len(refs)) if o.lengths[i] == [0] and L[i] == 0]
    assert quirk and all(z["rouge"][i] == 1.0 for i in quirk)
    assert any(o.lengths[i] == [0] and L[i] > 0 and z["rouge"][i] == 0.0 for i in range(len(refs)))


def test_oracle_matches_the_reference_scorers(golden):
    refs, hyps, end, z = golden
    o = MetricsOracle(refs, end_id=end)
    st = o.stats(hyps)
    assert st[:, 8].sum() == int(z["testlen"]) and st[:, 9].sum() == int(z["reflen"])
    np.testing.assert_allclose(o.bleu(hyps), z["bleu"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(o.rouge(hyps), z["rouge"], rtol=0, atol=1e-12)
    table = o.corpus(hyps)
    np.testing.assert_allclose([table[f"Bleu_{n}"] for n in (1, 2, 3, 4)], z["corpus_bleu"], rtol=0, atol=1e-12)
    assert abs(table["ROUGE_L"] - float(z["rouge_mean"])) <= 1e-12


def test_bit_parallel_lcs_equals_the_dp():
    rng = np.random.default_rng(5)
    pairs = []
    for _ in range(300):
        vocab = int(rng.choice([1, 2, 4, 12, 1000]))
        pairs.append((rng.integers(0, vocab, size=int(rng.integers(0, 65))).tolist(),
                      rng.integers(0, vocab, size=int(rng.integers(1, 101))).tolist()))
    for lr in (1, 63, 64, 65, 100):                    # L = 64 against every kind of length
        pairs.append((rng.integers(0, 3, size=64).tolist(), rng.integers(0, 3, size=lr).tolist()))
    pairs += [([7] * 64, [7] * 100), ([7] * 64, [7] * 10), ([7] * 5, [7] * 100),   # all-equal tokens
              ([1, 2, 3] * 21, [4, 5, 6] * 30), ([1] * 64, [2] * 64),               # no common token
              ([], [1, 2, 3]), ([1, 2, 3], []), ([], [])]
    assert len(pairs) >= 300
    for hyp, ref in pairs:
        assert lcs_bits(hyp, ref) == lcs_dp(ref, hyp) == lcs_dp(hyp, ref), (hyp, ref)
    assert lcs_bits([1, 2, 3, 4], [4, 3, 2, 1]) == 1 and lcs_bits([1, 2, 3, 4], [1, 9, 3, 4, 4]) == 3


def test_bleu_expression_by_hand():
    # 5 tokens, 4 / 2 / 1 / 0 matches against a closest reference of 7 tokens
    got = bleu_of([4, 2, 1, 0], [5, 4, 3, 2], 5, 7)
    bp = np.exp(1 - 7 / 5)
    want = [0.8, (0.8 * 0.5) ** 0.5, (0.8 * 0.5 / 3) ** (1 / 3), 0.0]
    np.testing.assert_allclose(got[:3], np.array(want[:3]) * bp, rtol=1e-8)
    assert 0 < got[3] < 1e-4                             # tiny / small keep it positive
    assert bleu_of([0] * 4, [0] * 4, 0, 6) == [0.0] * 4  # an empty caption: exp(-huge) = 0


@pytest.mark.parametrize("which", ["golden", "edge"])
def test_corpus_builder_matches_the_oracle(golden, which):
    from adaptive_amd.cider import pack_key
    from adaptive_amd.metrics import CaptionMetrics
    refs, end = (golden[0], golden[2]) if which == "golden" else (edge_cases()[0], 2)
    c = CaptionMetrics(refs, end_id=end)
    o = MetricsOracle(refs, end_id=end)
    flat_len = [l for img in o.lengths for l in img]
    flat_tok = [t for img in o.tokens for r in img for t in r]
    assert c.images == len(refs) and c.refs == len(flat_len)
    np.testing.assert_array_equal(c.img_ptr, np.concatenate([[0], np.cumsum([len(r) for r in refs])]))
    np.testing.assert_array_equal(c.ref_len, flat_len)
    np.testing.assert_array_equal(c.tok_ptr, np.concatenate([[0], np.cumsum(flat_len)]))
    np.testing.assert_array_equal(c.ref_tok, flat_tok)
    assert c.ref_tok.dtype == np.uint16 and c.clip_counts.dtype == np.int32 and c.clip_keys.dtype == np.uint64
    assert c.clip_ptr[0] == 0 and c.clip_ptr[-1] == c.clip_keys.size == c.clip_counts.size
    for i, most in enumerate(o.clip):
        lo, hi = c.clip_ptr[i], c.clip_ptr[i + 1]
        keys = c.clip_keys[lo:hi]
        assert (np.diff(keys.astype(object)) > 0).all()  # ascending, no duplicate
        assert dict(zip(keys.tolist(), c.clip_counts[lo:hi].tolist())) == {pack_key(g): n for g, n in most.items()}
    if which == "edge":
        assert max(flat_len) == 100 and 0 in flat_len and o.clip[6] == {} and o.clip[1][(3,)] == 5


def test_every_reference_empty():
    from adaptive_amd.metrics import CaptionMetrics
    c = CaptionMetrics([[[]], [[2, 5], []]])
    assert c.clip_keys.size == 0 and c.ref_tok.size == 0
    np.testing.assert_array_equal(c.clip_ptr, [0, 0, 0])
    np.testing.assert_array_equal(c.ref_len, [0, 0, 0])


def test_ciderd_is_unchanged_by_the_kept_token_stream(golden):
    from adaptive_amd.cider import CiderD, _Flat
    refs, _, end, _ = golden
    flat = _Flat(refs, end, "refs")
    assert flat.tok.size == flat.length.sum()
    o = MetricsOracle(refs, end_id=end)
    np.testing.assert_array_equal(flat.tok, [t for img in o.tokens for r in img for t in r])
    c = CiderD(refs, end_id=end)
    assert c.counts.sum() == sum(sum(ngram_counts(r).values()) for img in o.tokens for r in img)


def test_value_errors():
    from adaptive_amd.metrics import CaptionMetrics
    with pytest.raises(ValueError, match="no images"):
        CaptionMetrics([])
    with pytest.raises(ValueError, match="no reference"):
        CaptionMetrics([[[3, 4]], []])
    with pytest.raises(ValueError, match="outside"):
        CaptionMetrics([[[3, 65535]]])
    with pytest.raises(ValueError, match="outside"):
        CaptionMetrics([[[3, -1, 4]]])
    c = CaptionMetrics([[[3, 65534, 2, 70000]]])  # 65534 is the largest token; what follows end_id is cut
    assert c.ref_len[0] == 2 and c.ref_tok.tolist() == [3, 65534] and c.clip_counts.sum() == 3
    with pytest.raises(RuntimeError, match="to\\(device\\)"):
        c.score(None)


def test_mixed_reward_checks():
    from adaptive_amd.metrics import MixedReward

    def scorer(end_id=2, images=4, device="cuda:0"):
        return types.SimpleNamespace(end_id=end_id, images=images, device=device, _index=lambda i, R: ("index", i, R))

    m = MixedReward(scorer(), scorer(), bleu4_weight=0.5)
    assert (m.cider_weight, m.bleu4_weight, m.rouge_weight) == (1.0, 0.5, 0.0)
    assert m.device == "cuda:0" and m.end_id == 2 and m._index([1], 1) == ("index", [1], 1)
    with pytest.raises(ValueError, match="end_id"):
        MixedReward(scorer(end_id=2), scorer(end_id=0))
    with pytest.raises(ValueError, match="images"):
        MixedReward(scorer(images=4), scorer(images=5))
    with pytest.raises(ValueError, match="one device"):
        MixedReward(scorer(), scorer(device="cuda:1"))
    with pytest.raises(ValueError, match="one device"):
        MixedReward(scorer(device=None), scorer(device=None))
    with pytest.raises(ValueError, match="finite"):
        MixedReward(scorer(), scorer(), bleu4_weight=float("nan"))
    with pytest.raises(ValueError, match="every weight"):
        MixedReward(scorer(), scorer(), cider_weight=0.0)


def test_mixed_reward_sums_only_the_weighted_terms():
    import torch

    from adaptive_amd.metrics import MetricScores, MixedReward
    calls = []
    c = torch.tensor([1.0, 2.0, float("nan")], dtype=torch.float64)
    b = torch.tensor([[0, 0, 0, 0.25], [0, 0, 0, 0.5], [0, 0, 0, 1.0]], dtype=torch.float64)
    r = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    cider = types.SimpleNamespace(end_id=2, images=3, device="cpu", _index=None,
                                  score=lambda ids, idx=None: calls.append("cider") or c)
    metrics = types.SimpleNamespace(end_id=2, images=3, device="cpu",
                                    score=lambda ids, idx=None: calls.append("metrics") or MetricScores(b, r, None))
    assert MixedReward(cider, metrics).score(None) is not None and calls == ["cider"]  # weight 0: not computed
    assert torch.equal(MixedReward(cider, metrics).score(None)[:2], c[:2])
    got = MixedReward(cider, metrics, 1.0, 0.5, 2.0).score(None)
    assert torch.equal(got[:2], (1.0 * c + 0.5 * b[:, 3] + 2.0 * r)[:2]) and got[2].isnan()
    calls.clear()
    assert torch.equal(MixedReward(cider, metrics, 0.0, 0.0, 3.0).score(None), 3.0 * r) and calls == ["metrics"]


def test_package_exports_caption_metrics():
    import adaptive_amd
    from adaptive_amd.metrics import CaptionMetrics
    assert adaptive_amd.CaptionMetrics is CaptionMetrics and "CaptionMetrics" in adaptive_amd.__all__


def test_edge_batch_has_its_bad_rows():
    refs, rows = edge_cases()
    o = MetricsOracle(refs)
    bad = [i for i, (h, img) in enumerate(rows) if o.hypothesis(h, img) is None]
    assert bad == BAD_EDGE_ROWS
    # empty against an empty reference is 1, alone or among others; empty against tokens is 0 either way round
    assert o.rouge_one(*rows[18]) == 1.0 and o.rouge_one(*rows[16]) == 1.0
    assert o.rouge_one(*rows[19]) == 0.0 and o.rouge_one(*rows[0]) == 0.0


@pytest.fixture(scope="module")
def lib():
    from adaptive_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "adaptive_amd", "csrc")], check=True)
    return _lib.load()


def test_argument_codes_without_device_work(lib):
    from adaptive_amd import _lib
    P = 256  # a fake non-NULL pointer: every call below returns before any device work
    names = ("img_ptr", "clip_ptr", "clip_keys", "clip_counts", "ref_len", "tok_ptr", "ref_tok")

    def corpus(**kw):
        f = dict({k: P for k in names}, images=3, refs=5)
        f.update(kw)
        return ctypes.byref(_lib.MetricsCorpus(**f))

    def call(c, ids=P, R=4, T=20, ld=20, image=None, stats=P, bleu=P, rouge=P):
        return lib.aa_metrics_score(c, ids, R, T, ld, 2, image, stats, bleu, rouge, None)

    assert call(corpus(), R=-1) == -3
    assert call(corpus(), T=-1) == -3
    assert call(corpus(), T=65, ld=65) == -3
    assert call(corpus(), T=20, ld=19) == -3
    assert call(None, ids=None, R=0, stats=None, bleu=None, rouge=None) == 0  # an empty batch: no pointer is looked at
    assert call(None) == -1
    assert call(corpus(images=0)) == -3
    assert call(corpus(refs=0)) == -3
    for name in names:
        assert call(corpus(**{name: None})) == -1
    assert call(corpus(), ids=None) == -1
    for out in ("stats", "bleu", "rouge"):
        assert call(corpus(), **{out: None}) == -1
    assert lib.aa_bleu_corpus(P, -1, P, None) == -3
    assert lib.aa_bleu_corpus(None, 0, None, None) == 0
    assert lib.aa_bleu_corpus(None, 4, P, None) == -1
    assert lib.aa_bleu_corpus(P, 4, None, None) == -1
