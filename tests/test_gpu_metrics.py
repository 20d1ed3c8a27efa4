"""GPU: CaptionMetrics.score / corpus_score (aa_metrics_score / k_metrics, aa_bleu_corpus / k_bleu_corpus) and
MixedReward against the reference's recorded scores and the CPU oracle (tests/metrics_oracle.py).

The statistics are integers and must be equal.  Floats, where a test says RTOL / ATOL: both sides are float64
over the same integers and differ only by a few ulps of pow / exp / division in fewer than 20 operations per
value; rtol 1e-10 with atol 1e-12 is tests/test_gpu_cider.py's bound, taken for the same reason.  Each
comparison prints its worst error before it asserts.

Measured on an MI355X: profiles/metrics_errors.txt.
"""
import numpy as np
import pytest
import torch

from adaptive_amd.cider import CiderD
from adaptive_amd.metrics import CaptionMetrics, MixedReward
from cider_oracle import CiderOracle
from metrics_cases import BAD_EDGE_ROWS, END, edge_cases, golden_cases, padded
from metrics_oracle import MetricsOracle

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
NAMES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L")


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both = np.isfinite(got) & np.isfinite(want)
    err = np.abs(got - want)[both]
    rel = (err / np.maximum(np.abs(want[both]), 1e-300)).max() if err.size else 0.0
    print(f"metrics error: {what}: max abs {err.max() if err.size else 0.0:.3e}, max rel {rel:.3e} over {err.size} values")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True)


def check(scores, oracle, hyps, idx, what):
    """Every output of one score() call against the oracle's: statistics equal, floats close."""
    st = scores.stats.cpu().numpy()
    assert scores.stats.dtype == torch.int32 and scores.bleu.dtype == scores.rouge_l.dtype == torch.float64
    assert st.shape == (len(hyps), 10) and scores.bleu.shape == (len(hyps), 4) and scores.rouge_l.shape == (len(hyps),)
    np.testing.assert_array_equal(st, oracle.stats(hyps, idx))
    close(scores.bleu.cpu().numpy(), oracle.bleu(hyps, idx), what + " bleu")
    close(scores.rouge_l.cpu().numpy(), oracle.rouge(hyps, idx), what + " rouge_l")


def check_table(table, want, what):
    assert all(t.dtype == torch.float64 and t.dim() == 0 and t.device.type == "cuda" for t in table.values())
    close([table[k].item() for k in NAMES], [want[k] for k in NAMES], what + " corpus table")


@pytest.fixture(scope="module")
def golden():
    refs, hyps, end, z = golden_cases()
    return refs, hyps, end, z, MetricsOracle(refs, end_id=end)


@pytest.fixture(scope="module")
def edge():
    refs, rows = edge_cases()
    return refs, [r[0] for r in rows], [r[1] for r in rows], MetricsOracle(refs)


def test_golden(gpu_device, golden):
    refs, hyps, end, z, o = golden
    m = CaptionMetrics(refs, end_id=end).to(gpu_device)
    ids = torch.from_numpy(hyps).to(gpu_device)
    s = m.score(ids)
    check(s, o, hyps, None, "golden (oracle)")
    close(s.bleu.cpu().numpy(), z["bleu"], "golden (reference) bleu")
    close(s.rouge_l.cpu().numpy(), z["rouge"], "golden (reference) rouge_l")
    st = s.stats.cpu().numpy()
    assert st[:, 8].sum() == int(z["testlen"]) and st[:, 9].sum() == int(z["reflen"])
    table = m.corpus_score(ids)
    assert set(table) == set(NAMES)
    check_table(table, dict(zip(NAMES, list(z["corpus_bleu"]) + [float(z["rouge_mean"])])), "golden (reference)")
    check_table(table, o.corpus(hyps), "golden (oracle)")
    c = CiderD(refs, end_id=end).to(gpu_device)
    full = m.corpus_score(ids, cider=c)
    assert set(full) == set(NAMES) | {"CIDEr"} and all(torch.equal(full[k], table[k]) for k in NAMES)
    close(full["CIDEr"].item(), CiderOracle(refs, end_id=end).score(hyps).mean(), "golden CIDEr")


def test_edge_batch_against_the_oracle(gpu_device, edge):
    refs, hyps, idx, o = edge
    m = CaptionMetrics(refs).to(gpu_device)
    ids = torch.from_numpy(padded(hyps, 64)).to(gpu_device)
    s = m.score(ids, idx)
    check(s, o, hyps, idx, "edge T=64")
    nan_rows = torch.tensor(BAD_EDGE_ROWS)
    good = np.setdiff1d(np.arange(len(hyps)), BAD_EDGE_ROWS)
    assert s.bleu.cpu()[nan_rows].isnan().all() and s.rouge_l.cpu()[nan_rows].isnan().all()
    assert (s.stats.cpu()[nan_rows] == 0).all()                           # NaN floats, zero statistics
    assert s.bleu.cpu()[good].isfinite().all() and s.rouge_l.cpu()[good].isfinite().all()  # ... that row only
    assert (s.bleu[0] == 0).all() and (s.bleu[5] == 0).all() and s.rouge_l[0] == 0 and s.rouge_l[5] == 0  # empty
    assert s.rouge_l[18] == 1.0 and s.rouge_l[16] == 1.0 and s.rouge_l[19] == 0.0   # the empty-reference quirk
    assert s.stats[6, 0] == 5 and s.stats[13, :4].tolist() == [64, 63, 62, 61]      # clipping; 64 tokens, all found
    check_table(m.corpus_score(ids, idx), o.corpus(hyps, idx), "edge T=64")        # NaN rows left out on both sides
    # the same rows at T = 20, full-length rows without an end_id
    short = [(h, i) for h, i in zip(hyps, idx) if len(h) <= 20]
    t20 = padded([h for h, _ in short] + [refs[2][0][:20], refs[4][0][5:25]], 20)
    i20 = [i for _, i in short] + [2, 4]
    check(m.score(torch.from_numpy(t20).to(gpu_device), i20), o, list(t20), i20, "edge T=20")
    check_table(m.corpus_score(torch.from_numpy(t20).to(gpu_device), i20), o.corpus(list(t20), i20), "edge T=20")
    # a row pitch wider than T (a view of a wider tensor)
    wide = torch.from_numpy(padded(hyps, 64, fill=7)).to(gpu_device)[:, :5]
    assert wide.stride(0) == 64
    check(m.score(wide, idx), o, [h[:5] for h in padded(hyps, 64, fill=7)], idx, "edge pitch 64, T=5")
    # T = 0: every caption is empty
    none = m.score(torch.empty(3, 0, dtype=torch.int64, device=gpu_device), [0, 5, 6])
    check(none, o, [[], [], []], [0, 5, 6], "edge T=0")


def test_rows_are_independent_and_reproducible(gpu_device, golden):
    refs, hyps, end, _, o = golden
    m = CaptionMetrics(refs, end_id=end).to(gpu_device)
    order = [9, 9, 9, 4, 4, 4, 12, 12, 12, 0, 0, 0, 7, 7, 7, 11, 11, 11]  # N = 3 rows per image, not monotone
    rows = np.stack([hyps[(i + k) % len(hyps)] for k, i in enumerate(order)])
    ids = torch.from_numpy(rows).to(gpu_device)
    idx = torch.tensor(order, device=gpu_device)
    a, b = m.score(ids, idx), m.score(ids, idx)
    for x, y in zip(a, b):
        assert torch.equal(x, y)  # two runs: the same bits
    for r in range(len(order)):
        one = m.score(ids[r:r + 1], idx[r:r + 1])
        for x, y in zip(one, a):
            assert torch.equal(x, y[r:r + 1])
    ta, tb = m.corpus_score(ids, idx), m.corpus_score(ids, idx)
    assert all(torch.equal(ta[k], tb[k]) for k in NAMES)
    check(a, o, list(rows), order, "golden rows x 3")
    check_table(ta, o.corpus(list(rows), order), "golden rows x 3")


@pytest.mark.parametrize("R", [1, 1000])
def test_grid_sizes(gpu_device, golden, R):
    refs, hyps, end, _, o = golden
    m = CaptionMetrics(refs, end_id=end).to(gpu_device)
    rng = np.random.default_rng(R)
    idx = rng.integers(0, len(refs), size=R)
    pick = rng.integers(0, len(hyps), size=R)
    pairs = sorted(set(zip(pick.tolist(), idx.tolist())))   # the oracle once per distinct (caption, image)
    at = {p: k for k, p in enumerate(pairs)}
    sel = np.array([at[p] for p in zip(pick.tolist(), idx.tolist())])
    ph, pi = [hyps[p] for p, _ in pairs], [i for _, i in pairs]
    s = m.score(torch.from_numpy(hyps[pick]).to(gpu_device), torch.from_numpy(idx).to(gpu_device))
    want_stats = o.stats(ph, pi)[sel]
    np.testing.assert_array_equal(s.stats.cpu().numpy(), want_stats)
    close(s.bleu.cpu().numpy(), o.bleu(ph, pi)[sel], f"R={R} bleu")
    close(s.rouge_l.cpu().numpy(), o.rouge(ph, pi)[sel], f"R={R} rouge_l")
    # the corpus figures: the totals are exact int64, so the table is the oracle's expression on them
    from metrics_oracle import bleu_of
    tot = want_stats.sum(0)
    want = dict(zip(NAMES, bleu_of(tot[:4].tolist(), tot[4:8].tolist(), int(tot[8]), int(tot[9]))
                    + [o.rouge(ph, pi)[sel].mean()]))
    check_table(m.corpus_score(torch.from_numpy(hyps[pick]).to(gpu_device), torch.from_numpy(idx).to(gpu_device)),
                want, f"R={R}")


def test_no_rows(gpu_device, golden):
    refs, _, end, _, _ = golden
    m = CaptionMetrics(refs, end_id=end).to(gpu_device)
    s = m.score(torch.empty(0, 20, dtype=torch.int64, device=gpu_device))
    assert s.bleu.shape == (0, 4) and s.rouge_l.shape == (0,) and s.stats.shape == (0, 10)
    with pytest.raises(ValueError, match="exceeds"):
        m.score(torch.zeros(2, 65, dtype=torch.int64, device=gpu_device))
    with pytest.raises(ValueError, match="image_index"):
        m.score(torch.zeros(len(refs) + 1, 4, dtype=torch.int64, device=gpu_device))
    with pytest.raises(ValueError, match="int64"):
        m.score(torch.zeros(2, 4, dtype=torch.int32, device=gpu_device))


def test_end_to_end_from_the_decode(gpu_device):
    from adaptive_amd import Config, Encoder2Decoder, synth
    B, T = 8, 20
    model = Encoder2Decoder(Config()).to(gpu_device).load_synthetic(123)
    ids, _, _ = model.sampler(torch.from_numpy(synth.make_features(B, seed=0)).to(gpu_device), max_len=T)
    host = ids.cpu().numpy()
    refs = []
    for row in host:  # each image's references from its own caption: itself, one token changed, its first half
        other = row.copy()
        other[1] = 7 if other[1] != 7 else 8
        refs.append([row.tolist(), other.tolist(), row[:T // 2].tolist()])
    m = CaptionMetrics(refs).to(gpu_device)
    s = m.score(ids)  # straight from the decode's device tensor
    check(s, MetricsOracle(refs), list(host), None, "decode")
    has_tokens = torch.from_numpy(host[:, 0] != END)
    assert has_tokens.any()
    assert (s.rouge_l.cpu()[has_tokens] == 1.0).all() and (s.bleu.cpu()[has_tokens][:, 0] > 1 - 1e-8).all()


def _tiny(dev):
    from adaptive_amd import Config, Encoder2Decoder
    cf = Config(adaptive_word_embed_size=32, adaptive_lstm_hidden_size=256, vocab_length=100)
    return Encoder2Decoder(cf).to(dev).load_synthetic()


def test_self_critical_step_with_a_mixed_reward(gpu_device):
    from adaptive_amd import synth
    dev = gpu_device
    B, N, T = 3, 2, 6
    rng = np.random.default_rng(2)
    refs = [[rng.integers(3, 100, size=int(rng.integers(5, 8))).tolist() for _ in range(5)] for _ in range(B)]
    model = _tiny(dev)
    cider = CiderD(refs, end_id=END).to(dev)
    metrics = CaptionMetrics(refs, end_id=END).to(dev)
    feats = torch.from_numpy(synth.make_features(B, seed=1)).to(dev)
    kw = dict(num_samples=N, max_len=T, temperature=1.0, seed=4)
    loss, info = model.self_critical_loss(feats, MixedReward(cider, metrics, cider_weight=1.0, bleu4_weight=0.5), **kw)
    idx = torch.arange(B, device=dev, dtype=torch.int32)
    rows = idx.repeat_interleave(N)
    want_sample = 1.0 * cider.score(info.sample_ids, rows) + 0.5 * metrics.score(info.sample_ids, rows).bleu[:, 3]
    want_greedy = 1.0 * cider.score(info.greedy_ids, idx) + 0.5 * metrics.score(info.greedy_ids, idx).bleu[:, 3]
    assert torch.equal(info.reward_sample, want_sample) and torch.equal(info.reward_greedy, want_greedy)
    assert torch.equal(info.advantage, want_sample - want_greedy.repeat_interleave(N))
    assert info.reward_sample.dtype == torch.float64 and info.reward_sample.isfinite().all()
    # the BLEU term is the oracle's
    o = MetricsOracle(refs, end_id=END)
    close(metrics.score(info.sample_ids, rows).bleu.cpu().numpy(),
          o.bleu(list(info.sample_ids.cpu().numpy()), rows.tolist()), "self-critical samples bleu")
    loss.backward()
    assert torch.isfinite(loss).item()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert any(p.grad.any() for p in model.parameters())
    # weight 0: the CiderD-only step, bit for bit
    plain, pinfo = model.self_critical_loss(feats, cider, **kw)
    only, oinfo = model.self_critical_loss(feats, MixedReward(cider, metrics, cider_weight=1.0, bleu4_weight=0.0), **kw)
    assert torch.equal(only.detach(), plain.detach())
    for a, b in zip(oinfo, pinfo):
        assert torch.equal(a, b)
    # the images named explicitly
    _, swapped = model.self_critical_loss(feats, MixedReward(cider, metrics, 1.0, 0.5, 0.25), [2, 0, 1], **kw)
    sw = torch.tensor([2, 0, 1], device=dev, dtype=torch.int32)
    ms = metrics.score(swapped.greedy_ids, sw)
    assert torch.equal(swapped.reward_greedy,
                       1.0 * cider.score(swapped.greedy_ids, sw) + 0.5 * ms.bleu[:, 3] + 0.25 * ms.rouge_l)
