"""GPU: CiderD.score (aa_cider_score / k_cider) against the reference's recorded scores and the CPU oracle.

Tolerance where a test says RTOL / ATOL: both sides are float64 over the same host-computed weights and
differ only in the order of their sums (at most 64 non-negative terms each: about 64 * 2^-53 = 7e-15
relative) and a few ulps in sqrt / exp; rtol 1e-10 with atol 1e-12 is four orders above that bound.
"""
import numpy as np
import pytest
import torch

from adaptive_amd.cider import CiderD, splitmix64
from cider_cases import golden_cases, other_corpus
from cider_oracle import CiderOracle

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
END = 2


def padded(hyps, T, fill=END):
    out = np.full((len(hyps), T), fill, dtype=np.int64)
    for i, h in enumerate(hyps):
        out[i, :len(h)] = h
    return out


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True)


def test_golden(gpu_device):
    refs, hyps, end, scores, mean = golden_cases()
    c = CiderD(refs, end_id=end).to(gpu_device)
    m, per = c.corpus_score(torch.from_numpy(hyps).to(gpu_device))
    assert per.dtype == torch.float64 and per.shape == (len(refs),)
    close(per.cpu().numpy(), scores)
    close(m.item(), mean)
    close(c.score(torch.from_numpy(hyps).to(gpu_device)).cpu().numpy(), scores)


@pytest.fixture(scope="module")
def edge():
    """References of 6 images, a 40-image df corpus over tokens 3..11 in which token 3 is in every image
    (w = 0), and the rows to score as (caption, image)."""
    rng = np.random.default_rng(11)
    df_refs = [[[3] + rng.integers(5, 12, size=int(rng.integers(2, 9))).tolist() for _ in range(2)] for _ in range(40)]
    df_refs[0][0] += [65534, 65534, 5]
    long_ref = rng.integers(5, 12, size=80).tolist()  # longer than T: 79 bigrams
    refs = [
        [[5, 6, 7, 8, 9], [5, 6, 9, 9, 10, 11]],
        [[3, 3, 3, 3, 3], [3, 3, 5]],                       # order 1 has only w = 0 n-grams
        [long_ref, long_ref[:30]],
        [[65534, 65534, 5, 6], [7, 65534]],
        [[5, 6, 7, 8, 9, 10, 11] * 9 + [5]],                # 64 tokens
        [[30, 31, 32, 33, 34], [5, 30, 31, 6]],             # n-grams the df corpus never saw
    ]
    full64 = ([5, 6, 7, 8, 9, 10, 11] * 9 + [5])[:64]
    rows = [
        ([], 0), ([5], 0), ([5, 6], 0), ([5, 6, 9], 0),     # L = 0, 1, 2, 3
        ([END, 5, 6, 7], 0),                                # end_id at position 0
        ([3, 3, 3], 1), ([3, 3, 5, 3], 1),                  # norm_h,1 == 0: the undivided branch
        (long_ref[:64], 2), (long_ref[10:40], 2),           # a reference longer than T
        ([65534, 65534, 5], 3), ([7, 65534, 65534], 3),     # the largest token
        (full64, 4), (full64[:63], 4),                      # T = 64 without and with an end_id
        ([30, 31, 32, 33], 5), ([5, 30, 31, 40, 41], 5),    # unseen by the df corpus (and by everything)
        ([5, 6, END, 70000, -5], 0),                        # out of range after the end: ignored
        ([5, 70000, 6, END], 0), ([-1], 3), ([65535, 5], 3),  # out of range before it: NaN, that row only
        ([5, 6, 7, 8, 9], 0),
    ]
    return refs, df_refs, rows


def test_edge_batch_against_the_oracle(gpu_device, edge):
    refs, df_refs, rows = edge
    c = CiderD(refs, df_refs=df_refs).to(gpu_device)
    o = CiderOracle(refs, df_refs=df_refs)
    assert o.weight((3,)) == 0.0 and o.weight((30, 31)) == o.log_m
    hyps, idx = [r[0] for r in rows], [r[1] for r in rows]
    want = o.score(hyps, idx)
    assert np.isnan(want).sum() == 3 and (want[np.isfinite(want)] > 0).sum() >= 12
    got = c.score(torch.from_numpy(padded(hyps, 64)).to(gpu_device), idx).cpu().numpy()
    close(got, want)
    assert got[0] == 0.0 and got[4] == 0.0  # empty captions score exactly 0
    # the same rows at T = 20, full-length rows without an end_id
    short = [(h, i) for h, i in rows if len(h) <= 20]
    t20 = padded([h for h, _ in short] + [refs[2][0][:20]], 20)
    got20 = c.score(torch.from_numpy(t20).to(gpu_device), [i for _, i in short] + [2]).cpu().numpy()
    close(got20, o.score(list(t20), [i for _, i in short] + [2]))
    # a row pitch wider than T (a view of a wider tensor)
    wide = torch.from_numpy(padded(hyps, 64, fill=7)).to(gpu_device)[:, :5]
    close(c.score(wide, idx).cpu().numpy(), o.score([h[:5] for h in padded(hyps, 64, fill=7)], idx))


def test_identity_and_self_critical(gpu_device):
    cap = [5, 9, 7, 11, 6]
    df_refs = [[[5, 9, 7, 11, 6]], [[8, 8]], [[10, 12]]]  # every n-gram of cap in one image of three: w = log 3
    c = CiderD([[cap]], df_refs=df_refs).to(gpu_device)
    ids = torch.from_numpy(padded([cap], 8)).to(gpu_device)
    assert abs(c.score(ids).item() - 10.0) <= 1e-12
    refs = [[[5, 9, 7, 11, 6], [5, 9, 8, 8]], [[10, 12, 8, 8, 5], [6, 10, 12]]]
    c = CiderD(refs, df_refs=df_refs).to(gpu_device)
    o = CiderOracle(refs, df_refs=df_refs)
    greedy = padded([[5, 9, 7, 6], [10, 12, 8]], 8)
    g = torch.from_numpy(greedy).to(gpu_device)
    adv = c.self_critical(g, g, 1)
    assert adv.shape == (2,) and (adv == 0).all()
    rep = c.self_critical(g.repeat_interleave(3, 0), g, 3)
    assert rep.shape == (6,) and (rep == 0).all()
    sample = padded([[5, 9, 7, 11, 6], [9, 8, 8], [8, 5], [10, 12, 8, 8, 5], [6, 10], []], 8)  # N = 3, image-major
    adv = c.self_critical(torch.from_numpy(sample).to(gpu_device), g, 3).cpu().numpy()
    want = o.score(list(sample), [0, 0, 0, 1, 1, 1]) - np.repeat(o.score(list(greedy)), 3)
    assert (np.abs(want) > 1e-3).all()  # (no advantage of the pair is trivially 0)
    close(adv, want)
    # the images named explicitly, swapped
    adv = c.self_critical(torch.from_numpy(sample).to(gpu_device), g, 3, image_index=[1, 0]).cpu().numpy()
    close(adv, o.score(list(sample), [1, 1, 1, 0, 0, 0]) - np.repeat(o.score(list(greedy), [1, 0]), 3))


def test_rows_are_independent_and_reproducible(gpu_device):
    refs, hyps, end, _, _ = golden_cases()
    c = CiderD(refs, end_id=end, df_refs=other_corpus()).to(gpu_device)
    order = [9, 9, 9, 4, 4, 4, 12, 12, 12, 0, 0, 0, 7, 7, 7]  # N = 3 rows per image, not monotone
    rows = np.stack([hyps[(i + k) % len(hyps)] for k, i in enumerate(order)])
    ids = torch.from_numpy(rows).to(gpu_device)
    idx = torch.tensor(order, device=gpu_device)
    a = c.score(ids, idx)
    b = c.score(ids, idx)
    assert torch.equal(a, b)  # two runs: the same bits
    assert a.isfinite().all() and (a > 0).sum() >= 10
    for r in range(len(order)):
        assert torch.equal(c.score(ids[r:r + 1], idx[r:r + 1]), a[r:r + 1])
    close(a.cpu().numpy(), CiderOracle(refs, end_id=end, df_refs=other_corpus()).score(list(rows), order))


def test_collisions_and_wrap_around(gpu_device):
    """Single-token references whose unigram keys all have the table's last slot as their home: the table is
    the smallest the load factor allows (8 slots for 4 keys), three keys wrap to slots 0..2, and an unseen
    token with the same home walks the whole chain before it misses."""
    size = 8
    toks = np.arange(3, 65535)
    home = splitmix64((toks + 1).astype(np.uint64)) & np.uint64(size - 1)
    t = toks[home == size - 1][:5].tolist()
    refs = [[[t[0]], [t[1]]], [[t[1]], [t[2]]], [[t[2]]], [[t[3]], [t[0]], [t[3]]]]
    c = CiderD(refs).to(gpu_device)
    assert c.tab_keys.size == size and c.tab_keys[size - 1] != 0 and np.count_nonzero(c.tab_keys[:3]) == 3
    o = CiderOracle(refs)
    hyps = [[t[0]], [t[1], t[1]], [t[2], t[4]], [t[3], t[0], t[4], t[3]], [t[4]], [t[2]]]
    idx = [0, 1, 2, 3, 0, 1]
    want = o.score(hyps, idx)
    assert (want[[0, 1, 2, 3, 5]] > 0).all() and want[4] == 0
    close(c.score(torch.from_numpy(padded(hyps, 6)).to(gpu_device), idx).cpu().numpy(), want)


@pytest.mark.parametrize("R", [1, 1000])
def test_grid_sizes(gpu_device, R):
    refs, hyps, end, _, _ = golden_cases()
    c = CiderD(refs, end_id=end).to(gpu_device)
    o = CiderOracle(refs, end_id=end)
    rng = np.random.default_rng(R)
    idx = rng.integers(0, len(refs), size=R)
    rows = hyps[rng.integers(0, len(hyps), size=R)]
    table = np.array([[o.score_one(h, i) for i in range(len(refs))] for h in hyps])  # 14 x 14 oracle scores
    pick = np.array([np.nonzero((hyps == r).all(1))[0][0] for r in rows])
    got = c.score(torch.from_numpy(rows).to(gpu_device), torch.from_numpy(idx).to(gpu_device)).cpu().numpy()
    close(got, table[pick, idx])


def test_end_to_end_from_the_decode(gpu_device):
    from adaptive_amd import Config, Encoder2Decoder, synth
    B, T = 8, 20
    model = Encoder2Decoder(Config()).to(gpu_device).load_synthetic(123)
    ids, _, _ = model.sampler(torch.from_numpy(synth.make_features(B, seed=0)).to(gpu_device), max_len=T)
    host = ids.cpu().numpy()
    refs = []
    for row in host:  # each image's references from its own caption: itself, and a copy with one token changed
        other = row.copy()
        other[1] = 7 if other[1] != 7 else 8
        refs.append([row.tolist(), other.tolist()])
    rng = np.random.default_rng(3)
    df_refs = [[rng.integers(3, 200, size=10).tolist()] for _ in range(100)]
    c = CiderD(refs, df_refs=df_refs).to(gpu_device)
    got = c.score(ids).cpu().numpy()  # straight from the decode's device tensor
    want = CiderOracle(refs, df_refs=df_refs).score(list(host))
    close(got, want)
    has_tokens = host[:, 0] != END
    assert has_tokens.any() and (got[has_tokens] > 0).all()
