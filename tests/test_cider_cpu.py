"""CPU: the CIDEr-D oracle against the reference's recorded scores, the host corpus builder against the
oracle, the constructor's errors, and aa_cider_score's argument codes (no device work)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cider_cases import golden_cases, other_corpus
from cider_oracle import CiderOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return golden_cases()


def test_golden_covers_what_it_should(golden):
    refs, hyps, end, scores, _ = golden
    assert len(refs) >= 12 and sorted(set(len(r) for r in refs)) == [1, 2, 3, 4, 5, 6, 7]
    lens = [int((row == end).argmax()) if (row == end).any() else hyps.shape[1] for row in hyps]
    assert {0, 1, 2, 3, 20} <= set(lens)
    assert any(l == 6 and len(set(row[:6].tolist())) == 1 for row, l in zip(hyps, lens))
    assert any(l == max(len(r) for r in img) + 3 == min(len(r) for r in img) + 3 for l, img in zip(lens, refs))
    assert all(any(3 in r for r in img) for img in refs)  # a unigram with df = M
    assert scores[0] == 0.0 and (scores[1:] > 0).all()


def test_oracle_matches_the_reference_scorer(golden):
    refs, hyps, end, scores, mean = golden
    got = CiderOracle(refs, end_id=end).score(hyps)
    np.testing.assert_allclose(got, scores, rtol=0, atol=1e-12)
    assert abs(got.mean() - mean) <= 1e-12


@pytest.mark.parametrize("own_df", [True, False])
def test_corpus_builder_matches_the_oracle(golden, own_df):
    from adaptive_amd.cider import CiderD, key_order, pack_key
    refs, _, end, _, _ = golden
    df_refs = None if own_df else other_corpus()
    c = CiderD(refs, end_id=end, df_refs=df_refs)
    o = CiderOracle(refs, end_id=end, df_refs=df_refs)
    assert c.images == len(refs) and c.refs == sum(len(r) for r in refs)
    np.testing.assert_array_equal(c.img_ptr, np.concatenate([[0], np.cumsum([len(r) for r in refs])]))
    assert c.w_unseen == o.log_m
    flat = [cnt for img in o.crefs for cnt in img]
    for r, cnts in enumerate(flat):
        lo, hi = c.ref_ptr[r], c.ref_ptr[r + 1]
        keys = c.keys[lo:hi]
        assert (np.diff(keys.astype(object)) > 0).all()  # ascending, no duplicate
        want = {pack_key(g): n for g, n in cnts.items()}
        assert dict(zip(keys.tolist(), c.counts[lo:hi].tolist())) == want
        _, norm, length = o.counts2vec(cnts)
        np.testing.assert_allclose(c.ref_norm[r], norm, rtol=1e-14, atol=0)
        assert c.ref_len[r] == length
        for g in cnts:
            assert key_order([pack_key(g)])[0] == len(g)


@pytest.mark.parametrize("own_df", [True, False])
def test_idf_table(golden, own_df):
    from adaptive_amd.cider import CiderD, pack_key
    refs, _, end, _, _ = golden
    df_refs = None if own_df else other_corpus()
    c = CiderD(refs, end_id=end, df_refs=df_refs)
    o = CiderOracle(refs, end_id=end, df_refs=df_refs)
    size = c.tab_keys.size
    assert size & (size - 1) == 0 and c.tab_w.size == size
    assert np.count_nonzero(c.tab_keys) == len(o.df) and 2 * len(o.df) <= size  # load factor <= 0.5
    grams = list(o.df)
    got = c.weight([pack_key(g) for g in grams])
    np.testing.assert_array_equal(got, [o.weight(g) for g in grams])  # every corpus n-gram is found
    absent = [(50000,), (3, 50000), (50000, 3, 4, 5), (65534, 65534, 65534, 65534)]
    assert all(g not in o.df for g in absent)
    np.testing.assert_array_equal(c.weight([pack_key(g) for g in absent]), [o.log_m] * len(absent))


def test_collisions_and_wrap_around_in_the_builder():
    """Keys that share a home slot, the last one, are all found again, and an absent key that starts there
    misses after walking the same chain."""
    from adaptive_amd.cider import build_table, probe, splitmix64
    size = 16
    toks = np.arange(1, 65536, dtype=np.uint64)  # unigram keys
    home = splitmix64(toks) & np.uint64(size - 1)
    last = toks[home == size - 1][:7]
    tab_keys, tab_w = build_table(last[:6], np.arange(6, dtype=np.float64) + 1)
    assert tab_keys.size == size and tab_keys[size - 1] != 0 and np.count_nonzero(tab_keys[:5]) == 5  # wrapped
    np.testing.assert_array_equal(probe(tab_keys, tab_w, last[:6], -1.0), np.arange(6) + 1.0)
    assert probe(tab_keys, tab_w, last[6:7], -1.0)[0] == -1.0


def test_value_errors():
    from adaptive_amd.cider import CiderD
    with pytest.raises(ValueError, match="no reference"):
        CiderD([[[3, 4]], []])
    with pytest.raises(ValueError, match="no reference"):
        CiderD([[[3, 4]]], df_refs=[[]])
    with pytest.raises(ValueError, match="outside"):
        CiderD([[[3, 65535]]])
    with pytest.raises(ValueError, match="outside"):
        CiderD([[[3, -1, 4]]])
    with pytest.raises(ValueError, match="sigma"):
        CiderD([[[3, 4]]], sigma=0.0)
    c = CiderD([[[3, 65534, 2, 70000]]])  # 65534 is the largest token; what follows end_id is cut
    assert c.ref_len[0] == 1 and c.counts.sum() == 3


def test_package_exports_ciderd():
    import adaptive_amd
    from adaptive_amd.cider import CiderD
    assert adaptive_amd.CiderD is CiderD and "CiderD" in adaptive_amd.__all__


@pytest.fixture(scope="module")
def lib():
    from adaptive_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "adaptive_amd", "csrc")], check=True)
    return _lib.load()


def test_argument_codes_without_device_work(lib):
    from adaptive_amd import _lib
    assert lib.aa_abi_version() == 17
    P = 256  # a fake non-NULL pointer: every call below returns before any device work

    def corpus(**kw):
        f = dict(img_ptr=P, ref_ptr=P, keys=P, counts=P, ref_norm=P, ref_len=P, tab_keys=P, tab_w=P, images=3, refs=5,
                 tab_size=64, w_unseen=1.0, sigma=6.0)
        f.update(kw)
        return ctypes.byref(_lib.CiderCorpus(**f))

    def call(c, ids=P, R=4, T=20, ld=20, image=None, scores=P):
        return lib.aa_cider_score(c, ids, R, T, ld, 2, image, scores, None)

    assert call(corpus(), R=-1) == -3
    assert call(corpus(), T=-1) == -3
    assert call(corpus(), T=65, ld=65) == -3
    assert call(corpus(), T=20, ld=19) == -3
    assert call(None, ids=None, R=0, scores=None) == 0  # an empty batch: before any pointer is looked at
    assert call(None) == -1
    assert call(corpus(tab_size=48)) == -3
    assert call(corpus(tab_size=0)) == -3
    assert call(corpus(images=0)) == -3
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert call(corpus(sigma=s)) == -3
    for name in ("img_ptr", "ref_ptr", "keys", "counts", "ref_norm", "ref_len", "tab_keys", "tab_w"):
        assert call(corpus(**{name: None})) == -1
    assert call(corpus(), ids=None) == -1
    assert call(corpus(), scores=None) == -1
