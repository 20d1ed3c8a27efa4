"""Generate the CIDEr-D golden by running the REAL reference scorer,
``coco/pycocoevalcap/cider/cider_scorer.py`` (``CiderScorer.compute_score``), on seeded synthetic captions.

Run where the reference tree is present (it is not on the GPU box):

    python tests/golden/make_golden_cider.py

The scorer's file is loaded by path (the package around it wants Java tokenisers and Python 2 imports) and
fed token ids as space-joined strings: to the scorer an id is a word.  Tokens come from 20 ids so that
n-grams overlap across captions and images; purely random captions over a large vocabulary would score 0
everywhere.  The cases the 14 images cover are listed beside ``hyps`` below.

Writes ``cider_eval.npz`` (data only): the ragged references, the hypotheses padded with ``end_id``, the
reference's per-image scores and their mean.
"""
from __future__ import annotations

import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402

REF = "/root/reference"
END, T, LO, HI = 2, 20, 3, 23  # tokens in [3, 23); 3 is the unigram every image has
REFS_PER_IMAGE = [1, 2, 3, 4, 5, 6, 7, 1, 2, 3, 4, 5, 6, 7]


def load_scorer():
    path = os.path.join(REF, "coco", "pycocoevalcap", "cider", "cider_scorer.py")
    spec = importlib.util.spec_from_file_location("ref_cider_scorer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CiderScorer


def make_cases():
    rng = np.random.default_rng(20240607)
    refs = []
    for i, k in enumerate(REFS_PER_IMAGE):
        img = []
        for j in range(k):
            n = 8 if i == 6 else int(rng.integers(6, 13))
            cap = rng.integers(LO + 1, HI, size=n).tolist()
            if j == 0:
                cap[int(rng.integers(0, n))] = LO  # in every image: df = M, w = 0
            img.append(cap)
        refs.append(img)
    refs[5][0][2:5] = [7, 7, 7]  # a reference that repeats the token the hypothesis repeats
    refs[5][0][0] = LO

    def perturbed(cap, k):
        cap = list(cap)
        for p in rng.choice(len(cap), size=k, replace=False):
            cap[int(p)] = int(rng.integers(LO, HI))
        return cap

    hyps = [
        [],                                                  # 0: empty
        [refs[1][0][3]],                                     # 1: one token
        refs[2][1][:2],                                      # 2: two tokens
        refs[3][2][1:4],                                     # 3: three tokens
        (refs[4][0] + refs[4][3] + refs[4][1] + refs[4][2])[:T],         # 4: T tokens, no end_id
        [7] * 6,                                             # 5: one token six times (counts > 1, clipping)
        refs[6][0] + [5, 9, 12],                             # 6: three longer than every reference (penalty)
        list(refs[7][0]),                                    # 7: the only reference itself
        perturbed(refs[8][1], 1),
        perturbed(refs[9][0], 2),
        perturbed(refs[10][3], 1)[:-2],
        refs[11][2][:4] + refs[11][4][2:7],
        perturbed(refs[12][5], 3),
        refs[13][6][::-1],                                   # a reference reversed: unigrams only
    ]
    assert all(len(h) <= T for h in hyps) and len(hyps[4]) == T
    return refs, hyps


def main():
    CiderScorer = load_scorer()
    refs, hyps = make_cases()
    scorer = CiderScorer(n=4, sigma=6.0)
    for h, img in zip(hyps, refs):
        scorer += (" ".join(map(str, h)), [" ".join(map(str, r)) for r in img])
    mean, scores = scorer.compute_score()
    padded = np.full((len(hyps), T), END, dtype=np.int64)
    for i, h in enumerate(hyps):
        padded[i, :len(h)] = h
    flat = [r for img in refs for r in img]
    np.savez_compressed(
        os.path.join(HERE, "cider_eval.npz"),
        ref_tokens=np.concatenate([np.asarray(r, dtype=np.int16) for r in flat]),
        ref_lengths=np.asarray([len(r) for r in flat], dtype=np.int32),
        refs_per_image=np.asarray(REFS_PER_IMAGE, dtype=np.int32),
        hyps=padded.astype(np.int16), end_id=np.int64(END), sigma=np.float64(6.0),
        scores=np.asarray(scores, dtype=np.float64), mean=np.float64(mean))
    print("images", len(hyps), "mean", float(mean), "scores", np.round(scores, 4).tolist(), flush=True)


if __name__ == "__main__":
    main()
