"""Generate the BLEU / ROUGE-L golden by running the REAL reference scorers,
``coco/pycocoevalcap/bleu/bleu_scorer.py`` (``BleuScorer.compute_score(option='closest')``, as ``bleu/bleu.py``
calls it) and ``coco/pycocoevalcap/rouge/rouge.py`` (``Rouge.compute_score``), on seeded synthetic captions.

Run where the reference tree is present, naming its root:

    python tests/golden/make_golden_metrics.py /path/to/reference

The two files are loaded by path at run time (the package around them wants Java tokenisers) and fed token
ids as space-joined strings: to the scorers an id is a word.  Tokens come from 20 ids so that n-grams overlap.
The cases the 16 images cover are listed beside ``hyps`` below.

Writes ``metrics_eval.npz`` (data only): the ragged references, the hypotheses padded with ``end_id``, the
reference's per-caption ``bleu_list``, its corpus ``Bleu_1..4``, its totals ``_testlen`` / ``_reflen``, and its
per-caption ROUGE-L with the mean.
"""
from __future__ import annotations

import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402

END, T, LO, HI = 2, 20, 3, 23  # tokens in [3, 23)
REFS_PER_IMAGE = [1, 2, 3, 4, 5, 6, 7, 1, 3, 2, 2, 4, 1, 5, 6, 1]


def load(ref_root, *parts):
    path = os.path.join(ref_root, "coco", "pycocoevalcap", *parts)
    spec = importlib.util.spec_from_file_location("ref_" + parts[-1][:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_cases():
    rng = np.random.default_rng(20240911)
    refs = [[rng.integers(LO, HI, size=int(rng.integers(6, 13))).tolist() for _ in range(k)] for k in REFS_PER_IMAGE]
    refs[5][0][2:5] = [7, 7, 7]                       # a reference that repeats the token the hypothesis repeats
    refs[5][1] = [t if t != 7 else 8 for t in refs[5][1]][:6] + [7]   # ... and one that has it once
    refs[9] = [refs[9][0][:6], (refs[9][1] * 2)[:10]]  # lengths 6 and 10: a hypothesis of 8 is between them
    refs[11][2] = []                                   # an empty reference among others
    refs[12] = [[]]                                    # the only reference is empty
    refs[15] = [[]]

    def perturbed(cap, k):
        cap = list(cap)
        for p in rng.choice(len(cap), size=k, replace=False):
            cap[int(p)] = int(rng.integers(LO, HI))
        return cap

    hyps = [
        [],                                                   # 0: empty
        [refs[1][0][3]],                                      # 1: one token (guess_2..4 = 0)
        refs[2][1][:2],                                       # 2: two tokens
        refs[3][2][1:4],                                      # 3: three tokens
        (refs[4][0] + refs[4][3] + refs[4][1] + refs[4][2])[:T],   # 4: T tokens, no end_id
        [7] * 6,                                              # 5: one token six times: clipped at 3
        refs[6][int(np.argmax([len(r) for r in refs[6]]))] + [5, 9, 12],  # 6: longer than every reference: no penalty
        list(refs[7][0]),                                     # 7: the only reference itself
        refs[8][int(np.argmin([len(r) for r in refs[8]]))][:4],  # 8: shorter than every reference: penalty
        (refs[9][1][:5] + refs[9][0][:3]),                    # 9: 8 tokens between 6 and 10: reflen 6
        refs[10][1][::-1],                                    # 10: a reference reversed: LCS << length
        perturbed(refs[11][0], 2),                            # 11: an empty reference among the image's
        [],                                                   # 12: empty against an empty only reference: ROUGE-L 1
        perturbed(refs[13][3], 1)[:-2],
        refs[14][2][:4] + refs[14][4][2:7],
        refs[1][0][:5],                                       # 15: tokens against an empty only reference
    ]
    assert all(len(h) <= T for h in hyps) and len(hyps[4]) == T and len(hyps[9]) == 8
    assert len(hyps) == len(refs) == len(REFS_PER_IMAGE) and [len(r) for r in refs] == REFS_PER_IMAGE
    return refs, hyps


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ADAPTIVE_REFERENCE", "")
    if not os.path.isdir(ref_root):
        sys.exit("usage: make_golden_metrics.py /path/to/reference")
    BleuScorer = load(ref_root, "bleu", "bleu_scorer.py").BleuScorer
    Rouge = load(ref_root, "rouge", "rouge.py").Rouge
    refs, hyps = make_cases()
    words = lambda cap: " ".join(map(str, cap))  # noqa: E731
    scorer = BleuScorer(n=4)
    gts, res = {}, {}
    for i, (h, img) in enumerate(zip(hyps, refs)):
        scorer += (words(h), [words(r) for r in img])
        gts[i], res[i] = [words(r) for r in img], [words(h)]
    corpus_bleu, bleu_list = scorer.compute_score(option="closest", verbose=0)
    rouge_mean, rouge = Rouge().compute_score(gts, res)
    padded = np.full((len(hyps), T), END, dtype=np.int64)
    for i, h in enumerate(hyps):
        padded[i, :len(h)] = h
    flat = [r for img in refs for r in img]
    np.savez_compressed(
        os.path.join(HERE, "metrics_eval.npz"),
        ref_tokens=np.concatenate([np.asarray(r, dtype=np.int16) for r in flat]),
        ref_lengths=np.asarray([len(r) for r in flat], dtype=np.int32),
        refs_per_image=np.asarray(REFS_PER_IMAGE, dtype=np.int32),
        hyps=padded.astype(np.int16), end_id=np.int64(END),
        bleu=np.asarray(bleu_list, dtype=np.float64).T.copy(),       # [images][4]
        corpus_bleu=np.asarray(corpus_bleu, dtype=np.float64),
        testlen=np.int64(scorer._testlen), reflen=np.int64(scorer._reflen),
        rouge=np.asarray(rouge, dtype=np.float64), rouge_mean=np.float64(rouge_mean))
    print("images", len(hyps), "Bleu", np.round(corpus_bleu, 4).tolist(), "testlen", scorer._testlen, "reflen",
          scorer._reflen, "ROUGE_L", float(rouge_mean), "per caption", np.round(rouge, 4).tolist(), flush=True)


if __name__ == "__main__":
    main()
