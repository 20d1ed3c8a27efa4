"""CPU restatement of the CIDEr-D scorer on token ids (checker only; never on the product path).

The semantics are the reference's ``coco/pycocoevalcap/cider/cider_scorer.py`` (``compute_doc_freq``,
``counts2vec``, ``sim``, ``compute_cider``), restated with ``Counter``s over tuples of ids;
``tests/golden/cider_eval.npz`` (recorded from the reference's own file) pins it.  Two things the
reference does not have: the document frequencies may come from another corpus (``df_refs``), and any
number of hypotheses may be scored per image (``image_index``).

Reproduced on purpose: ``length`` is the number of *bigrams* (the reference adds the term frequency where
its zero-based order index is 1).
"""
from __future__ import annotations

from collections import Counter

import numpy as np

N = 4
TOKEN_LIMIT = 65535


def cut(seq, end_id):
    """The ids before the first end_id."""
    out = []
    for t in np.asarray(seq).reshape(-1).tolist():
        if t == end_id:
            break
        out.append(int(t))
    return out


def ngram_counts(tokens):
    c = Counter()
    for n in range(1, N + 1):
        for i in range(len(tokens) - n + 1):
            c[tuple(tokens[i:i + n])] += 1
    return c


class CiderOracle:
    def __init__(self, refs, end_id=2, sigma=6.0, df_refs=None):
        self.end_id, self.sigma = end_id, float(sigma)
        self.crefs = [[ngram_counts(cut(r, end_id)) for r in img] for img in refs]
        dfc = self.crefs if df_refs is None else [[ngram_counts(cut(r, end_id)) for r in img] for img in df_refs]
        self.df = Counter()
        for img in dfc:
            for g in set(g for ref in img for g in ref):
                self.df[g] += 1
        self.log_m = np.log(float(len(dfc)))

    def weight(self, g):
        return self.log_m - np.log(max(1.0, float(self.df.get(g, 0))))

    def counts2vec(self, cnts):
        vec = [dict() for _ in range(N)]
        norm = [0.0] * N
        length = 0
        for g, tf in cnts.items():
            n = len(g) - 1
            vec[n][g] = float(tf) * self.weight(g)
            norm[n] += pow(vec[n][g], 2)
            if n == 1:
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    def sim(self, vh, vr, nh, nr, lh, lr):
        delta = float(lh - lr)
        val = np.zeros(N)
        for n in range(N):
            for g in vh[n]:
                val[n] += min(vh[n][g], vr[n].get(g, 0.0)) * vr[n].get(g, 0.0)
            if nh[n] != 0 and nr[n] != 0:
                val[n] /= nh[n] * nr[n]
            val[n] *= np.e ** (-(delta ** 2) / (2 * self.sigma ** 2))
        return val

    def score_one(self, hyp, image):
        """hyp: an id sequence (cut at end_id here).  NaN for a token outside [0, 65535) before the end."""
        tokens = cut(hyp, self.end_id)
        if any(t < 0 or t >= TOKEN_LIMIT for t in tokens):
            return float("nan")
        vec, norm, length = self.counts2vec(ngram_counts(tokens))
        score = np.zeros(N)
        refs = self.crefs[image]
        for ref in refs:
            vr, nr, lr = self.counts2vec(ref)
            score += self.sim(vec, vr, norm, nr, length, lr)
        s = np.mean(score)
        s /= len(refs)
        s *= 10.0
        return float(s)

    def score(self, hyps, image_index=None):
        idx = range(len(hyps)) if image_index is None else [int(i) for i in image_index]
        return np.array([self.score_one(h, i) for h, i in zip(hyps, idx)], dtype=np.float64)
