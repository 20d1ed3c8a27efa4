"""CPU restatement of BLEU-1..4 and ROUGE-L on token ids (checker only; never on the product path).

The semantics are the reference's ``coco/pycocoevalcap/bleu/bleu_scorer.py`` (``precook``, ``cook_refs``,
``cook_test``, ``compute_score(option='closest')``) and ``rouge/rouge.py`` (``my_lcs``, ``calc_score``),
restated with ``Counter``s over tuples of ids and a plain dynamic programme;
``tests/golden/metrics_eval.npz`` (recorded from the reference's own files) pins it.  One thing the reference
does not have: any number of hypotheses may be scored per image (``image_index``).

Reproduced on purpose: ROUGE-L's word lists come from ``"".split(" ")``, which turns an empty caption into
one empty word, so the lengths it divides by are ``max(len, 1)`` and two empty captions have an LCS of 1.
"""
from __future__ import annotations

import math
from collections import Counter

import numpy as np

from cider_oracle import TOKEN_LIMIT, cut, ngram_counts

N = 4
BETA = 1.2
SMALL, TINY = 1e-9, 1e-15


def lcs_dp(a, b):
    """Length of the longest common subsequence: the textbook table, row by row."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def lcs_bits(hyp, ref):
    """The kernel's form, for len(hyp) <= 64: one 64-bit word V, bit i for hypothesis position i; per
    reference token U = V & M, V = (V + U) | (V - U) modulo 2^64; the LCS is the number of zeros among
    V's low len(hyp) bits."""
    assert len(hyp) <= 64
    full = (1 << 64) - 1
    v = full
    for y in ref:
        m = sum(1 << i for i, x in enumerate(hyp) if x == y)
        u = v & m
        v = ((v + u) | (v - u)) & full
    return bin(~v & ((1 << len(hyp)) - 1)).count("1")


def bleu_of(correct, guess, testlen, reflen):
    """bleu_1..4 of the ten statistics, a sentence's or a corpus's totals."""
    out, b = [], 1.0
    for k in range(N):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [x * math.exp(1 - 1 / ratio) for x in out]
    return out


class MetricsOracle:
    def __init__(self, refs, end_id=2):
        self.end_id = end_id
        self.tokens = [[cut(r, end_id) for r in img] for img in refs]
        self.lengths = [[len(r) for r in img] for img in self.tokens]
        self.clip = []
        for img in self.tokens:
            most = Counter()
            for r in img:
                for g, c in ngram_counts(r).items():
                    most[g] = max(most[g], c)
            self.clip.append(most)

    def hypothesis(self, hyp, image):
        """The cut tokens, or None for a bad row (a token outside [0, 65535) or an image outside the corpus)."""
        tokens = cut(hyp, self.end_id)
        if any(t < 0 or t >= TOKEN_LIMIT for t in tokens) or not 0 <= image < len(self.tokens):
            return None
        return tokens

    def stats_one(self, hyp, image):
        """[correct_1..4, guess_1..4, testlen, reflen]; zeros for a bad row."""
        tokens = self.hypothesis(hyp, image)
        if tokens is None:
            return [0] * 10
        L = len(tokens)
        correct = [0] * N
        for g, c in ngram_counts(tokens).items():
            correct[len(g) - 1] += min(c, self.clip[image].get(g, 0))
        guess = [max(0, L - n + 1) for n in range(1, N + 1)]
        reflen = min((abs(l - L), l) for l in self.lengths[image])[1]
        return correct + guess + [L, reflen]

    def bleu_one(self, hyp, image):
        if self.hypothesis(hyp, image) is None:
            return [float("nan")] * N
        s = self.stats_one(hyp, image)
        return bleu_of(s[:4], s[4:8], s[8], s[9])

    def rouge_one(self, hyp, image):
        tokens = self.hypothesis(hyp, image)
        if tokens is None:
            return float("nan")
        prec, rec = [], []
        for ref in self.tokens[image]:
            if len(tokens) == 0 and len(ref) == 0:
                lcs = 1
            else:
                lcs = lcs_dp(ref, tokens)
            prec.append(lcs / float(max(len(tokens), 1)))
            rec.append(lcs / float(max(len(ref), 1)))
        p, r = max(prec), max(rec)
        if p != 0 and r != 0:
            return ((1 + BETA ** 2) * p * r) / float(r + BETA ** 2 * p)
        return 0.0

    def _idx(self, hyps, image_index):
        return range(len(hyps)) if image_index is None else [int(i) for i in image_index]

    def stats(self, hyps, image_index=None):
        return np.array([self.stats_one(h, i) for h, i in zip(hyps, self._idx(hyps, image_index))],
                        dtype=np.int64).reshape(-1, 10)

    def bleu(self, hyps, image_index=None):
        return np.array([self.bleu_one(h, i) for h, i in zip(hyps, self._idx(hyps, image_index))],
                        dtype=np.float64).reshape(-1, N)

    def rouge(self, hyps, image_index=None):
        return np.array([self.rouge_one(h, i) for h, i in zip(hyps, self._idx(hyps, image_index))], dtype=np.float64)

    def corpus(self, hyps, image_index=None):
        """eval.py's figures over the rows that are not bad: Bleu_1..4 from the totals, ROUGE_L the mean."""
        idx = list(self._idx(hyps, image_index))
        good = [(h, i) for h, i in zip(hyps, idx) if self.hypothesis(h, i) is not None]
        tot = np.array([self.stats_one(h, i) for h, i in good], dtype=np.int64).reshape(-1, 10).sum(0)
        b = bleu_of([int(x) for x in tot[:4]], [int(x) for x in tot[4:8]], int(tot[8]), int(tot[9]))
        table = {f"Bleu_{n + 1}": b[n] for n in range(N)}
        table["ROUGE_L"] = float(np.mean([self.rouge_one(h, i) for h, i in good]))
        return table
