"""BLEU-1..4 and ROUGE-L on token ids, scored on the device (C-ABI ``aa_metrics_score`` / ``aa_bleu_corpus``,
``csrc/aa_metrics.hip``), beside ``cider.CiderD``.

The reference's ``coco_eval`` reports ``Bleu_1..4``, ``METEOR``, ``ROUGE_L`` and ``CIDEr`` through
``coco/pycocoevalcap/eval.py``.  ``CaptionMetrics`` computes what ``bleu/bleu_scorer.py`` (as ``bleu/bleu.py``
calls it: ``option='closest'``, n = 4) and ``rouge/rouge.py`` compute, on the decode's id tensor: words and the
PTB tokeniser stay outside, and a caption is the ids before the row's first ``end_id``, as for ``CiderD``.
METEOR (a Java jar and WordNet data) and SPICE (a parser) are not built.

Semantics (include/adaptive_amd.h states them in full; tests/metrics_oracle.py restates them with Counters and
a plain DP).  For a hypothesis of L tokens: ``guess_n = max(0, L - n + 1)``, ``correct_n`` the n-gram counts
clipped by the largest count in one reference of the image, ``reflen`` the reference length closest to L (a
tie goes to the shorter); sentence BLEU ``b *= (correct_n + 1e-15) / (guess_n + 1e-9)``, ``bleu_n = b ** (1 / n)``,
times ``exp(1 - 1 / ratio)`` when ``ratio = (L + 1e-15) / (reflen + 1e-9) < 1``; corpus BLEU the same on the
integer totals.  ROUGE-L with beta = 1.2 from the largest precision and the largest recall over the
references, each on its own -- and **1 when hypothesis and reference are both empty**, because the reference
splits ``""`` into one empty word (reproduced, not corrected).

The corpus is built once on the host with vectorised numpy from ``cider._Flat`` and uploaded: per image a CSR
of clip counts (keys ascending, value = the maximum over the image's references of the n-gram's count, so the
kernel searches once per n-gram and not once per reference), the references' lengths, and their tokens as a
CSR for the LCS.  References may be empty and may be longer than 64 tokens; hypotheses have ``T <= 64``.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np

from .cider import MAX_T, _Flat

STATS = 10  # correct_1..4, guess_1..4, testlen, reflen


class MetricScores(NamedTuple):
    """``CaptionMetrics.score``'s result (device tensors): ``bleu`` [R, 4] and ``rouge_l`` [R] float64,
    ``stats`` [R, 10] int32 (correct_1..4, guess_1..4, testlen, reflen)."""
    bleu: object
    rouge_l: object
    stats: object


class CaptionMetrics:
    """BLEU-1..4 and ROUGE-L of id captions against ``refs``.

    ``refs``: per image, a list of token-id sequences (each cut before its first ``end_id``), the form
    ``CiderD`` takes.  Raises ``ValueError`` for an image without references and for a token outside
    ``[0, 65535)``.
    """

    def __init__(self, refs, end_id: int = 2):
        self.end_id = int(end_id)
        flat = _Flat(refs, self.end_id, "refs")
        self.images, self.refs = flat.images, flat.caps
        self.img_ptr = flat.img_ptr.astype(np.int32)
        self.ref_len = flat.length.astype(np.int32)
        tok_ptr = np.concatenate([[0], np.cumsum(flat.length)])
        self.ref_tok = flat.tok.astype(np.uint16)
        # clip counts: the (caption, key, count) entries regrouped by (image, key), the largest count kept
        _, cap, keys, cnt = flat.counts()
        img = flat.cap_image[cap]
        order = np.lexsort((keys, img))
        i, k, c = img[order], keys[order], cnt[order]
        if k.size:
            first = np.ones(k.size, dtype=bool)
            first[1:] = (k[1:] != k[:-1]) | (i[1:] != i[:-1])
            at = np.nonzero(first)[0]
            self.clip_keys = k[at]
            self.clip_counts = np.maximum.reduceat(c, at).astype(np.int32)
            per_image = np.bincount(i[at], minlength=self.images)
        else:  # every reference is empty
            self.clip_keys = np.empty(0, dtype=np.uint64)
            self.clip_counts = np.empty(0, dtype=np.int32)
            per_image = np.zeros(self.images, dtype=np.int64)
        clip_ptr = np.concatenate([[0], np.cumsum(per_image)])
        if clip_ptr[-1] >= 1 << 31 or tok_ptr[-1] >= 1 << 31:
            raise ValueError("refs: more than 2**31 n-gram entries or tokens")
        self.clip_ptr = clip_ptr.astype(np.int32)
        self.tok_ptr = tok_ptr.astype(np.int32)
        self.device = None
        self._dev = None     # the uploaded arrays (kept alive) and the C struct over them
        self._struct = None

    _ARRAYS = ("img_ptr", "clip_ptr", "clip_keys", "clip_counts", "ref_len", "tok_ptr", "ref_tok")

    def to(self, device) -> "CaptionMetrics":
        import torch

        from . import _lib
        device = torch.device(device)

        def up(a):  # (an empty array still gets an address: one element of padding)
            a = np.ascontiguousarray(a)
            if a.dtype == np.uint64:
                a = a.view(np.int64)
            if a.dtype == np.uint16:
                a = a.view(np.int16)
            if a.size == 0:
                a = np.zeros(1, dtype=a.dtype)
            return torch.from_numpy(a).to(device)

        d = {k: up(getattr(self, k)) for k in self._ARRAYS}
        self._dev = d
        self._struct = _lib.MetricsCorpus(*(d[k].data_ptr() for k in self._ARRAYS), self.images, self.refs)
        self.device = device
        return self

    def _index(self, image_index, R: int):
        import torch
        if image_index is None:
            if R > self.images:
                raise ValueError(f"{R} rows for {self.images} images: pass image_index")
            return None
        idx = torch.as_tensor(image_index, device=self.device).to(torch.int32).contiguous()
        if idx.shape != (R,):
            raise ValueError(f"image_index must have shape ({R},), got {tuple(idx.shape)}")
        return idx

    def score(self, ids, image_index=None) -> MetricScores:
        """ids ``[R, T]`` int64 on the corpus's device (T <= 64) -> ``MetricScores`` of device tensors: row r
        against image ``image_index[r]`` (default: image r).  One launch on the current stream and no
        host synchronisation.  A token outside ``[0, 65535)`` before the row's first ``end_id``, or an
        image outside the corpus, gives that row NaN floats and zero statistics."""
        import torch

        from . import _lib
        if self._struct is None:
            raise RuntimeError("CaptionMetrics: call .to(device) before score()")
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int64 and ids.dim() == 2):
            raise ValueError("ids must be an int64 tensor [R, T]")
        if ids.device != self.device:
            raise ValueError(f"ids are on {ids.device}, the corpus on {self.device}")
        R, T = ids.shape
        if T > MAX_T:
            raise ValueError(f"T = {T} exceeds {MAX_T}")
        if T > 0 and ids.stride(1) != 1:
            ids = ids.contiguous()
        idx = self._index(image_index, R)
        out = MetricScores(torch.empty(R, 4, dtype=torch.float64, device=self.device),
                           torch.empty(R, dtype=torch.float64, device=self.device),
                           torch.empty(R, STATS, dtype=torch.int32, device=self.device))
        if R == 0:
            return out
        with _lib.on_device(self.device):
            rc = _lib.load().aa_metrics_score(ctypes.byref(self._struct), ids.data_ptr() if T else None, R, T,
                                              ids.stride(0) if T else 0, self.end_id, _lib.ptr(idx),
                                              out.stats.data_ptr(), out.bleu.data_ptr(), out.rouge_l.data_ptr(),
                                              _lib.stream_handle())
        _lib.check(rc, "metrics_score")
        return out

    def corpus_score(self, ids, image_index=None, cider=None) -> dict:
        """``coco_eval``'s table under ``eval.py``'s names, as 0-dim float64 device tensors: ``Bleu_1..4``
        from the integer totals of the rows' statistics (``aa_bleu_corpus``), ``ROUGE_L`` the mean of the
        rows' scores, and ``CIDEr`` (the mean of ``cider.score``) when a ``CiderD`` on the same device is
        passed.  A row with NaN scores (see ``score``) is left out of every figure: its statistics are 0 and
        the means skip it.  No host synchronisation."""
        import torch

        from . import _lib
        per = self.score(ids, image_index)
        R = per.stats.shape[0]
        bleu = torch.zeros(4, dtype=torch.float64, device=self.device)  # (no rows: the expression gives 0)
        if R > 0:
            with _lib.on_device(self.device):
                rc = _lib.load().aa_bleu_corpus(per.stats.data_ptr(), R, bleu.data_ptr(), _lib.stream_handle())
            _lib.check(rc, "bleu_corpus")
        table = {f"Bleu_{n + 1}": bleu[n] for n in range(4)}
        table["ROUGE_L"] = per.rouge_l.nanmean()
        if cider is not None:
            if cider.device != self.device:
                raise ValueError(f"the CiderD is on {cider.device}, the metrics corpus on {self.device}")
            if cider.end_id != self.end_id:
                raise ValueError(f"end_id differs: CiderD {cider.end_id}, CaptionMetrics {self.end_id}")
            table["CIDEr"] = cider.score(ids, image_index).nanmean()
        return table


class MixedReward:
    """A self-critical reward mixed from CIDEr-D, sentence BLEU-4 and ROUGE-L:
    ``cider_weight * CIDEr-D + bleu4_weight * BLEU-4 + rouge_weight * ROUGE-L`` per caption, float64 on the
    device.  It offers what ``Encoder2Decoder.self_critical_loss`` asks of a scorer (``device``, ``end_id``,
    ``_index``, ``score``).  A term whose weight is 0 is not computed, so with only ``cider_weight = 1`` the
    reward is ``cider.score``'s bit for bit.  Both scorers must be on one device, with one ``end_id`` and
    the same number of images."""

    def __init__(self, cider, metrics, cider_weight: float = 1.0, bleu4_weight: float = 0.0,
                 rouge_weight: float = 0.0):
        weights = tuple(float(w) for w in (cider_weight, bleu4_weight, rouge_weight))
        if not all(math.isfinite(w) for w in weights):
            raise ValueError(f"weights must be finite, got {weights}")
        if all(w == 0.0 for w in weights):
            raise ValueError("every weight is 0")
        if cider.end_id != metrics.end_id:
            raise ValueError(f"end_id differs: CiderD {cider.end_id}, CaptionMetrics {metrics.end_id}")
        if cider.images != metrics.images:
            raise ValueError(f"images differ: CiderD {cider.images}, CaptionMetrics {metrics.images}")
        if cider.device is None or cider.device != metrics.device:
            raise ValueError(f"the scorers must be on one device: CiderD on {cider.device}, "
                             f"CaptionMetrics on {metrics.device}")
        self.cider, self.metrics = cider, metrics
        self.cider_weight, self.bleu4_weight, self.rouge_weight = weights
        self.device, self.end_id, self.images = cider.device, cider.end_id, cider.images

    def _index(self, image_index, R: int):
        return self.cider._index(image_index, R)

    def score(self, ids, image_index=None):
        """ids ``[R, T]`` -> float64 ``[R]``: the weighted sum, its terms added in the order CIDEr-D,
        BLEU-4, ROUGE-L.  No host synchronisation."""
        total = None
        if self.cider_weight != 0.0:
            total = self.cider_weight * self.cider.score(ids, image_index)
        if self.bleu4_weight != 0.0 or self.rouge_weight != 0.0:
            m = self.metrics.score(ids, image_index)
            if self.bleu4_weight != 0.0:
                term = self.bleu4_weight * m.bleu[:, 3]
                total = term if total is None else total + term
            if self.rouge_weight != 0.0:
                term = self.rouge_weight * m.rouge_l
                total = term if total is None else total + term
        return total
