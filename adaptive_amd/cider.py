"""CIDEr-D on token ids, scored on the device (C-ABI ``aa_cider_score``, ``csrc/aa_cider.hip``).

The reference selects its models by CIDEr: ``coco_eval`` (``code_src/tools/utils.py:108-250``) decodes,
turns ids into sentences and hands them to ``coco/pycocoevalcap/cider/cider_scorer.py``; ``train.py:150-181``
keeps the best figure.  ``CiderD`` computes that scorer's number -- count clipping and the Gaussian length
penalty included, so CIDEr-D whatever the file is called -- directly on the decode's id tensor, and gives
``sample(num_samples=N)`` the per-caption reward it was built for.  Words and the PTB tokeniser stay outside:
the vocabulary has mapped words to ids before this point, and a caption is the ids before the row's first
``end_id`` (as ``captions.ids_to_sentences`` cuts it).

Semantics (include/adaptive_amd.h states them in full; tests/cider_oracle.py restates them with Counters):
``w(g) = log M - log max(1, df(g))`` over the M images of the document-frequency corpus, ``vec = c w``,
per reference and order ``min(vec_h, vec_r) vec_r`` summed over the hypothesis's n-grams, divided by the two
norms when both are non-zero, times ``exp(-(len_h - len_r)^2 / (2 sigma^2))`` where **len is the number of
bigrams** (the reference's quirk, reproduced), and ``10 * mean over the four orders / #refs``.

The corpus is built once on the host with vectorised numpy (one sort of the packed n-gram keys) and uploaded:
CSR references with ascending uint64 keys, and an open-addressing table of the weights that the kernel
probes with the ``splitmix64`` of ``adaptive_amd.synth``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import numpy as np

from .synth import MIX1, MIX2

NGRAM = 4
TOKEN_LIMIT = 65535  # tokens are in [0, TOKEN_LIMIT): a 16-bit field holds tok + 1, and 0 is "no token"
MAX_T = 64


def splitmix64(z: np.ndarray) -> np.ndarray:
    """The finaliser ``synth._mix_int`` / the kernels' ``splitmix`` on a uint64 array."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
    return z ^ (z >> np.uint64(31))


def pack_key(tokens: Sequence[int]) -> int:
    """key(g) = sum_j (tok_j + 1) << 16 j of one n-gram (1 <= n <= 4)."""
    k = 0
    for j, t in enumerate(tokens):
        k |= (int(t) + 1) << (16 * j)
    return k


def key_order(keys: np.ndarray) -> np.ndarray:
    """The order n of packed keys: the number of non-zero 16-bit fields."""
    k = np.asarray(keys, dtype=np.uint64)
    return (1 + (k >> np.uint64(16) != 0).astype(np.int64) + (k >> np.uint64(32) != 0)
            + (k >> np.uint64(48) != 0))


class _Flat:
    """A corpus flattened: per image its captions, each cut before its first end_id."""

    def __init__(self, refs, end_id: int, what: str):
        if len(refs) == 0:
            raise ValueError(f"{what}: no images")
        caps, per_image = [], np.empty(len(refs), dtype=np.int64)
        for i, img in enumerate(refs):
            per_image[i] = len(img)
            if per_image[i] == 0:
                raise ValueError(f"{what}: image {i} has no reference caption")
            for c in img:
                if hasattr(c, "detach"):
                    c = c.detach().cpu().numpy()
                caps.append(np.asarray(c, dtype=np.int64).reshape(-1))
        self.images = len(refs)
        self.img_ptr = np.concatenate([[0], np.cumsum(per_image)]).astype(np.int64)
        ncap = len(caps)
        raw_len = np.fromiter((c.size for c in caps), dtype=np.int64, count=ncap)
        tok = np.concatenate(caps) if ncap else np.empty(0, dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(raw_len)])[:-1]
        cid = np.repeat(np.arange(ncap), raw_len)
        pos = np.arange(tok.size) - start[cid]
        # cut before the first end_id
        length = raw_len.copy()
        is_end = tok == end_id
        np.minimum.at(length, cid[is_end], pos[is_end])
        keep = pos < length[cid]
        tok, cid = tok[keep], cid[keep]
        if tok.size and (tok.min() < 0 or tok.max() >= TOKEN_LIMIT):
            bad = tok[(tok < 0) | (tok >= TOKEN_LIMIT)][0]
            raise ValueError(f"{what}: token {int(bad)} outside [0, {TOKEN_LIMIT})")
        self.length = length                                  # tokens per caption
        self.tok = tok                                        # the cut captions' tokens, caption after caption
        self.cap_image = np.repeat(np.arange(self.images), per_image)
        self.caps = ncap
        # every n-gram of every caption as (caption, key); a caption's tokens are contiguous in tok
        tok1 = (tok + 1).astype(np.uint64)
        start = np.concatenate([[0], np.cumsum(length)])[:-1]
        pos = np.arange(tok.size) - start[cid]
        e_cap, e_key = [], []
        for n in range(1, NGRAM + 1):
            idx = np.nonzero(pos + n <= length[cid])[0]
            k = tok1[idx].copy()
            for j in range(1, n):
                k |= tok1[idx + j] << np.uint64(16 * j)
            e_cap.append(cid[idx])
            e_key.append(k)
        self.e_cap = np.concatenate(e_cap)
        self.e_key = np.concatenate(e_key)

    def document_frequency(self):
        """(keys ascending, df): the number of images with the key in any of their captions."""
        img = self.cap_image[self.e_cap]
        order = np.lexsort((img, self.e_key))
        k, i = self.e_key[order], img[order]
        first = np.ones(k.size, dtype=bool)
        first[1:] = (k[1:] != k[:-1]) | (i[1:] != i[:-1])  # one entry per (key, image)
        return np.unique(k[first], return_counts=True)

    def counts(self):
        """CSR of the captions' n-gram counts: (ref_ptr, keys ascending within a caption, counts)."""
        order = np.lexsort((self.e_key, self.e_cap))
        c, k = self.e_cap[order], self.e_key[order]
        first = np.ones(k.size, dtype=bool)
        first[1:] = (k[1:] != k[:-1]) | (c[1:] != c[:-1])
        at = np.nonzero(first)[0]
        cnt = np.diff(np.append(at, k.size))
        cap = c[at]
        ref_ptr = np.concatenate([[0], np.cumsum(np.bincount(cap, minlength=self.caps))])
        return ref_ptr, cap, k[at], cnt


def build_table(keys: np.ndarray, values: np.ndarray):
    """Open addressing with linear probing at load factor <= 0.5: (tab_keys, tab_w), size a power of two.
    A key sits at ``splitmix64(key) & (size - 1)`` or the first free slot after it (wrapping)."""
    keys = np.asarray(keys, dtype=np.uint64)
    size = 2
    while size < 2 * keys.size:
        size *= 2
    tab_keys = np.zeros(size, dtype=np.uint64)
    tab_w = np.zeros(size, dtype=np.float64)
    mask = np.uint64(size - 1)
    pending = np.arange(keys.size)
    slot = splitmix64(keys) & mask
    while pending.size:  # one round per probe distance; a slot never empties, so earlier probes stay valid
        s = slot[pending]
        free = tab_keys[s] == 0
        _, firsts = np.unique(s, return_index=True)  # one claimant per slot and round
        win = np.zeros(pending.size, dtype=bool)
        win[firsts] = True
        win &= free
        tab_keys[s[win]] = keys[pending[win]]
        tab_w[s[win]] = values[pending[win]]
        pending = pending[~win]
        slot[pending] = (slot[pending] + np.uint64(1)) & mask
    return tab_keys, tab_w


def probe(tab_keys: np.ndarray, tab_w: np.ndarray, keys: np.ndarray, miss: float) -> np.ndarray:
    """The kernel's table look-up restated: at most ``size`` probes from the key's home slot."""
    keys = np.atleast_1d(np.asarray(keys, dtype=np.uint64))
    size = tab_keys.size
    mask = np.uint64(size - 1)
    out = np.full(keys.size, miss, dtype=np.float64)
    slot = splitmix64(keys) & mask
    live = np.arange(keys.size)
    for _ in range(size):
        if not live.size:
            break
        tk = tab_keys[slot[live]]
        hit = tk == keys[live]
        out[live[hit]] = tab_w[slot[live[hit]]]
        live = live[~hit & (tk != 0)]
        slot[live] = (slot[live] + np.uint64(1)) & mask
    return out


class CiderD:
    """CIDEr-D of id captions against ``refs``.

    ``refs``: per image, a list of token-id sequences (each cut before its first ``end_id``).
    ``df_refs``: the corpus the document frequencies come from, in the same form; by default ``refs``
    itself, which is the reference's ``compute_score`` (evaluation).  A reward against fixed training
    statistics passes the training references here.  Raises ``ValueError`` for an image without
    references and for a token outside ``[0, 65535)``.
    """

    def __init__(self, refs, end_id: int = 2, sigma: float = 6.0, df_refs=None):
        sigma = float(sigma)
        if not (math.isfinite(sigma) and sigma > 0.0):
            raise ValueError(f"sigma must be finite and > 0, got {sigma}")
        self.end_id, self.sigma = int(end_id), sigma
        flat = _Flat(refs, self.end_id, "refs")
        df_flat = flat if df_refs is None else _Flat(df_refs, self.end_id, "df_refs")
        df_keys, df = df_flat.document_frequency()
        self.df_images = df_flat.images
        self.w_unseen = float(np.log(float(df_flat.images)))
        df_w = self.w_unseen - np.log(np.maximum(1.0, df.astype(np.float64)))
        self.tab_keys, self.tab_w = build_table(df_keys, df_w)
        ref_ptr, cap, keys, cnt = flat.counts()
        at = np.minimum(np.searchsorted(df_keys, keys), max(df_keys.size - 1, 0))
        w = np.where(df_keys[at] == keys, df_w[at], self.w_unseen) if df_keys.size else np.full(keys.size, self.w_unseen)
        vec = cnt.astype(np.float64) * w
        norm2 = np.bincount(cap * NGRAM + (key_order(keys) - 1), weights=vec * vec, minlength=NGRAM * flat.caps)
        self.images, self.refs = flat.images, flat.caps
        self.img_ptr = flat.img_ptr.astype(np.int32)
        self.ref_ptr = ref_ptr.astype(np.int32)
        self.keys = keys
        self.counts = cnt.astype(np.int32)
        self.ref_norm = np.sqrt(norm2).reshape(flat.caps, NGRAM)
        self.ref_len = np.maximum(flat.length - 1, 0).astype(np.int32)  # bigrams
        if ref_ptr[-1] >= 1 << 31:
            raise ValueError("refs: more than 2**31 n-gram entries")
        self.device = None
        self._dev = None     # the uploaded arrays (kept alive) and the C struct over them
        self._struct = None

    def weight(self, keys) -> np.ndarray:
        """w(g) of packed keys, looked up as the kernel does (a miss is ``log M``)."""
        return probe(self.tab_keys, self.tab_w, keys, self.w_unseen)

    def to(self, device) -> "CiderD":
        import torch

        from . import _lib
        device = torch.device(device)

        def up(a, dtype=None):  # (an empty array still gets an address: one element of padding)
            a = np.ascontiguousarray(a)
            if a.dtype == np.uint64:
                a = a.view(np.int64)
            if a.size == 0:
                a = np.zeros(1, dtype=a.dtype)
            return torch.from_numpy(a).to(device)

        d = {k: up(getattr(self, k)) for k in ("img_ptr", "ref_ptr", "keys", "counts", "ref_norm", "ref_len",
                                               "tab_keys", "tab_w")}
        self._dev = d
        self._struct = _lib.CiderCorpus(*(d[k].data_ptr() for k in ("img_ptr", "ref_ptr", "keys", "counts", "ref_norm",
                                                                   "ref_len", "tab_keys", "tab_w")),
                                        self.images, self.refs, self.tab_keys.size, self.w_unseen, self.sigma)
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

    def score(self, ids, image_index=None):
        """ids ``[R, T]`` int64 on the corpus's device (T <= 64) -> float64 ``[R]`` on the device: row r
        against image ``image_index[r]`` (default: image r).  One launch on the current stream and no
        host synchronisation.  A token outside ``[0, 65535)`` before the row's first ``end_id``, or an
        image outside the corpus, gives that row NaN."""
        import torch

        from . import _lib
        if self._struct is None:
            raise RuntimeError("CiderD: call .to(device) before score()")
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
        out = torch.empty(R, dtype=torch.float64, device=self.device)
        if R == 0:
            return out
        with _lib.on_device(self.device):
            rc = _lib.load().aa_cider_score(ctypes.byref(self._struct), ids.data_ptr() if T else None, R, T,
                                            ids.stride(0) if T else 0, self.end_id, _lib.ptr(idx), out.data_ptr(),
                                            _lib.stream_handle())
        _lib.check(rc, "cider_score")
        return out

    def corpus_score(self, ids, image_index=None):
        """``coco_eval``'s CIDEr (``utils.py:234-250``): ``(mean, per_caption)``, both on the device --
        the mean over the scored captions as a 0-dim float64 tensor and the scores ``[R]``."""
        per = self.score(ids, image_index)
        return per.mean(), per

    def self_critical(self, sample_ids, greedy_ids, num_samples: int, image_index=None):
        """The self-critical advantage ``[B * N]``: ``score(sample) - score(greedy)`` with the greedy score
        repeated N times per image, in ``sample(num_samples=N)``'s image-major row order (row ``b N + n``).
        ``sample_ids`` ``[B * N, T]``, ``greedy_ids`` ``[B, T']``; ``image_index`` ``[B]`` names the images
        (default: image b)."""
        import torch
        N = int(num_samples)
        if N < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        B = greedy_ids.shape[0]
        if sample_ids.shape[0] != B * N:
            raise ValueError(f"{sample_ids.shape[0]} sampled rows for {B} images x {N} samples")
        if self.device is None:
            raise RuntimeError("CiderD: call .to(device) before self_critical()")
        idx = torch.arange(B, device=self.device, dtype=torch.int32) if image_index is None else self._index(image_index, B)
        base = self.score(greedy_ids, idx)
        return self.score(sample_ids, idx.repeat_interleave(N)) - base.repeat_interleave(N)
