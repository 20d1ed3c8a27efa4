"""CPU oracle of the constrained beam search (``Encoder2Decoder.beam_search(suppress_ids=, min_length=,
no_repeat_ngram=, no_end_after=)``, ``aa_beam_decode_cx``) -- TEST INFRASTRUCTURE ONLY.  It restates the
specification of include/adaptive_amd.h in the oracle's dtype: the loop of ``BeamDivOracle.beam_search_div``
with a forbidden mask applied to the candidates before the finished-beam override.

A live hypothesis at step t has emitted ``y_0 .. y_{t-1}`` (traced through its parents; ``<start>`` is not
among them), and ``y_{-1} = 1`` (``<start>``).  Candidate token v is forbidden iff

1. ``v in suppress_ids``;
2. ``v == end_id`` and ``t < min_length``;
3. ``v == end_id`` and ``y_{t-1} in no_end_after``;
4. ``n = no_repeat_ngram >= 1`` and some j in ``[n-1, t-1]`` has
   ``(y_{j-n+1} .. y_{j-1}) == (y_{t-n+1} .. y_{t-1})`` and ``v == y_j``.

A forbidden candidate scores -inf in the selection; the survivors keep ``cum + log_softmax(logits)`` over the
*full* vocabulary (no renormalisation).  A finished beam keeps its single carried ``<end>``: no constraint
applies to it.  Everything else -- step-0 liveness, the groups, the tie order, the final ranking -- is
``beam_search_div``'s.

``blocked``: per constraint kind (``suppress``, ``min_length``, ``no_end_after``, ``ngram``), the number of
forbidden candidates that stood in the *unmasked* top Kg of their group (the group's augmented ranking on the
candidates without the mask, carried ``<end>`` and step-0 liveness as usual), summed over images, steps and
groups: a case table asserts from it that a constraint really changes a selection.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn.functional as F

from oracle.adaptive_oracle import ATT
from beam_div_oracle import BeamDivOracle

KINDS = ("suppress", "min_length", "no_end_after", "ngram")


class BeamConsOracle(BeamDivOracle):
    @staticmethod
    def forbidden(hist: torch.Tensor, t: int, nv: int, end_id: int, suppress_ids: Sequence[int], min_length: int,
                  no_repeat_ngram: int, no_end_after: Sequence[int]) -> Dict[str, torch.Tensor]:
        """hist [B,K,t] (the rows' own tokens) -> per kind a bool mask [B,K,nv] of the forbidden candidates."""
        B, K = hist.shape[:2]
        m = {k: torch.zeros(B, K, nv, dtype=torch.bool) for k in KINDS}
        for v in suppress_ids:
            m["suppress"][:, :, v] = True
        if end_id >= 0 and t < min_length:
            m["min_length"][:, :, end_id] = True
        if end_id >= 0 and len(no_end_after):
            last = hist[:, :, t - 1] if t else torch.ones(B, K, dtype=torch.long)
            hit = torch.zeros(B, K, dtype=torch.bool)
            for v in no_end_after:
                hit |= last == v
            m["no_end_after"][:, :, end_id] = hit
        n = int(no_repeat_ngram)
        if n >= 1:
            for j in range(n - 1, t):
                eq = torch.ones(B, K, dtype=torch.bool)
                for i in range(1, n):
                    eq &= hist[:, :, j - i] == hist[:, :, t - i]
                bb, kk = eq.nonzero(as_tuple=True)
                m["ngram"][bb, kk, hist[bb, kk, j]] = True
        return m

    @torch.no_grad()
    def beam_search_cons(self, images: torch.Tensor, max_len: int = 20, beam_size: int = 3, end_id: int = 2,
                         groups: int = 1, diversity: float = 0.0, length_penalty: float = 0.0,
                         suppress_ids: Sequence[int] = (), min_length: int = 0, no_repeat_ngram: int = 0,
                         no_end_after: Sequence[int] = ()) -> Dict[str, object]:
        """-> what ``beam_search_div`` returns, and ``blocked``: dict kind -> count (see the module docstring)."""
        K, G, T = int(beam_size), int(groups), int(max_len)
        assert G >= 1 and K % G == 0 and diversity >= 0 and length_penalty >= 0
        assert min_length >= 0 and no_repeat_ngram >= 0 and end_id not in suppress_ids
        assert end_id >= 0 or (min_length == 0 and not len(no_end_after))
        Kg = K // G
        sel_margin, penalised = float("inf"), 0
        blocked = {k: 0 for k in KINDS}
        V, v_g, (h, c), _ = self.encoder(images)
        B = images.size(0)
        Vk = V.repeat_interleave(K, 0)
        vgk = v_g.repeat_interleave(K, 0)
        states = (h.repeat_interleave(K, 1), c.repeat_interleave(K, 1))
        nv = self.w["decoder.adaptive.mlp.weight"].shape[0]
        assert all(0 <= v < nv for v in tuple(suppress_ids) + tuple(no_end_after))
        assert nv - len(suppress_ids) - 1 - (T if no_repeat_ngram else 0) >= K
        tok = torch.ones(B * K, 1, dtype=torch.long)                               # <start> = 1
        cum = torch.zeros(B, K, dtype=self.dtype)
        fin = torch.zeros(B, K, dtype=torch.bool)
        hist = torch.zeros(B, K, 0, dtype=torch.long)                              # the rows' own tokens so far
        lam = torch.tensor(diversity, dtype=self.dtype)
        ninf = -float("inf")
        htok, hpar, hal, hbe = [], [], [], []
        base = (torch.arange(B) * K).unsqueeze(1)
        for t in range(T):
            scores, alpha, beta, states = self.decoder(Vk, vgk, tok, states)
            logp = F.log_softmax(scores[:, 0, :], dim=1).view(B, K, nv)
            free = cum.unsqueeze(2) + logp                                         # the candidates without the mask
            kinds = self.forbidden(hist, t, nv, end_id, suppress_ids, min_length, no_repeat_ngram, no_end_after)
            banned = kinds["suppress"] | kinds["min_length"] | kinds["no_end_after"] | kinds["ngram"]
            cand = free.masked_fill(banned, ninf)
            carry = torch.zeros(B, K, nv, dtype=torch.bool)
            if t == 0:
                dead = torch.arange(K) % Kg != 0
                cand[:, dead, :] = ninf
                free[:, dead, :] = ninf
            if end_id >= 0 and fin.any():
                bb, kk = fin.nonzero(as_tuple=True)
                for x in (cand, free):
                    x[bb, kk, :] = ninf
                    x[bb, kk, end_id] = cum[bb, kk]
                carry[bb, kk, end_id] = True
            n = torch.zeros(B, nv, dtype=self.dtype)
            parent = torch.zeros(B, K, dtype=torch.long)
            token = torch.zeros(B, K, dtype=torch.long)
            new_cum = torch.zeros(B, K, dtype=self.dtype)
            for g in range(G):
                sl = slice(g * Kg, (g + 1) * Kg)
                raw = cand[:, sl, :]
                pen = lam * n.unsqueeze(1)
                aug = torch.where(carry[:, sl, :], raw, raw - pen)
                vals, idx = torch.sort(aug.reshape(B, Kg * nv), dim=1, descending=True, stable=True)
                assert bool(torch.isfinite(vals[:, :Kg]).all()), "the selection ran dry"
                gaps = vals[:, :Kg] - vals[:, 1:Kg + 1]
                gaps = gaps[torch.isfinite(gaps)]
                if gaps.numel():
                    sel_margin = min(sel_margin, float(gaps.min()))
                # what the unmasked ranking would have taken: forbidden candidates among its best Kg
                ufree = torch.where(carry[:, sl, :], free[:, sl, :], free[:, sl, :] - pen).reshape(B, Kg * nv)
                uvals, uidx = torch.sort(ufree, dim=1, descending=True, stable=True)
                took = torch.isfinite(uvals[:, :Kg]) & ~carry[:, sl, :].reshape(B, Kg * nv).gather(1, uidx[:, :Kg])
                for kind in KINDS:
                    blocked[kind] += int((kinds[kind][:, sl, :].reshape(B, Kg * nv).gather(1, uidx[:, :Kg]) & took).sum())
                idx = idx[:, :Kg]
                p, v = idx // nv, idx % nv
                newly = ~carry[:, sl, :].reshape(B, Kg * nv).gather(1, idx)
                penalised += int((newly & (n.gather(1, v) > 0)).sum())
                parent[:, sl], token[:, sl] = p + g * Kg, v
                new_cum[:, sl] = raw.reshape(B, Kg * nv).gather(1, idx)          # the raw score
                n.scatter_add_(1, v, newly.to(self.dtype))
            cum = new_cum
            fin = fin.gather(1, parent) | ((token == end_id) if end_id >= 0 else torch.zeros_like(fin))
            rows = (base + parent).view(-1)
            states = (states[0][:, rows], states[1][:, rows])
            tok = token.reshape(B * K, 1)
            hist = torch.cat([hist.gather(1, parent.unsqueeze(2).expand(-1, -1, t)), token.unsqueeze(2)], dim=2)
            htok.append(token)
            hpar.append(parent)
            hal.append(alpha[:, 0].view(B, K, -1))
            hbe.append(beta[:, 0, 0].view(B, K))
        # backtrace of every slot
        seqs = torch.zeros(B, K, T, dtype=torch.long)
        al = torch.zeros(B, K, T, hal[0].size(2) if T else ATT, dtype=self.dtype)
        be = torch.zeros(B, K, T, 1, dtype=self.dtype)
        j = torch.arange(K).expand(B, K).clone()
        for t in range(T - 1, -1, -1):
            seqs[:, :, t] = htok[t].gather(1, j)
            p = hpar[t].gather(1, j)
            al[:, :, t] = hal[t].gather(1, p.unsqueeze(2).expand(-1, -1, hal[t].size(2)))
            be[:, :, t, 0] = hbe[t].gather(1, p)
            j = p
        assert torch.equal(seqs, hist)
        # final ranking
        is_end = (seqs == end_id) if end_id >= 0 else torch.zeros_like(seqs, dtype=torch.bool)
        first = torch.where(is_end.any(2), is_end.to(torch.int64).argmax(2), torch.full((B, K), T - 1, dtype=torch.long))
        lengths = first + 1
        rank = cum / lengths.to(self.dtype) ** torch.tensor(length_penalty, dtype=self.dtype)
        rs, order = torch.sort(rank, dim=1, descending=True, stable=True)
        rgaps = rs[:, :-1] - rs[:, 1:]
        rank_margin = float(rgaps.min()) if rgaps.numel() else float("inf")
        ar = torch.arange(B).unsqueeze(1)
        return {"ids": seqs[ar, order][:, 0].clone(), "alpha": al[ar, order][:, 0].clone(),
                "beta": be[ar, order][:, 0].clone(), "seqs": seqs[ar, order], "scores": cum.gather(1, order),
                "lengths": lengths.gather(1, order).to(torch.int32), "rank_scores": rs,
                "group": (order // Kg).to(torch.int32), "sel_margin": sel_margin, "rank_margin": rank_margin,
                "penalised": penalised, "blocked": blocked}
