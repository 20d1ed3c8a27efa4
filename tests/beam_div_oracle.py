"""CPU oracle of the diverse-group beam search with a length-normalised final ranking
(``Encoder2Decoder.beam_search(groups=, diversity=, length_penalty=)``, ``aa_beam_decode_ex``) -- TEST
INFRASTRUCTURE ONLY.  It restates the specification of include/adaptive_amd.h in the oracle's dtype:

* rows ``b*K + k``; group g owns the slots ``g*Kg .. (g+1)*Kg - 1`` (Kg = K / G); a beam's parent is in
  its own group;
* raw candidates as ``BeamOracle``: ``cum + log_softmax(logits)``; at step 0 only slot 0 *of each group*
  is live; a finished beam has the single carry-over candidate ``end_id`` at its unchanged score;
* per step the groups select in order over a per-image count ``n[v]`` that starts at 0: group g ranks its
  Kg*V candidates by ``raw - diversity * n[v]`` (a carry-over is never penalised), descending, ties to
  the smaller ``q*V + v`` (q the parent's slot; a stable sort); the best Kg survive, in that order, with
  their *raw* score as the new ``cum``; then ``n[v] += 1`` for each survivor that newly emitted v
  (carry-overs do not count);
* final ranking: ``len`` = position of the first ``end_id`` + 1, or T; ``rank = cum / len**length_penalty``;
  the K beams of an image are sorted by rank descending, ties to the lower slot (stable).

Margins (how much score error the result can absorb): ``sel_margin`` is the smallest gap between
consecutive augmented scores among each group's Kg + 1 best, over images, steps and groups;
``rank_margin`` the smallest gap between consecutive final ranks of an image.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle.adaptive_oracle import ATT, BeamOracle


class BeamDivOracle(BeamOracle):
    @torch.no_grad()
    def beam_search_div(self, images: torch.Tensor, max_len: int = 20, beam_size: int = 3, end_id: int = 2,
                        groups: int = 1, diversity: float = 0.0, length_penalty: float = 0.0) -> Dict[str, object]:
        """-> dict: ids [B,T], alpha [B,T,49], beta [B,T,1] of the first-ranked beam; seqs [B,K,T], scores
        [B,K] (raw cum), lengths [B,K], rank_scores [B,K], group [B,K] in rank order; sel_margin,
        rank_margin; penalised (the number of survivors chosen although their token carried a penalty)."""
        K, G, T = int(beam_size), int(groups), int(max_len)
        assert G >= 1 and K % G == 0 and diversity >= 0 and length_penalty >= 0
        Kg = K // G
        sel_margin, penalised = float("inf"), 0
        V, v_g, (h, c), _ = self.encoder(images)
        B = images.size(0)
        Vk = V.repeat_interleave(K, 0)
        vgk = v_g.repeat_interleave(K, 0)
        states = (h.repeat_interleave(K, 1), c.repeat_interleave(K, 1))
        nv = self.w["decoder.adaptive.mlp.weight"].shape[0]
        tok = torch.ones(B * K, 1, dtype=torch.long)                               # <start> = 1
        cum = torch.zeros(B, K, dtype=self.dtype)
        fin = torch.zeros(B, K, dtype=torch.bool)
        lam = torch.tensor(diversity, dtype=self.dtype)
        ninf = -float("inf")
        htok, hpar, hal, hbe = [], [], [], []
        base = (torch.arange(B) * K).unsqueeze(1)
        for t in range(T):
            scores, alpha, beta, states = self.decoder(Vk, vgk, tok, states)
            logp = F.log_softmax(scores[:, 0, :], dim=1).view(B, K, nv)
            cand = cum.unsqueeze(2) + logp
            carry = torch.zeros(B, K, nv, dtype=torch.bool)
            if t == 0:
                dead = torch.arange(K) % Kg != 0
                cand[:, dead, :] = ninf
            if end_id >= 0 and fin.any():
                bb, kk = fin.nonzero(as_tuple=True)
                cand[bb, kk, :] = ninf
                cand[bb, kk, end_id] = cum[bb, kk]
                carry[bb, kk, end_id] = True
            n = torch.zeros(B, nv, dtype=self.dtype)
            parent = torch.zeros(B, K, dtype=torch.long)
            token = torch.zeros(B, K, dtype=torch.long)
            new_cum = torch.zeros(B, K, dtype=self.dtype)
            for g in range(G):
                sl = slice(g * Kg, (g + 1) * Kg)
                raw = cand[:, sl, :]
                aug = torch.where(carry[:, sl, :], raw, raw - lam * n.unsqueeze(1))
                vals, idx = torch.sort(aug.reshape(B, Kg * nv), dim=1, descending=True, stable=True)
                gaps = vals[:, :Kg] - vals[:, 1:Kg + 1]
                gaps = gaps[torch.isfinite(gaps)]
                if gaps.numel():
                    sel_margin = min(sel_margin, float(gaps.min()))
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
                "penalised": penalised}
