"""CPU oracle for the baseline spatial-attention greedy decode — TEST INFRASTRUCTURE ONLY.

A PyTorch-CPU fp32 restatement of the reference's baseline model
(``code_src/models/baseline_attention.py``): ``Atten.forward`` (:78-96), ``AdaptiveBlock.forward``
(:116-128) and ``Encoder2Decoder.sampler`` (:233-280), op for op.  The encoder tail and the LSTM
recurrence of ``Decoder.forward`` are the adaptive oracle's (the two models share them).

Pinned by ``tests/golden/make_golden_baseline.py``, which runs the real reference module, through
``tests/test_baseline_cpu.py``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.adaptive_oracle import OracleModel


class BaselineOracle(OracleModel):
    """``state``: the baseline state dict (no sentinel keys, no ``atten.affine_s``)."""

    # ---- Atten.forward (baseline_attention.py:78-96) --------------------------------------------
    def atten(self, V, h_t):
        w = self.w
        Wv = w["decoder.adaptive.atten.affine_v.weight"]
        Wg = w["decoder.adaptive.atten.affine_g.weight"]
        wh = w["decoder.adaptive.atten.affine_h.weight"]
        content_v = F.linear(V, Wv).unsqueeze(1) + F.linear(h_t, Wg).unsqueeze(2)          # :86-87
        z_t = F.linear(torch.tanh(content_v), wh).squeeze(3)                               # :90
        alpha_t = F.softmax(z_t.view(-1, z_t.size(2)), dim=1).view(z_t.size(0), z_t.size(1), -1)  # :91
        c_t = torch.bmm(alpha_t, V).squeeze(2)                                             # :94
        return c_t, alpha_t

    # ---- AdaptiveBlock.forward (baseline_attention.py:116-128) ----------------------------------
    def adaptive(self, x, hiddens, cells, V):
        """-> (scores, alpha, None): the inherited ``decoder`` unpacks three values; there is no beta."""
        w = self.w
        c_hat, alpha = self.atten(V, hiddens)                                              # :122
        scores = F.linear(c_hat + hiddens, w["decoder.adaptive.mlp.weight"], w["decoder.adaptive.mlp.bias"])  # :126
        return scores, alpha, None

    # ---- Encoder2Decoder.sampler (baseline_attention.py:233-280) --------------------------------
    @torch.no_grad()
    def sampler(self, images: torch.Tensor, max_len: int = 30, keep_scores: bool = False):
        """-> (ids, alpha) (+ the per-step logits [B,T,V] with ``keep_scores``)."""
        V, v_g, states, _ = self.encoder(images)                                           # :248-252
        captions = torch.LongTensor(images.size(0), 1).fill_(1)                            # :257 <start> = 1
        sampled_ids, attention, all_scores = [], [], []
        for _ in range(max_len):                                                            # :263
            scores, atten_weights, _, states = self.decoder(V, v_g, captions, states)
            predicted = scores.max(2)[1]                                                    # :267
            captions = predicted
            sampled_ids.append(captions)
            attention.append(atten_weights)
            if keep_scores:
                all_scores.append(scores)
        out = (torch.cat(sampled_ids, dim=1), torch.cat(attention, dim=1))
        if keep_scores:
            return out + (torch.cat(all_scores, dim=1),)
        return out
