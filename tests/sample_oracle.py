"""CPU oracle for the seeded temperature-sampling decode — TEST INFRASTRUCTURE ONLY.

The reference has no sampling decode, so (as ``BeamOracle`` is for beam search) this restatement *is*
the specification ``aa_sample_decode`` / ``Encoder2Decoder.sample`` are tested against.  Each step runs
the reference's own decoder step (``Decoder.forward`` with one token, through
``oracle.adaptive_oracle.OracleModel.decoder``), then, for batch row b at step t with fp32 logits x:

    y[v]  = x[v] / tau                                   (fp32)
    e     = ((row0 + b) * T + t) * V + v                 (element counter)
    g[v]  = synth.gumbel_f32(stream_key(seed, "sample"), e, 1)
    token = argmax_v fp32(y[v] + g[v])                   (first index on ties)
    logp  = y[token] - (max y + log sum exp(y - max y))  (float64 over the fp32 y, cast to fp32)

and the token feeds the next step.  All T steps run.
"""
from __future__ import annotations

import numpy as np
import torch

from adaptive_amd import synth
from oracle.adaptive_oracle import ATT, OracleModel


class SampleOracle(OracleModel):
    @torch.no_grad()
    def sample(self, feats, T: int, tau: float = 1.0, seed: int = 0, row0: int = 0, return_margin: bool = False):
        """feats: [B,C,7,7] numpy or tensor -> ids [B,T] int64, logp [B,T] fp32, alpha [B,T,49],
        beta [B,T,1] (tensors) (+ margin: the smallest gap, over rows and steps, between the best and
        the second-best perturbed score -- how much error in y + g the draw can absorb)."""
        images = torch.as_tensor(np.ascontiguousarray(feats)) if not torch.is_tensor(feats) else feats
        B = images.size(0)
        nv = self.w["decoder.adaptive.mlp.weight"].shape[0]
        key = synth.stream_key(int(seed), "sample")
        tau32 = np.float32(tau)
        V, v_g, states, _ = self.encoder(images)
        tok = torch.ones(B, 1, dtype=torch.long)                                   # <start> = 1
        ids = np.zeros((B, T), np.int64)
        logp = np.zeros((B, T), np.float32)
        al, be = [], []
        margin = float("inf")
        for t in range(T):
            scores, alpha, beta, states = self.decoder(V, v_g, tok, states)
            y = scores[:, 0, :].numpy().astype(np.float32) / tau32                 # fp32 division
            assert y.dtype == np.float32
            for b in range(B):
                g = synth.gumbel_f32(key, ((row0 + b) * T + t) * nv, nv)
                z = y[b] + g                                                       # fp32 add
                c = int(np.argmax(z))                                              # first maximal index
                top2 = np.partition(z, nv - 2)[nv - 2:] if nv > 1 else None
                if top2 is not None:
                    margin = min(margin, float(top2[1]) - float(top2[0]))
                y64 = y[b].astype(np.float64)
                mx = y64.max()
                logp[b, t] = np.float32(y64[c] - (mx + np.log(np.exp(y64 - mx).sum())))
                ids[b, t] = c
            tok = torch.from_numpy(ids[:, t:t + 1].copy())
            al.append(alpha)
            be.append(beta)
        alpha = torch.cat(al, dim=1) if T else torch.zeros(B, 0, ATT)
        beta = torch.cat(be, dim=1) if T else torch.zeros(B, 0, 1)
        out = (torch.from_numpy(ids), torch.from_numpy(logp), alpha, beta)
        return out + ((margin,) if return_margin else ())
