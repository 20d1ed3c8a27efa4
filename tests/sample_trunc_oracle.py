"""CPU oracle for the truncated (top-k / nucleus) sampling decode and N draws per image — TEST
INFRASTRUCTURE ONLY.

A subclass of ``SampleOracle``: the same decoder step, the same noise.  Per row and step, over the fp32
``y = x / tau`` and in float64 from there on, with ``m = max y`` and ``e_v = exp(y_v - m)``:

    S_k   = { v : #{ w : y_w > y_v } < top_k }                       (top_k == 0 or >= V: everything)
    Z_k   = sum_{S_k} e_v,  G(v) = sum_{w in S_k, y_w > y_v} e_w
    S     = { v in S_k : G(v) < p Z_k },  p = float32(top_p)          (p == 1: S = S_k, by rule)
    theta = min_{v in S} y_v,  kept = |S|
    token = argmax_{v in S} fp32(y_v + g_v)                           (first index on ties)
    logp  = y_token - (m + log sum_{v in S} e_v)

``select`` works on y sorted descending, where S is a prefix.  It also evaluates the same definition with
every comparison moved by a tolerance (``kept_size`` with ``dv`` / ``mf`` / ``ma``): the *inner* set is
what survives when each value comparison ``y_w > y_v`` is read as ``y_w > y_v - 2 delta`` (w != v) and
each mass ratio ``G / Z_k`` as ``(G / Z_k) e^{2 delta} + 1e-6``; the *outer* set moves them the other
way.  An implementation whose y is within delta of the oracle's (so a difference of two within
2 delta, a ratio of two exponentials within e^{+-2 delta}) keeps a set between the two.

``num_samples = N``: the encoder runs once on the B images and every image's state is repeated N times;
row ``b N + n`` draws with the noise of global row ``row0 N + b N + n``.
"""
from __future__ import annotations

import numpy as np
import torch

from adaptive_amd import synth
from oracle.adaptive_oracle import ATT
from sample_oracle import SampleOracle

MASS_EPS = 1e-6  # fixed-point masses and fp32 exponentials against float64


def kept_size(ys: np.ndarray, es: np.ndarray, top_k: int, top_p: float, dv: float = 0.0, mf: float = 1.0,
              ma: float = 0.0) -> int:
    """Size of the kept prefix of ``ys`` (float64, descending; ``es = exp(ys - ys[0])``) when ``y_w > y_v`` is
    read as ``y_w > y_v + dv`` (w != v) and ``G / Z_k`` as ``G / Z_k * mf + ma``.  dv = 0, mf = 1, ma = 0
    is the definition; dv < 0, mf > 1, ma > 0 shrink the set; the opposite signs grow it."""
    V = ys.shape[0]
    # above[i] = #{ w != i : ys[w] > ys[i] + dv }: -ys ascends; with dv < 0 the count includes i itself
    above = np.searchsorted(-ys, -(ys + dv), side="left") - (1 if dv < 0 else 0)
    nk = V
    if 0 < top_k < V:
        nk = int(np.count_nonzero(above < top_k))           # above is non-decreasing: a prefix
    p = float(np.float32(top_p))
    if p == 1.0:
        return nk
    cs = np.concatenate([[0.0], np.cumsum(es)])
    G = cs[np.minimum(above + (1 if dv < 0 else 0), nk)] - (es if dv < 0 else 0.0)  # mass above, within S_k
    keep = (G[:nk] / cs[nk]) * mf + ma < p
    return int(np.argmin(keep)) if not keep.all() else nk    # G is non-decreasing: the first False ends the prefix


def select(y: np.ndarray, g: np.ndarray, top_k: int, top_p: float, delta: float | None = None) -> dict:
    """One row's selection.  y, g: fp32 [V].  Returns token, logp (fp32), kept, theta (fp32), and with
    ``delta`` the band: kept_in / kept_out, theta_in / theta_out, robust."""
    assert y.dtype == np.float32 and g.dtype == np.float32
    order = np.argsort(-y, kind="stable")                    # descending, ties by the smaller index
    ys = y[order].astype(np.float64)
    es = np.exp(ys - ys[0])
    kept = kept_size(ys, es, top_k, top_p)
    assert kept >= 1 and (kept == ys.shape[0] or ys[kept] < ys[kept - 1]), "S is a union of whole tie groups"
    z = y + g                                                # fp32 add
    zs = z[order]
    members = order[:kept]
    best = float(zs[:kept].max())
    token = int(members[zs[:kept] == np.float32(best)].min())  # first index on ties
    out = {"token": token, "kept": kept, "theta": np.float32(ys[kept - 1]),
           "logp": np.float32(np.float64(y[token]) - (ys[0] + np.log(es[:kept].sum()))), "order": order}
    if delta is not None:
        gf = float(np.exp(2 * delta))
        kin = kept_size(ys, es, top_k, top_p, -2 * delta, gf, MASS_EPS)
        kout = kept_size(ys, es, top_k, top_p, 2 * delta, 1.0 / gf, -MASS_EPS)
        assert 0 <= kin <= kept <= kout
        zo = zs[:kout].astype(np.float64)
        a = int(np.argmax(zo))
        lead = float(zo[a] - np.partition(zo, kout - 2)[kout - 2]) if kout > 1 else float("inf")
        out.update(kept_in=kin, kept_out=kout, theta_in=np.float32(ys[kin - 1]) if kin else np.float32(np.inf),
                   theta_out=np.float32(ys[kout - 1]), lead=lead,
                   robust=bool(kin >= 1 and a < kin and lead > 4 * delta and int(order[a]) == token))
    return out


def logp_for_kept(y: np.ndarray, token: int, kept: int) -> np.float32:
    """logp of ``token`` when the kept set is the ``kept`` best columns of y (fp32 [V]), in float64."""
    ys = np.sort(y.astype(np.float64))[::-1]
    return np.float32(np.float64(y[token]) - (ys[0] + np.log(np.exp(ys[:kept] - ys[0]).sum())))


class SampleTruncOracle(SampleOracle):
    @torch.no_grad()
    def sample_trunc(self, feats, T: int, tau: float = 1.0, seed: int = 0, row0: int = 0, top_k: int = 0,
                     top_p: float = 1.0, num_samples: int = 1, delta: float | None = None, keep_y: bool = False):
        """feats [B,C,7,7] -> dict: ids [R,T] int64, logp [R,T] fp32, alpha [R,T,49], beta [R,T,1] (tensors),
        kept [R,T] int32, theta [R,T] fp32, R = B num_samples; with ``delta`` also kept_in / kept_out /
        theta_in / theta_out / robust / lead [R,T]; with ``keep_y`` the fp32 y [R,T,V]."""
        images = torch.as_tensor(np.ascontiguousarray(feats)) if not torch.is_tensor(feats) else feats
        B, N = images.size(0), int(num_samples)
        R = B * N
        nv = self.w["decoder.adaptive.mlp.weight"].shape[0]
        key = synth.stream_key(int(seed), "sample")
        tau32 = np.float32(tau)
        V, v_g, states, _ = self.encoder(images)
        if N > 1:  # one encoder pass; the rows of an image share its outputs
            V, v_g = V.repeat_interleave(N, 0), v_g.repeat_interleave(N, 0)
            states = tuple(s.repeat_interleave(N, 1) for s in states)
        tok = torch.ones(R, 1, dtype=torch.long)
        names = ["kept", "theta"] + (["kept_in", "kept_out", "theta_in", "theta_out", "robust", "lead"]
                                     if delta is not None else [])
        dt = {"kept": np.int32, "kept_in": np.int32, "kept_out": np.int32, "robust": bool, "lead": np.float64}
        res = {n: np.zeros((R, T), dt.get(n, np.float32)) for n in names}
        ids = np.zeros((R, T), np.int64)
        logp = np.zeros((R, T), np.float32)
        ys = np.zeros((R, T, nv), np.float32) if keep_y else None
        al, be = [], []
        for t in range(T):
            scores, alpha, beta, states = self.decoder(V, v_g, tok, states)
            y = scores[:, 0, :].numpy().astype(np.float32) / tau32
            assert y.dtype == np.float32
            for r in range(R):
                g = synth.gumbel_f32(key, ((row0 * N + r) * T + t) * nv, nv)
                s = select(y[r], g, top_k, top_p, delta)
                ids[r, t], logp[r, t] = s["token"], s["logp"]
                for n in names:
                    res[n][r, t] = s[n]
            if keep_y:
                ys[:, t] = y
            tok = torch.from_numpy(ids[:, t:t + 1].copy())
            al.append(alpha)
            be.append(beta)
        res.update(ids=torch.from_numpy(ids), logp=torch.from_numpy(logp),
                   alpha=torch.cat(al, dim=1) if T else torch.zeros(R, 0, ATT),
                   beta=torch.cat(be, dim=1) if T else torch.zeros(R, 0, 1))
        if keep_y:
            res["y"] = ys
        return res
