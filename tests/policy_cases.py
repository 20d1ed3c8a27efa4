"""End-to-end cases of the self-critical step, their float64 reference and the ReLU kink mask -- TEST
INFRASTRUCTURE ONLY (shared by tests/test_policy_cpu.py and tests/test_gpu_policy.py).

A case trains R = B * N captions of T tokens: weights ``synth.make_weights(11, Dims(E, H, V),
bias_noise=0.01)`` and features ``synth.make_features(B, seed=9)`` (tests/train_cases.py's seeds), ids
from ``default_rng(21)`` in [3, V) with ``<end>`` = 2 then placed by hand (row 0 at its last position,
row 1 at position 1, row 2 twice; the other rows have none), advantages
``policy_oracle.make_advantage(R)``.  The ids do not come from ``sample()``: the reference must not
depend on the code under test.

The reference is ``TrainOracle(state, dtype).forward(feats repeated N times per image, [<start>,
ids[:, :T-1]], [T] * R)`` followed by ``policy_oracle.policy_loss`` and autograd; the gradient of the
features is summed over the N repeats by autograd.  Computed once per (case, dtype) and shared:
callers must not modify what they get.  With ``gate=True`` the reference is that of
``forward_sampled(sampler_gate=True)``: the sentinel gate without its ``h_{t-1} W_h`` term at every step,
which is the same oracle with ``decoder.adaptive.sentinel.affine_h.weight`` set to 0 (that weight's own
gradient then says nothing and is dropped from the reference: the product's is an exact zero).  The kink
mask is tests/train_cases.py's (a pre-activation of affine_a / affine_b within ``KINK_REL`` rms of 0, in
float64), on these features.
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple

import numpy as np
import torch

import policy_oracle as po
import train_cases as tc
from adaptive_amd import synth

IDS_SEED = 21
SENT_H = "decoder.adaptive.sentinel.affine_h.weight"


class Case(NamedTuple):
    H: int
    E: int
    V: int
    B: int
    N: int
    T: int
    bf16: bool

    @property
    def R(self) -> int:
        return self.B * self.N


CASES: Dict[str, Case] = {
    "P1": Case(256, 32, 37, 3, 2, 5, True),
    "P2": Case(1024, 96, 3001, 2, 3, 4, False),
    "P3": Case(512, 256, 10123, 2, 2, 3, True),
}


def dims(case: Case) -> synth.Dims:
    return synth.Dims(embed=case.E, hidden=case.H, vocab=case.V)


def state(case: Case):
    return synth.make_weights(tc.WEIGHT_SEED, dims(case), bias_noise=tc.BIAS_NOISE)


def features(case: Case) -> np.ndarray:
    return synth.make_features(case.B, seed=tc.FEAT_SEED)


def ids(case: Case) -> np.ndarray:
    out = po.make_ids(np.random.default_rng(IDS_SEED), case.R, case.T, case.V)
    out[0, case.T - 1] = po.END
    out[1, min(1, case.T - 1)] = po.END
    out[2, 0] = po.END
    out[2, case.T - 1] = po.END
    return out


def input_captions(sample_ids: np.ndarray) -> np.ndarray:
    caps = np.empty_like(sample_ids)
    caps[:, 0] = 1
    caps[:, 1:] = sample_ids[:, :-1]
    return caps


def run_oracle(case: Case, dtype: torch.dtype, gate: bool = False):
    """-> (loss, scores [T*R, V], {param: grad}, dfeats [B, C, 7, 7], logp [R, T], sum_live |A logp| /
    count) as numpy arrays of ``dtype`` (the two scalars Python floats)."""
    from oracle.adaptive_oracle import TrainOracle
    st = dict(state(case))
    if gate:
        st[SENT_H] = np.zeros_like(st[SENT_H])
    oracle = TrainOracle(st, dtype=dtype)
    feats = torch.from_numpy(features(case)).to(dtype).requires_grad_(True)
    sid = torch.from_numpy(ids(case))
    packed = oracle.forward(feats.repeat_interleave(case.N, 0), torch.from_numpy(input_captions(ids(case))),
                            [case.T] * case.R)
    scores = packed[0]
    adv = torch.from_numpy(po.make_advantage(case.R))
    loss, count, logp, _ = po.policy_loss(scores, sid, adv, po.END, 1.0)
    loss.backward()
    mag = float((adv.to(dtype).unsqueeze(1) * logp.detach()).abs().sum() / count)
    grads = {k: v.grad.detach().numpy() for k, v in oracle.w.items() if not (gate and k == SENT_H)}
    return loss.item(), scores.detach().numpy(), grads, feats.grad.detach().numpy(), logp.detach().numpy(), mag


@functools.lru_cache(maxsize=None)
def reference(name: str, dtype: torch.dtype = torch.float64, gate: bool = False):
    return run_oracle(CASES[name], dtype, gate)


@functools.lru_cache(maxsize=None)
def kink_mask(name: str):
    """-> near_a [B, 49, H], near_b [B, E] (bool): tests/train_cases.py's ``_kink`` on this case."""
    case = CASES[name]
    w = state(case)
    A = features(case).astype(np.float64).reshape(case.B, -1, 49).transpose(0, 2, 1)
    a_g = features(case).astype(np.float64).reshape(case.B, -1, 49).mean(axis=2)
    pre_a = A @ w["encoder.affine_a.weight"].astype(np.float64).T + w["encoder.affine_a.bias"].astype(np.float64)
    pre_b = a_g @ w["encoder.affine_b.weight"].astype(np.float64).T + w["encoder.affine_b.bias"].astype(np.float64)
    near_a = np.abs(pre_a) < tc.KINK_REL * np.sqrt(np.mean(pre_a ** 2))
    near_b = np.abs(pre_b) < tc.KINK_REL * np.sqrt(np.mean(pre_b ** 2))
    return near_a, near_b


def tight_entries(name: str, key: str):
    """tests/train_cases.py's ``tight_entries`` for these cases (``"dfeats"`` as [B, C, 49]); None for
    the tensors no ReLU lies upstream of."""
    c = CASES[name]
    near_a, near_b = kink_mask(name)
    C = synth.Dims().channels
    if key in ("encoder.affine_a.weight", "encoder.affine_a.bias"):
        rows = ~near_a.any(axis=(0, 1))
        return np.broadcast_to(rows[:, None], (c.H, C)).copy() if key.endswith("weight") else rows
    if key in ("encoder.affine_b.weight", "encoder.affine_b.bias"):
        rows = ~near_b.any(axis=0)
        return np.broadcast_to(rows[:, None], (c.E, C)).copy() if key.endswith("weight") else rows
    if key == "dfeats":
        ok = ~near_a.any(axis=2) & ~near_b.any(axis=1)[:, None]
        return np.broadcast_to(ok[:, None, :], (c.B, C, 49)).copy()
    return None


def gradient_errors(name: str, grads: Dict[str, np.ndarray], dfeats: np.ndarray, gate: bool = False):
    """-> {tensor: (rel Frobenius, max-entry / max|ref| over the entries the kink mask leaves, max-entry
    / max|ref| over the masked ones)} of float64 arrays against the float64 reference (``gate``: without
    the sentinel's W_h, which that reference does not have)."""
    _, _, rgrads, rdfeats, _, _ = reference(name, torch.float64, gate)
    B = CASES[name].B
    out = {}
    pairs = [(k, np.asarray(g, np.float64), rgrads[k]) for k, g in grads.items() if k in rgrads]
    pairs.append(("dfeats", np.asarray(dfeats, np.float64).reshape(B, -1, 49), rdfeats.reshape(B, -1, 49)))
    for k, g, r in pairs:
        assert g.shape == r.shape, k
        scale = max(np.abs(r).max(), 1e-300)
        tight = tight_entries(name, k)
        if tight is None:
            tight = np.ones(r.shape, bool)
        loose = float(np.abs(g - r)[~tight].max() / scale) if (~tight).any() else 0.0
        rel = float(np.linalg.norm(g[tight] - r[tight]) / max(np.linalg.norm(r[tight]), 1e-300))
        out[k] = (rel, float(np.abs(g - r)[tight].max() / scale), loose)
    return out
