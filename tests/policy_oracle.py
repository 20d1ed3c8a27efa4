"""The policy-gradient (self-critical) loss restated in float64 torch ops -- TEST INFRASTRUCTURE ONLY
(the reference of tests/test_policy_cpu.py and tests/test_gpu_policy.py for aa_policy_loss_* /
adaptive_amd.optim.policy_gradient_loss; semantics in include/adaptive_amd.h).

``scores`` [T*R, V], t-major (row ``t*R + r``); ``ids`` [R, T]; ``advantage`` [R].  A position is live
when no ``end_id`` occurs before it in its caption; ``logp = log_softmax(scores / temperature)[id]``;
``loss = -(sum_live A_r logp) / #live``.  Gradients come from autograd.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

END = 2


def live_mask(ids: torch.Tensor, end_id: int = END) -> torch.Tensor:
    """[R, T] bool: no ``end_id`` among the caption's earlier tokens (``end_id < 0``: all live)."""
    if end_id < 0:
        return torch.ones_like(ids, dtype=torch.bool)
    ended = (ids == end_id).to(torch.int64).cumsum(1)          # ends up to and including t
    return (ended - (ids == end_id).to(torch.int64)) == 0      # ends strictly before t


def policy_loss(scores: torch.Tensor, ids: torch.Tensor, advantage: torch.Tensor, end_id: int = END,
                temperature: float = 1.0):
    """-> (loss, count, logp [R, T] with 0 at dead positions, live [R, T]) in ``scores``' dtype;
    differentiable in ``scores``."""
    R, T = ids.shape
    V = scores.size(1)
    live = live_mask(ids, end_id)
    # the kernel divides by the fp32 temperature
    tau = float(np.float32(temperature))
    lsm = F.log_softmax(scores / tau, dim=1).view(T, R, V).transpose(0, 1)               # [R, T, V]
    safe = torch.where(live, ids, torch.zeros_like(ids))                                  # dead ids are not looked at
    logp = lsm.gather(2, safe.unsqueeze(2)).squeeze(2)
    logp = torch.where(live, logp, torch.zeros_like(logp))
    count = live.sum()
    loss = -(advantage.to(scores.dtype).unsqueeze(1) * logp).sum() / count
    return loss, count, logp, live


def make_ids(rng: np.random.Generator, R: int, T: int, V: int) -> np.ndarray:
    """[R, T] ids in [3, V) (or 0 where the vocabulary has no such token), no ``<end>`` yet."""
    if V > 3:
        return rng.integers(3, V, size=(R, T)).astype(np.int64)
    return np.zeros((R, T), dtype=np.int64)


def make_advantage(R: int) -> np.ndarray:
    """default_rng(7).normal(0.3, 1.0, R), float64, with two rows exactly 0: rows 3 and R - 1 (beside
    the rows ``place_ends`` writes to), rows 1 and R - 1 when R < 5; R < 3 has no two rows to spare:
    row 0 alone."""
    a = np.random.default_rng(7).normal(0.3, 1.0, R)
    if R >= 3:
        a[3 if R >= 5 else 1] = a[R - 1] = 0.0
    else:
        a[0] = 0.0
    return a


def place_ends(ids: np.ndarray, V: int) -> np.ndarray:
    """``<end>`` = 2 placed by hand, in place: row 0 at position 0, row 1 at position T - 1, row 2 twice
    (positions 1 and T - 1; 0 and T - 1 when T == 2); the remaining rows have none.  Nothing is placed
    when the vocabulary has no token 2."""
    R, T = ids.shape
    if V <= END:
        return ids
    ids[0, 0] = END
    if R > 1:
        ids[1, T - 1] = END
    if R > 2 and T >= 2:
        ids[2, 1 if T >= 3 else 0] = END
        ids[2, T - 1] = END
    return ids
