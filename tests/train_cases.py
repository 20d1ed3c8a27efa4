"""Training-step cases at every supported model size, their float64 reference and the ReLU kink mask
-- TEST INFRASTRUCTURE ONLY (shared by tests/test_train_cases_cpu.py and tests/test_gpu_train_dims.py).

Every case goes through the product's own inputs: ``synth.make_weights(11, Dims(E, H, V),
bias_noise=0.01)`` (what ``load_synthetic(11, bias_noise=0.01)`` loads), ``synth.make_features(B,
seed=9)`` and captions ``default_rng(5).integers(0, V, (B, T + 2))`` with column 0 = 1 (<start>).

The reference is ``TrainOracle(state, dtype=torch.float64)``: the CPU oracle's program text (pinned to
the reference's own goldens in fp32 by tests/test_oracle.py) evaluated in double.  Each case's
reference is computed once per process and shared; callers must not modify what they get.

The kink mask: V = relu(A W_a^T + b_a) and v_g = relu(a_g W_b^T + b_b).  A pre-activation within fp32
rounding of 0 may land on the other side of the ReLU in an fp32 evaluation; that flips one term of one
row of dW_a / db_a (or dW_b / db_b) and one position of dL/dA.  ``near_a`` / ``near_b`` name exactly the
pre-activations closer to 0 than ``KINK_REL`` times the tensor's RMS, computed in float64, so that
everything else can be held to tight bounds.
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple, Tuple

import numpy as np
import torch

from adaptive_amd import synth

WEIGHT_SEED, BIAS_NOISE, FEAT_SEED, CAPS_SEED = 11, 0.01, 9, 5
KINK_REL = 1e-5
MASK_MAX_SHARE = 0.15  # of any tensor's rows (condition of the tight bounds, asserted on the CPU)


class Case(NamedTuple):
    H: int
    E: int
    V: int
    lengths: Tuple[int, ...]
    T: int        # lengths[0], restated
    total: int    # sum(lengths), restated
    constant_captions: bool
    reaches: str

    @property
    def B(self) -> int:
        return len(self.lengths)


def _ramp(B: int, T: int) -> Tuple[int, ...]:
    return tuple(sorted((max(1, T - i * T // B) for i in range(B)), reverse=True))


CASES: Dict[str, Case] = {
    "A": Case(256, 32, 37, (4, 3, 3, 1, 1), 4, 12, False, "HPT = 1; V < 64, odd; 2E = 64"),
    "B": Case(768, 96, 100, (7,), 7, 7, False, "HPT = 3; B = 1; 2E = 192"),
    "C": Case(1024, 96, 3001, (6,) * 3 + (5,) * 4 + (3,) * 5 + (1,) * 5, 6, 58, False,
              "1024-thread attention workgroup; HPT = 4; second LSTM row block with one live row"),
    "D": Case(256, 32, 37, (1, 1, 1), 1, 3, False, "T = 1: the K = 0 / M = 0 GEMMs"),
    "E": Case(256, 32, 37, _ramp(300, 40), 40, 6160, False,
              "T = 40 > TRA_TS; two step groups in both attention passes; embedding runs of ~300 rows"),
    "F": Case(256, 32, 37, _ramp(100, 7), 7, 403, False, "groups 3,3,1 (forward) and 2,2,2,1 (backward)"),
    "G": Case(256, 32, 37, (4, 3, 3, 1, 1), 4, 12, True, "one embedding run of length R"),
}
BF16_CASES = ("A", "C", "D", "F")


def dims(case: Case) -> synth.Dims:
    return synth.Dims(embed=case.E, hidden=case.H, vocab=case.V)


def state(case: Case) -> Dict[str, np.ndarray]:
    return synth.make_weights(WEIGHT_SEED, dims(case), bias_noise=BIAS_NOISE)


def features(case: Case) -> np.ndarray:
    return synth.make_features(case.B, seed=FEAT_SEED)


def captions(case: Case) -> np.ndarray:
    rng = np.random.default_rng(CAPS_SEED)
    caps = rng.integers(0, case.V, size=(case.B, case.T + 2)).astype(np.int64)
    caps[:, 0] = 1
    if case.constant_captions:
        caps[:] = 1
    return caps


def run_oracle(case: Case, dtype: torch.dtype):
    """-> (loss, packed scores [N, V], {param: grad}, dfeats [B, C, 7, 7]) of ``TrainOracle`` in
    ``dtype``, as numpy arrays of that dtype (loss a Python float)."""
    from oracle.adaptive_oracle import TrainOracle
    oracle = TrainOracle(state(case), dtype=dtype)
    feats = torch.from_numpy(features(case)).to(dtype).requires_grad_(True)
    loss, packed = oracle.loss(feats, torch.from_numpy(captions(case)), list(case.lengths))
    loss.backward()
    grads = {k: v.grad.detach().numpy() for k, v in oracle.w.items()}
    return loss.item(), packed[0].detach().numpy(), grads, feats.grad.detach().numpy()


@functools.lru_cache(maxsize=None)
def _reference(name: str):
    return run_oracle(CASES[name], torch.float64)


def reference(case) -> tuple:
    """The float64 reference of a case (or a case id), computed once per process."""
    name = case if isinstance(case, str) else next(k for k, v in CASES.items() if v is case)
    return _reference(name)


@functools.lru_cache(maxsize=None)
def _kink(name: str):
    case = CASES[name]
    w = state(case)
    A = features(case).astype(np.float64).reshape(case.B, -1, 49).transpose(0, 2, 1)   # [B, 49, C]
    a_g = features(case).astype(np.float64).reshape(case.B, -1, 49).mean(axis=2)         # [B, C]
    pre_a = A @ w["encoder.affine_a.weight"].astype(np.float64).T + w["encoder.affine_a.bias"].astype(np.float64)
    pre_b = a_g @ w["encoder.affine_b.weight"].astype(np.float64).T + w["encoder.affine_b.bias"].astype(np.float64)
    near_a = np.abs(pre_a) < KINK_REL * np.sqrt(np.mean(pre_a ** 2))
    near_b = np.abs(pre_b) < KINK_REL * np.sqrt(np.mean(pre_b ** 2))
    return near_a, near_b


def kink_mask(case):
    """-> near_a [B, 49, H], near_b [B, E] (bool)."""
    name = case if isinstance(case, str) else next(k for k, v in CASES.items() if v is case)
    return _kink(name)


def tight_entries(case, name: str) -> np.ndarray:
    """Bool mask, shaped like gradient ``name`` (a parameter key, or ``"dfeats"`` as [B, C, 49]), of
    the entries no near-kink pre-activation can reach; None for the tensors no ReLU lies upstream of (every entry is tight)."""
    c = CASES[case] if isinstance(case, str) else case
    near_a, near_b = kink_mask(case)
    C = synth.Dims().channels
    if name in ("encoder.affine_a.weight", "encoder.affine_a.bias"):
        rows = ~near_a.any(axis=(0, 1))                                  # [H]
        return np.broadcast_to(rows[:, None], (c.H, C)).copy() if name.endswith("weight") else rows
    if name in ("encoder.affine_b.weight", "encoder.affine_b.bias"):
        rows = ~near_b.any(axis=0)                                       # [E]
        return np.broadcast_to(rows[:, None], (c.E, C)).copy() if name.endswith("weight") else rows
    if name == "dfeats":
        ok = ~near_a.any(axis=2) & ~near_b.any(axis=1)[:, None]          # [B, 49]
        return np.broadcast_to(ok[:, None, :], (c.B, C, 49)).copy()
    return None
