"""Beam-search and sampling cases at every supported hidden size and at small vocabularies, with their
CPU oracles -- TEST INFRASTRUCTURE ONLY (shared by tests/test_decode_cases_cpu.py,
tests/test_gpu_beam_dims.py and tests/test_gpu_sample_dims.py).

Every case goes through the product's own inputs: ``synth.make_weights(weight_seed, Dims(E, H, V))``
with the ``<end>`` (id 2) entry of the output bias raised by ``end_boost`` (test_gpu_beam._weights'
rule), and ``synth.make_features(B, seed=feature_seed)``.

The specifications are ``BeamOracle`` (oracle/adaptive_oracle.py), ``SampleOracle``
(tests/sample_oracle.py) and ``SampleTruncOracle`` (tests/sample_trunc_oracle.py).  Each is run twice
per case, once per process: in fp32, whose selection margin decides whether the case may be used at
all, and in float64 (``dtype=torch.float64`` on ``feats.double()``: the same program text in double),
whose scores the GPU's are compared with.  Callers must not modify what they get.

Admissibility (the rule of test_gpu_beam.py and test_gpu_sample.py, unchanged): a beam case needs an
fp32-oracle selection margin above 4 x SCORE_TOL; a sampling case above 4 x SCORE_TOL x max(1, 1/tau).
The margin written beside each case was measured with the fp32 oracle on the CPU; a margin moves by
a few 1e-6 with the CPU's GEMM blocking, which is why every case keeps well clear of the bar.
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple

import numpy as np
import torch

from adaptive_amd import synth

SCORE_TOL = 5e-5   # test_gpu_beam.py / test_gpu_sample.py
ATT_TOL = 2e-5
MLP_B = "decoder.adaptive.mlp.bias"
SAMPLE_WEIGHT_SEED = 7


class Beam(NamedTuple):
    H: int
    E: int
    V: int
    B: int
    T: int
    K: int
    end_boost: float
    weight_seed: int
    feature_seed: int
    finishes: bool    # the oracle's beams contain <end> (asserted)
    reaches: str

    @property
    def few_granules(self) -> bool:
        """Fewer non-empty 32-column granules than beams: k_beam_select3 runs out of granule maxima."""
        return -(-self.V // 32) < self.K

    @property
    def tile(self) -> int:
        """Fast mode's vocabulary tile: 256 (k_vbeam5) when the vocabulary padded to 128 is whole
        256-column tiles, else 128 (k_vbeam4)."""
        return 256 if (-(-self.V // 128) * 128) % 256 == 0 else 128


class Sample(NamedTuple):
    H: int
    E: int
    V: int
    B: int
    T: int
    tau: float
    seed: int
    N: int            # num_samples
    feature_seed: int
    row0: int
    top_k: int
    top_p: float
    reaches: str

    @property
    def truncated(self) -> bool:
        return self.top_k != 0 or self.top_p != 1.0


# (H, E, V, B, T, K, end_boost, weight seed, feature seed, beams finish, what it reaches)      margin
BEAM: Dict[str, Beam] = {
    # hidden 256: k_lstm<256, gather>, k_atten<1> with kdiv = K, k_vbeam4<256> / k_vbeam5<256>
    "h256_k3":     Beam(256, 256, 3100, 9, 10, 3, 2.0, 7, 0, True, "128-column fast tile"),                   # 1.26e-3
    "h256_ragged": Beam(256, 256, 3100, 67, 6, 3, 2.0, 7, 1, True,
                        "R = 201: a tail in k_lstm's 64-row and k_vbeam4's 128-row tiles"),                   # 4.1e-4
    "h256_k8":     Beam(256, 256, 3001, 9, 10, 8, 2.0, 7, 0, True, "256-column fast tile, K = 8"),            # 9.0e-4
    "h256_k5":     Beam(256, 96, 3100, 6, 8, 5, 2.0, 7, 3, True, "E = 96"),                                   # 9.2e-4
    "h256_k2":     Beam(256, 256, 3001, 6, 8, 2, 2.0, 7, 1, True, "K = 2"),                                   # 1.44e-3
    "h256_v37":    Beam(256, 32, 37, 5, 8, 3, 0.5, 7, 0, True, "2 non-empty granules < K = 3; E = 32"),      # 1.39e-3
    # hidden 768: k_lstm<768, gather>, k_atten<3> with kdiv = K, k_vbeam4<768> / k_vbeam5<768>
    "h768_k5":     Beam(768, 256, 3001, 6, 8, 5, 3.0, 7, 3, True, "256-column fast tile"),                    # 3.5e-3
    "h768_k8":     Beam(768, 96, 3001, 4, 8, 8, 3.0, 7, 1, True, "E = 96, K = 8"),                            # 9.6e-4
    "h768_k3":     Beam(768, 256, 3100, 6, 8, 3, 3.0, 7, 3, True, "128-column fast tile"),                    # 5.4e-3
    "h768_k2":     Beam(768, 256, 3100, 6, 8, 2, 3.0, 7, 2, True, "K = 2"),                                   # 2.9e-3
    "h768_v100":   Beam(768, 96, 100, 5, 8, 8, 2.0, 7, 6, True, "4 non-empty granules < K = 8"),             # 1.31e-3
    # hidden 1024: k_lstm<1024, gather>, k_atten5<1024> with kdiv = K, k_vbeam4<1024> / k_vbeam5<1024>
    "h1024_k3":    Beam(1024, 256, 3001, 5, 6, 3, 3.0, 7, 1, True, "256-column fast tile"),                   # 1.44e-3
    "h1024_k8":    Beam(1024, 256, 3001, 4, 6, 8, 3.0, 7, 1, True, "K = 8"),                                  # 4.3e-4
    "h1024_k2":    Beam(1024, 96, 3100, 4, 6, 2, 3.0, 7, 0, True, "128-column fast tile, E = 96"),            # 6.6e-3
    "h1024_k5":    Beam(1024, 256, 3100, 5, 6, 5, 3.0, 7, 1, True, "K = 5"),                                  # 8.5e-4
    "h1024_v65":   Beam(1024, 96, 65, 4, 6, 4, 1.0, 7, 3, False, "3 non-empty granules < K = 4"),            # 1.03e-3
    # hidden 512, the default vocabulary: k_atten5b<512, 2> and <512, 4>; k_atten5<512> with kdiv = 6, 7
    "h512_k2":     Beam(512, 256, 10123, 3, 6, 2, 2.6, 7, 0, True, "k_atten5b<512, 2>"),                      # 1.64e-2
    "h512_k4":     Beam(512, 256, 10123, 3, 6, 4, 2.6, 7, 0, True, "k_atten5b<512, 4>"),                      # 1.64e-2
    "h512_k6":     Beam(512, 256, 10123, 3, 6, 6, 2.6, 7, 2, True, "k_atten5<512>, kdiv = 6"),                # 6.4e-3
    "h512_k7":     Beam(512, 256, 10123, 3, 6, 7, 2.6, 7, 3, True, "k_atten5<512>, kdiv = 7"),                # 2.4e-3
    "h512_v37":    Beam(512, 256, 37, 5, 8, 3, 1.0, 7, 1, True,
                        "2 non-empty granules < K = 3; k_vbeam4<512>; k_atten5b<512, 3>"),                    # 7.4e-3
}

# (H, E, V, B, T, tau, seed, N, feature seed, row0, top_k, top_p, what it reaches)               margin
SAMPLE: Dict[str, Sample] = {
    "h256_ragged": Sample(256, 256, 3100, 67, 6, 1.0, 0, 1, 3, 0, 0, 1.0, "B = 67: a tail in the 64-row tiles"),      # 1.83e-3
    "h256_n3":     Sample(256, 32, 3001, 5, 6, 1.0, 1, 3, 3, 2, 0, 1.0, "k_atten<1>, kdiv = 3; E = 32; row0 = 2"),   # 1.91e-2
    "h768_tau":    Sample(768, 256, 3001, 20, 6, 0.7, 1, 1, 3, 0, 0, 1.0, "tau = 0.7"),                               # 8.0e-3
    "h768_n3":     Sample(768, 96, 3100, 5, 6, 1.0, 0, 3, 4, 2, 0, 1.0, "k_atten<3>, kdiv = 3; E = 96; row0 = 2"),   # 1.63e-2
    "h1024":       Sample(1024, 256, 3001, 9, 6, 1.0, 2, 1, 3, 0, 0, 1.0, "k_lstm<1024>, k_atten5<1024>"),            # 1.43e-2
    "h1024_v300":  Sample(1024, 256, 300, 9, 6, 2.0, 2, 1, 3, 0, 0, 1.0, "V = 300, tau = 2"),                         # 5.5e-3
    "h1024_n3":    Sample(1024, 256, 3100, 5, 6, 0.7, 2, 3, 4, 2, 0, 1.0, "k_atten5<1024>, kdiv = 3; tau = 0.7"),     # 2.76e-2
    # truncated: every (row, step) robust on the oracle (tests/test_gpu_sample_trunc.py's rule)      smallest lead
    "h768_trunc":  Sample(768, 256, 3001, 6, 6, 1.0, 1, 1, 3, 0, 50, 0.9, "top_k = 50 then top_p = 0.9: kept 44"),       # 4.1e-2
    "h1024_trunc": Sample(1024, 96, 3100, 4, 6, 0.7, 1, 3, 4, 1, 0, 0.8,
                          "top_p = 0.8 with num_samples = 3, row0 = 1: kept 1295..1390"),                              # 5.4e-2
}

SMALL_VOCAB = tuple(k for k, c in BEAM.items() if c.few_granules)


def dims(case) -> synth.Dims:
    return synth.Dims(embed=case.E, hidden=case.H, vocab=case.V)


@functools.lru_cache(maxsize=2)  # both oracles and the GPU model of a case share one generation
def state(case) -> Dict[str, np.ndarray]:
    """The case's state dict (shared: callers must not modify it)."""
    if isinstance(case, Sample):
        return synth.make_weights(SAMPLE_WEIGHT_SEED, dims(case))
    sd = synth.make_weights(case.weight_seed, dims(case))
    if case.end_boost:
        b = sd[MLP_B].copy()
        b[2] = np.float32(b[2] + np.float32(case.end_boost))  # make <end> (id 2) competitive
        sd[MLP_B] = b
    return sd


def features(case) -> np.ndarray:
    return synth.make_features(case.B, seed=case.feature_seed)


def sample_tol(case: Sample) -> float:
    return SCORE_TOL * max(1.0, 1.0 / case.tau)


def run_beam(case: Beam, dtype: torch.dtype):
    """-> ids, alpha, beta, seqs, scores, margin of ``BeamOracle`` in ``dtype``."""
    from oracle.adaptive_oracle import BeamOracle
    feats = torch.from_numpy(features(case)).to(dtype)
    return BeamOracle(state(case), dtype=dtype).beam_search(feats, case.T, case.K, return_margin=True)


def run_sample(case: Sample, dtype: torch.dtype):
    """Plain case -> ids, logp, alpha, beta, margin of ``SampleOracle`` in ``dtype``; the rows are
    those of ``sample(num_samples=N, row0=row0)``: the oracle decodes the features repeated N times
    from global row ``row0 * N``, as ``Encoder2Decoder.sample`` documents.  Truncated case -> the dict
    of ``SampleTruncOracle.sample_trunc`` with the band of ``delta = sample_tol(case)`` and the fp32 y."""
    feats = torch.from_numpy(features(case)).to(dtype)
    if case.truncated:
        from sample_trunc_oracle import SampleTruncOracle
        return SampleTruncOracle(state(case), dtype=dtype).sample_trunc(
            feats, case.T, case.tau, case.seed, row0=case.row0, top_k=case.top_k, top_p=case.top_p,
            num_samples=case.N, delta=sample_tol(case), keep_y=True)
    from sample_oracle import SampleOracle
    return SampleOracle(state(case), dtype=dtype).sample(feats.repeat_interleave(case.N, 0), case.T, case.tau, case.seed,
                                                         row0=case.row0 * case.N, return_margin=True)


@functools.lru_cache(maxsize=None)
def _beam(name: str, double: bool):
    return run_beam(BEAM[name], torch.float64 if double else torch.float32)


@functools.lru_cache(maxsize=None)
def _sample(name: str, double: bool):
    return run_sample(SAMPLE[name], torch.float64 if double else torch.float32)


def beam_oracle(name: str, dtype: torch.dtype = torch.float32):
    """The oracle's result for a beam case id, computed once per process and dtype."""
    return _beam(name, dtype == torch.float64)


def sample_oracle(name: str, dtype: torch.dtype = torch.float32):
    """The oracle's result for a sampling case id, computed once per process and dtype."""
    return _sample(name, dtype == torch.float64)
