"""Cases of the diverse-group beam search with a length-normalised final ranking -- TEST INFRASTRUCTURE
ONLY (shared by tests/test_beam_div_cpu.py and tests/test_gpu_beam_div.py).

A case is a ``decode_cases.BEAM`` entry (its weights, features, B, T, K) with (groups G, diversity,
length_penalty).  The specification is ``BeamDivOracle`` (tests/beam_div_oracle.py), run once per process
in fp32, whose margins decide whether the case may be used at all, and once in float64, whose scores the
GPU's are compared with.  Callers must not modify what they get.

Admissibility (asserted on the CPU in tests/test_beam_div_cpu.py): both margins of the fp32 oracle --
selection (consecutive augmented scores among each group's Kg + 1 best) and rank (consecutive final
ranks) -- exceed 4 x SCORE_TOL = 2e-4, so a score error of SCORE_TOL on either side of a comparison
cannot change its outcome twice over; the fp32 and float64 oracles agree on seqs, lengths and group; and
``<end>`` occurs exactly where the base case says beams finish.  The margins beside each case were
measured with the fp32 oracle on the CPU.

Not admissible (kept out, and asserted so): ``h256_k8`` at diversity 0.5 (two groups converge on one
sequence: the rank gap is exactly 0) and ``h768_v100`` at G = 4, diversity 2, length_penalty 1 (selection
margin 1.4e-4).

At diversity 2.0 no penalised token is ever chosen in these cases (the penalty only excludes); at 0.5
several are (``penalised``: the oracle's count, asserted, so the table keeps cases in which a penalised
candidate really wins on its augmented score beside cases in which the penalty only excludes).
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple

import torch

import decode_cases as dc
from beam_div_oracle import BeamDivOracle

MARGIN = 4 * dc.SCORE_TOL


class Div(NamedTuple):
    base: str            # decode_cases.BEAM key
    G: int
    diversity: float
    length_penalty: float
    penalised: int       # survivors chosen although their token carried a penalty (the fp32 oracle's count)
    reaches: str

    @property
    def beam(self) -> dc.Beam:
        return dc.BEAM[self.base]

    @property
    def Kg(self) -> int:
        return self.beam.K // self.G


#                        base        G  diversity  length_penalty                          selection / rank margin
DIV: Dict[str, Div] = {
    "h256_k8":     Div("h256_k8", 4, 2.0, 1.0, 0, "k_atten<1>; Kg = 2; the near-limit case"),             # 2.1e-4 / 4.5e-4
    "h256_ragged": Div("h256_ragged", 3, 0.5, 0.7, 21,
                       "Kg = 1; B = 67 crosses the 64-row boundary; penalised tokens still chosen"),      # 2.7e-4 / 2.5e-3
    "h256_v37":    Div("h256_v37", 3, 0.5, 0.7, 0, "2 non-empty granules < K"),                           # 1.4e-3 / 0.13
    "h768_k8":     Div("h768_k8", 4, 0.5, 0.0, 3, "Kg = 2; no length penalty"),                           # 8.8e-4 / 8.8e-4
    "h768_v100":   Div("h768_v100", 8, 0.5, 0.7, 41, "G = K = 8; 4 granules < K; many penalised picks"),   # 2.6e-4 / 1.3e-2
    "h768_neg":    Div("h768_neg", 3, 2.0, 1.0, 0, "every logit negative beside padding"),                # 9.6e-4 / 1.1e-2
    "h1024_k8":    Div("h1024_k8", 2, 0.5, 0.7, 10, "Kg = 4; penalised picks"),                            # 1.1e-3 / 7.1e-3
    "h1024_v65":   Div("h1024_v65", 2, 0.5, 0.0, 4, "no beam finishes: len = T"),                         # 2.7e-3 / 4.9e-3
    "h512_k4":     Div("h512_k4", 2, 0.5, 0.7, 2, "k_atten5b<512, 4>"),                                   # 3.3e-3 / 2.1e-2
    "h512_k6":     Div("h512_k6", 3, 0.5, 0.7, 13, "k_atten5<512>, kdiv = 6; penalised picks"),            # 7.1e-4 / 3.4e-2
}

# what the admissibility rule keeps out (tests/test_beam_div_cpu.py asserts that it does)
INADMISSIBLE: Dict[str, Div] = {
    "h256_k8_l05":   Div("h256_k8", 4, 0.5, 1.0, 0, "two groups converge: rank gap 0"),
    "h768_v100_g4":  Div("h768_v100", 4, 2.0, 1.0, 0, "selection margin 1.4e-4"),
}


def run(case: Div, dtype: torch.dtype) -> Dict[str, object]:
    b = case.beam
    feats = torch.from_numpy(dc.features(b)).to(dtype)
    return BeamDivOracle(dc.state(b), dtype=dtype).beam_search_div(
        feats, b.T, b.K, groups=case.G, diversity=case.diversity, length_penalty=case.length_penalty)


@functools.lru_cache(maxsize=None)
def _oracle(name: str, double: bool):
    return run(DIV[name], torch.float64 if double else torch.float32)


def oracle(name: str, dtype: torch.dtype = torch.float32) -> Dict[str, object]:
    """The oracle's result for a case id, computed once per process and dtype."""
    return _oracle(name, dtype == torch.float64)


def kwargs(case: Div) -> Dict[str, object]:
    return {"groups": case.G, "diversity": case.diversity, "length_penalty": case.length_penalty}
