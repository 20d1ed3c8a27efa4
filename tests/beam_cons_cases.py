"""Cases of the constrained beam search (suppressed tokens, minimum length, no repeated n-grams, no
``<end>`` after given tokens) -- TEST INFRASTRUCTURE ONLY (shared by tests/test_beam_cons_cpu.py and
tests/test_gpu_beam_cons.py).

A case is a ``decode_cases.BEAM`` entry (its weights, features, B, T, K) with (groups G, diversity,
length_penalty) and the four constraints.  The specification is ``BeamConsOracle``
(tests/beam_cons_oracle.py), run once per process in fp32, whose margins decide whether the case may be used
at all, and once in float64, whose scores the GPU's are compared with.  Callers must not modify what they get.

``suppress_ids`` / ``no_end_after`` are the most frequent non-``<end>`` tokens of the base case's
unconstrained beams, so the constraints bind: ``blocked`` is the oracle's count, per kind (suppress,
min_length, no_end_after, ngram), of forbidden candidates that stood in the unmasked top Kg of their group
(asserted equal, so the table keeps showing that every kind of constraint changes a selection somewhere).

Admissibility (asserted on the CPU in tests/test_beam_cons_cpu.py): both margins of the fp32 oracle --
selection and rank -- exceed 4 x SCORE_TOL = 2e-4, and the fp32 and float64 oracles agree on seqs, lengths
and group.  The margins beside each case were measured with the fp32 oracle on the CPU.

Not admissible (kept out, and asserted so): ``h256_ragged`` at G = 3, 0.5, 0.7 with min_length 4, n = 2
(selection margin 8.6e-6) and ``h768_k5`` at length_penalty 0.7, min_length 5, n = 2 with two suppressed
tokens (selection margin 3.8e-6).
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple, Tuple

import torch

import decode_cases as dc
from beam_cons_oracle import KINDS, BeamConsOracle

MARGIN = 4 * dc.SCORE_TOL


class Cons(NamedTuple):
    base: str            # decode_cases.BEAM key
    G: int
    diversity: float
    length_penalty: float
    min_length: int
    ngram: int
    suppress: Tuple[int, ...]
    no_end_after: Tuple[int, ...]
    blocked: Tuple[int, int, int, int]   # the fp32 oracle's counts, in the order of KINDS
    reaches: str

    @property
    def beam(self) -> dc.Beam:
        return dc.BEAM[self.base]

    @property
    def Kg(self) -> int:
        return self.beam.K // self.G


#                          base       G  div  lp  min n  suppress  no_end_after  blocked          selection / rank margin
CONS: Dict[str, Cons] = {
    "h256_k3":      Cons("h256_k3", 1, 0.0, 0.0, 0, 1, (1587,), (), (9, 0, 0, 0), "n = 1: no token twice"),   # 5.8e-3 / 0.14
    "h256_ragged":  Cons("h256_ragged", 3, 0.5, 0.7, 0, 2, (1587,), (1006,), (191, 0, 69, 5),   # 1.6e-3 / 0.20
                         "B = 67; Kg = 1 groups with diversity and a length penalty"),
    "h256_v37":     Cons("h256_v37", 1, 0.0, 0.0, 5, 1, (16, 18), (1,), (31, 36, 4, 6),   # 6.2e-4 / 7.4e-3
                         "V = 37: 2 granules < K; no <end> right after <start>"),
    "h256_v37_all": Cons("h256_v37", 3, 0.5, 0.7, 8, 2, (16,), (), (44, 67, 0, 3), "min_length = T: no beam finishes"),   # 3.2e-4 / 2.0e-3
    "h768_k8":      Cons("h768_k8", 4, 0.5, 0.0, 3, 2, (529,), (1622,), (103, 23, 12, 13), "K = 8 in 4 groups"),   # 2.6e-4 / 4.9e-3
    "h768_k5":      Cons("h768_k5", 1, 0.0, 0.0, 0, 3, (1622,), (), (35, 0, 0, 2), "n = 3"),   # 8.3e-4 / 6.5e-2
    "h768_neg":     Cons("h768_neg", 1, 0.0, 1.0, 4, 2, (529,), (1622,), (12, 12, 17, 14), "every logit negative"),   # 5.5e-4 / 7.8e-3
    "h1024_k8":     Cons("h1024_k8", 2, 0.5, 0.7, 3, 1, (2557,), (), (98, 13, 0, 23), "Kg = 4, n = 1"),   # 4.0e-4 / 5.6e-3
    "h1024_v65":    Cons("h1024_v65", 1, 0.0, 0.0, 3, 2, (53,), (63,), (72, 0, 0, 5), "V = 65: 3 granules < K"),   # 3.5e-4 / 1.6e-3
    "h512_k2":      Cons("h512_k2", 1, 0.0, 0.0, 3, 2, (7136,), (), (32, 3, 0, 1), "the default vocabulary, K = 2"),   # 1.3e-3 / 2.1e-3
    "h512_k4":      Cons("h512_k4", 2, 0.5, 0.7, 4, 1, (7136,), (1283,), (59, 8, 1, 3), "the default vocabulary, grouped"),   # 2.4e-3 / 8.4e-4
    "h512_k6":      Cons("h512_k6", 1, 0.0, 0.0, 3, 3, (), (7136,), (0, 6, 3, 16), "no suppressed token; n = 3"),   # 2.6e-3 / 2.2e-2
    "h512_v37":     Cons("h512_v37", 1, 0.0, 0.0, 4, 2, (30,), (15,), (18, 5, 0, 49), "V = 37 at hidden 512"),   # 1.6e-3 / 7.7e-3
}

# what the admissibility rule keeps out (tests/test_beam_cons_cpu.py asserts that it does)
INADMISSIBLE: Dict[str, Cons] = {
    "h256_ragged_min4": Cons("h256_ragged", 3, 0.5, 0.7, 4, 2, (), (), (0, 0, 0, 0), "selection margin 8.6e-6"),
    "h768_k5_two":      Cons("h768_k5", 1, 0.0, 0.7, 5, 2, (1622, 529), (), (0, 0, 0, 0), "selection margin 3.8e-6"),
}


def kwargs(case: Cons) -> Dict[str, object]:
    return {"groups": case.G, "diversity": case.diversity, "length_penalty": case.length_penalty,
            "suppress_ids": case.suppress, "min_length": case.min_length, "no_repeat_ngram": case.ngram,
            "no_end_after": case.no_end_after}


def run(case: Cons, dtype: torch.dtype) -> Dict[str, object]:
    b = case.beam
    feats = torch.from_numpy(dc.features(b)).to(dtype)
    return BeamConsOracle(dc.state(b), dtype=dtype).beam_search_cons(feats, b.T, b.K, **kwargs(case))


@functools.lru_cache(maxsize=None)
def _oracle(name: str, double: bool):
    return run(CONS[name], torch.float64 if double else torch.float32)


def oracle(name: str, dtype: torch.dtype = torch.float32) -> Dict[str, object]:
    """The oracle's result for a case id, computed once per process and dtype."""
    return _oracle(name, dtype == torch.float64)


def blocked(o: Dict[str, object]) -> Tuple[int, ...]:
    return tuple(o["blocked"][k] for k in KINDS)
