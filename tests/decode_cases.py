"""Beam-search, sampling and greedy cases at every supported hidden size and at small vocabularies, with
their CPU oracles -- TEST INFRASTRUCTURE ONLY (shared by tests/test_decode_cases_cpu.py,
tests/test_gpu_beam_dims.py, tests/test_gpu_sample_dims.py and tests/test_gpu_greedy_dims.py).

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

``bias_shift`` is added to every entry of the output bias.  A shift below minus the largest logit makes
every logit of every row and step negative: the screen's order-preserving keys then carry their granule
position in the low bits of a negative value, and the padding columns V .. Vp-1 (zero weights, logit 0
if one were ever left unmasked) would beat every real column.

Greedy cases (``GREEDY``; the specification is ``OracleModel.sampler``).  Admissibility: the fp32
oracle's smallest top-1 / top-2 logit gap over all (row, step) exceeds 4 x SCORE_TOL.  A *plain* case
is synthetic weights at a batch that fills the kernels' row tiles.  An *adversarial* case replaces a few
columns of the vocabulary projection by near-ties built against the oracle's step-0 ``u`` (the
projection's input, which does not depend on the projection): see ``adversarial_vocab``.  In such a
case the bf16 products the vocabulary screen computes rank a decoy above the true winner by most of the
screen bound's w-term, so a screen whose bound lacks that term, or carries it materially too small,
drops the winner (``screen_candidates`` is the numpy emulation that shows it on the CPU).

What the adversarial cases do not reach: the ``||du|| W_g`` term of the bound (``u`` is the model's to
compute, not the test's to place, so ``u - bf16(u)`` cannot be lined up against a column), and
``SC_ACC(H)``, which is about forty times smaller than the w-term and cannot be isolated end to end.
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from adaptive_amd import synth

SCORE_TOL = 5e-5   # test_gpu_beam.py / test_gpu_sample.py
ATT_TOL = 2e-5
MLP_B = "decoder.adaptive.mlp.bias"
MLP_W = "decoder.adaptive.mlp.weight"
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
    bias_shift: float = 0.0

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
    bias_shift: float = 0.0

    @property
    def truncated(self) -> bool:
        return self.top_k != 0 or self.top_p != 1.0


class Adversarial(NamedTuple):
    """Near-tie columns for the first ``len(groups)`` rows: group i = (winner, decoy[, second decoy])
    column ids of row i (``adversarial_vocab``)."""
    groups: tuple
    scale: float = 3.0    # ||w|| of a designed column
    share: float = 0.15   # of the elements on which the winner shares the decoy's bf16 value
    seed: int = 0


class Greedy(NamedTuple):
    H: int
    E: int
    V: int
    B: int
    T: int
    weight_seed: int
    feature_seed: int
    bias_shift: float
    adversarial: Optional[Adversarial]
    reaches: str

    @property
    def wide(self) -> bool:
        """The 128 x 160 screen (k_vscreen8 / k_vscreen2): the vocabulary padded to 128 is whole
        160-column tiles and H <= 512; else the 64 x 64 k_vscreen."""
        return (-(-self.V // 128) * 128) % 160 == 0 and self.H <= 512

    @property
    def tile(self) -> int:
        return 160 if self.wide else 64

    @property
    def negative(self) -> bool:
        return self.bias_shift < 0


def placements(V: int, tile: int) -> tuple:
    """Column ids of seven designed rows, (winner, decoys...), where the screen's indexing could go
    wrong: column 0; column V - 1 (beside the padding when V is no multiple of 32); pairs inside one
    32-column granule, in two granules of one ``tile``-column tile, and in two tiles (two workgroups,
    whose summaries meet only in the rescoring); one triple inside one granule.  Of the six pairs
    three have the decoy at the lower index and three at the higher, so a first-index rule cannot
    rescue a screen that kept only the decoy."""
    last, nt = (V - 1) // 32 * 32, V // tile
    assert V - 1 > last and nt >= 9
    return ((0, 9),                                        # one granule; winner at column 0; decoy higher
            (V - 1, last),                                 # one granule; winner at column V - 1; decoy lower
            (tile + 40, tile + 3),                         # two granules of tile 1; decoy lower
            (2 * tile + 5, 2 * tile + 60),                 # two granules of tile 2; decoy higher
            (3 * tile + 7, (nt // 2) * tile + 50),         # two tiles; decoy higher
            ((nt - 2) * tile + 33, 5 * tile + 1),          # two tiles; decoy lower
            (7 * tile + 52, 7 * tile + 34, 7 * tile + 61))  # a triple in one granule, decoys on both sides


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
    # every logit negative (bias_shift = -16), 71 padding columns behind V = 3001
    "h768_neg":    Beam(768, 96, 3001, 4, 6, 3, 3.0, 7, 1, True, "negative logits beside padding columns", -16.0),  # 1.03e-2
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
    # every logit negative (bias_shift = -16), 71 padding columns behind V = 3001
    "h256_neg":    Sample(256, 32, 3001, 5, 6, 1.0, 0, 1, 3, 0, 0, 1.0, "negative logits beside padding columns", -16.0),  # 4.9e-2
    # truncated: every (row, step) robust on the oracle (tests/test_gpu_sample_trunc.py's rule)      smallest lead
    "h768_trunc":  Sample(768, 256, 3001, 6, 6, 1.0, 1, 1, 3, 0, 50, 0.9, "top_k = 50 then top_p = 0.9: kept 44"),       # 4.1e-2
    "h1024_trunc": Sample(1024, 96, 3100, 4, 6, 0.7, 1, 3, 4, 1, 0, 0.8,
                          "top_p = 0.8 with num_samples = 3, row0 = 1: kept 1295..1390"),                              # 5.4e-2
}


def _adv(V: int, tile: int, **kw) -> Adversarial:
    return Adversarial(placements(V, tile), **kw)


# (H, E, V, B, T, weight seed, feature seed, bias shift, adversarial columns, what it reaches)       smallest gap
GREEDY: Dict[str, Greedy] = {
    # plain: synthetic weights, the smallest batches that fill the row tiles
    "h256_wide":     Greedy(256, 32, 3200, 131, 4, 7, 7, 0.0, None,
                            "k_vscreen8<256>: a 128-row tile and a tail of 3; k_lstm<256>: two 64-row tiles "
                            "and a tail; E = 32"),                                                              # 8.8e-4
    "h256_narrow":   Greedy(256, 256, 3001, 67, 4, 7, 8, 0.0, None, "k_vscreen<256>: a 64-row tile and a tail"),  # 2.2e-3
    "h768":          Greedy(768, 96, 3001, 67, 4, 7, 2, 0.0, None, "k_vscreen<768>, k_lstm<768>: a tail; E = 96"),  # 6.1e-4
    "h1024":         Greedy(1024, 256, 3100, 67, 4, 7, 3, 0.0, None, "k_vscreen<1024>, k_lstm<1024>: a tail"),   # 5.1e-3
    "h512_narrow":   Greedy(512, 256, 3001, 67, 4, 7, 4, 0.0, None, "k_vscreen<512>: the 64 x 64 screen at 512"),  # 1.16e-3
    "h256_v100_neg": Greedy(256, 32, 100, 9, 4, 7, 5, -16.0, None,
                            "every logit negative; 28 padding columns behind V = 100; E = 32"),                 # 4.2e-3
    # adversarial: T = 1 is rescored by k_vrescore, T = 2 by the rescoring fused into step 1's k_lstm
    "h256_wide_adv":   Greedy(256, 256, 3200, 7, 1, 7, 0, 0.0, _adv(3200, 160, seed=1),
                              "k_vscreen8<256> (k_vscreen2<256>) + k_vrescore<256>"),                           # 4.2e-3
    "h256_narrow_adv": Greedy(256, 256, 3001, 7, 2, 7, 1, 0.0, _adv(3001, 64, seed=2),
                              "k_vscreen<256> + k_lstm<256, RS>"),                                              # 4.4e-3
    "h512_adv":        Greedy(512, 256, 10123, 7, 2, 7, 2, 0.0, _adv(10123, 160, seed=3),
                              "k_vscreen8<512> (k_vscreen2<512>) + k_lstm<512, RS>: the product's own screen"),  # 9.1e-3
    "h768_adv":        Greedy(768, 256, 3001, 7, 1, 7, 3, 0.0, _adv(3001, 64, seed=4),
                              "k_vscreen<768> + k_vrescore<768>"),                                              # 1.18e-2
    "h1024_adv":       Greedy(1024, 96, 3100, 7, 2, 7, 4, 0.0, _adv(3100, 64, seed=5),
                              "k_vscreen<1024> + k_lstm<1024, RS>; E = 96"),                                    # 1.23e-2
    "h768_adv_neg":    Greedy(768, 96, 3001, 7, 2, 7, 5, -64.0, _adv(3001, 64, seed=6),
                              "every logit negative; the winner of row 1 at column V - 1 beside 71 padding columns"),  # 1.32e-2
}

SMALL_VOCAB = tuple(k for k, c in BEAM.items() if c.few_granules)


def dims(case) -> synth.Dims:
    return synth.Dims(embed=case.E, hidden=case.H, vocab=case.V)


@functools.lru_cache(maxsize=2)  # both oracles and the GPU model of a case share one generation
def state(case) -> Dict[str, np.ndarray]:
    """The case's state dict (shared: callers must not modify it)."""
    sd = synth.make_weights(SAMPLE_WEIGHT_SEED if isinstance(case, Sample) else case.weight_seed, dims(case))
    if isinstance(case, Beam) and case.end_boost:
        b = sd[MLP_B].copy()
        b[2] = np.float32(b[2] + np.float32(case.end_boost))  # make <end> (id 2) competitive
        sd[MLP_B] = b
    if case.bias_shift:
        sd[MLP_B] = sd[MLP_B] + np.float32(case.bias_shift)
    if isinstance(case, Greedy) and case.adversarial:
        # step 0's u = c_hat + h does not depend on the vocabulary projection: take it from the float64
        # oracle on the synthetic weights, then replace the designed columns
        u0 = _greedy_run(sd, features(case)[:len(case.adversarial.groups)], 1, torch.float64)["u"][:, 0].numpy()
        cols, rows, _ = adversarial_vocab(u0, case.adversarial, case.V)
        w = sd[MLP_W].copy()
        w[cols] = rows
        sd[MLP_W] = w
    return sd


def bf16(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest, ties to even) -> fp32, in numpy."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def adversarial_vocab(u0: np.ndarray, spec: Adversarial, V: int):
    """-> (column ids [n], their fp32 weight rows [n, H], designed), designed = one (row, winner, decoys)
    per group of ``spec``: near-tie vocabulary columns against rows 0 .. len(groups)-1 of ``u0`` [B, H].

    For row b take v = scale x u_b / ||u_b||, so that b's own columns lead every other row's (rows'
    u have cosine ~0.99).  Per element k: m_k the bf16 rounding midpoint next to |v_k| (between the two
    neighbouring bf16 values), ulp_k their distance, s_k = sign(u_k).  With d = ulp_k / 256:

      decoy        w_k = s_k (m_k + d) everywhere: every element rounds away from zero in bf16, every
                   product gains |u_k| ulp_k / 2.
      winner       on the k whose pseudo-random r_k < ``share``, w_k = s_k (m_k + ulp_k / 2 - d): the same
                   bf16 value as the decoy's, but really larger by almost ulp_k / 2; elsewhere
                   w_k = s_k (m_k - d): rounds toward zero.
      second decoy (a triple) as the decoy where r_k < ``share`` + 0.1, as the winner's "elsewhere" on
                   the rest: its true logit is just below the decoy's, and in bf16 it trails the decoy by
                   too much for a bound without the w-term to expand the granule, yet leads the winner,
                   which so ranks third in the granule.

    In exact arithmetic the winner leads by ~ share x sum |u_k| ulp_k / 2; in bf16 products the decoy
    leads by ~ (1 - share) x sum |u_k| ulp_k.  Every value is exact in fp32 (17 significant bits)."""
    cols, rows, designed = [], [], []
    for b, group in enumerate(spec.groups):
        assert all(0 <= n < V for n in group) and len(set(group)) == len(group)
        u = np.asarray(u0[b], np.float64)
        a = np.abs(u) * (spec.scale / np.linalg.norm(u))
        a = np.maximum(a, 2.0 ** -60)
        ulp = np.exp2(np.frexp(a)[1] - 1 - 7)           # bf16: 8 significant bits
        mid = np.floor(a / ulp) * ulp + ulp / 2
        s = np.where(u < 0, -1.0, 1.0)
        d = ulp / 256
        H = u.size
        r = synth.uniform24(synth.stream_key(spec.seed, f"adversarial.{b}"), 0, H)
        w = [s * np.where(r < spec.share, mid + ulp / 2 - d, mid - d), s * (mid + d),
             s * np.where(r < spec.share + 0.1, mid + d, mid - d)]
        for n, x in zip(group, w):
            x32 = x.astype(np.float32)
            assert np.array_equal(x32.astype(np.float64), x)
            cols.append(n)
            rows.append(x32)
        designed.append((b, group[0], tuple(group[1:])))
    assert len(set(cols)) == len(cols)
    return np.asarray(cols), np.stack(rows), tuple(designed)


def designed(case: Greedy) -> tuple:
    """(row, winner, decoys) of an adversarial case's designed rows."""
    return tuple((b, g[0], tuple(g[1:])) for b, g in enumerate(case.adversarial.groups))


# aa_kernels.hip's screen_bound and the factors its operands are inflated by at their source
SC_BF, EPS_ABS, NORM_INFLATE = 1.005, 1e-5, 1.0001


def sc_acc(H: int) -> float:
    return max(1.1 * (H + H // 8 + 8) * 2.0 ** -24, 5e-5)


def screen_candidates(u: np.ndarray, W: np.ndarray, b: np.ndarray, with_D: bool = True, scale: float = 1.0) -> np.ndarray:
    """numpy emulation (float64 arithmetic) of the vocabulary screen's summaries and the rescoring's
    candidate rule for fp32 rows ``u`` [R, H] -> bool [R, V], the columns that get an exact logit.
    Per (row, 32-column granule): the two largest screened logits A = bf16(u) . bf16(w) + b, and the
    bound E = ``scale`` x screen_bound (aa_kernels.hip; ``with_D=False`` leaves out ||u|| D_g).  With
    M = max over granules of (A1 - E): a granule whose A2 + E >= M contributes all of its columns, else
    one whose A1 + E >= M its arg-max column (rescore_row, aa_lstm.hpp)."""
    G = 32
    R, H = u.shape
    V = W.shape[0]
    Vp = -(-V // G) * G
    ub, wb = bf16(u).astype(np.float64), bf16(W).astype(np.float64)
    u, W, b = u.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    A = np.full((R, Vp), -np.inf)
    A[:, :V] = ub @ wb.T + b

    def per_granule(x):
        return np.concatenate([x, np.zeros(Vp - V)]).reshape(-1, G).max(1)
    Wg = per_granule(np.linalg.norm(W, axis=1)) * NORM_INFLATE
    Dg = per_granule(np.linalg.norm(W - wb, axis=1)) * NORM_INFLATE
    Bg = per_granule(np.abs(b))
    un = np.linalg.norm(u, axis=1)[:, None] * NORM_INFLATE
    dun = np.linalg.norm(u - ub, axis=1)[:, None] * NORM_INFLATE
    E = scale * (SC_BF * (dun * Wg + (un * Dg if with_D else 0.0)) + sc_acc(H) * un * Wg + EPS_ABS * (un * Wg + Bg))
    Ag = A.reshape(R, -1, G)
    top = -np.sort(-Ag, axis=2)[:, :, :2]
    M = (top[:, :, 0] - E).max(1, keepdims=True)
    whole = top[:, :, 1] + E >= M
    one = (top[:, :, 0] + E >= M) & ~whole
    keep = np.repeat(whole, G, axis=1)
    r, g = np.nonzero(one)
    keep[r, g * G + Ag[r, g].argmax(1)] = True
    return keep[:, :V]


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


def _greedy_run(sd: Dict[str, np.ndarray], feats: np.ndarray, T: int, dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """``OracleModel.sampler`` in ``dtype`` -> ids [B,T], alpha, beta, u [B,T,H] (the vocabulary
    projection's input c_hat + h, taken where ``Atten.forward`` returns), and per (row, step) the
    largest logit ``top`` and its lead over the second largest ``gap``."""
    from oracle.adaptive_oracle import OracleModel
    m = OracleModel(sd, dtype=dtype)
    us, inner = [], m.atten

    def atten(V, h_t, s_t):
        c_hat, a, b = inner(V, h_t, s_t)
        us.append((c_hat + h_t).clone())
        return c_hat, a, b
    m.atten = atten
    ids, al, be, scores = m.sampler(torch.from_numpy(np.ascontiguousarray(feats)).to(dtype), max_len=T, keep_scores=True)
    k = min(2, scores.shape[-1])
    t2 = scores.topk(k, dim=-1).values
    return {"ids": ids, "alpha": al, "beta": be, "u": torch.cat(us, dim=1), "top": t2[..., 0], "gap": t2[..., 0] - t2[..., -1]}


def run_greedy(case: Greedy, dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    return _greedy_run(state(case), features(case), case.T, dtype)


@functools.lru_cache(maxsize=None)
def _greedy(name: str, double: bool):
    return run_greedy(GREEDY[name], torch.float64 if double else torch.float32)


def greedy_oracle(name: str, dtype: torch.dtype = torch.float32) -> Dict[str, torch.Tensor]:
    """The oracle's result for a greedy case id, computed once per process and dtype."""
    return _greedy(name, dtype == torch.float64)


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
