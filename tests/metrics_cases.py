"""Inputs shared by the BLEU / ROUGE-L tests: the golden corpus and an edge batch."""
import numpy as np

from conftest import load_golden

END = 2


def golden_cases():
    """(refs, hyps [M, 20] int64, end_id, the golden's other arrays as a dict)."""
    z = load_golden("metrics_eval")
    caps = np.split(z["ref_tokens"].astype(np.int64), np.cumsum(z["ref_lengths"])[:-1])
    it = iter(caps)
    refs = [[next(it).tolist() for _ in range(k)] for k in z["refs_per_image"]]
    return refs, z["hyps"].astype(np.int64), int(z["end_id"]), z


def padded(hyps, T, fill=END):
    out = np.full((len(hyps), T), fill, dtype=np.int64)
    for i, h in enumerate(hyps):
        out[i, :len(h)] = h
    return out


def edge_cases():
    """References of 7 images and the rows to score as (caption, image): the lengths 0..4, an end_id at
    position 0, 64 tokens with and without an end_id, a 100-token reference, the largest token, empty
    references, ids out of range after and before the end, an image outside the corpus."""
    rng = np.random.default_rng(11)
    long_ref = rng.integers(5, 12, size=100).tolist()   # longer than T
    cyc = [5, 6, 7, 8, 9, 10, 11] * 9 + [5]              # 64 tokens
    refs = [
        [[5, 6, 7, 8, 9], [5, 6, 9, 9, 10, 11]],
        [[3, 3, 3, 3, 3], [3, 3, 5]],
        [long_ref, long_ref[:30]],
        [[65534, 65534, 5, 6], [7, 65534]],
        [cyc, cyc[::-1] + [6, 7]],
        [[], [5, 30, 31, 6]],                            # an empty reference among others
        [[]],                                            # only an empty reference
    ]
    rows = [
        ([], 0), ([5], 0), ([5, 6], 0), ([5, 6, 9], 0), ([5, 6, 9, 9], 0),   # L = 0..4
        ([END, 5, 6, 7], 0),                                 # end_id at position 0
        ([3, 3, 3, 3, 3, 3, 3], 1), ([3, 3, 5, 3], 1),       # clipping at 5 and at 1
        (long_ref[:64], 2), (long_ref[10:40], 2), (long_ref[36:100], 2),   # a reference longer than T
        ([65534, 65534, 5], 3), ([7, 65534, 65534], 3),      # the largest token
        (cyc, 4), (cyc[:63], 4), (cyc[::-1], 4),             # T = 64 without and with an end_id
        ([], 5), ([30, 31, 5], 5), ([], 6), ([5, 6], 6),     # empty references: the ROUGE-L = 1 quirk at row 18
        ([5, 6, END, 70000, -5], 0),                         # out of range after the end: ignored
        ([5, 70000, 6, END], 0), ([-1], 3), ([65535, 5], 3),  # out of range before it: NaN, that row only
        ([5, 6, 7], 7), ([5, 6, 7], -1),                     # an image outside the corpus
        ([5, 6, 7, 8, 9], 0),
    ]
    return refs, rows


BAD_EDGE_ROWS = [21, 22, 23, 24, 25]
