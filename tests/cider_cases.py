"""Inputs shared by the CIDEr-D tests: the golden corpus and a second corpus for df_refs."""
import numpy as np

from conftest import load_golden


def golden_cases():
    """(refs, hyps [M, 20] int64, end_id, the reference's per-image scores, their mean)."""
    z = load_golden("cider_eval")
    caps = np.split(z["ref_tokens"].astype(np.int64), np.cumsum(z["ref_lengths"])[:-1])
    it = iter(caps)
    refs = [[next(it).tolist() for _ in range(k)] for k in z["refs_per_image"]]
    return refs, z["hyps"].astype(np.int64), int(z["end_id"]), z["scores"], float(z["mean"])


def other_corpus(images=30, seed=5):
    """A second corpus for df_refs: other images, a wider vocabulary."""
    rng = np.random.default_rng(seed)
    return [[rng.integers(3, 40, size=int(rng.integers(1, 12))).tolist() for _ in range(int(rng.integers(1, 4)))]
            for _ in range(images)]
