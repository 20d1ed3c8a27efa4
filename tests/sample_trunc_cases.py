"""Hand-built logit rows for the truncated selection's tests — TEST INFRASTRUCTURE ONLY.

Every margin is large by construction (value gaps >= 0.1, mass ratios at least 1 % from a threshold), so
kept, theta and the token of an fp32 implementation must equal the float64 oracle's.
"""
from __future__ import annotations

import numpy as np

POISON = np.float32(1e30)  # in the padding columns V .. Vp - 1: they must take no part


def padded(rows: np.ndarray, Vp: int) -> np.ndarray:
    """[R, V] -> [R, Vp] with the padding poisoned."""
    R, V = rows.shape
    out = np.full((R, Vp), POISON, np.float32)
    out[:, :V] = rows
    return out


def geometric(R: int = 4, V: int = 300, seed: int = 0) -> np.ndarray:
    """y_v = -0.5 rank(v), through one column permutation per row.  Renormalised masses: token j holds
    (1 - q) q^j, q = e^-0.5; the mass strictly above token j is 1 - q^j: 0.865 above token 4 (the fifth),
    0.918 above token 5."""
    rng = np.random.default_rng(seed)
    rows = np.empty((R, V), np.float32)
    for r in range(R):
        rows[r, rng.permutation(V)] = -0.5 * np.arange(V, dtype=np.float32)
    return rows


# (top_k, top_p) -> kept on the geometric rows.  top_k = 3 then top_p = 0.8: the renormalised mass above
# the third token is (1 + q) / (1 + q + q^2) = 0.814 >= 0.8
GEOMETRIC_KEPT = {(0, 0.9): 5, (3, 1.0): 3, (3, 0.8): 2, (3, 0.9): 3}


def ties(R: int = 4, V: int = 300, seed: int = 1) -> np.ndarray:
    """[2, 2, 2, 1, 1, 0, -50 ...] through a column permutation per row."""
    rng = np.random.default_rng(seed)
    base = np.full(V, -50.0, np.float32)
    base[:6] = [2, 2, 2, 1, 1, 0]
    rows = np.empty((R, V), np.float32)
    for r in range(R):
        rows[r, rng.permutation(V)] = base
    return rows


# top_k = 2 keeps the three 2s; top_p = 0.5: the mass above the 2s is 0 < 0.5 and above the 1s it is
# 3 e^2 / (3 e^2 + 2 e + 1) = 0.775 >= 0.5; top_k = 4 keeps the 2s and both 1s
TIES_KEPT = {(2, 1.0): 3, (0, 0.5): 3, (4, 1.0): 5}


def bites(R: int = 8, V: int = 10123) -> np.ndarray:
    """[3, 2.9, 2.8, 0 ...] at columns 5000, 17, 9999: the three hold 54.7 / (54.7 + 10120) = 0.538 % of
    the mass, so an untruncated draw lands among the 10,120 zeros.  The masses strictly above the second,
    the third and the zeros are 0.197 %, 0.376 % and 0.538 %: top_p = 0.005 (0.5 %) keeps exactly the three
    -- the truncation bites -- while top_p = 0.5 keeps every column (the zeros are one tie group with
    0.538 % < 50 % above it: kept whole) and so draws the untruncated token."""
    rows = np.zeros((R, V), np.float32)
    rows[:, 5000], rows[:, 17], rows[:, 9999] = 3.0, 2.9, 2.8
    return rows


BITES_HIGH = (5000, 17, 9999)
BITES_P = 0.005


def spread(R: int, V: int, seed: int) -> np.ndarray:
    """Distinct values -0.1 rank(v) through a permutation (gaps of 0.1): for the vocabulary-size cases."""
    rng = np.random.default_rng(seed)
    rows = np.empty((R, V), np.float32)
    for r in range(R):
        rows[r, rng.permutation(V)] = -0.1 * np.arange(V, dtype=np.float32)
    return rows
