"""CPU: a numpy float16 emulation of the two-way fp16 split behind k_enc_v4's fast path (three products
hi.W_hi + hi.W_lo + lo.W_hi instead of bf16x3's six), with the scales the kernel uses.

The products are summed in float64, so only the representation error shows (the fp32 accumulation is the
same in both schemes and is what the GPU tests measure).  Bound: the scheme's own, max error <= 2^-21 of
sum_k |a_k w_k| per output (lo's rounding 2^-22 on either side plus the dropped lo.lo), at K = 2048.

The scale constants are read from aa_internal.hpp (what the kernel compiles) and asserted equal to
``adaptive_amd._lib``'s copies, which the emulation uses.
"""
import os
import re

import numpy as np
import pytest

from adaptive_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M, N = 2048, 48, 64
BOUND = 2.0 ** -21


def header_constants():
    text = open(os.path.join(ROOT, "adaptive_amd", "csrc", "aa_internal.hpp")).read()
    out = {}
    for name in ("ENC_F16_A_EXP", "ENC_F16_A_MAX", "ENC_F16_W_TOP", "ENC_F16_W_ECLAMP"):
        m = re.search(r"constexpr\s+(?:int|float)\s+%s\s*=\s*([-0-9.]+)f?\s*;" % name, text)
        assert m, name
        out[name] = float(m.group(1))
    return out


def test_constants_match_the_kernel_header():
    h = header_constants()
    assert h == {"ENC_F16_A_EXP": _lib.ENC_F16_A_EXP, "ENC_F16_A_MAX": _lib.ENC_F16_A_MAX,
                 "ENC_F16_W_TOP": _lib.ENC_F16_W_TOP, "ENC_F16_W_ECLAMP": _lib.ENC_F16_W_ECLAMP}
    # the two feature constants multiply to 2^15: hi of any feature under the threshold is finite in fp16
    assert _lib.ENC_F16_A_MAX * 2.0 ** _lib.ENC_F16_A_EXP == 2.0 ** 15 < 65504
    assert 2.0 ** (_lib.ENC_F16_W_TOP + 1) < 65504


def w_exponent(W):
    """k_w4h_scale: e with max|W| 2^e in [2^W_TOP, 2^(W_TOP + 1)), clamped; 0 for zero / subnormal / non-finite."""
    mx = np.abs(W.astype(np.float32)).max()
    if not np.isfinite(mx) or mx < np.finfo(np.float32).tiny:
        return 0
    e = _lib.ENC_F16_W_TOP - int(np.floor(np.log2(float(mx))))
    return int(np.clip(e, -_lib.ENC_F16_W_ECLAMP, _lib.ENC_F16_W_ECLAMP))


def split2(x32):
    """split2h: hi = fp16(x), lo = fp16(x - hi), the difference taken in fp32 (exact)."""
    assert x32.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x32.astype(np.float16)
        lo = (x32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def guard(x32):
    """The staging threads' predicate: !(|x| < ENC_F16_A_MAX)."""
    return ~(np.abs(x32) < np.float32(_lib.ENC_F16_A_MAX))


def emulate(A, W):
    """[M, K] features x [N, K] weights through the split; products summed in float64."""
    e = w_exponent(W)
    As = A * np.float32(2.0 ** _lib.ENC_F16_A_EXP)
    Ws = W * np.float32(2.0 ** e)
    assert As.dtype == Ws.dtype == np.float32
    ah, al = (x.astype(np.float64) for x in split2(As))
    wh, wl = (x.astype(np.float64) for x in split2(Ws))
    assert np.isfinite(ah).all() and np.isfinite(wh).all()
    out = al @ wh.T + ah @ wl.T + ah @ wh.T
    return out * 2.0 ** -(e + _lib.ENC_F16_A_EXP)


def rel_err(A, W):
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    return float((np.abs(emulate(A, W) - A64 @ W64.T) / (np.abs(A64) @ np.abs(W64).T)).max())


RNG = np.random.default_rng(20240607)
UNDER = np.nextafter(np.float32(_lib.ENC_F16_A_MAX), np.float32(0))
FEATURES = {
    "uniform01": RNG.random((M, K), dtype=np.float32),
    "small_1e-6_1e-3": (1e-6 + RNG.random((M, K)) * (1e-3 - 1e-6)).astype(np.float32),
    "just_under_threshold": np.minimum((_lib.ENC_F16_A_MAX * (1.0 - RNG.random((M, K)) * 2.0 ** -9)).astype(np.float32), UNDER),
    "mixed_signs": (2.0 * RNG.random((M, K)) - 1.0).astype(np.float32),
}
FEATURES["just_under_threshold"][0, :8] = UNDER
W_MAX = float(np.sqrt(6.0 / K))  # the synthetic affine_a's bound, U(-0.054, 0.054)
WEIGHTS = {
    "affine_a_like": ((2.0 * RNG.random((N, K)) - 1.0) * W_MAX).astype(np.float32),
    "span_2^-20_to_1": (np.sign(RNG.random((N, K)) - 0.5) * W_MAX * 2.0 ** (-20.0 * RNG.random((N, K)))).astype(np.float32),
}
WEIGHTS["span_2^-20_to_1"][:, 0] = W_MAX  # the top of the span is there in every row


@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("fname", list(FEATURES))
def test_representation_error_within_the_schemes_bound(fname, wname):
    A, W = FEATURES[fname], WEIGHTS[wname]
    assert not guard(A).any()
    err = rel_err(A, W)
    print(f"fp16x2 {fname} x {wname}: e = {w_exponent(W)}, max error / sum|a w| = {err:.3e} (bound {BOUND:.3e})")
    assert err <= BOUND


def test_weight_scale_leaves_headroom_and_normal_lo_parts():
    for W in WEIGHTS.values():
        e = w_exponent(W)
        top = float(np.abs(W).max()) * 2.0 ** e
        assert 2.0 ** _lib.ENC_F16_W_TOP <= top < 2.0 ** (_lib.ENC_F16_W_TOP + 1)
        # a weight down to 2^-17 of the largest keeps a normal lo part: |w| 2^e >= 2^-4 > 2^-14 x 2^10
        assert 2.0 ** _lib.ENC_F16_W_TOP * 2.0 ** -17 >= 2.0 ** -14 * 2.0 ** 10
    assert w_exponent(np.zeros((2, 2), np.float32)) == 0
    assert w_exponent(np.array([[np.inf, 1.0]], np.float32)) == 0
    assert w_exponent(np.array([[1e-30, 0.0]], np.float32)) == _lib.ENC_F16_W_ECLAMP


def test_guard_fires_exactly_outside_the_fast_paths_range():
    thr = np.float32(_lib.ENC_F16_A_MAX)
    inside = np.array([0.0, -0.0, 1e-30, 1.0, -1.0, UNDER, -UNDER], np.float32)
    outside = np.array([thr, -thr, np.nextafter(thr, np.float32(np.inf)), 300.0 * thr, -300.0 * thr,
                        np.finfo(np.float32).max, np.inf, -np.inf, np.nan], np.float32)
    assert not guard(inside).any()
    assert guard(outside).all()
    # whatever passes the guard splits into finite halves
    hi, lo = split2(inside * np.float32(2.0 ** _lib.ENC_F16_A_EXP))
    assert np.isfinite(hi.astype(np.float32)).all() and np.isfinite(lo.astype(np.float32)).all()
