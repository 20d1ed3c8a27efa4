"""GPU: k_enc_v4's two-way fp16 split (the default: three MFMA products per block) against float64 and
against its own bf16x3 body (``_lib.DECODE_ENC_BF16X3``: six products, what every workgroup ran before
and what a workgroup whose features leave the fp16 range falls back to).

Hidden 256 (k_enc_v4<2>, 8 waves) and 512 (k_enc_v4<2, 16>); B = 1 (a last workgroup holding one
image), 2 (one full workgroup), 3 (odd), 67 (test_gpu_parity's row count).  The error measure is
test_split_bf16_encoder_is_fp32_accurate's: |V - ref| / (sum_k |a_k w_k| + |b|), ref in float64.

Bound of the accuracy test: 32 x the bf16x3 body's measured maximum on the same inputs + 1e-7
(32 = the per-term ratio 2^-21 / 2^-24 of the two schemes with a 4x margin).

Measured on an MI355X (the lines this module prints; maximum over the four batch sizes, which B = 67
sets; the bound is 32 x the second figure + 1e-7, 5.4e-6 .. 7.8e-6):

    hidden  features       fp16x2    bf16x3
    256     U[0,1)         1.70e-7   2.40e-7
    256     U[0,1) x 1e-4  5.22e-7   1.64e-7
    256     U[0,1) x 100   1.42e-7   2.26e-7
    512     U[0,1)         1.70e-7   2.40e-7
    512     U[0,1) x 1e-4  5.30e-7   1.64e-7
    512     U[0,1) x 100   1.58e-7   2.26e-7

(Both carry the fp32 accumulation over K = 2048 and the final fp32 rounding of V; the x 1e-4 rows show
the fp16 split's subnormal lo parts: 2^-25 absolute on the scaled features, still 10x inside the bound
and 4x inside test_split_bf16_encoder_is_fp32_accurate's 2e-6.)
"""
import functools

import numpy as np
import pytest
import torch

from adaptive_amd import Config, Encoder2Decoder, _lib, synth

pytestmark = pytest.mark.gpu

HIDDEN = (256, 512)
BATCHES = (1, 2, 3, 67)
SCALES = (1.0, 1e-4, 100.0)
VOCAB = 1003
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def model(H):
    cf = Config(adaptive_lstm_hidden_size=H, vocab_length=VOCAB)
    return Encoder2Decoder(cf).to(DEV).load_synthetic(123, bias_noise=0.01)


@functools.lru_cache(maxsize=None)
def features(scale):
    """The 67-image batch (seed 3) times ``scale``; a smaller batch is its first rows."""
    return (synth.make_features(max(BATCHES), seed=3) * np.float32(scale)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(H, scale):
    """float64 V of the 67 images and the error measure's denominator."""
    w = synth.make_weights(123, synth.Dims(hidden=H, vocab=VOCAB), bias_noise=0.01)
    W = w["encoder.affine_a.weight"].astype(np.float64)
    b = w["encoder.affine_a.bias"].astype(np.float64)
    B = max(BATCHES)
    A = features(scale).astype(np.float64).reshape(B, 2048, 49).transpose(0, 2, 1)
    ref = np.maximum(A @ W.T + b, 0.0)
    den = np.abs(A) @ np.abs(W).T + np.abs(b)
    return ref, den


def encode(H, feats, forced):
    """(V, a_g) as numpy, through the default fast path or the forced bf16x3 body."""
    m = model(H)
    m.decode_extra_flags = _lib.DECODE_ENC_BF16X3 if forced else 0
    try:
        out = m._encode(torch.from_numpy(feats).to(DEV))
    finally:
        m.decode_extra_flags = 0
    return out[0].cpu().numpy(), out[3].cpu().numpy()


@functools.lru_cache(maxsize=None)
def encoded(H, B, scale, forced):
    return encode(H, np.ascontiguousarray(features(scale)[:B]), forced)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("H", HIDDEN)
def test_fp16_split_is_fp32_accurate(H, B, scale, gpu_device):
    ref, den = reference(H, scale)
    ref, den = ref[:B], den[:B]
    V2 = encoded(H, B, scale, False)[0].astype(np.float64)
    V3 = encoded(H, B, scale, True)[0].astype(np.float64)
    e2 = float((np.abs(V2 - ref) / den).max())
    e3 = float((np.abs(V3 - ref) / den).max())
    bound = 32.0 * e3 + 1e-7
    print(f"enc_f16 H={H} B={B} scale={scale:g}: fp16x2 {e2:.3e}, bf16x3 {e3:.3e}, bound {bound:.3e}")
    assert np.isfinite(V2).all()
    assert e2 <= bound, (e2, e3)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("H", HIDDEN)
def test_a_g_is_bitwise_the_bf16x3_bodys(H, B, scale, gpu_device):
    a2, a3 = encoded(H, B, scale, False)[1], encoded(H, B, scale, True)[1]
    assert a2.shape == (B, 2048)
    assert np.array_equal(bits(a2), bits(a3))


@pytest.mark.parametrize("value", [300.0 * _lib.ENC_F16_A_MAX, float("inf"), float("nan")], ids=["300x", "inf", "nan"])
@pytest.mark.parametrize("H", HIDDEN)
def test_range_guard_falls_back_to_the_bf16x3_body(H, value, gpu_device):
    """One out-of-range feature in image 1 of 3: that image comes out bit for bit as the bf16x3 body
    computes it, and the other images' decode does not change."""
    B, img = 3, 1
    clean = np.ascontiguousarray(features(1.0)[:B])
    feats = clean.copy()
    feats[img, 777, 3, 4] = value
    V2, a2 = encode(H, feats, False)
    V3, a3 = encode(H, feats, True)
    assert np.array_equal(bits(V2[img]), bits(V3[img]))
    assert np.array_equal(bits(a2[img]), bits(a3[img]))
    assert np.array_equal(bits(a2), bits(a3))
    # image 2 (a workgroup of its own) stayed on the fast path: its V is the clean batch's
    assert np.array_equal(bits(V2[2]), bits(encoded(H, B, 1.0, False)[0][2]))
    m = model(H)
    others = [i for i in range(B) if i != img]
    ids_bad = m.sampler(torch.from_numpy(feats).to(DEV), max_len=3)[0].cpu()
    ids_clean = m.sampler(torch.from_numpy(clean).to(DEV), max_len=3)[0].cpu()
    assert torch.equal(ids_bad[others], ids_clean[others])
    assert bool(((ids_bad >= 0) & (ids_bad < VOCAB)).all())


@pytest.mark.parametrize("H", HIDDEN)
def test_decode_ids_equal_the_forced_bf16x3_decode(H, gpu_device):
    m = model(H)
    feats = torch.from_numpy(np.ascontiguousarray(features(1.0)[:3])).to(DEV)
    ids = m.sampler(feats, max_len=3)[0].cpu()
    m.decode_extra_flags = _lib.DECODE_ENC_BF16X3
    try:
        ids3 = m.sampler(feats, max_len=3)[0].cpu()
    finally:
        m.decode_extra_flags = 0
    assert ids.shape == (3, 3) and torch.equal(ids, ids3)
