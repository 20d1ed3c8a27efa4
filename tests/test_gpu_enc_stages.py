"""GPU: k_enc_v4's stage loop at small channel counts, where the prologue, the s + 1 / s + 2 prefetch
clamps and the last stage are most of the K loop (at C = 2048 they are three stages of 64).

The Python model fixes C = 2048, so the C ABI is driven directly (aa_pack_weights / aa_encoder_tail with
``Dims.channels``): C = 64, 128, 192 (two, four, six 32-channel stages: the shortest loops the library
admits), hidden 256 (8 waves) and 512 (16 waves), B = 1 (the last workgroup holds one image), 2 and 3.
aa_check_dims admits only multiples of 64 channels, so an odd count of 32-channel stages (C = 96) never
reaches the kernel: that is asserted here.

V against float64 with test_gpu_encoder_f16's error measure and rule for the bound (32 x the forced
bf16x3 body's measured maximum on the same inputs + 1e-7); a_g bitwise against the forced bf16x3 body
and against torch's avg_pool2d on the CPU; a feature outside the fp16 range in the first stage (which
the prologue stores), a middle and the last stage of an image sends its workgroup through the bf16x3
body bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from adaptive_amd import _lib, synth

pytestmark = pytest.mark.gpu

HIDDEN = (256, 512)
CHANNELS = (64, 128, 192)
BATCHES = (1, 2, 3)
EMBED, VOCAB = 256, 257
DEV = "cuda:0"


def dims(H, C):
    return synth.Dims(embed=EMBED, hidden=H, vocab=VOCAB, channels=C)


@functools.lru_cache(maxsize=None)
def packed(H, C):
    """(aa_model, the tensors it points into) for synthetic weights of a model with C channels."""
    lib = _lib.load()
    cd = _lib.Dims(EMBED, H, VOCAB, C, 49)
    _lib.check(lib.aa_check_dims(cd), "dims")
    w = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_weights(123, dims(H, C), bias_noise=0.01).items()}
    nbytes = lib.aa_packed_bytes(cd)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    model = _lib.Model(cd, buf.data_ptr(), nbytes)
    ref = _lib.RefWeights(**{f: w[k].data_ptr() for f, k in _lib.WEIGHT_FIELDS})
    with torch.cuda.device(DEV):
        _lib.check(lib.aa_pack_weights(model, ref, _lib.stream_handle()), "pack_weights")
    torch.cuda.synchronize()
    return model, (buf, w)


def encode(H, C, feats, forced):
    """(V [B, 49, H], a_g [B, C]) as numpy, through the default path or the forced bf16x3 body."""
    model, _ = packed(H, C)
    B = feats.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(feats)).to(DEV)
    new = lambda *shape: torch.empty(*shape, device=DEV)
    a_g, V, v_g, h0, c0, VWv = new(B, C), new(B, 49, H), new(B, EMBED), new(B, H), new(B, H), new(B, 49, 64)
    with torch.cuda.device(DEV):
        rc = _lib.load().aa_encoder_tail(model, x.data_ptr(), B, a_g.data_ptr(), V.data_ptr(), v_g.data_ptr(),
                                         h0.data_ptr(), c0.data_ptr(), VWv.data_ptr(),
                                         _lib.DECODE_ENC_BF16X3 if forced else 0, _lib.stream_handle())
    _lib.check(rc, "encoder_tail")
    torch.cuda.synchronize()
    return V.cpu().numpy(), a_g.cpu().numpy()


@functools.lru_cache(maxsize=None)
def features(C):
    return synth.make_features(max(BATCHES), seed=3, d=dims(512, C))


@functools.lru_cache(maxsize=None)
def encoded(H, C, B, forced):
    return encode(H, C, features(C)[:B], forced)


@functools.lru_cache(maxsize=None)
def reference(H, C):
    """float64 V of the three images and the error measure's denominator."""
    w = synth.make_weights(123, dims(H, C), bias_noise=0.01)
    W = w["encoder.affine_a.weight"].astype(np.float64)
    b = w["encoder.affine_a.bias"].astype(np.float64)
    A = features(C).astype(np.float64).reshape(max(BATCHES), C, 49).transpose(0, 2, 1)
    return np.maximum(A @ W.T + b, 0.0), np.abs(A) @ np.abs(W).T + np.abs(b)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_channel_counts_are_multiples_of_64():
    lib = _lib.load()
    assert lib.aa_check_dims(_lib.Dims(EMBED, 512, VOCAB, 96, 49)) == -2
    assert lib.aa_check_dims(_lib.Dims(EMBED, 512, VOCAB, 64, 49)) == 0


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("H", HIDDEN)
def test_v_is_fp32_accurate(H, C, B, gpu_device):
    ref, den = reference(H, C)
    ref, den = ref[:B], den[:B]
    V2 = encoded(H, C, B, False)[0].astype(np.float64)
    V3 = encoded(H, C, B, True)[0].astype(np.float64)
    e2 = float((np.abs(V2 - ref) / den).max())
    e3 = float((np.abs(V3 - ref) / den).max())
    bound = 32.0 * e3 + 1e-7
    print(f"enc_stages H={H} C={C} B={B}: fp16x2 {e2:.3e}, bf16x3 {e3:.3e}, bound {bound:.3e}")
    assert np.isfinite(V2).all()
    assert e2 <= bound, (e2, e3)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("H", HIDDEN)
def test_a_g_is_bitwise_the_bf16x3_bodys_and_atens(H, C, B, gpu_device):
    a2, a3 = encoded(H, C, B, False)[1], encoded(H, C, B, True)[1]
    assert a2.shape == (B, C)
    assert np.array_equal(bits(a2), bits(a3))
    pooled = torch.nn.functional.avg_pool2d(torch.from_numpy(features(C)[:B]), 7).reshape(B, C).numpy()
    assert np.array_equal(bits(a2), bits(pooled))


@pytest.mark.parametrize("value", [1e3, float("inf"), float("nan")], ids=["1e3", "inf", "nan"])
@pytest.mark.parametrize("stage", [0, 3, 5], ids=["first", "middle", "last"])
@pytest.mark.parametrize("H", HIDDEN)
def test_out_of_range_feature_in_any_stage_takes_the_bf16x3_body(H, stage, value, gpu_device):
    """C = 192 (six 32-channel stages: stage 0 is stored by the prologue, 5 is the last), B = 3, one bad
    feature in image 1: the workgroup of images 0 and 1 comes out bit for bit as the forced bf16x3 run;
    image 2 (a workgroup of its own) stays on the fast path."""
    C, B = 192, 3
    feats = features(C).copy()
    feats[1, 32 * stage + 5, 5, 2] = value
    V2, a2 = encode(H, C, feats, False)
    V3, a3 = encode(H, C, feats, True)
    assert np.array_equal(bits(V2[:2]), bits(V3[:2]))
    assert np.array_equal(bits(a2), bits(a3))
    assert np.array_equal(bits(V2[2]), bits(encoded(H, C, B, False)[0][2]))


def test_guard_at_2048_channels_is_bitwise_the_bf16x3_body(gpu_device):
    """C = 2048, B = 3: an infinite feature in the last stage of image 2 (the last workgroup)."""
    H, C = 512, 2048
    feats = synth.make_features(3, seed=3).copy()
    feats[2, 2047, 6, 6] = float("inf")
    V2, a2 = encode(H, C, feats, False)
    V3, a3 = encode(H, C, feats, True)
    assert np.array_equal(bits(V2[2]), bits(V3[2]))
    assert np.array_equal(bits(a2), bits(a3))
    assert np.isfinite(V2[:2]).all() and not np.array_equal(bits(V2[:2]), bits(V3[:2]))
