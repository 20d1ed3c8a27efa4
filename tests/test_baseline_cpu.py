"""CPU: the baseline spatial-attention model (adaptive_amd.baseline_attention) without a GPU.

* the CPU restatement tests/baseline_oracle.py against goldens written by the REAL reference
  baseline sampler (tests/golden/make_golden_baseline.py) -- with test_oracle.py's tolerances;
* the module surface against the reference's baseline state dict;
* the C-ABI's argument checks for AA_DECODE_BASELINE / aa_baseline_decode_step (no device work: fake
  aligned pointers as in test_capi.py).
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

from adaptive_amd import synth
from baseline_oracle import BaselineOracle

ABSENT = ("decoder.adaptive.sentinel.affine_x.weight", "decoder.adaptive.sentinel.affine_h.weight",
          "decoder.adaptive.atten.affine_s.weight")
# name: weight seed, bias_noise, feature seed, B
CASES = {"base_b4": (123, 0.0, 0, 4), "base_biased_b16": (99, 0.02, 5, 16), "base_b67": (123, 0.0, 0, 67),
         "base_b130": (11, 0.02, 9, 130)}


def baseline_weights(seed, bias_noise=0.0):
    return {k: v for k, v in synth.make_weights(seed, bias_noise=bias_noise).items() if k not in ABSENT}


@pytest.fixture(scope="module")
def bmanifest():
    with open(os.path.join(GOLDEN, "manifest_baseline.json")) as f:
        return json.load(f)


# ---- the oracle against the reference ---------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_baseline_oracle_matches_reference_golden(case, bmanifest):
    seed, noise, fseed, B = CASES[case]
    g = load_golden(case)
    entry = bmanifest["cases"][case]
    assert (entry["weight_seed"], entry["bias_noise"], entry["feature_seed"], entry["B"]) == (seed, noise, fseed, B)
    assert entry["min_margin"] >= bmanifest["min_margin_required"] == 5e-5
    state = baseline_weights(seed, noise)
    assert synth.digest(state) == entry["weights_sha256"]
    feats = synth.make_features(B, seed=fseed)
    assert synth.digest({"f": feats})["f"] == entry["features_sha256"]
    ids, alpha, scores = BaselineOracle(state).sampler(torch.from_numpy(feats), max_len=20, keep_scores=True)
    assert np.array_equal(ids.numpy(), g["ids"].astype(np.int64))
    if "alpha" in g:
        np.testing.assert_allclose(alpha.numpy(), g["alpha"], atol=1e-6, rtol=0)
    else:
        np.testing.assert_allclose(alpha.numpy()[::4], g["alpha_s4"], atol=1e-6, rtol=0)  # every 4th row
    if "scores_t0" in g:
        np.testing.assert_allclose(scores[:, 0].numpy(), g["scores_t0"], atol=1e-5, rtol=0)
    if "scores_r01_t01" in g:
        np.testing.assert_allclose(scores[:2, :2].numpy(), g["scores_r01_t01"], atol=1e-5, rtol=0)


# ---- module surface -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bmodel():
    from adaptive_amd.baseline_attention import Config, Encoder2Decoder
    return Encoder2Decoder(Config())


def test_state_dict_matches_reference_baseline(bmodel, bmanifest, manifest):
    ref = bmanifest["state_dict"]
    ours = {k: list(v.shape) for k, v in bmodel.state_dict().items()}
    assert ours == ref and len(ours) == 18
    assert set(manifest["state_dict"]) - set(ours) == set(ABSENT)  # the adaptive list minus the sentinel's three
    assert not hasattr(bmodel.decoder.adaptive, "sentinel") and not hasattr(bmodel.decoder.adaptive.atten, "affine_s")


def test_strict_load_of_an_adaptive_state_dict_raises(bmodel):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_weights(123).items()}
    with pytest.raises(RuntimeError, match="sentinel"):
        bmodel.load_state_dict(sd, strict=True)
    bmodel.load_synthetic(123)  # the same weights minus the three keys load
    assert torch.equal(bmodel.decoder.adaptive.mlp.weight, sd["decoder.adaptive.mlp.weight"])


def test_lazy_export_and_get_model():
    import adaptive_amd
    from adaptive_amd import adaptive_attention, baseline_attention
    assert adaptive_amd.baseline_attention.Encoder2Decoder is baseline_attention.Encoder2Decoder

    class Cf:
        atten_model_name = "baseline_attention"
        base_word_embed_size, base_lstm_hidden_size = 32, 256
        adaptive_word_embed_size, adaptive_lstm_hidden_size = 64, 256
        vocab_length = 50

    m = adaptive_amd.get_model(Cf())
    assert type(m) is baseline_attention.Encoder2Decoder and m.dims.embed == 32
    Cf.atten_model_name = "adaptive_attention"
    m = adaptive_amd.get_model(Cf())
    assert type(m) is adaptive_attention.Encoder2Decoder and m.dims.embed == 64
    Cf.atten_model_name = "rnn_attention"
    with pytest.raises(NotImplementedError, match="rnn_attention"):
        adaptive_amd.get_model(Cf())


def test_unsupported_paths_raise_without_a_library_call(bmodel, monkeypatch):
    from adaptive_amd import _lib

    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", no_library)
    x = torch.zeros(2, 2048, 7, 7)
    caps = torch.zeros(2, 5, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="baseline"):
        bmodel(x, caps, [4, 3])
    with pytest.raises(NotImplementedError, match="baseline"):
        bmodel.beam_search(x)
    with pytest.raises(NotImplementedError, match="baseline"):
        bmodel.sharded_sampler(x)
    with pytest.raises(NotImplementedError, match="baseline"):
        bmodel.decoder(torch.zeros(2, 49, 512), torch.zeros(2, 256), caps, (torch.zeros(1, 2, 512),) * 2)
    for attr in ("device_parallel", "distributed_sampler"):
        monkeypatch.setattr(bmodel, attr, True)
        with pytest.raises(NotImplementedError, match="baseline"):
            bmodel.sampler(x)
        monkeypatch.setattr(bmodel, attr, False)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="GPU|CUDA"):  # as the adaptive model: no CPU path
        bmodel.sampler(x)


# ---- C-ABI, no device work --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from adaptive_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "adaptive_amd", "csrc")], check=True)
    return _lib.load()


def _model(hidden=512, ptr=256, nbytes=10 ** 9):
    from adaptive_amd import _lib
    return _lib.Model(_lib.Dims(256, hidden, 10123, 2048, 49), ptr, nbytes)


def test_baseline_flag_keeps_the_argument_errors(lib):
    from adaptive_amd import _lib
    assert _lib.DECODE_BASELINE == 8192 and _lib.ABI_VERSION == 17 == lib.aa_abi_version()
    F = _lib.DECODE_BASELINE
    for flags in (F, F | _lib.DECODE_EXACT_VOCAB | _lib.DECODE_SPLIT_RESCORE):
        assert lib.aa_greedy_decode(None, None, 1, 1, None, None, None, None, 0, None, flags, None) == -1
        assert lib.aa_greedy_decode(_model(nbytes=10), None, 1, 1, None, None, None, None, 0, None, flags, None) == -4
        assert lib.aa_greedy_decode(_model(ptr=256 + 16), None, 1, 1, None, None, None, None, 0, None, flags, None) == -5
        m = _model()
        assert lib.aa_greedy_decode(m, None, -1, 1, None, None, None, None, 0, None, flags, None) == -3
        assert lib.aa_greedy_decode(m, None, 0, 20, None, None, None, None, 0, None, flags, None) == 0
        assert lib.aa_greedy_decode(m, None, 4, 20, None, None, None, None, 0, None, flags, None) == -1
        assert lib.aa_greedy_decode_aux(m, None, -1, 1, None, None, None, None, 0, None, flags, None, None) == -3
        assert lib.aa_greedy_decode_aux(m, None, 0, 20, None, None, None, None, 0, None, flags, None, None) == 0
        assert lib.aa_greedy_decode_aux(m, 256, 4, 20, None, None, None, 256, 10 ** 9, None, flags, None, None) == -1
        h = ctypes.c_void_p()
        ref = ctypes.byref(h)
        assert lib.aa_decode_plan_create(m, 256, 0, 20, 256, None, None, 256, 10 ** 9, flags, ref) == -3
        assert lib.aa_decode_plan_create(m, None, 4, 20, 256, None, None, 256, 10 ** 9, flags, ref) == -1
        assert h.value is None


@pytest.mark.parametrize("hidden", [256, 1024])
def test_baseline_flag_rejects_other_hidden_sizes(lib, hidden):
    """Only H = 512 has no-sentinel kernels: AA_ERR_DIMS before anything else, the empty batch included."""
    from adaptive_amd import _lib
    F = _lib.DECODE_BASELINE
    m = _model(hidden)
    assert lib.aa_greedy_decode(m, None, 0, 20, None, None, None, None, 0, None, 0, None) == 0  # without the flag
    assert lib.aa_greedy_decode(m, None, 0, 20, None, None, None, None, 0, None, F, None) == -2
    assert lib.aa_greedy_decode(m, 256, 4, 20, 256, None, None, 256, 10 ** 9, None, F, None) == -2
    assert lib.aa_greedy_decode_aux(m, 256, 4, 20, 256, None, None, 256, 10 ** 9, None, F, None, None) == -2
    h = ctypes.c_void_p()
    assert lib.aa_decode_plan_create(m, 256, 4, 20, 256, None, None, 256, 10 ** 9, F, ctypes.byref(h)) == -2
    assert h.value is None
    assert lib.aa_baseline_decode_step(m, 0, None, None, None, None, None, None, None, None, None, None, None, None,
                                       0, None) == -2
    assert lib.aa_decode_step(m, 0, None, None, None, None, None, None, None, None, None, None, None, None, None,
                              0, None) == 0


def test_pack_rejects_one_sentinel_weight_without_the_other(lib):
    """Both of sent_affine_x_w / att_affine_s_w NULL is a baseline model; one alone is AA_ERR_NULL
    (returned before any device work)."""
    from adaptive_amd import _lib
    fields = {f: 256 for f, _ in _lib.WEIGHT_FIELDS}
    for missing in ("sent_affine_x_w", "att_affine_s_w"):
        w = _lib.RefWeights(**{f: (None if f == missing else p) for f, p in fields.items()})
        assert lib.aa_pack_weights(_model(), w, None) == -1, missing
    w = _lib.RefWeights(**{f: (None if f == "att_affine_g_w" else p) for f, p in fields.items()})
    assert lib.aa_pack_weights(_model(), w, None) == -1  # (any other weight: required, as before)


def test_baseline_decode_step_argument_checks(lib):
    from adaptive_amd import _lib
    step = lib.aa_baseline_decode_step
    p = 256  # fake aligned pointer
    big = 10 ** 9

    def call(m, B=4, V=p, VWv=None, v_g=p, h_in=p, c_in=p, h_out=p, c_out=p, tok_out=p, ws=p, ws_bytes=big):
        return step(m, B, None, V, VWv, v_g, h_in, c_in, h_out, c_out, None, tok_out, None, ws, ws_bytes, None)

    assert call(None) == -1
    assert call(_model(nbytes=10)) == -4
    assert call(_model(ptr=256 + 16)) == -5
    m = _model()
    assert call(m, B=-1) == -3
    assert call(m, B=0, V=None, ws=None) == 0  # empty batch: nothing is looked at
    for missing in ("V", "v_g", "h_in", "c_in", "h_out", "c_out", "tok_out", "ws"):
        assert call(m, **{missing: None}) == -1, missing
    for odd in ("V", "VWv", "v_g", "h_in", "c_in", "h_out", "c_out", "ws"):
        assert call(m, **{odd: p + 4}) == -5, odd
    need = lib.aa_step_workspace_bytes(_lib.Dims(256, 512, 10123, 2048, 49), 4)
    assert need > 0 and call(m, ws_bytes=need - 1) == -4
