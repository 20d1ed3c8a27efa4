"""CPU: the seeded temperature-sampling decode without a GPU.

* ``synth.gumbel_f32`` — the host statement of the noise — against values worked out from the
  definition with Python integers and ``math.log``;
* the CPU oracle tests/sample_oracle.py: an image's draw depends only on its global row, and on the seed;
* ``Encoder2Decoder.sample``'s argument errors, raised before the library is touched, and the baseline
  model's refusal;
* the C-ABI's argument checks (no device work: fake aligned pointers as in test_capi.py).
"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

from adaptive_amd import synth
from sample_oracle import SampleOracle

KEY0 = 0x67BA3DCA1B1358DB  # synth.stream_key(0, "sample")
# element counter -> (k23, g): k23 = splitmix64(KEY0 + (e + 1) GOLDEN) >> 41 in Python integers,
# g = -log(-log((2 k23 + 1) / 2^24)) with math.log (float64)
PINNED = {0: (228551, -1.2817302798975831), 1: (4629570, 0.5201851280997938), 2: (64980, -1.5811500878542066),
          809839: (2820899, -0.08601143397426209), 3 * 2 ** 32: (2766625, -0.10368072917406881),
          3 * 2 ** 32 + 65535: (8119853, 3.4245944884342454)}


def test_stream_key_and_pinned_values():
    assert synth.stream_key(0, "sample") == KEY0
    for e, (k23, g) in PINNED.items():
        u = synth.gumbel_uniform(KEY0, e, 1)[0]
        assert u == (2 * k23 + 1) / 2 ** 24
        got = synth.gumbel_f32(KEY0, e, 1)
        assert got.dtype == np.float32 and got[0] == np.float32(g)


def test_uniform_is_strictly_inside_the_unit_interval_and_exact_in_fp32():
    u = synth.gumbel_uniform(KEY0, 3 * 2 ** 32, 1 << 16)
    assert u.dtype == np.float64
    assert u.min() >= 2.0 ** -24 and u.max() <= 1.0 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)       # 24 significant bits
    assert np.all((u * 2 ** 24) % 2 == 1)                                    # the odd grid points
    # the extreme grid points stay finite: |g| < 17
    for uu in (2.0 ** -24, 1.0 - 2.0 ** -24):
        assert abs(-math.log(-math.log(uu))) < 17
    g = synth.gumbel_f32(KEY0, 3 * 2 ** 32, 1 << 16)
    assert np.isfinite(g).all() and np.abs(g).max() < 17
    assert abs(float(g.mean()) - 0.5772) < 0.02                              # Euler-Mascheroni: a Gumbel's mean


def test_stream_in_two_pieces_equals_the_whole():
    start, n, cut = 3 * 2 ** 32 - 100, 1000, 357
    whole = synth.gumbel_f32(KEY0, start, n)
    a, b = synth.gumbel_f32(KEY0, start, cut), synth.gumbel_f32(KEY0, start + cut, n - cut)
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert not np.array_equal(synth.gumbel_f32(synth.stream_key(1, "sample"), start, n), whole)


@pytest.fixture(scope="module")
def oracle():
    return SampleOracle(synth.make_weights(123))


def test_oracle_draw_depends_only_on_the_global_row(oracle):
    """Rows 3..5 of an 8-image batch equal a 3-image batch with row0 = 3."""
    T, tau, seed = 6, 0.8, 2
    feats = synth.make_features(8, seed=0)
    ids, logp, al, be, margin = oracle.sample(feats, T, tau, seed, return_margin=True)
    assert ids.shape == (8, T) and logp.shape == (8, T) and al.shape == (8, T, 49) and be.shape == (8, T, 1)
    assert margin > 1e-4  # far above the CPU GEMM's batch-size-dependent rounding
    s_ids, s_logp, s_al, s_be = oracle.sample(feats[3:6], T, tau, seed, row0=3)
    assert torch.equal(s_ids, ids[3:6])
    np.testing.assert_allclose(s_logp.numpy(), logp[3:6].numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(s_al.numpy(), al[3:6].numpy(), atol=1e-6, rtol=0)
    # without the row offset the same images draw other tokens
    assert not torch.equal(oracle.sample(feats[3:6], T, tau, seed)[0], ids[3:6])
    assert bool((logp <= 0).all())


def test_oracle_seed_changes_the_draw_and_low_temperature_approaches_greedy(oracle):
    feats = synth.make_features(4, seed=0)
    a = oracle.sample(feats, 8, 1.0, 0)[0]
    assert torch.equal(a, oracle.sample(feats, 8, 1.0, 0)[0])
    assert not torch.equal(a, oracle.sample(feats, 8, 1.0, 1)[0])
    greedy = oracle.sampler(torch.from_numpy(feats), max_len=1)[0]
    assert torch.equal(oracle.sample(feats, 1, 1e-4, 0)[0], greedy)  # noise / 1e4: the argmax of the logits


def _no_library():
    raise AssertionError("the library must not be touched")


def test_python_argument_errors_before_the_library(monkeypatch):
    from adaptive_amd import Config, Encoder2Decoder, _lib
    m = Encoder2Decoder(Config())
    monkeypatch.setattr(_lib, "load", _no_library)
    x = torch.zeros(2, 2048, 7, 7)
    for tau in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e39):
        with pytest.raises(ValueError, match="temperature"):
            m.sample(x, 5, temperature=tau)
    for seed in (-1, 1 << 63):
        with pytest.raises(ValueError, match="seed"):
            m.sample(x, 5, seed=seed)
    with pytest.raises(ValueError, match="row0"):
        m.sample(x, 5, row0=-1)
    with pytest.raises(ValueError, match="max_len"):
        m.sample(x, -1)
    with pytest.raises(ValueError, match="images"):
        m.sample(torch.zeros(2, 3, 7, 7), 5)
    with pytest.raises(RuntimeError, match="GPU|CUDA"):  # valid arguments, CPU tensor: no CPU path
        m.sample(x, 5, temperature=0.7, seed=(1 << 63) - 1, row0=3)


def test_baseline_model_refuses_sample(monkeypatch):
    from adaptive_amd import _lib
    from adaptive_amd.baseline_attention import Config, Encoder2Decoder
    m = Encoder2Decoder(Config())
    monkeypatch.setattr(_lib, "load", _no_library)
    with pytest.raises(NotImplementedError, match="baseline.*sample"):
        m.sample(torch.zeros(2, 2048, 7, 7))
    with pytest.raises(NotImplementedError, match="baseline.*sample"):
        m.sample(torch.zeros(2, 2048, 7, 7), 5, temperature=0.5, seed=1, row0=2)


# ---- C-ABI, no device work --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from adaptive_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "adaptive_amd", "csrc")], check=True)
    return _lib.load()


def _model(vocab=10123, ptr=256, nbytes=10 ** 9):
    from adaptive_amd import _lib
    return _lib.Model(_lib.Dims(256, 512, vocab, 2048, 49), ptr, nbytes)


def test_sample_argument_errors_without_device_work(lib):
    from adaptive_amd import _lib
    p, big = 256, 10 ** 9  # fake aligned pointer

    def call(m, B=4, T=20, tau=1.0, key=1, row0=0, feats=p, ids=p, logp=p, alpha=p, beta=p, ws=p, ws_bytes=big,
             flags=0):
        return lib.aa_sample_decode(m, feats, B, T, tau, key, row0, ids, logp, alpha, beta, ws, ws_bytes, flags, None,
                                    None)

    assert _lib.ABI_VERSION == 17 == lib.aa_abi_version()
    assert call(None) == -1
    assert call(_model(nbytes=10)) == -4
    assert call(_model(ptr=256 + 16)) == -5
    assert call(_model(vocab=256 * 64 + 1)) == -2  # one thread holds at most 64 columns' worth, as beam search
    m = _model()
    assert call(m, B=-1) == -3 and call(m, T=-1) == -3
    for tau in (0.0, -0.5, float("nan"), float("inf")):
        assert call(m, tau=tau) == -3, tau
    assert call(m, row0=-1) == -3
    assert call(m, row0=1 << 62) == -3  # the element counter would leave 62 bits
    for flags in (_lib.DECODE_BASELINE, _lib.DECODE_EXACT_VOCAB, _lib.BEAM_FAST, _lib.DECODE_ONE_STREAM,
                  _lib.DECODE_FP32_ENCODER | _lib.DECODE_BASELINE):
        assert call(m, flags=flags) == -3, flags
    assert call(m, flags=_lib.DECODE_FP32_ENCODER, ws_bytes=1) == -4  # the one accepted flag passes the check
    # empty batch / no steps: AA_OK before any pointer is looked at -- but not before the argument checks
    for B, T in ((0, 20), (4, 0)):
        assert call(m, B=B, T=T, feats=None, ids=None, logp=None, alpha=None, beta=None, ws=None, ws_bytes=0) == 0
        assert call(m, B=B, T=T, tau=0.0) == -3
        assert call(m, B=B, T=T, flags=_lib.DECODE_BASELINE) == -3
    for missing in ("feats", "ids", "logp", "ws"):
        assert call(m, **{missing: None}) == -1, missing
    for odd in ("feats", "ws"):
        assert call(m, **{odd: p + 4}) == -5, odd
    d = _lib.Dims(256, 512, 10123, 2048, 49)
    need = lib.aa_sample_workspace_bytes(d, 4, 20)
    assert need > 4 * 49 * 512 * 4 + 4 * 10240 * 4  # holds V and one step's logits
    assert call(m, ws_bytes=need - 1) == -4
    assert lib.aa_sample_workspace_bytes(d, 4, 20) == lib.aa_sample_workspace_bytes(d, 4, 7)  # no per-step history
    assert lib.aa_sample_workspace_bytes(d, 0, 20) == 0
    assert lib.aa_sample_workspace_bytes(d, -1, 20) == 0
    assert lib.aa_sample_workspace_bytes(_lib.Dims(256, 500, 10123, 2048, 49), 4, 20) == 0
    assert lib.aa_sample_workspace_bytes(_lib.Dims(256, 512, 256 * 64 + 1, 2048, 49), 4, 20) == 0
    # the noise generator
    assert lib.aa_synth_gumbel(None, 0, 1, 0, None) == 0
    assert lib.aa_synth_gumbel(None, 16, 1, 0, None) == -1
    assert lib.aa_synth_gumbel(p, -1, 1, 0, None) == -3
    assert lib.aa_synth_gumbel(p, 16, 1, -1, None) == -3
