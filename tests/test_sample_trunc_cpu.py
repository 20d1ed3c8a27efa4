"""CPU: top-k / nucleus truncation and N draws per image of the sampling decode, without a GPU.

* the oracle tests/sample_trunc_oracle.py: truncations off equal ``SampleOracle.sample``; ``top_k = 1`` is
  the greedy decode with logp 0; ``num_samples`` equals the ``repeat_interleave`` call; tie groups are kept
  whole; the hand-built cases of tests/sample_trunc_cases.py keep what their tables say;
* ``Encoder2Decoder.sample``'s new argument errors, raised before the library is touched;
* the C-ABI's argument checks (no device work: fake aligned pointers as in test_sample_cpu.py).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

from adaptive_amd import synth
import sample_trunc_cases as cases
from sample_trunc_oracle import SampleTruncOracle, kept_size, logp_for_kept, select


@pytest.fixture(scope="module")
def oracle():
    return SampleTruncOracle(synth.make_weights(123))


def _noise(V, row=0):
    return synth.gumbel_f32(synth.stream_key(0, "sample"), row * V, V)


def test_truncations_off_equal_the_plain_oracle(oracle):
    feats = synth.make_features(3, seed=0)
    ids, logp, al, be = oracle.sample(feats, 5, 0.8, 2, row0=4)
    r = oracle.sample_trunc(feats, 5, 0.8, 2, row0=4)
    assert torch.equal(r["ids"], ids)
    np.testing.assert_allclose(r["logp"].numpy(), logp.numpy(), atol=1e-6, rtol=0)  # float64 sums in another order
    assert torch.equal(r["alpha"], al) and torch.equal(r["beta"], be)
    assert (r["kept"] == 10123).all()
    # top_k >= V and top_p == 1 are "off" too
    r2 = oracle.sample_trunc(feats, 5, 0.8, 2, row0=4, top_k=10123, top_p=1.0)
    assert torch.equal(r2["ids"], ids) and (r2["kept"] == 10123).all()


def test_top_k_1_is_the_greedy_decode_with_logp_0(oracle):
    feats = synth.make_features(3, seed=1)
    greedy = oracle.sampler(torch.from_numpy(feats), max_len=6)[0]
    r = oracle.sample_trunc(feats, 6, 1.0, 5, top_k=1)
    assert torch.equal(r["ids"], greedy)
    assert (r["logp"].numpy() == 0).all() and (r["kept"] == 1).all()


def test_num_samples_equals_the_repeat_interleave_call(oracle):
    B, N, T = 3, 3, 4
    feats = synth.make_features(B, seed=2)
    a = oracle.sample_trunc(feats, T, 0.9, 1, row0=2, top_k=40, top_p=0.95, num_samples=N)
    b = oracle.sample_trunc(np.repeat(feats, N, axis=0), T, 0.9, 1, row0=2 * N, top_k=40, top_p=0.95)
    assert a["ids"].shape == (B * N, T) and a["alpha"].shape == (B * N, T, 49)
    assert torch.equal(a["ids"], b["ids"]) and np.array_equal(a["kept"], b["kept"])
    np.testing.assert_allclose(a["logp"].numpy(), b["logp"].numpy(), atol=1e-5, rtol=0)
    # the rows of one image differ from each other (their noise does), and from the rows drawn without the offset
    assert not torch.equal(a["ids"][0], a["ids"][1])
    c = oracle.sample_trunc(feats, T, 0.9, 1, row0=0, top_k=40, top_p=0.95, num_samples=N)
    assert not torch.equal(c["ids"], a["ids"])


def test_tie_groups_are_kept_whole():
    y = cases.ties(R=1)[0]
    g = _noise(y.shape[0])
    for (k, p), kept in cases.TIES_KEPT.items():
        s = select(y, g, k, p)
        assert s["kept"] == kept, (k, p)
        assert s["theta"] == (2.0 if kept == 3 else 1.0)
        assert y[s["token"]] >= s["theta"]
    # all equal: one tie group, whatever the truncation
    flat = np.zeros(50, np.float32)
    for k, p in ((1, 1.0), (0, 0.01), (3, 0.5)):
        s = select(flat, _noise(50), k, p)
        assert s["kept"] == 50 and s["token"] == int(np.argmax(flat + _noise(50)))
    # -0 and +0 are one value
    z = np.array([0.0, -0.0, -1.0], np.float32)
    assert select(z, _noise(3), 1, 1.0)["kept"] == 2


def test_hand_built_cases_keep_what_their_tables_say():
    y = cases.geometric(R=1)[0]
    g = _noise(y.shape[0])
    for (k, p), kept in cases.GEOMETRIC_KEPT.items():
        s = select(y, g, k, p, delta=5e-5)
        assert s["kept"] == kept == s["kept_in"] == s["kept_out"], (k, p, s["kept"], s["kept_in"], s["kept_out"])
        assert s["theta"] == np.float32(-0.5 * (kept - 1))
        assert s["logp"] == logp_for_kept(y, s["token"], kept)
    rows = cases.bites(R=8)
    for r in range(8):
        g = _noise(10123, r)
        assert select(rows[r], g, 0, 1.0)["token"] not in cases.BITES_HIGH
        s = select(rows[r], g, 0, cases.BITES_P, delta=5e-5)
        assert s["kept"] == 3 == s["kept_in"] == s["kept_out"] and s["token"] in cases.BITES_HIGH
        s = select(rows[r], g, 0, 0.5)
        assert s["kept"] == 10123 and s["token"] == select(rows[r], g, 0, 1.0)["token"]


def test_band_sets_bracket_the_kept_set():
    rng = np.random.default_rng(3)
    y = rng.normal(0, 1, 2000).astype(np.float32)
    ys = np.sort(y.astype(np.float64))[::-1]
    es = np.exp(ys - ys[0])
    for k, p in ((0, 0.9), (50, 1.0), (50, 0.5), (0, 0.3)):
        d = 1e-3
        kin = kept_size(ys, es, k, p, -2 * d, float(np.exp(2 * d)), 1e-6)
        kout = kept_size(ys, es, k, p, 2 * d, float(np.exp(-2 * d)), -1e-6)
        kept = kept_size(ys, es, k, p)
        assert 1 <= kin <= kept <= kout
        # a y perturbed by less than d keeps a set between the two
        yp = (y.astype(np.float64) + rng.uniform(-d, d, y.shape) * 0.99).astype(np.float32)
        kp = select(yp, _noise(2000), k, p)["kept"]
        assert kin <= kp <= kout, (k, p, kin, kp, kout)


def _no_library():
    raise AssertionError("the library must not be touched")


def test_python_argument_errors_before_the_library(monkeypatch):
    from adaptive_amd import Config, Encoder2Decoder, _lib
    m = Encoder2Decoder(Config())
    monkeypatch.setattr(_lib, "load", _no_library)
    x = torch.zeros(2, 2048, 7, 7)
    for k in (-1, 1.5, "3", None, True, 1 << 31):
        with pytest.raises(ValueError, match="top_k"):
            m.sample(x, 5, top_k=k)
    for p in (0.0, -0.1, 1.0001, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="top_p"):
            m.sample(x, 5, top_p=p)
    for n in (0, -2, 1.0, None, True):
        with pytest.raises(ValueError, match="num_samples"):
            m.sample(x, 5, num_samples=n)
    with pytest.raises(TypeError):  # keyword-only
        m.sample(x, 5, 1.0, 0, 0, None, 50)
    with pytest.raises(ValueError, match="temperature"):  # the earlier checks still come first
        m.sample(x, 5, temperature=0.0, top_k=-1)
    with pytest.raises(RuntimeError, match="GPU|CUDA"):  # valid arguments, CPU tensor: no CPU path
        m.sample(x, 5, top_k=50, top_p=0.9, num_samples=3, return_kept=True)


def test_baseline_model_still_refuses_sample(monkeypatch):
    from adaptive_amd import _lib
    from adaptive_amd.baseline_attention import Config, Encoder2Decoder
    m = Encoder2Decoder(Config())
    monkeypatch.setattr(_lib, "load", _no_library)
    with pytest.raises(NotImplementedError, match="baseline.*sample"):
        m.sample(torch.zeros(2, 2048, 7, 7), 5, top_k=50, top_p=0.9, num_samples=2)


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


def test_decode_ex_argument_errors_without_device_work(lib):
    from adaptive_amd import _lib
    p, big = 256, 10 ** 9  # fake aligned pointer

    def call(m, B=4, T=20, tau=1.0, row0=0, ws=p, ws_bytes=big, flags=0, top_k=0, top_p=1.0, N=1, opts=True,
             ids=p):
        o = ctypes.byref(_lib.SampleOpts(top_k, top_p, N, None, None)) if opts else None
        return lib.aa_sample_decode_ex(m, p, B, T, tau, 1, row0, ids, p, p, p, ws, ws_bytes, flags, None, None, o)

    assert _lib.ABI_VERSION == 17 == lib.aa_abi_version()
    m = _model()
    assert call(None) == -1 and call(_model(nbytes=10)) == -4 and call(_model(vocab=256 * 64 + 1)) == -2
    assert call(m, top_k=-1) == -3
    for top_p in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(m, top_p=top_p) == -3, top_p
    assert call(m, N=0) == -3 and call(m, N=-1) == -3
    assert call(m, B=1 << 20, N=17) == -3            # B N > 2^24
    assert call(m, row0=(1 << 62) // (3 * 20 * 10123), N=3) == -3  # (row0 + B) N T V > 2^62
    assert call(m, row0=(1 << 62) // (3 * 20 * 10123) - 4, N=3, ws_bytes=1) == -4  # at the bound: passes the check
    for flags in (_lib.DECODE_BASELINE, _lib.DECODE_EXACT_VOCAB, _lib.BEAM_FAST, _lib.DECODE_ONE_STREAM):
        assert call(m, flags=flags, top_k=5) == -3, flags
    # the option checks come before the empty-batch return, the pointer checks after it
    for B, T in ((0, 20), (4, 0)):
        assert call(m, B=B, T=T, ws=None, ws_bytes=0, ids=None, top_k=5, top_p=0.5, N=3) == 0
        assert call(m, B=B, T=T, top_k=-1) == -3 and call(m, B=B, T=T, top_p=0.0) == -3 and call(m, B=B, T=T, N=0) == -3
    assert call(m, ids=None, top_k=5) == -1 and call(m, ws=p + 4, top_k=5) == -5
    # opts == NULL: the defaults, i.e. aa_sample_decode
    d = _lib.Dims(256, 512, 10123, 2048, 49)
    need1 = lib.aa_sample_workspace_bytes(d, 4, 20)
    assert lib.aa_sample_workspace_bytes_ex(d, 4, 20, 1) == need1
    assert call(m, opts=False, ws_bytes=need1 - 1) == -4
    assert call(m, flags=_lib.DECODE_FP32_ENCODER, top_k=5, top_p=0.9, ws_bytes=need1 - 1) == -4
    # N rows per image: the encoder outputs for B images, the rest for B N rows
    need3 = lib.aa_sample_workspace_bytes_ex(d, 4, 20, 3)
    assert call(m, N=3, ws_bytes=need3 - 1) == -4
    need12 = lib.aa_sample_workspace_bytes(d, 12, 20)
    assert need1 + 8 * 10240 * 4 < need3  # the logits of 8 more rows
    assert need12 - need3 > 8 * 49 * 512 * 4 - 4 * 5 * 512 * 4 - 4096  # V of 8 images saved; x_g of 4 images staged
    assert lib.aa_sample_workspace_bytes_ex(d, 4, 20, 0) == 0
    assert lib.aa_sample_workspace_bytes_ex(d, 1 << 20, 20, 17) == 0
    assert lib.aa_sample_workspace_bytes_ex(d, 0, 20, 3) == 0


def test_select_argument_errors_without_device_work(lib):
    p = 256

    def call(R=4, V=300, Vp=320, T=5, t=0, tau=1.0, row0=0, top_k=0, top_p=1.0, logits=p, tok=p, ids=p, logp=p):
        return lib.aa_sample_select(logits, R, V, Vp, T, t, tau, 1, row0, top_k, top_p, tok, ids, logp, None, None, None)

    assert call(R=-1) == -3 and call(R=(1 << 24) + 1) == -3
    assert call(V=0) == -3 and call(V=256 * 64 + 1, Vp=256 * 64 + 128) == -3 and call(Vp=299) == -3
    assert call(T=0) == -3 and call(t=-1) == -3 and call(t=5) == -3
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call(tau=tau) == -3
    assert call(row0=-1) == -3 and call(row0=1 << 62) == -3
    assert call(top_k=-1) == -3
    for top_p in (0.0, 1.5, float("nan")):
        assert call(top_p=top_p) == -3
    assert call(R=0, logits=None, tok=None, ids=None, logp=None) == 0
    assert call(R=0, top_k=-1) == -3
    for missing in ("logits", "tok", "ids", "logp"):
        assert call(**{missing: None}) == -1, missing
