"""Seeded temperature-sampling decode on the GPU (C-ABI aa_sample_decode / aa_synth_gumbel, through
``Encoder2Decoder.sample``) against tests/sample_oracle.py SampleOracle.

The reference has no sampling decode, so SampleOracle — the reference's own decoder step under
build-defined Gumbel-max selection with counter-based noise — is the specification.  Tokens must be
identical; ``logp`` within SCORE_TOL * max(1, 1/tau) (SCORE_TOL as in test_gpu_beam.py: a log-softmax
over fp32 logits accumulated in another order; a logit difference is divided by tau); alpha / beta
within 2e-5 as in the greedy tests.  Every oracle case first asserts its selection margin (smallest gap
between the best and second-best perturbed score over all rows and steps) above 4x that tolerance,
the beam tests' rule, so an equal draw is implied by the data."""
import numpy as np
import pytest
import torch

from adaptive_amd import Config, Encoder2Decoder, _lib, synth
from sample_oracle import SampleOracle

pytestmark = pytest.mark.gpu

SCORE_TOL = 5e-5
ATT_TOL = 2e-5


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(123)


@pytest.fixture(scope="module")
def model(gpu_device, weights):
    m = Encoder2Decoder(Config()).to(gpu_device)
    m.load_state_dict({k: torch.from_numpy(v).to(gpu_device) for k, v in weights.items()})
    return m


@pytest.fixture(scope="module")
def oracle(weights):
    return SampleOracle(weights)


def test_gumbel_noise_matches_host_statement(gpu_device):
    """aa_synth_gumbel against synth.gumbel_f32 over 2^16 counters starting at 3 * 2^32 (the 64-bit
    counter).  |g| < 17, so one fp32 ulp is at most 1.9e-6; atol = 1e-5 leaves a few ulps for the two
    logf calls."""
    lib = _lib.load()
    n, start, key = 1 << 16, 3 * 2 ** 32, synth.stream_key(0, "sample")
    dst = torch.full((n + 8,), 123.0, dtype=torch.float32, device=gpu_device)
    with torch.cuda.device(gpu_device):
        _lib.check(lib.aa_synth_gumbel(dst.data_ptr(), n, key, start, _lib.stream_handle()), "synth_gumbel")
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    ref = synth.gumbel_f32(key, start, n)
    d = float(np.abs(got[:n] - ref).max())
    print(f"gumbel max |gpu - host| = {d:.3e}")
    np.testing.assert_allclose(got[:n], ref, atol=1e-5, rtol=0)
    assert np.all(got[n:] == 123.0)  # nothing written past n
    # a low counter range too, and another key
    key1 = synth.stream_key(7, "sample")
    with torch.cuda.device(gpu_device):
        _lib.check(lib.aa_synth_gumbel(dst.data_ptr(), 1000, key1, 5, _lib.stream_handle()), "synth_gumbel")
    torch.cuda.synchronize()
    np.testing.assert_allclose(dst[:1000].cpu().numpy(), synth.gumbel_f32(key1, 5, 1000), atol=1e-5, rtol=0)


# B, T, tau, seed, feature seed: margins measured on the oracle 1.05e-2, 8.6e-3, 2.7e-3, 1.0e-3, 6.4e-2,
# 3.5e-3.  B = 67 / 130 cross the 64-row tiles of k_lstm and k_vexact with a ragged tail; tau = 0.05 /
# 2 stretch the division.
CASES = [(4, 20, 1.0, 0, 0), (4, 20, 0.7, 1, 0), (67, 12, 1.0, 4, 3), (130, 6, 0.5, 4, 1), (8, 20, 0.05, 0, 0),
         (8, 20, 2.0, 0, 0)]


@pytest.mark.parametrize("B,T,tau,seed,fseed", CASES)
def test_sample_vs_oracle(B, T, tau, seed, fseed, model, oracle, gpu_device):
    feats = synth.make_features(B, seed=fseed)
    o_ids, o_logp, o_al, o_be, margin = oracle.sample(feats, T, tau, seed, return_margin=True)
    tol = SCORE_TOL * max(1.0, 1.0 / tau)
    assert margin > 4 * tol, f"oracle case too close to call: margin {margin}"
    greedy = oracle.sampler(torch.from_numpy(feats), max_len=T)[0]
    assert (o_ids != greedy).float().mean().item() > 0.5, "case meant to differ from the greedy decode"
    ids, logp, al, be = model.sample(torch.from_numpy(feats).to(gpu_device), T, temperature=tau, seed=seed)
    assert ids.shape == (B, T) and logp.shape == (B, T) and al.shape == (B, T, 49) and be.shape == (B, T, 1)
    print(f"B={B} T={T} tau={tau}: margin {margin:.3e}, max |logp - oracle| = "
          f"{float((logp.cpu() - o_logp).abs().max()):.3e} (tol {tol:.1e}), "
          f"alpha {float((al.cpu() - o_al).abs().max()):.2e}, beta {float((be.cpu() - o_be).abs().max()):.2e}")
    assert torch.equal(ids.cpu(), o_ids)
    np.testing.assert_allclose(logp.cpu().numpy(), o_logp.numpy(), atol=tol, rtol=0)
    np.testing.assert_allclose(al.cpu().numpy(), o_al.numpy(), atol=ATT_TOL, rtol=0)
    np.testing.assert_allclose(be.cpu().numpy(), o_be.numpy(), atol=ATT_TOL, rtol=0)


@pytest.mark.parametrize("vocab", [150, 300])
def test_sample_small_vocabulary_vs_oracle(vocab, gpu_device):
    """Vocabularies below one pass of the workgroup: V = 150 leaves 106 threads (two whole waves) of
    k_sample_select without a column, V = 300 gives threads one or two.  Oracle margins 1.2e-1 and 2.8e-2."""
    B, T, tau, seed = 5, 8, 1.0, 0
    m = Encoder2Decoder(Config(vocab_length=vocab)).to(gpu_device)
    m.load_synthetic(11)
    feats = synth.make_features(B, seed=8)
    o_ids, o_logp, o_al, o_be, margin = SampleOracle(synth.make_weights(11, m.dims)).sample(
        feats, T, tau, seed, return_margin=True)
    assert margin > 4 * SCORE_TOL, f"oracle case too close to call: margin {margin}"
    ids, logp, al, be = m.sample(torch.from_numpy(feats).to(gpu_device), T, temperature=tau, seed=seed)
    assert torch.equal(ids.cpu(), o_ids)
    np.testing.assert_allclose(logp.cpu().numpy(), o_logp.numpy(), atol=SCORE_TOL, rtol=0)
    np.testing.assert_allclose(al.cpu().numpy(), o_al.numpy(), atol=ATT_TOL, rtol=0)
    np.testing.assert_allclose(be.cpu().numpy(), o_be.numpy(), atol=ATT_TOL, rtol=0)


def test_sample_is_deterministic_and_seeded(model, gpu_device):
    f = torch.from_numpy(synth.make_features(16, seed=2)).to(gpu_device)
    a = model.sample(f, 12, temperature=0.9, seed=5)
    b = model.sample(f, 12, temperature=0.9, seed=5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = model.sample(f, 12, temperature=0.9, seed=6)
    assert not torch.equal(a[0], c[0])
    assert bool((a[1] <= 0).all()) and bool(((a[0] >= 0) & (a[0] < model.dims.vocab)).all())


def test_sample_batch_and_shard_invariance(model, gpu_device):
    """An image's draw depends only on its global row: rows 5..8 of the full call equal, bitwise, a
    call on those four images with row0 = 5."""
    feats = torch.from_numpy(synth.make_features(37, seed=4)).to(gpu_device)
    big = model.sample(feats, 12, temperature=0.8, seed=3)
    small = model.sample(feats[5:9].contiguous(), 12, temperature=0.8, seed=3, row0=5)
    for a, b in zip(big, small):
        assert torch.equal(a[5:9], b)
    other = model.sample(feats[5:9].contiguous(), 12, temperature=0.8, seed=3)  # row0 = 0: other noise
    assert not torch.equal(other[0], big[0][5:9])


def test_sample_logp_agrees_with_the_models_own_logits(model, gpu_device):
    """T = 1, tau = 1: logp[:, 0] is log_softmax of the one-token decoder step's logits at the drawn
    token (both sides GPU results)."""
    B = 8
    f = torch.from_numpy(synth.make_features(B, seed=5)).to(gpu_device)
    ids, logp, al, be = model.sample(f, 1, temperature=1.0, seed=9)
    V, v_g, states = model.encoder(f)
    start = torch.ones(B, 1, dtype=torch.int64, device=gpu_device)
    scores, d_al, d_be, _ = model.decoder(V, v_g, start, states)
    ref = torch.log_softmax(scores[:, 0, :].double(), dim=1).gather(1, ids[:, :1]).float()
    torch.testing.assert_close(logp, ref, atol=SCORE_TOL, rtol=0)
    torch.testing.assert_close(al, d_al, atol=ATT_TOL, rtol=0)
    torch.testing.assert_close(be, d_be, atol=ATT_TOL, rtol=0)


def test_sample_errors_are_loud(model, gpu_device):
    f = torch.from_numpy(synth.make_features(2)).to(gpu_device)
    for kw in ({"temperature": 0.0}, {"temperature": -1.0}, {"temperature": float("nan")},
               {"temperature": float("inf")}, {"seed": -1}, {"seed": 1 << 63}, {"row0": -1}, {"max_len": -1}):
        with pytest.raises(ValueError):
            model.sample(f, **{"max_len": 5, **kw})
        assert model.sample(f, 3)[0].shape == (2, 3)  # the model still decodes
    with pytest.raises(RuntimeError, match="GPU|CUDA"):
        model.sample(f.cpu(), 5)
    with pytest.raises(RuntimeError, match="code -3"):  # (row0 + B) T V beyond 62 bits: the library's check
        model.sample(f, 5, row0=1 << 62)
    out = model.sample(f[:0], 5)
    assert out[0].shape == (0, 5) and out[1].shape == (0, 5) and out[2].shape == (0, 5, 49) and out[3].shape == (0, 5, 1)
    out = model.sample(f, 0)
    assert out[0].shape == (2, 0) and out[2].shape == (2, 0, 49)
    ids, logp, al, be = model.sample(f, 5, seed=1)
    assert torch.equal(ids, model.sample(f, 5, seed=1)[0])
    g_ids, g_al, g_be = model.sampler(f, max_len=5)  # the greedy decode is unaffected by a sampling call before it
    assert g_ids.shape == (2, 5)
    torch.testing.assert_close(al[:, 0], g_al[:, 0], atol=ATT_TOL, rtol=0)  # step 0 does not depend on the draw
