"""Truncated sampling (top-k / nucleus) and N draws per image on the GPU (C-ABI aa_sample_decode_ex,
through ``Encoder2Decoder.sample``) against tests/sample_trunc_oracle.py SampleTruncOracle.

With these weights the kept set cannot be required to equal the oracle's (set margins lie below the
logit tolerance), so the comparison is banded, with delta = SCORE_TOL * max(1, 1/tau) (test_gpu_sample.py's
logit tolerance).  The oracle returns, per (row, step), the inner and the outer set: every value comparison
moved by 2 delta, every mass ratio by e^{+-2 delta} and 1e-6 (fixed-point masses, fp32 exponentials), in the
direction that shrinks / grows S.  A (row, step) is *robust* when the perturbed-score arg-max over the outer
set lies in the inner set and leads the outer set's runner-up by more than 4 delta; every case asserts, before
the GPU is touched, that all its (row, step)s are robust (checked on the CPU when the cases were chosen).
Then: ids equal; |S_in| <= kept <= |S_out|; theta between the two sets' thresholds +- 2 delta; logp within
delta of the oracle's value for the best ``kept`` tokens (the prefix size the GPU reports); alpha / beta
within 2e-5."""
import numpy as np
import pytest
import torch

from adaptive_amd import Config, Encoder2Decoder, synth
from sample_trunc_oracle import SampleTruncOracle, logp_for_kept

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
    return SampleTruncOracle(weights)


# B, T, tau, seed, feature seed, top_k, top_p.  On the oracle: kept 40; 5; 7,235-7,410; 2,397-2,551; 43-44;
# 2,847-3,222; 44-45; 7,200-7,482 -- smallest lead of the draw 2.7e-2, 5.6e-2, 3.1e-2, 8.7e-3, 2.9e-2,
# 1.4e-2, 1.0e-3, 8.8e-3.  B = 67 crosses the 64-row tiles with a ragged tail.
CASES = [(4, 12, 1.0, 0, 0, 40, 1.0), (4, 12, 1.0, 3, 0, 5, 1.0), (4, 12, 1.0, 0, 0, 0, 0.9), (4, 12, 1.0, 0, 0, 0, 0.5),
         (4, 12, 0.7, 1, 0, 50, 0.9), (4, 12, 0.5, 2, 1, 0, 0.8), (67, 6, 1.0, 5, 3, 50, 0.9), (67, 6, 1.0, 5, 3, 0, 0.9)]


@pytest.mark.parametrize("B,T,tau,seed,fseed,top_k,top_p", CASES)
def test_truncated_sample_vs_oracle(B, T, tau, seed, fseed, top_k, top_p, model, oracle, gpu_device):
    feats = synth.make_features(B, seed=fseed)
    delta = SCORE_TOL * max(1.0, 1.0 / tau)
    o = oracle.sample_trunc(feats, T, tau, seed, top_k=top_k, top_p=top_p, delta=delta, keep_y=True)
    assert o["robust"].all(), f"case not robust at {np.argwhere(~o['robust']).tolist()}: pick another seed"
    ids, logp, al, be, kept, theta = model.sample(torch.from_numpy(feats).to(gpu_device), T, temperature=tau,
                                                  seed=seed, top_k=top_k, top_p=top_p, return_kept=True)
    assert ids.shape == (B, T) and logp.shape == (B, T) and kept.shape == (B, T) and theta.shape == (B, T)
    assert kept.dtype == torch.int32 and theta.dtype == torch.float32
    ids, logp, kept, theta = ids.cpu(), logp.cpu().numpy(), kept.cpu().numpy(), theta.cpu().numpy()
    print(f"B={B} T={T} tau={tau} k={top_k} p={top_p}: kept {kept.min()}..{kept.max()} (oracle "
          f"{o['kept'].min()}..{o['kept'].max()}, band <= {(o['kept_out'] - o['kept_in']).max()}), "
          f"kept != oracle at {(kept != o['kept']).sum()} of {kept.size}")
    assert torch.equal(ids, o["ids"])
    assert (o["kept_in"] <= kept).all() and (kept <= o["kept_out"]).all()
    assert (theta >= o["theta_out"] - 2 * delta).all() and (theta <= o["theta_in"] + 2 * delta).all()
    ref = np.array([[logp_for_kept(o["y"][r, t], int(ids[r, t]), int(kept[r, t])) for t in range(T)] for r in range(B)])
    print(f"  max |logp - oracle(kept)| = {np.abs(logp - ref).max():.3e} (tol {delta:.1e})")
    np.testing.assert_allclose(logp, ref, atol=delta, rtol=0)
    np.testing.assert_allclose(al.cpu().numpy(), o["alpha"].numpy(), atol=ATT_TOL, rtol=0)
    np.testing.assert_allclose(be.cpu().numpy(), o["beta"].numpy(), atol=ATT_TOL, rtol=0)


def test_top_k_1_is_the_exact_greedy_decode(model, gpu_device):
    f = torch.from_numpy(synth.make_features(67, seed=3)).to(gpu_device)
    g_ids = model.sampler(f, max_len=12, exact_vocab=True)[0]
    ids, logp, al, be, kept, theta = model.sample(f, 12, temperature=1.0, seed=9, top_k=1, return_kept=True)
    assert torch.equal(ids, g_ids)
    assert bool((logp == 0).all()) and bool((kept == 1).all())


def test_truncations_off_are_the_plain_decode_bitwise(model, gpu_device):
    f = torch.from_numpy(synth.make_features(9, seed=6)).to(gpu_device)
    plain = model.sample(f, 8, temperature=0.8, seed=2, row0=3)
    V = model.dims.vocab
    for kw in ({"top_k": V}, {"top_k": V + 1, "top_p": 1.0}, {"return_kept": True}):
        out = model.sample(f, 8, temperature=0.8, seed=2, row0=3, **kw)
        for a, b in zip(plain, out):
            assert torch.equal(a, b)
        if len(out) == 6:
            assert bool((out[4] == V).all()) and bool((out[5] < 0).all())


def _equal_to_repeat(m, feats, N, T, row0=0, **kw):
    a = m.sample(feats, T, row0=row0, num_samples=N, return_kept=True, **kw)
    b = m.sample(feats.repeat_interleave(N, 0), T, row0=row0 * N, return_kept=True, **kw)
    assert a[0].shape == (feats.size(0) * N, T) and a[2].shape == (feats.size(0) * N, T, 49)
    for name, x, y in zip(("ids", "logp", "alpha", "beta", "kept", "theta"), a, b):
        assert torch.equal(x, y), name
    return a


# (3, 3) and (23, 3): one workgroup per image in the attention (rows cross a 64-row tile inside image 21);
# (4, 7): the rows-per-image form of the plain attention kernels
@pytest.mark.parametrize("B,N,kw", [(3, 3, {}), (23, 3, {}), (4, 7, {}), (5, 2, {"top_k": 50, "top_p": 0.9}),
                                    (3, 5, {"top_p": 0.5})])
def test_num_samples_equals_repeat_interleave(B, N, kw, model, gpu_device):
    f = torch.from_numpy(synth.make_features(B, seed=7)).to(gpu_device)
    a = _equal_to_repeat(model, f, N, 6, temperature=0.9, seed=4, **kw)
    ids = a[0].view(B, N, 6)
    assert not torch.equal(ids[:, 0], ids[:, 1])  # an image's rows draw with their own noise


def test_num_samples_hidden_256(gpu_device):
    m = Encoder2Decoder(Config(adaptive_lstm_hidden_size=256)).to(gpu_device)
    m.load_synthetic(5)
    f = torch.from_numpy(synth.make_features(5, seed=1)).to(gpu_device)
    _equal_to_repeat(m, f, 3, 5, temperature=1.0, seed=1)
    _equal_to_repeat(m, f, 3, 5, temperature=1.0, seed=1, top_k=20)


def test_num_samples_shard(model, gpu_device):
    """Images 5..8 of 12 with row0 = 5, N = 3: rows 15..26 of the whole batch, bitwise."""
    f = torch.from_numpy(synth.make_features(12, seed=9)).to(gpu_device)
    kw = dict(temperature=0.8, seed=3, num_samples=3, top_p=0.9, return_kept=True)
    big = model.sample(f, 6, **kw)
    part = model.sample(f[5:9].contiguous(), 6, row0=5, **kw)
    for a, b in zip(big, part):
        assert torch.equal(a[15:27], b)
    assert not torch.equal(model.sample(f[5:9].contiguous(), 6, **kw)[0], big[0][15:27])


def test_errors_are_loud_and_leave_the_process_usable(model, gpu_device):
    f = torch.from_numpy(synth.make_features(2)).to(gpu_device)
    for kw in ({"top_k": -1}, {"top_k": 2.5}, {"top_p": 0.0}, {"top_p": 1.5}, {"top_p": float("nan")},
               {"num_samples": 0}, {"num_samples": -3}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            model.sample(f, 5, **kw)
        assert model.sample(f, 3, top_k=5)[0].shape == (2, 3)  # the model still decodes
    with pytest.raises(RuntimeError, match="code -3"):  # (row0 + B) N T V beyond 62 bits: the library's check
        model.sample(f, 5, row0=1 << 60, num_samples=8, top_k=5)
    out = model.sample(f[:0], 5, num_samples=3, top_k=4, return_kept=True)
    assert [tuple(o.shape) for o in out] == [(0, 5), (0, 5), (0, 5, 49), (0, 5, 1), (0, 5), (0, 5)]
    out = model.sample(f, 0, num_samples=3, return_kept=True)
    assert out[0].shape == (6, 0) and out[4].shape == (6, 0)
    a = model.sample(f, 5, seed=1, top_k=30, top_p=0.8, num_samples=2)
    assert len(a) == 4 and torch.equal(a[0], model.sample(f, 5, seed=1, top_k=30, top_p=0.8, num_samples=2)[0])
    assert bool((a[1] <= 0).all())
