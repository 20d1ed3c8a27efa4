"""CPU: the float64 training reference of tests/train_cases.py and the conditions its GPU tests
(tests/test_gpu_train_dims.py) rest on.

* ``TrainOracle(state, dtype=torch.float64)`` is the fp32 oracle's program text in double: the two
  agree on every case within 4x the fp32 oracle's measured distance from float64 (worst over the seven
  cases: scores 2.5e-6 max abs, loss 9.2e-8 relative, any gradient 2.0e-6 relative Frobenius and
  1.7e-6 of its largest magnitude entry-wise, dfeats 7.7e-7 relative Frobenius).
* The default dtype is unchanged: ``TrainOracle(state)`` and ``TrainOracle(state, dtype=torch.float32)``
  give the same bits, and both still meet the reference's own training golden (train_b4).
* The kink mask excludes at most 15 % of any tensor's rows and ``near_b`` is empty, on every case.
* The case table is what it says: lengths sorted and positive, T and the packed row count as listed.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

import train_cases as tc
from adaptive_amd import synth

# CPU fp32 oracle vs float64, worst over the seven cases (see above), times 4
SCORE_ABS, LOSS_REL, GRAD_REL, GRAD_ENTRY, DFEATS_REL = 4 * 2.5e-6, 4 * 9.2e-8, 4 * 2.0e-6, 4 * 1.7e-6, 4 * 7.7e-7


def _rel(got, ref):
    return np.linalg.norm(np.asarray(got, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_float64_oracle_agrees_with_fp32_oracle(name):
    case = tc.CASES[name]
    loss, scores, grads, dfeats = tc.reference(name)
    assert scores.dtype == np.float64 and dfeats.dtype == np.float64
    assert all(g.dtype == np.float64 for g in grads.values())
    loss32, scores32, grads32, dfeats32 = tc.run_oracle(case, torch.float32)
    assert scores32.dtype == np.float32 and scores.shape == (case.total, case.V)
    print(f"{name}: scores max abs {np.abs(scores32 - scores).max():.2e}, loss rel {abs(loss32 - loss) / abs(loss):.2e}, "
          f"dfeats rel {_rel(dfeats32, dfeats):.2e}")
    assert np.abs(scores32 - scores).max() <= SCORE_ABS
    assert abs(loss32 - loss) <= LOSS_REL * abs(loss)
    assert _rel(dfeats32, dfeats) <= DFEATS_REL
    for k, r in grads.items():
        g = grads32[k].astype(np.float64)
        tight = tc.tight_entries(name, k)
        if tight is not None:  # an fp32 ReLU may take the other side at a near-kink entry
            g, r = g[tight], r[tight]
        scale = max(np.abs(grads[k]).max(), 1e-300)
        if r.size == 0 or not np.any(grads[k]):
            assert not np.any(g), k
            continue
        print(f"   {k:48s} rel {_rel(g, r):.2e} entry {np.abs(g - r).max() / scale:.2e}")
        assert _rel(g, r) <= GRAD_REL, k
        assert np.abs(g - r).max() <= GRAD_ENTRY * scale, k


def test_default_dtype_is_fp32_and_unchanged():
    """dtype left out == dtype=torch.float32, bit for bit (loss, scores, every gradient), with fp32
    tensors throughout, and the result still meets the reference's own golden as tests/test_oracle.py
    asks of it.  (With fp32 the keyword changes no operation: ``.to(torch.float32)`` of an fp32 array,
    ``nn.LSTM(...).to(torch.float32)`` and ``torch.zeros(..., dtype=torch.float32)`` are what the text
    without the keyword did; when it was added, loss, scores and every gradient on train_b4 were
    compared bit for bit with the previous text's.  No digest of them is stored: the bits of a CPU
    GEMM depend on the thread count.)"""
    from oracle.adaptive_oracle import TrainOracle
    g = load_golden("train_b4")
    state = synth.make_weights(123, bias_noise=0.02)
    feats = torch.from_numpy(synth.make_features(4, seed=7))
    caps = torch.from_numpy(g["captions"])
    out = []
    for kw in ({}, {"dtype": torch.float32}):
        m = TrainOracle(state, **kw)
        assert all(v.dtype == torch.float32 for v in m.w.values())
        assert all(p.dtype == torch.float32 for p in m.lstm.parameters())
        loss, packed = m.loss(feats, caps, g["lengths"].tolist())
        loss.backward()
        assert loss.dtype == torch.float32 and packed[0].dtype == torch.float32
        out.append((loss.detach(), packed[0].detach(), {k: v.grad for k, v in m.w.items()}))
    (l0, s0, g0), (l1, s1, g1) = out
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    for k in g0:
        assert g0[k].dtype == torch.float32 and torch.equal(g0[k], g1[k]), k
    np.testing.assert_allclose(s0.numpy(), g["scores"], atol=1e-5, rtol=0)
    assert abs(l0.item() - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    for k, p in g0.items():
        got = p.numpy().reshape(-1).astype(np.float64)
        idx = g["g:" + k + ":idx"] if "g:" + k + ":idx" in g else slice(None)
        ref = np.asarray(g["g:" + k], np.float64)
        assert np.abs(got[idx] - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-30), k


@pytest.mark.parametrize("name", list(tc.CASES))
def test_kink_mask_caps(name):
    case = tc.CASES[name]
    near_a, near_b = tc.kink_mask(name)
    assert near_a.shape == (case.B, 49, case.H) and near_b.shape == (case.B, case.E)
    assert not near_b.any()
    rows_a = near_a.any(axis=(0, 1)).mean()
    pos = near_a.any(axis=2).mean()
    print(f"{name}: W_a rows masked {rows_a:.3%}, dfeats positions masked {pos:.3%}")
    assert rows_a <= tc.MASK_MAX_SHARE and pos <= tc.MASK_MAX_SHARE
    for k in ("encoder.affine_a.weight", "encoder.affine_a.bias", "encoder.affine_b.weight", "encoder.affine_b.bias",
              "dfeats"):
        tight = tc.tight_entries(name, k)
        assert 1.0 - tight.mean() <= tc.MASK_MAX_SHARE, k
    assert tc.tight_entries(name, "decoder.adaptive.mlp.weight") is None


@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_table(name):
    case = tc.CASES[name]
    L = list(case.lengths)
    assert all(n >= 1 for n in L) and L == sorted(L, reverse=True)
    assert L[0] == case.T and sum(L) == case.total
    assert case.H in (256, 512, 768, 1024) and case.E % 32 == 0
    caps = tc.captions(case)
    assert caps.shape == (case.B, case.T + 2) and (caps[:, 0] == 1).all()
    assert caps.min() >= 0 and caps.max() < case.V
    assert (caps == 1).all() == case.constant_captions
    assert tc.features(case).shape == (case.B, 2048, 7, 7)


def test_case_table_reaches_what_it_claims():
    """The sizes the table is there for, restated from the host code of aa_train.hip (decoder_core,
    atb_groups; the GEMMs it launches are aa_tgemm.hip's)."""
    c = tc.CASES
    assert (c["A"].B, c["B"].B, c["C"].B, c["D"].B, c["E"].B, c["F"].B) == (5, 1, 17, 3, 300, 100)
    assert c["C"].lengths == (6, 6, 6, 5, 5, 5, 5, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1)
    assert c["G"].lengths == c["A"].lengths and c["G"].constant_captions

    def fwd_groups(B, T, ts_max=32):   # decoder_core's step groups of k_tr_atten_img
        G = max(min(-(-256 // B), T), -(-T // ts_max))
        TS = -(-T // G)
        return [min(TS, T - g * TS) for g in range(-(-T // TS))]

    def bwd_groups(B, T):              # atb_groups
        g = max(min(-(-512 // B), T), 1)
        TS = -(-T // g)
        return [min(TS, T - i * TS) for i in range(-(-T // TS))]

    assert fwd_groups(300, 40) == [20, 20] and bwd_groups(300, 40) == [20, 20]
    assert fwd_groups(100, 7) == [3, 3, 1] and bwd_groups(100, 7) == [2, 2, 2, 1]
    # case E: every token of the 37 occurs in runs of hundreds of rows
    caps = tc.captions(c["E"])[:, :40]
    assert np.bincount(caps.reshape(-1), minlength=37).min() >= 200
