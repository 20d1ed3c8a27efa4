"""CPU: the float64 restatement of the policy-gradient loss (tests/policy_oracle.py), the conditions
tests/test_gpu_policy.py rests on (tests/policy_cases.py's kink mask), and the host side of the
feature: argument codes of aa_policy_loss_* on fake pointers (no device work: there is no GPU here) and
the Python-level errors of adaptive_amd.optim.policy_gradient_loss / Encoder2Decoder.forward_sampled."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import policy_cases as pc
import policy_oracle as po
import train_cases as tc


@pytest.fixture(scope="module")
def lib():
    from adaptive_amd import _lib
    return _lib.load()


def _random_case(R=5, T=4, V=37, seed=0):
    rng = np.random.default_rng(seed)
    scores = torch.from_numpy(rng.normal(0.0, 4.0, (T * R, V))).requires_grad_(True)
    ids = po.make_ids(rng, R, T, V)
    return scores, ids


# ---- 1. oracle properties ---------------------------------------------------------------------------
def test_oracle_is_cross_entropy_without_mask_and_weights():
    R, T, V = 5, 4, 37
    scores, ids = _random_case(R, T, V)
    loss, count, logp, live = po.policy_loss(scores, torch.from_numpy(ids), torch.ones(R, dtype=torch.float64))
    assert live.all() and int(count) == R * T
    targets = torch.from_numpy(ids).t().reshape(-1)               # packed: row t*R + r
    ce = F.cross_entropy(scores, targets)
    assert abs(loss.item() - ce.item()) <= 1e-14 * abs(ce.item())
    g, = torch.autograd.grad(loss, scores)
    g_ce, = torch.autograd.grad(ce, scores)
    assert (g - g_ce).abs().max().item() <= 1e-15


def test_oracle_mask_zero_rows_row_sums_and_linearity():
    R, T, V = 5, 4, 37
    scores, ids = _random_case(R, T, V)
    ids[0, 0] = po.END          # only position 0 live
    ids[1, T - 1] = po.END      # every position live
    ids[2, 1] = ids[2, 2] = po.END
    tid = torch.from_numpy(ids)
    live = po.live_mask(tid)
    assert live.tolist() == [[True, False, False, False], [True] * 4, [True, True, False, False], [True] * 4,
                             [True] * 4]
    assert po.live_mask(tid, -1).all()
    adv = torch.from_numpy(po.make_advantage(R))
    assert (adv == 0).sum() == 2
    for tau in (1.0, 0.7):
        loss, count, logp, _ = po.policy_loss(scores, tid, adv, po.END, tau)
        assert int(count) == int(live.sum()) == 15
        assert (logp[~live] == 0).all() and (logp[live] < 0).all()
        g, = torch.autograd.grad(loss, scores)
        g = g.view(T, R, V).transpose(0, 1)
        dead = ~live | (adv == 0).unsqueeze(1)
        assert not g[dead].any()
        assert g[~dead].abs().sum(-1).min() > 0
        assert g.sum(-1).abs().max().item() <= 1e-15      # softmax minus one-hot: every row sums to 0
        loss2, _, _, _ = po.policy_loss(scores, tid, adv * -2.5, po.END, tau)
        assert abs(loss2.item() + 2.5 * loss.item()) <= 1e-14 * abs(loss.item())
    # an id at a dead position is not looked at
    ids2 = ids.copy()
    ids2[0, 2] = V + 5
    assert po.policy_loss(scores, torch.from_numpy(ids2), adv)[0].item() == po.policy_loss(scores, tid, adv)[0].item()


@pytest.mark.parametrize("name", list(pc.CASES))
def test_policy_cases_and_their_kink_mask(name):
    """The cases are what the table says, and the kink mask may exclude at most MASK_MAX_SHARE of any
    tensor (the condition of tests/test_gpu_policy.py's tight bounds)."""
    case = pc.CASES[name]
    ids = pc.ids(case)
    assert ids.shape == (case.R, case.T) and ids.min() >= 2 and ids.max() < case.V
    live = po.live_mask(torch.from_numpy(ids)).numpy()
    assert live[0].all() and ids[0, -1] == po.END                      # <end> at T - 1: all trained
    assert live[1].sum() == min(2, case.T)                             # <end> at position 1
    assert live[2].sum() == 1 and (ids[2] == po.END).sum() == 2        # <end> at 0 and again later
    assert live[3:].all() and not (ids[3:] == po.END).any()            # absent
    adv = po.make_advantage(case.R)
    assert (adv == 0).sum() == 2 and adv[0] != 0
    assert (adv.reshape(case.B, case.N) != 0).any(axis=1).all()        # every image has a caption that counts
    caps = pc.input_captions(ids)
    assert (caps[:, 0] == 1).all() and (caps[:, 1:] == ids[:, :-1]).all()
    near_a, near_b = pc.kink_mask(name)
    assert near_a.shape == (case.B, 49, case.H) and near_b.shape == (case.B, case.E)
    assert near_a.any(axis=(0, 1)).mean() <= tc.MASK_MAX_SHARE and near_a.any(axis=2).mean() <= tc.MASK_MAX_SHARE
    for k in ("encoder.affine_a.weight", "encoder.affine_a.bias", "encoder.affine_b.weight", "encoder.affine_b.bias",
              "dfeats"):
        assert 1.0 - pc.tight_entries(name, k).mean() <= tc.MASK_MAX_SHARE, k
    assert pc.tight_entries(name, "decoder.adaptive.mlp.weight") is None


# ---- 2. argument codes and Python-level errors ------------------------------------------------------
def test_capi_argument_codes(lib):
    assert lib.aa_abi_version() == 17
    wb = lib.aa_policy_loss_workspace_bytes
    assert wb(6, 20) == 6 * 20 * 12 and wb(1, 1) == 12
    assert wb(0, 5) == 0 and wb(5, 0) == 0 and wb(-1, 5) == 0
    assert wb(65536, 32768) == 0                                   # R T = 2^31
    assert wb(65536, 32767) == (2 ** 31 - 65536) * 12
    P = 256  # a fake, aligned, non-NULL pointer: every call below returns before any device work
    fwd, bwd = lib.aa_policy_loss_forward, lib.aa_policy_loss_backward

    def f(logits=P, ldx=40, R=6, T=5, V=37, ids=P, ids_ld=5, adv=P, end_id=2, tau=1.0, loss=P, count=P, logp=None,
          ws=P, nbytes=360):
        return fwd(logits, ldx, R, T, V, ids, ids_ld, adv, end_id, tau, loss, count, logp, ws, nbytes, None)

    def b(logits=P, ldx=40, R=6, T=5, V=37, ids=P, ids_ld=5, adv=P, end_id=2, tau=1.0, dloss=P, count=P, ws=P,
          nbytes=360, dlogits=512, lddx=37):
        return bwd(logits, ldx, R, T, V, ids, ids_ld, adv, end_id, tau, dloss, count, ws, nbytes, dlogits, lddx, None)

    for kw in (dict(R=0), dict(T=0), dict(V=0), dict(R=-1), dict(ldx=36), dict(ids_ld=4), dict(tau=0.0),
               dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(R=65536, T=32768, ids_ld=32768)):
        assert f(**kw) == -3, kw
        assert b(**kw) == -3, kw
    assert b(lddx=36) == -3
    assert b(dlogits=P, lddx=37) == -3                             # in place with another pitch
    # the shape is judged before the pointers, the pointers before the workspace size
    assert f(R=0, logits=None) == -3 and f(logits=None, nbytes=0) == -1
    assert b(lddx=36, dlogits=None) == -3 and b(dlogits=None, nbytes=0) == -1
    for kw in (dict(logits=None), dict(ids=None), dict(adv=None), dict(loss=None), dict(count=None), dict(ws=None)):
        assert f(**kw) == -1, kw
    for kw in (dict(logits=None), dict(ids=None), dict(adv=None), dict(dloss=None), dict(count=None), dict(ws=None),
               dict(dlogits=None)):
        assert b(**kw) == -1, kw
    assert f(nbytes=359) == -4 and b(nbytes=359) == -4


def test_policy_gradient_loss_python_errors(lib):
    """Shapes, dtypes and the temperature are judged first; right arguments on the CPU then raise, as
    the rest of adaptive_amd.optim does (there is no CPU path)."""
    from adaptive_amd.optim import PolicyGradientLoss, policy_gradient_loss as f
    R, T, V = 3, 4, 10
    scores, ids, adv = torch.zeros(T * R, V), torch.zeros(R, T, dtype=torch.int64), torch.zeros(R)
    for a in (adv, adv.double()):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            f(scores, ids, a)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        f(scores, ids, adv, end_id=-1, temperature=0.7, return_logp=True)
    crit = PolicyGradientLoss(end_id=3, temperature=0.5)
    assert (crit.end_id, crit.temperature) == (3, 0.5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        crit(scores, ids, adv)
    with pytest.raises(TypeError):
        f(scores.double(), ids, adv)
    with pytest.raises(ValueError):
        f(scores.view(-1), ids, adv)
    with pytest.raises(ValueError):
        f(scores[:-1], ids, adv)                      # not T * R rows
    with pytest.raises(ValueError):
        f(scores, ids.view(-1), adv)
    with pytest.raises(TypeError):
        f(scores, ids.int(), adv)
    with pytest.raises(ValueError):
        f(scores, ids, adv[:-1])
    with pytest.raises(TypeError):
        f(scores, ids, adv.half())
    for tau in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            f(scores, ids, adv, temperature=tau)


def test_forward_sampled_python_errors():
    from adaptive_amd import Config, Encoder2Decoder
    model = Encoder2Decoder(Config(adaptive_word_embed_size=32, adaptive_lstm_hidden_size=256, vocab_length=37))
    feats = torch.zeros(2, 2048, 7, 7)
    ok = torch.zeros(4, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CUDA"):      # right shapes, CPU tensors
        model.forward_sampled(feats, ok, num_samples=2)
    with pytest.raises(ValueError):
        model.forward_sampled(feats, ok, num_samples=0)
    with pytest.raises(ValueError, match=r"\[6, T >= 1\]"):
        model.forward_sampled(feats, ok, num_samples=3)  # ids are not [B * N, T]
    with pytest.raises(ValueError):
        model.forward_sampled(feats, ok)                 # num_samples defaults to 1
    with pytest.raises(ValueError):
        model.forward_sampled(feats, torch.zeros(4, dtype=torch.int64), num_samples=2)
    with pytest.raises(ValueError):
        model.forward_sampled(feats, torch.zeros(4, 0, dtype=torch.int64), num_samples=2)
    with pytest.raises(TypeError):
        model.forward_sampled(feats, ok.int(), num_samples=2)
