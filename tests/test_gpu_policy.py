"""GPU: the self-critical (policy-gradient) step -- aa_policy_loss_* / adaptive_amd.optim.policy_gradient_loss,
Encoder2Decoder.forward_sampled / self_critical_loss, and the decode after an optim.Adam step.

The reference is the float64 restatement tests/policy_oracle.py (mask, tempered log_softmax, gather,
weighted token mean, autograd), for the end-to-end cases behind ``TrainOracle(state, float64)``
(tests/policy_cases.py).  Ids of the numeric tests come from a fixed ``default_rng`` in [3, V) with
``<end>`` = 2 placed by hand, advantages from ``default_rng(7).normal(0.3, 1, R)`` with rows set to 0.

Bounds.  Loss kernels on random logits (``test_gpu_optim._scores``'s recipe at scale 4): tests/test_gpu_optim.py's own,
the operations being the same (fp32 exp / log, sums in another order): |loss - ref| <= 1e-5 sum_live
|A logp| / count + 1e-7 (the sum of magnitudes: the terms have both signs), max |dlogits - ref| <= 1e-5
max |ref|, logp within 1e-5 max(1, |ref|).  End to end, fp32: scores 2e-5 max abs; per tensor
max(the project's bound, 4 x the distance of the CPU fp32 oracle from the float64 one on the same case),
the project's being 2e-5 relative Frobenius and 3e-5 of the largest entry (1e-6 of sum |A logp| / count
for the loss): signed advantages cancel, which raises the relative error of reference and kernels alike;
entries the ReLU kink mask names keep 1e-2 of the largest entry, as in tests/test_gpu_train_dims.py.
bf16: tests/test_gpu_train.py's bounds (scores 2e-2 relative Frobenius, loss 1e-3 of sum |A logp| /
count, each parameter gradient 5e-2 relative Frobenius; dL/dfeats finite, as there).
``self_critical_loss``: |logp of the training forward - logp of the decode| <= 5e-5 + 4e-5 / tau at live
positions (the decode's own logp bound against float64, plus two score errors of 2e-5 each over tau).
``forward_sampled(sampler_gate=True)``, which ``self_critical_loss`` uses, has the same bounds against the
same oracle with the sentinel's W_h set to 0, and an exact-zero gradient for that weight.

Measured on an MI355X: profiles/scst_errors.txt.
"""
import numpy as np
import pytest
import torch

import policy_cases as pc
import policy_oracle as po
import train_cases as tc
from test_gpu_configs import GRAD_ENTRY, GRAD_REL, LOSS_REL, SCORE_TOL
from test_gpu_optim import _scores
from test_gpu_train import BF16_GRAD_REL, BF16_LOSS_REL, BF16_SCORE_REL
from test_gpu_train import GRAD_ENTRY as KINK_ENTRY

from adaptive_amd import Config, Encoder2Decoder, _lib, synth

pytestmark = pytest.mark.gpu

assert (SCORE_TOL, LOSS_REL, GRAD_REL, GRAD_ENTRY) == (2e-5, 1e-6, 2e-5, 3e-5)
assert (BF16_SCORE_REL, BF16_LOSS_REL, BF16_GRAD_REL, KINK_ENTRY) == (2e-2, 1e-3, 5e-2, 1e-2)

SHAPES = [(5, 4, 37, 37), (3, 1, 1, 1), (7, 6, 3001, 3001), (6, 20, 10123, 10200), (2, 3, 12289, 12289)]
UPSTREAM = 1.7


def _inputs(dev, R, T, V, pitch, seed=0):
    """-> logits [T*R, V] (a view of a [T*R, pitch] buffer), ids [R, T] with the hand-placed ends,
    advantage [R] float64, all on the device."""
    wide, _ = _scores(dev, T * R, pitch, seed=seed, scale=4.0)
    ids = po.place_ends(po.make_ids(np.random.default_rng(13 + seed), R, T, V), V)
    return wide[:, :V], torch.from_numpy(ids).to(dev), torch.from_numpy(po.make_advantage(R)).to(dev)


def capi(x, ids, adv, end_id, tau, dloss=UPSTREAM, in_place=False, want_logp=True):
    """aa_policy_loss_forward / _backward through ctypes -> (loss, count, logp, dlogits [T*R, V])."""
    lib = _lib.load()
    dev = x.device
    R, T = ids.shape
    V = x.size(1)
    adv = adv.float().contiguous()
    nbytes = lib.aa_policy_loss_workspace_bytes(R, T)
    assert nbytes == R * T * 12
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss = torch.full((), 7.0, device=dev)
    count = torch.full((1,), 7.0, device=dev)
    logp = torch.full((R, T), 7.0, device=dev) if want_logp else None
    d = torch.full((), dloss, device=dev)
    if in_place:  # a private copy of the buffer, pitch and all
        buf = torch.empty(x.size(0), x.stride(0), device=dev)
        x = buf[:, :V].copy_(x)
        dx = x
    else:
        dx = torch.full((R * T, V), 7.0, device=dev)
    with torch.cuda.device(dev):
        rc = lib.aa_policy_loss_forward(x.data_ptr(), x.stride(0), R, T, V, ids.data_ptr(), ids.stride(0),
                                        adv.data_ptr(), end_id, tau, loss.data_ptr(), count.data_ptr(), _lib.ptr(logp),
                                        ws.data_ptr(), nbytes, _lib.stream_handle())
        _lib.check(rc, "policy_loss_forward")
        rc = lib.aa_policy_loss_backward(x.data_ptr(), x.stride(0), R, T, V, ids.data_ptr(), ids.stride(0),
                                         adv.data_ptr(), end_id, tau, d.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                         nbytes, dx.data_ptr(), dx.stride(0), _lib.stream_handle())
        _lib.check(rc, "policy_loss_backward")
    torch.cuda.synchronize(dev)
    return loss, count, logp, dx


def _reference(x, ids, adv, end_id, tau):
    xr = x.detach().cpu().double().contiguous().requires_grad_(True)
    loss, count, logp, live = po.policy_loss(xr, ids.cpu(), adv.cpu().float().double(), end_id, tau)
    (loss * UPSTREAM).backward()
    mag = float((adv.cpu().float().double().unsqueeze(1) * logp.detach()).abs().sum() / count)
    return loss.item(), int(count), logp.detach(), live, xr.grad, mag


def _dead_rows(live, adv, R, T):
    """[T*R] bool, t-major: the rows whose gradient must be an exact +0."""
    dead = ~live | (adv.cpu() == 0).unsqueeze(1)
    return dead.t().reshape(-1)


# ---- 3. the loss kernels against the float64 oracle -------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 0.7])
@pytest.mark.parametrize("R,T,V,pitch", SHAPES)
def test_loss_kernels_vs_float64(gpu_device, R, T, V, pitch, tau):
    from adaptive_amd.optim import policy_gradient_loss
    dev = gpu_device
    x, ids, adv = _inputs(dev, R, T, V, pitch)
    assert x.stride(0) == pitch
    for end_id in (po.END, -1):
        rloss, rcount, rlogp, live, rgrad, mag = _reference(x, ids, adv, end_id, tau)
        xa = x.detach().requires_grad_(True)
        loss, logp = policy_gradient_loss(xa, ids, adv, end_id, tau, return_logp=True)
        (loss * UPSTREAM).backward()
        g = xa.grad
        l_err = abs(loss.item() - rloss)
        p_err = float(((logp.cpu().double() - rlogp).abs() / rlogp.abs().clamp_min(1.0)).max())
        g_err = float((g.cpu().double() - rgrad).abs().max())
        g_max = float(rgrad.abs().max())
        print(f"R={R} T={T} V={V} tau={tau} end_id={end_id}: live {rcount}/{R * T}, loss err {l_err:.2e} (bound "
              f"{1e-5 * mag + 1e-7:.2e}), logp err {p_err:.2e}, dlogits err / max|ref| "
              f"{g_err / max(g_max, 1e-300):.2e}")
        assert l_err <= 1e-5 * mag + 1e-7
        assert p_err <= 1e-5
        assert g_err <= 1e-5 * g_max
        # the C-ABI directly: the same bits as the autograd function, and the exact count
        closs, ccount, clogp, cdx = capi(x, ids, adv, end_id, tau)
        assert ccount.item() == rcount == int(live.sum())
        assert torch.equal(closs, loss.detach()) and torch.equal(clogp, logp) and torch.equal(cdx, g)
        assert (logp.cpu()[~live] == 0).all()
        # dead rows and rows of an advantage-0 caption: +0, bit for bit
        dead = _dead_rows(live, adv, R, T).to(dev)
        if end_id == po.END and V > po.END and R > 1:
            assert dead.any() and not dead.all()
        assert not g[dead].any() and not torch.signbit(g[dead]).any()
        # ... and never read: NaN logits there change nothing (no logp output: the forward skips them too)
        xn = x.clone()
        xn[dead] = float("nan")
        xn.requires_grad_(True)
        loss_n = policy_gradient_loss(xn, ids, adv, end_id, tau)
        (loss_n * UPSTREAM).backward()
        assert torch.equal(loss_n.detach(), loss.detach())
        assert torch.equal(xn.grad, g)
        assert not torch.signbit(xn.grad[dead]).any()


# ---- 4. determinism, in place, poisoning ------------------------------------------------------------
@pytest.mark.parametrize("R,T,V,pitch", [(6, 20, 10123, 10200), (2, 3, 12289, 12300)])
def test_deterministic_in_place_and_poisoned(gpu_device, R, T, V, pitch):
    dev = gpu_device
    x, ids, adv = _inputs(dev, R, T, V, pitch, seed=3)
    tau = 0.7
    a = capi(x, ids, adv, po.END, tau)
    b = capi(x, ids, adv, po.END, tau)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    assert torch.isfinite(a[0]) and torch.isfinite(a[3]).all()
    c = capi(x, ids, adv, po.END, tau, in_place=True)   # dlogits over the logits, the same pitch
    for p, q in zip(a, c):
        assert torch.equal(p, q)
    # an id == V after <end> (row 0 ends at position 0): not looked at
    late = ids.clone()
    late[0, T - 1] = V
    for p, q in zip(a, capi(x, late, adv, po.END, tau)):
        assert torch.equal(p, q)
    # the same id at a live position (row 1 is live throughout): NaN loss, NaN gradient row, the rest as before
    bad = ids.clone()
    bad[1, 0] = V
    loss, count, logp, dx = capi(x, bad, adv, po.END, tau)
    assert torch.isnan(loss).item() and count.item() == a[1].item()
    assert torch.isnan(logp[1, 0]).item() and torch.isnan(dx[1]).all()    # row t*R + r = 0*R + 1
    keep = torch.ones(R * T, dtype=torch.bool, device=dev)
    keep[1] = False
    assert torch.equal(dx[keep], a[3][keep])


# ---- 5. end to end against float64 --------------------------------------------------------------------
def model_for(case, dev):
    cf = Config(adaptive_word_embed_size=case.E, adaptive_lstm_hidden_size=case.H, vocab_length=case.V)
    return Encoder2Decoder(cf).to(dev).load_synthetic(tc.WEIGHT_SEED, bias_noise=tc.BIAS_NOISE)


def gpu_step(name, dev, bf16, gate=False):
    from adaptive_amd.optim import policy_gradient_loss
    case = pc.CASES[name]
    model = model_for(case, dev)
    model.train_bf16 = bf16
    feats = torch.from_numpy(pc.features(case)).to(dev).requires_grad_(True)
    ids = torch.from_numpy(pc.ids(case)).to(dev)
    adv = torch.from_numpy(po.make_advantage(case.R)).to(dev)           # float64, as CiderD's
    scores = model.forward_sampled(feats, ids, case.N, sampler_gate=gate)
    assert scores.shape == (case.T * case.R, case.V)
    loss, logp = policy_gradient_loss(scores, ids, adv, po.END, 1.0, return_logp=True)
    loss.backward()
    torch.cuda.synchronize(dev)
    grads = {k: p.grad.detach().cpu().double().numpy() for k, p in model.named_parameters()}
    assert set(grads) == {k for _, k in _lib.WEIGHT_FIELDS}
    assert feats.grad.shape == feats.shape
    return loss.item(), scores.detach().cpu().double().numpy(), grads, feats.grad.cpu().double().numpy(), logp.cpu()


def rel_fro(got, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_end_to_end_fp32_vs_float64(gpu_device, name, gate):
    rloss, rscores, rgrads, rdfeats, rlogp, mag = pc.reference(name, torch.float64, gate)
    # the CPU fp32 oracle's own distance from float64 on this case: measures the reference, not the kernels
    oloss, _, ograds, odfeats, _, _ = pc.reference(name, torch.float32, gate)
    own = pc.gradient_errors(name, ograds, odfeats, gate)
    own_loss = abs(oloss - rloss) / mag
    loss, scores, grads, dfeats, logp = gpu_step(name, gpu_device, False, gate)
    s_err = float(np.abs(scores - rscores).max())
    l_err = abs(loss - rloss) / mag
    errs = pc.gradient_errors(name, grads, dfeats, gate)
    if gate:  # the weight is not in the gated forward: an exact zero, and the scores are not the default's
        assert not np.any(grads[pc.SENT_H])
        assert np.abs(scores - pc.reference(name)[1]).max() > 10 * SCORE_TOL  # (each is within SCORE_TOL of its own)
    print(f"case {name} fp32{' (sampler gate)' if gate else ''}: scores max abs {s_err:.2e}, loss err / (sum|A logp|/count) {l_err:.2e} "
          f"(CPU fp32 oracle {own_loss:.2e})")
    for k, (rel, ent, loose) in errs.items():
        print(f"   {k:48s} rel-Frobenius {rel:.2e} (oracle {own[k][0]:.2e})  max-entry/max {ent:.2e} "
              f"(oracle {own[k][1]:.2e})  masked max-entry/max {loose:.2e}")
    assert s_err <= SCORE_TOL
    assert l_err <= max(LOSS_REL, 4 * own_loss)
    assert float((logp.double() - torch.from_numpy(rlogp)).abs().max()) <= 2 * SCORE_TOL
    for k, (rel, ent, loose) in errs.items():
        assert np.any(rgrads[k]) if k != "dfeats" else np.any(rdfeats), k
        assert (k == pc.SENT_H) <= (not gate)
        assert rel <= max(GRAD_REL, 4 * own[k][0]), (k, rel)
        assert ent <= max(GRAD_ENTRY, 4 * own[k][1]), (k, ent)
        assert loose <= KINK_ENTRY, (k, loose)


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("name", [k for k, c in pc.CASES.items() if c.bf16])
def test_end_to_end_bf16_vs_float64(gpu_device, name, gate):
    rloss, rscores, rgrads, rdfeats, _, mag = pc.reference(name, torch.float64, gate)
    loss, scores, grads, dfeats, _ = gpu_step(name, gpu_device, True, gate)
    if gate:
        assert not np.any(grads.pop(pc.SENT_H))
    s_err = rel_fro(scores, rscores)
    l_err = abs(loss - rloss) / mag
    print(f"case {name} bf16{' (sampler gate)' if gate else ''}: scores rel-Frobenius {s_err:.2e}, loss err / (sum|A logp|/count) {l_err:.2e}")
    errs = {k: rel_fro(g, rgrads[k]) for k, g in grads.items()}
    for k, e in errs.items():
        print(f"   {k:48s} rel-Frobenius {e:.2e}")
    print(f"   {'dfeats (reported only)':48s} rel-Frobenius {rel_fro(dfeats, rdfeats):.2e}")
    assert np.isfinite(dfeats).all()
    assert s_err <= BF16_SCORE_REL
    assert l_err <= BF16_LOSS_REL
    for k, e in errs.items():
        assert e <= BF16_GRAD_REL, (k, e)


# ---- 6. decode sees the optimiser's step ------------------------------------------------------------
def _tiny(dev):
    cf = Config(adaptive_word_embed_size=32, adaptive_lstm_hidden_size=256, vocab_length=100)
    return cf, Encoder2Decoder(cf).to(dev).load_synthetic()


def test_decode_sees_adam_step(gpu_device):
    """optim.Adam updates the parameters through raw pointers; the decode's packed weights must follow."""
    from adaptive_amd.optim import Adam
    dev = gpu_device
    cf, model = _tiny(dev)
    feats = torch.from_numpy(synth.make_features(4, seed=0)).to(dev)

    def decodes(m):
        return (m.sampler(feats, 8)[0], *m.sample(feats, 8, seed=3)[:2], *m.beam_search(feats, 8, 3)[3:])

    before = decodes(model)
    g = torch.Generator().manual_seed(0)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    # lr: the first Adam step moves every weight by lr * sign(gradient); the synthetic weights at this size
    # decode one token throughout, and 1.0 is what it takes for the reloaded model to decode another
    # (0.05, 0.2 and 0.5 leave the CPU oracle's greedy ids nearly or wholly unchanged)
    Adam(model.parameters(), lr=1.0).step()
    after = decodes(model)
    fresh = Encoder2Decoder(cf).to(dev)
    fresh.load_state_dict(model.state_dict())
    want = decodes(fresh)
    torch.cuda.synchronize(dev)
    for what, b, a, w in zip(("sampler ids", "sample ids", "sample logp", "beam seqs", "beam scores"), before, after,
                             want):
        assert not torch.equal(w, b), what + ": the step changed nothing (precondition)"
        assert torch.equal(a, w), what + ": decoded with the weights packed before the step"


# ---- 7. the whole step on a tiny corpus -------------------------------------------------------------
def _tiny_refs(B):
    """Five made-up references of 5..7 tokens per image."""
    rng = np.random.default_rng(2)
    return [[rng.integers(3, 100, size=int(rng.integers(5, 8))).tolist() for _ in range(5)] for _ in range(B)]


def test_self_critical_step(gpu_device):
    from adaptive_amd.cider import CiderD
    from adaptive_amd.optim import Adam, clip_grad_norm_, policy_gradient_loss
    dev = gpu_device
    B, N, T, tau, seed = 3, 2, 6, 1.0, 4
    cf, model = _tiny(dev)
    scorer = CiderD(_tiny_refs(B), end_id=po.END).to(dev)
    feats = torch.from_numpy(synth.make_features(B, seed=1)).to(dev)
    kw = dict(num_samples=N, max_len=T, temperature=tau, seed=seed)
    loss, info = model.self_critical_loss(feats, scorer, **kw)
    loss2, info2 = model.self_critical_loss(feats, scorer, **kw)
    assert torch.equal(loss2.detach(), loss.detach())
    for a, b in zip(info, info2):
        assert torch.equal(a, b)
    assert all(isinstance(t, torch.Tensor) and t.device.type == "cuda" for t in info)
    assert info.sample_ids.shape == (B * N, T) and info.greedy_ids.shape == (B, T)
    assert info.advantage.shape == (B * N,) and info.advantage.dtype == torch.float64
    # the pieces are what the public calls give
    sid, slogp = model.sample(feats, T, tau, seed, num_samples=N)[:2]
    assert torch.equal(info.sample_ids, sid) and torch.equal(info.sample_logp, slogp)
    assert torch.equal(info.greedy_ids, model.sampler(feats, T)[0])
    assert torch.equal(info.advantage, scorer.self_critical(info.sample_ids, info.greedy_ids, N))
    assert torch.equal(info.reward_sample - info.reward_greedy.repeat_interleave(N), info.advantage)
    assert info.advantage.ne(0).any(), "every advantage is 0: the corpus gives the step nothing to learn from"
    scores = model.forward_sampled(feats, info.sample_ids, N, sampler_gate=True)
    l3, logp3 = policy_gradient_loss(scores, info.sample_ids, info.advantage, po.END, tau, return_logp=True)
    assert torch.equal(l3.detach(), loss.detach()) and torch.equal(logp3, info.logp)
    live = po.live_mask(info.sample_ids.cpu()).to(dev)
    assert (info.logp[~live] == 0).all() and (info.logp[live] < 0).all()
    # backward, clip, Adam, and the next step
    opt = Adam(model.parameters(), lr=1e-3)
    loss.backward()
    clip_grad_norm_(model.decoder.LSTM.parameters(), 5.0)
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert any(p.grad.any() for p in model.parameters())
    opt.step()
    opt.zero_grad()
    loss4, info4 = model.self_critical_loss(feats, scorer, **kw)
    loss4.backward()
    assert torch.isfinite(loss4).item()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


def test_training_forward_reproduces_the_sampling_policy(gpu_device):
    """|logp of the training forward - logp of the decode| <= 5e-5 + 4e-5 / tau at every live position of
    ``self_critical_loss``'s draws.

    ``self_critical_loss`` runs ``forward_sampled(sampler_gate=True)``: the decoders' one-token step
    computes the sentinel gate without its ``h_{t-1} W_h`` term, as the reference's ``sampler`` does
    (Decoder.forward with a single token starts from a zero ``hiddens_t_1``, adaptive_attention.py:116-122),
    and the loss must differentiate the distribution the tokens were drawn from.  The default,
    teacher-forced gate has the term from step 1 on and is a different distribution: measured on an MI355X
    at this size, 1.06e-2 from the decode's logp at the later positions against 4.8e-7 at step 0, which
    the last assertion states as a lower bound of 10 x the tolerance."""
    from adaptive_amd.cider import CiderD
    dev = gpu_device
    B, N, T, tau = 3, 2, 6, 1.0
    _, model = _tiny(dev)
    scorer = CiderD(_tiny_refs(B), end_id=po.END).to(dev)
    feats = torch.from_numpy(synth.make_features(B, seed=1)).to(dev)
    _, info = model.self_critical_loss(feats, scorer, num_samples=N, max_len=T, temperature=tau, seed=4)
    live = po.live_mask(info.sample_ids.cpu()).to(dev)
    gap = (info.logp - info.sample_logp).abs()
    print(f"max |logp(train forward) - logp(decode)|: step 0 {gap[:, 0].max().item():.2e}, live positions "
          f"{gap[live].max().item():.2e} (live {int(live.sum())}/{B * N * T})")
    assert gap[live].max().item() <= 5e-5 + 4e-5 / tau
    from adaptive_amd.optim import policy_gradient_loss
    plain = model.forward_sampled(feats, info.sample_ids, N)
    _, logp_tf = policy_gradient_loss(plain, info.sample_ids, info.advantage, po.END, tau, return_logp=True)
    gap_tf = (logp_tf - info.sample_logp).abs()
    print(f"teacher-forced gate: step 0 {gap_tf[:, 0].max().item():.2e}, live positions {gap_tf[live].max().item():.2e}")
    assert gap_tf[:, 0].max().item() <= 5e-5 + 4e-5 / tau
    assert gap_tf[live].max().item() > 10 * (5e-5 + 4e-5 / tau)
