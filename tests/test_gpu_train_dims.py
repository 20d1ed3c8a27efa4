"""The teacher-forced training step (aa_train_forward / aa_train_backward and their _aux forms,
aa_decoder_forward) at every supported hidden size and at the shape edges of the training step's host
code (aa_train.hip; the GEMM launches and their split-K decisions in aa_tgemm.hip),
against a float64 evaluation of the CPU oracle (tests/train_cases.py: the case table, the reference
and the ReLU kink mask; its conditions are asserted on the CPU in tests/test_train_cases_cpu.py).

Every case runs the product path: ``Encoder2Decoder(Config(E, H, V)).load_synthetic(11,
bias_noise=0.01)``, ``synth.make_features(B, seed=9)``, captions from ``default_rng(5)``, features
with ``requires_grad`` so that dL/dfeats is produced.

Bounds.  fp32 step: the project's measured fp32 bounds, the config-5 constants of
tests/test_gpu_configs.py (profiles/r05_train_tolerances.txt: 4x the GPU's recorded worst at the
default sizes, 8x or more above the CPU fp32 oracle's own distance from float64 on these cases):
packed scores 2e-5 max abs, loss 1e-6 relative, each gradient 2e-5 relative Frobenius and 3e-5 of the
parameter's largest magnitude entry-wise.  For the four tensors downstream of a ReLU (affine_a,
affine_b weight and bias) and dL/dfeats these hold on the entries the kink mask does not touch; a
masked entry (a pre-activation within 1e-5 rms of 0, which fp32 may put on the other side of the ReLU)
keeps tests/test_gpu_train.py's entry bound, 1e-2 of the largest magnitude.  bf16 step (cases A, C, D,
F): tests/test_gpu_train.py's bounds, derived there from the bf16 unit roundoff: scores 2e-2 relative
Frobenius, loss 1e-3 relative, each parameter gradient 5e-2 relative Frobenius.  dL/dfeats of a bf16
step is checked for finiteness and reported only: V = relu(.) comes out of a bf16 GEMM there, so a
fraction f of its entries (those within the GEMM's error, ~2^-8 rms, of the kink) takes the other side,
each such entry of dV is off by its whole value, and dL/dfeats = dV W_a is off by ~sqrt(f) -- a few per
cent by construction, which says nothing about the kernels.

Measured on an MI355X (profiles/train_dims_errors.txt, tools/train_tolerances.py --cases all;
measurements only, the bounds are the ones above):

    fp32   scores max abs   loss rel   worst gradient rel-Frobenius / entry   worst masked entry
    A      9.6e-7           2.0e-8     3.4e-6 / 3.4e-6 (atten.affine_g / _v)  none masked
    B      9.1e-7           6.1e-9     2.2e-6 / 2.7e-6 (atten.affine_v)       none masked
    C      1.3e-6           5.3e-8     1.3e-6 / 2.3e-6 (dfeats / affine_a)    6.9e-3 (dfeats)
    D      9.6e-7           8.5e-8     3.9e-6 / 4.4e-6 (atten.affine_g / _v)  none masked
    E      1.4e-6           8.5e-8     1.5e-6 / 2.6e-6 (dfeats)               4.9e-3 (dfeats)
    F      1.5e-6           1.7e-9     1.4e-6 / 1.8e-6 (dfeats)               4.3e-3 (dfeats)
    G      1.1e-6           5.9e-9     2.6e-6 / 2.3e-6 (atten.affine_g / _v)  none masked
    bf16   scores rel-Frobenius   loss rel   worst parameter gradient rel-Frobenius   dfeats (reported)
    A      1.9e-3                 2.3e-5     9.3e-3 (encoder.affine_a.weight)         4.6e-2
    C      2.8e-3                 1.8e-5     8.0e-3 (encoder.affine_b.weight)         3.3e-2
    D      1.9e-3                 2.0e-4     9.6e-3 (encoder.affine_a.weight)         3.9e-2
    F      2.0e-3                 4.8e-5     7.6e-3 (encoder.affine_b.bias)           3.4e-2

aa_decoder_forward, max abs: scores 1.2e-6, alpha 3.6e-8, beta 2.5e-8, h 1.0e-7, c 2.4e-7.  No case
exceeded a bound, on any tensor: the new sizes and shape edges exposed no defect in the training
step (aa_train.hip, aa_tgemm.hip).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence

import train_cases as tc
from test_gpu_configs import (DECODER_ATT_TOL, DECODER_SCORE_TOL, DECODER_STATE_TOL, GRAD_ENTRY, GRAD_REL, LOSS_REL,
                              SCORE_TOL)
from test_gpu_train import BF16_GRAD_REL, BF16_LOSS_REL, BF16_SCORE_REL
from test_gpu_train import GRAD_ENTRY as KINK_ENTRY

from adaptive_amd import Config, Encoder2Decoder, _lib, synth

pytestmark = pytest.mark.gpu

assert (SCORE_TOL, LOSS_REL, GRAD_REL, GRAD_ENTRY) == (2e-5, 1e-6, 2e-5, 3e-5)
assert (BF16_SCORE_REL, BF16_LOSS_REL, BF16_GRAD_REL, KINK_ENTRY) == (2e-2, 1e-3, 5e-2, 1e-2)
assert (DECODER_SCORE_TOL, DECODER_ATT_TOL, DECODER_STATE_TOL) == (2e-5, 5e-7, 5e-6)

ALL = list(tc.CASES)
SENT_H = "decoder.adaptive.sentinel.affine_h.weight"


def model_for(case, dev):
    cf = Config(adaptive_word_embed_size=case.E, adaptive_lstm_hidden_size=case.H, vocab_length=case.V)
    return Encoder2Decoder(cf).to(dev).load_synthetic(tc.WEIGHT_SEED, bias_noise=tc.BIAS_NOISE)


def gpu_step(name, dev, bf16, two_streams=True):
    """One training step of case ``name`` through the product path -> (loss, packed scores, {param:
    grad}, dfeats), tensors on the device."""
    case = tc.CASES[name]
    model = model_for(case, dev)
    model.train_bf16 = bf16
    model.train_aux_stream = two_streams
    feats = torch.from_numpy(tc.features(case)).to(dev).requires_grad_(True)
    caps = torch.from_numpy(tc.captions(case)).to(dev)
    lengths = list(case.lengths)
    packed = model(feats, caps, lengths)
    assert packed[0].shape == (case.total, case.V)
    targets = pack_padded_sequence(caps[:, 1:], lengths, batch_first=True)[0]
    loss = F.cross_entropy(packed[0], targets)
    loss.backward()
    torch.cuda.synchronize(dev)
    grads = {k: p.grad.detach() for k, p in model.named_parameters()}
    assert set(grads) == {k for _, k in _lib.WEIGHT_FIELDS}
    return loss.item(), packed[0].detach(), grads, feats.grad.detach()


_steps = {}


def step(name, dev, bf16):
    """gpu_step with the default two streams, once per (case, mode) and shared; read-only."""
    key = (name, bool(bf16))
    if key not in _steps:
        _steps[key] = gpu_step(name, dev, bf16)
    return _steps[key]


def rel_fro(got, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def f64(t):
    return t.cpu().double().numpy()


def gradient_errors(name, grads, dfeats):
    """-> {tensor: (rel Frobenius and max-entry / max|ref| over the entries the kink mask leaves,
    max-entry / max|ref| over the masked ones (0 if none))} against the float64 reference."""
    _, _, rgrads, rdfeats = tc.reference(name)
    out = {}
    pairs = [(k, f64(g), rgrads[k]) for k, g in grads.items()]
    pairs.append(("dfeats", f64(dfeats).reshape(dfeats.size(0), -1, 49), rdfeats.reshape(dfeats.size(0), -1, 49)))
    for k, g, r in pairs:
        assert g.shape == r.shape, k
        scale = max(np.abs(r).max(), 1e-300)
        tight = tc.tight_entries(name, k)
        if tight is None:
            tight = np.ones(r.shape, bool)
        loose = float(np.abs(g - r)[~tight].max() / scale) if (~tight).any() else 0.0
        out[k] = (rel_fro(g[tight], r[tight]), float(np.abs(g - r)[tight].max() / scale), loose)
    return out


# ---- accuracy against float64 ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_fp32_step_vs_float64(gpu_device, name):
    rloss, rscores, rgrads, _ = tc.reference(name)
    loss, scores, grads, dfeats = step(name, gpu_device, False)
    s_err = float(np.abs(f64(scores) - rscores).max())
    l_err = abs(loss - rloss) / abs(rloss)
    errs = gradient_errors(name, grads, dfeats)
    print(f"case {name} fp32: scores max abs {s_err:.2e}, loss rel {l_err:.2e}")
    for k, (rel, ent, loose) in errs.items():
        print(f"   {k:48s} rel-Frobenius {rel:.2e}  max-entry/max {ent:.2e}  masked max-entry/max {loose:.2e}")
    assert s_err <= SCORE_TOL
    assert l_err <= LOSS_REL
    for k, (rel, ent, loose) in errs.items():
        if k == SENT_H and not np.any(rgrads[k]):
            assert not np.any(f64(grads[k])), k   # T = 1: an exact zero (see the exactness test)
            continue
        assert rel <= GRAD_REL, (k, rel)
        assert ent <= GRAD_ENTRY, (k, ent)
        assert loose <= KINK_ENTRY, (k, loose)


@pytest.mark.parametrize("name", tc.BF16_CASES)
def test_bf16_step_vs_float64(gpu_device, name):
    rloss, rscores, rgrads, rdfeats = tc.reference(name)
    loss, scores, grads, dfeats = step(name, gpu_device, True)
    s_err = rel_fro(f64(scores), rscores)
    l_err = abs(loss - rloss) / abs(rloss)
    print(f"case {name} bf16: scores rel-Frobenius {s_err:.2e}, loss rel {l_err:.2e}")
    errs = {k: rel_fro(f64(g), rgrads[k]) for k, g in grads.items() if np.any(rgrads[k])}
    for k, e in errs.items():
        print(f"   {k:48s} rel-Frobenius {e:.2e}")
    print(f"   {'dfeats (reported only)':48s} rel-Frobenius {rel_fro(f64(dfeats), rdfeats):.2e}")
    assert torch.isfinite(dfeats).all()
    assert s_err <= BF16_SCORE_REL
    assert l_err <= BF16_LOSS_REL
    for k, e in errs.items():
        assert e <= BF16_GRAD_REL, (k, e)
    # the flag reaches the kernels: not the fp32 step's bits
    assert not torch.equal(scores, step(name, gpu_device, False)[1])


# ---- exact properties -------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_exact_zeros_and_shared_bias_gradient(gpu_device, name, bf16):
    case = tc.CASES[name]
    _, _, grads, _ = step(name, gpu_device, bf16)
    # tokens that occur nowhere in the T columns the steps read get no embedding gradient at all
    used = np.unique(tc.captions(case)[:, :case.T])
    unused = np.setdiff1d(np.arange(case.V), used)
    dE = grads["decoder.embed.weight"].cpu()
    assert torch.isfinite(dE).all()
    assert not dE[torch.from_numpy(unused)].any()
    assert dE[torch.from_numpy(used)].any()
    # b_ih and b_hh enter the gates as a sum: one gradient, bit for bit
    assert torch.equal(grads["decoder.LSTM.bias_hh_l0"], grads["decoder.LSTM.bias_ih_l0"])
    if case.T == 1:
        # the sentinel's h_{t-1} is 0 at t = 0, the only step: the reference's gradient is an exact 0
        assert not np.any(tc.reference(name)[2][SENT_H])
        assert not grads[SENT_H].any()


# ---- outputs are assigned, not accumulated ----------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", ["A", "D"])
def test_outputs_assigned_not_accumulated(gpu_device, name, bf16):
    """aa_train_forward / aa_train_backward through ctypes, the way _TeacherForced calls them, with
    the scores, every gradient buffer and dfeats full of NaN beforehand (outputs only: the workspace
    stays as allocated): every output element finite afterwards and bit-equal to the product path's."""
    case = tc.CASES[name]
    dev = gpu_device
    _, want_scores, want_grads, want_dfeats = step(name, dev, bf16)
    lib = _lib.load()
    model = model_for(case, dev)
    params = [p.detach() for p in model._ref_params()]
    d = model._c_dims()
    B, T, N = case.B, case.T, case.total
    feats = torch.from_numpy(tc.features(case)).to(dev)
    caps = torch.from_numpy(tc.captions(case)).to(dev)
    len_dev = torch.tensor(case.lengths, dtype=torch.int32, device=dev)
    flags = _lib.TRAIN_BF16 if bf16 else 0
    nbytes = lib.aa_train_workspace_bytes(d, B, T)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    scores = torch.full((N, case.V), float("nan"), device=dev)
    w = _lib.RefWeights(*[p.data_ptr() for p in params])
    with torch.cuda.device(dev):
        rc = lib.aa_train_forward(w, d, feats.data_ptr(), B, T, caps.data_ptr(), caps.stride(0), len_dev.data_ptr(),
                                  scores.data_ptr(), N, ws.data_ptr(), nbytes, flags, _lib.stream_handle())
    _lib.check(rc, "train_forward")
    assert torch.equal(scores, want_scores)
    leaf = scores.clone().requires_grad_(True)
    targets = pack_padded_sequence(caps[:, 1:], list(case.lengths), batch_first=True)[0]
    F.cross_entropy(leaf, targets).backward()
    dscores = leaf.grad.contiguous()
    grads = [torch.full_like(p, float("nan")) for p in params]
    dfeats = torch.full_like(feats, float("nan"))
    g = _lib.RefWeights(*[t.data_ptr() for t in grads])
    with torch.cuda.device(dev):
        rc = lib.aa_train_backward(w, d, feats.data_ptr(), B, T, caps.data_ptr(), caps.stride(0), len_dev.data_ptr(),
                                   dscores.data_ptr(), N, g, dfeats.data_ptr(), ws.data_ptr(), nbytes, flags,
                                   _lib.stream_handle())
    _lib.check(rc, "train_backward")
    torch.cuda.synchronize(dev)
    for (_, key), got in zip(_lib.WEIGHT_FIELDS, grads):
        assert torch.isfinite(got).all(), key
        assert torch.equal(got, want_grads[key]), key
    assert torch.isfinite(dfeats).all()
    assert torch.equal(dfeats, want_dfeats)


# ---- two streams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
def test_two_streams_bit_identical_to_one_h1024(gpu_device, bf16):
    two = step("C", gpu_device, bf16)
    one = gpu_step("C", gpu_device, bf16, two_streams=False)
    assert two[0] == one[0]
    assert torch.equal(two[1], one[1])
    for k in two[2]:
        assert torch.equal(two[2][k], one[2][k]), k
    assert torch.equal(two[3], one[3])


# ---- aa_decoder_forward at other sizes --------------------------------------------------------------
@pytest.mark.parametrize("H,E,V,B,T", [(1024, 96, 3001, 5, 3), (256, 32, 37, 17, 34)])
def test_decoder_whole_captions_other_sizes_vs_float64(gpu_device, H, E, V, B, T):
    """decoder(V, v_g, captions, states) against the float64 OracleModel.decoder on the same inputs:
    V, v_g and the states of the float64 encoder, rounded to fp32 for both sides."""
    from oracle.adaptive_oracle import OracleModel
    dev = gpu_device
    dims = synth.Dims(embed=E, hidden=H, vocab=V)
    o = OracleModel(synth.make_weights(tc.WEIGHT_SEED, dims, bias_noise=tc.BIAS_NOISE), dtype=torch.float64)
    feats = torch.from_numpy(synth.make_features(B, seed=tc.FEAT_SEED)).double()
    caps = torch.from_numpy(np.random.default_rng(tc.CAPS_SEED).integers(0, V, size=(B, T)).astype(np.int64))
    caps[:, 0] = 1
    with torch.no_grad():
        V64, vg64, (h64, c64), _ = o.encoder(feats)
        Vf, vgf, hf, cf_ = (x.float().contiguous() for x in (V64, vg64, h64, c64))   # what both sides see
        osc, oal, obe, (oh, oc) = o.decoder(Vf.double(), vgf.double(), caps, (hf.double(), cf_.double()))
    m = Encoder2Decoder(Config(adaptive_word_embed_size=E, adaptive_lstm_hidden_size=H, vocab_length=V)).to(dev)
    m.load_synthetic(tc.WEIGHT_SEED, bias_noise=tc.BIAS_NOISE)
    sc, al, be, (h, c) = m.decoder(Vf.to(dev), vgf.to(dev), caps.to(dev), (hf.to(dev), cf_.to(dev)))
    assert sc.shape == (B, T, V) and al.shape == (B, T, 49) and be.shape == (B, T, 1)
    assert h.shape == (1, B, H) and c.shape == (1, B, H)
    errs = {n: float((x.cpu().double() - y).abs().max())
            for n, x, y in (("scores", sc, osc), ("alpha", al, oal), ("beta", be, obe), ("h", h, oh), ("c", c, oc))}
    print(f"decoder H={H} E={E} V={V} B={B} T={T}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert errs["scores"] <= DECODER_SCORE_TOL
    assert errs["alpha"] <= DECODER_ATT_TOL and errs["beta"] <= DECODER_ATT_TOL
    assert errs["h"] <= DECODER_STATE_TOL and errs["c"] <= DECODER_STATE_TOL
