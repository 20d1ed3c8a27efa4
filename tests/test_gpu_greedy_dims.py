"""Greedy decode (aa_greedy_decode, through ``Encoder2Decoder.sampler``) at hidden 256, 768, 1024 and the
64 x 64 screen of hidden 512, on batches that fill a second row tile, on adversarial near-ties for the
bf16 vocabulary screen, and on all-negative logits, against ``OracleModel.sampler`` (tests/decode_cases.py:
the ``GREEDY`` table, its oracles and the adversarial builder; its conditions are asserted on the CPU in
tests/test_decode_cases_cpu.py).

Every case runs every launch structure of the decode: the default (bf16 screen, rescoring fused into the
next step's k_lstm, the last step's in k_vrescore), ``exact_vocab=True`` (k_vocab: every fp32 logit),
DECODE_SPLIT_RESCORE (k_vrescore every step), DECODE_RS_SELF (the LSTM workgroups rescore) and, where the
screen is the wide one, DECODE_SCREEN4 (k_vscreen2 in place of k_vscreen8).  What the cases reach that no
other test does:

    k_vscreen8<256>, two 128-row tiles; k_lstm<256>, three 64-row tiles     h256_wide (B = 131, E = 32)
    k_vscreen<256 | 768 | 1024>, k_lstm<..>: a tail behind a full tile      h256_narrow, h768, h1024 (B = 67)
    k_vscreen<512> (no other test runs it)                                  h512_narrow
    E = 32 / 96 in the greedy decode                                        h256_wide, h768, h1024_adv
    keys of negative logits, padding columns that would win if unmasked     h256_v100_neg, h768_adv_neg
    a screen that must not lose a winner the bf16 products rank second or third:
      through k_vrescore (T = 1)                                            h256_wide_adv, h768_adv
      through the rescoring in step 1's k_lstm (T = 2)                      h256_narrow_adv, h512_adv,
                                                                            h1024_adv, h768_adv_neg
    DecodePlan off hidden 512                                               h256_wide, h768, h1024

An adversarial case's step 0 has, per row, a decoy column whose bf16 logit leads the true winner's by
0.76 .. 0.92 of 2 ||u|| ||w - bf16(w)||, placed at column 0, at column V - 1, inside one granule, across
granules, across tiles, and as a triple whose winner is third in its granule (so reachable only through
the granule expansion).  The decoy sits below the winner in half of the pairs and above it in the other
half, so neither tie rule can hide a dropped winner.  A screen whose bound lacks the ``||u|| D_g`` term
returns decoys on these rows: checked once against such a build of the library (not kept), which
returned the decoy on all 7 rows of every adversarial case in every screened structure and passed every
plain case here and every greedy test that existed before.  Not reached: the ``||du|| W_g`` term (``u`` is not the
test's to place) and ``SC_ACC(H)`` (forty times smaller than the w-term).

Bounds: the project's own -- ids equal to the oracle's (the fp32 oracle's smallest top-1 / top-2 gap is
asserted above 4 x SCORE_TOL first, and the float64 oracle picks the same ids), alpha / beta within
ATT_TOL = 2e-5 of the float64 oracle, every structure bit for bit equal to the default, ids in [0, V).

Measured on an MI355X: profiles/greedy_dims_errors.txt (the lines this module prints); worst alpha 1.6e-7
and beta 7.0e-8 (both h1024), every row of every structure equal to the oracle's.
"""
import pytest
import torch

import decode_cases as dc
from test_gpu_beam_dims import model_for
from test_gpu_parity import ATT_TOL

from adaptive_amd import DecodePlan, _lib

pytestmark = pytest.mark.gpu

assert ATT_TOL == dc.ATT_TOL == 2e-5


def structures(case):
    out = [("default", 0, {}), ("exact_vocab", 0, {"exact_vocab": True}),
           ("split_rescore", _lib.DECODE_SPLIT_RESCORE, {}), ("rs_self", _lib.DECODE_RS_SELF, {})]
    if case.wide:
        out.append(("screen4", _lib.DECODE_SCREEN4, {}))
    return out


def decode(m, feats, T, extra=0, **kw):
    m.decode_extra_flags = extra
    try:
        return [x.cpu() for x in m.sampler(feats, max_len=T, **kw)]
    finally:
        m.decode_extra_flags = 0


@pytest.mark.parametrize("name", list(dc.GREEDY))
def test_greedy_vs_oracle(name, gpu_device):
    case = dc.GREEDY[name]
    o, d = dc.greedy_oracle(name), dc.greedy_oracle(name, torch.float64)
    gap = float(o["gap"].min())
    assert gap > 4 * dc.SCORE_TOL, f"oracle case too close to call: gap {gap}"
    assert torch.equal(o["ids"], d["ids"])
    if case.negative:
        assert float(o["top"].max()) < 0
    m = model_for(case, gpu_device)
    feats = torch.from_numpy(dc.features(case)).to(gpu_device)
    out = {mode: decode(m, feats, case.T, extra, **kw) for mode, extra, kw in structures(case)}
    failures = []
    for mode, (ids, al, be) in out.items():
        assert ids.shape == (case.B, case.T) and al.shape == (case.B, case.T, 49) and be.shape == (case.B, case.T, 1)
        same = float((ids == o["ids"]).all(1).float().mean())
        e_al = float((al.double() - d["alpha"]).abs().max())
        e_be = float((be.double() - d["beta"]).abs().max())
        print(f"greedy {name} H={case.H} E={case.E} V={case.V} B={case.B} T={case.T} {mode}: gap {gap:.3e}, "
              f"rows equal {same:.3f}, alpha {e_al:.2e}, beta {e_be:.2e} (tol {ATT_TOL:.0e})")
        if not bool(((ids >= 0) & (ids < case.V)).all()):
            failures.append(f"{mode}: token outside [0, {case.V})")
        if case.adversarial:
            for r, win, decoys in dc.designed(case):
                if int(ids[r, 0]) != win:
                    failures.append(f"{mode}: row {r} step 0 gave {int(ids[r, 0])}, the designed winner is {win} "
                                    f"(decoys {decoys})")
        if not torch.equal(ids, o["ids"]):
            failures.append(f"{mode}: ids differ from the oracle's on {1 - same:.1%} of the rows")
        if not (e_al <= ATT_TOL and e_be <= ATT_TOL):
            failures.append(f"{mode}: alpha / beta error {e_al:.3e} / {e_be:.3e}")
        for n, x, y in zip(("ids", "alpha", "beta"), out["default"], (ids, al, be)):
            if not torch.equal(x, y):
                failures.append(f"default and {mode} differ bitwise in {n}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact_vocab"])
@pytest.mark.parametrize("name", ["h256_wide", "h768", "h1024"])
def test_decode_plan_replay_equals_sampler(name, exact, gpu_device):
    """A captured DecodePlan gives ``sampler``'s results bit for bit off hidden 512 too, twice over."""
    case = dc.GREEDY[name]
    m = model_for(case, gpu_device)
    feats = torch.from_numpy(dc.features(case)).to(gpu_device)
    ref = m.sampler(feats, max_len=case.T, exact_vocab=exact)
    assert torch.equal(ref[0].cpu(), dc.greedy_oracle(name)["ids"])
    plan = DecodePlan(m, case.B, max_len=case.T, exact_vocab=exact)
    try:
        for _ in range(2):
            got = plan(feats)
            for n, r, g in zip(("ids", "alpha", "beta"), ref, got):
                assert torch.equal(r, g), n
    finally:
        plan.close()


@pytest.mark.parametrize("mode", ["default", "exact_vocab", "split_rescore", "rs_self", "screen4"])
def test_greedy_batch_invariance_hidden_256_wide(mode, gpu_device):
    """A row's decode does not depend on the rest of the batch (bit-exact): rows 126..130 of the 131 of
    h256_wide (across the 128-row boundary of k_vscreen8 / k_vscreen2 and k_lstm's second 64-row
    boundary, into the tail of 3) alone."""
    case = dc.GREEDY["h256_wide"]
    _, extra, kw = next(s for s in structures(case) if s[0] == mode)
    m = model_for(case, gpu_device)
    feats = torch.from_numpy(dc.features(case)).to(gpu_device)
    big = decode(m, feats, case.T, extra, **kw)
    small = decode(m, feats[126:131].contiguous(), case.T, extra, **kw)
    for n, a, b in zip(("ids", "alpha", "beta"), big, small):
        assert torch.equal(a[126:131], b), n
    assert torch.equal(big[0], dc.greedy_oracle("h256_wide")["ids"])
