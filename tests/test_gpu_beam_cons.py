"""The constrained beam search (aa_beam_decode_cx, through ``Encoder2Decoder.beam_search(suppress_ids=,
min_length=, no_repeat_ngram=, no_end_after=)``, and aa_beam_select_step) against ``BeamConsOracle``
(tests/beam_cons_oracle.py) on the cases of tests/beam_cons_cases.py, whose admissibility is asserted on the
CPU in tests/test_beam_cons_cpu.py, against oracle-free bitwise identities, and -- the selection kernel alone,
on hand-built logits -- against a numpy restatement.

Bounds: seqs, ids, lengths and group equal the oracle's (both fp32 margins exceed 4 x SCORE_TOL); scores within
SCORE_TOL = 5e-5 and alpha / beta within ATT_TOL = 2e-5 of the float64 oracle -- the project's beam bounds,
from tests/test_gpu_beam.py; rank_scores within SCORE_TOL + 1e-6 |rank| (tests/test_gpu_beam_div.py's bound);
the default and ``exact_vocab=True`` agree bit for bit.  ``fast=True`` runs on the cases whose base
tests/test_gpu_beam_div.py runs it on, to the same bounds.

Measured on an MI355X: profiles/beam_cons_errors.txt (the lines this module prints).
"""
import ctypes

import numpy as np
import pytest
import torch

import beam_cons_cases as cases
import beam_div_cases
import decode_cases as dc
from beam_cons_oracle import BeamConsOracle
from test_gpu_beam import ATT_TOL, SCORE_TOL
from test_gpu_beam_dims import MODES, model_for

from adaptive_amd import Config, Encoder2Decoder, _lib

pytestmark = pytest.mark.gpu

assert (SCORE_TOL, ATT_TOL) == (dc.SCORE_TOL, dc.ATT_TOL) == (5e-5, 2e-5)
RANK_REL = 1e-6
NAMES = ("ids", "alpha", "beta", "seqs", "scores", "lengths", "rank_scores", "group")
END = 2
FAST_BASES = {c.base for c in beam_div_cases.DIV.values()}


def _compare(tag, b, got, o, d, failures):
    """One mode's outputs against the fp32 oracle's decisions and the float64 oracle's numbers."""
    ids, al, be, seqs, sc, lengths, rank, group = got
    assert seqs.shape == (b.B, seqs.size(1), b.T) and sc.shape == lengths.shape == rank.shape == group.shape
    same = float((seqs == o["seqs"]).flatten(1).all(1).float().mean())
    e_sc = float((sc.double() - d["scores"]).abs().max())
    e_al = float((al.double() - d["alpha"]).abs().max())
    e_be = float((be.double() - d["beta"]).abs().max())
    r_err = (rank.double() - d["rank_scores"]).abs()
    r_tol = SCORE_TOL + RANK_REL * d["rank_scores"].abs()
    print(f"beam_cons {tag}: margins {o['sel_margin']:.3e} / {o['rank_margin']:.3e}, images equal {same:.3f}, "
          f"max |score - float64| {e_sc:.3e} (tol {SCORE_TOL:.0e}), |rank - float64| {float(r_err.max()):.3e} "
          f"(tol {float(r_tol.min()):.3e}), alpha {e_al:.2e}, beta {e_be:.2e} (tol {ATT_TOL:.0e})")
    if not bool(((seqs >= 0) & (seqs < b.V)).all()):
        failures.append(f"{tag}: token outside [0, {b.V})")
    if not torch.equal(seqs, o["seqs"]):
        failures.append(f"{tag}: seqs differ from the oracle's on {1 - same:.1%} of the images")
    for k, x in (("ids", ids), ("lengths", lengths), ("group", group)):
        if not torch.equal(x, o[k]):
            failures.append(f"{tag}: {k} differ from the oracle's")
    if not e_sc <= SCORE_TOL:
        failures.append(f"{tag}: score error {e_sc:.3e}")
    if not bool((r_err <= r_tol).all()):
        failures.append(f"{tag}: rank score error {float(r_err.max()):.3e}")
    if not (e_al <= ATT_TOL and e_be <= ATT_TOL):
        failures.append(f"{tag}: alpha / beta error {e_al:.3e} / {e_be:.3e}")


@pytest.mark.parametrize("name", list(cases.CONS))
def test_beam_cons_vs_oracle(name, gpu_device):
    case = cases.CONS[name]
    b = case.beam
    o, d = cases.oracle(name), cases.oracle(name, torch.float64)
    assert o["sel_margin"] > 4 * SCORE_TOL and o["rank_margin"] > 4 * SCORE_TOL, "oracle case too close to call"
    for k in ("seqs", "lengths", "group", "ids"):
        assert torch.equal(o[k], d[k]), k
    assert cases.blocked(o) == case.blocked
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    out, failures = {}, []
    for mode, kw in MODES:
        if mode == "fast" and case.base not in FAST_BASES:
            continue
        out[mode] = [x.cpu() for x in m.beam_search(feats, b.T, b.K, **kw, **cases.kwargs(case), return_details=True)]
        tag = (f"{name} H={b.H} V={b.V} B={b.B} T={b.T} K={b.K} G={case.G} diversity={case.diversity} length_penalty="
               f"{case.length_penalty} min_length={case.min_length} n={case.ngram} suppress={case.suppress} "
               f"no_end_after={case.no_end_after} {mode}")
        _compare(tag, b, out[mode], o, d, failures)
    for n, x, y in zip(NAMES, out["default"], out["exact_vocab"]):
        if not torch.equal(x, y):
            failures.append(f"default and exact_vocab differ bitwise in {n}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("name,grouped", [("h256_k3", False), ("h768_k8", True), ("h512_v37", False), ("h1024_v65", True)])
def test_constraints_that_cannot_bind_change_no_bit(name, grouped, gpu_device):
    """min_length = 0, no_repeat_ngram = T + 1 (no n-gram that long exists) and a suppressed id whose logit its
    bias drives to -1e30, below every real logit as the padding columns are: every output tensor is bitwise the
    unconstrained call's, plain and grouped, on every vocabulary stage.  And the four keywords at their defaults
    are today's call."""
    b = dc.BEAM[name]
    dead = b.V - 1
    sd = dict(dc.state(b))
    bias = sd[dc.MLP_B].copy()
    bias[dead] = np.float32(-1e30)
    sd[dc.MLP_B] = bias
    cf = Config(adaptive_word_embed_size=b.E, adaptive_lstm_hidden_size=b.H, vocab_length=b.V)
    m = Encoder2Decoder(cf).to(gpu_device)
    m.load_state_dict({k: torch.from_numpy(v).to(gpu_device) for k, v in sd.items()})
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    extra = {"groups": 2 if b.K % 2 == 0 else 1, "diversity": 0.5, "length_penalty": 0.7} if grouped else {}
    for mode, kw in MODES:
        free = m.beam_search(feats, b.T, b.K, **kw, **extra, return_details=True)
        assert not bool((free[3] == dead).any())
        bound = m.beam_search(feats, b.T, b.K, **kw, **extra, return_details=True, suppress_ids=(dead, dead),
                              min_length=0, no_repeat_ngram=b.T + 1)
        for n, x, y in zip(NAMES, free, bound):
            assert torch.equal(x, y), (mode, n)
        off = m.beam_search(feats, b.T, b.K, **kw, **extra, return_details=True, suppress_ids=(), min_length=0,
                            no_repeat_ngram=0, no_end_after=())
        for n, x, y in zip(NAMES, free, off):
            assert torch.equal(x, y), (mode, n)
        if not grouped:   # the plain entry point (aa_beam_decode) with a constraint: k_beam_select3c<false>
            plain = m.beam_search(feats, b.T, b.K, **kw)
            bound = m.beam_search(feats, b.T, b.K, **kw, suppress_ids=(dead,), no_repeat_ngram=b.T + 1)
            assert len(plain) == len(bound) == 5
            for n, x, y in zip(NAMES, plain, bound):
                assert torch.equal(x, y), (mode, n)


# ---- the selection kernel alone: aa_beam_select_step on hand-built logits -------------------------------
def _select_step(dev, B, K, V, Vp, t, logits, cum, fin, htok, hpar, cons=None, end_id=END):
    lib = _lib.load()
    R = B * K
    ws = torch.empty(lib.aa_beam_select_step_workspace_bytes(B, K, V, Vp, t), dtype=torch.uint8, device=dev)
    tok = torch.empty(R, dtype=torch.int64, device=dev)
    par = torch.empty(R, dtype=torch.int32, device=dev)
    cum_out = torch.empty(R, dtype=torch.float32, device=dev)
    fin_out = torch.empty(R, dtype=torch.int32, device=dev)
    keep, c = [], None
    if cons is not None:
        sup, nmin, n, nea = cons
        keep = [torch.tensor(x, dtype=torch.int32, device=dev) if len(x) else None for x in (sup, nea)]
        c = ctypes.byref(_lib.BeamConstraints(_lib.ptr(keep[0]), len(sup), nmin, n, _lib.ptr(keep[1]), len(nea)))
    with torch.cuda.device(dev):
        rc = lib.aa_beam_select_step(B, K, V, Vp, t, end_id, logits.data_ptr(), cum.data_ptr(), fin.data_ptr(),
                                     _lib.ptr(htok), _lib.ptr(hpar), None, c, tok.data_ptr(), par.data_ptr(),
                                     cum_out.data_ptr(), fin_out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    _lib.check(rc, "beam_select_step")
    torch.cuda.synchronize(dev)
    return tok.cpu().numpy(), par.cpu().numpy(), cum_out.cpu().numpy(), fin_out.cpu().numpy()


def _own_tokens(htok, hpar, b, k, K, t):
    y, j = [], k
    for s in range(t - 1, -1, -1):
        y.append(int(htok[s, b * K + j]))
        j = int(hpar[s, b * K + j])
    return y[::-1]


def _forbidden(y, t, V, sup, nmin, n, nea):
    f = set(sup)
    if t < nmin or (y[-1] if t else 1) in nea:
        f.add(END)
    if n >= 1:
        for j in range(n - 1, t):
            if y[j - n + 1:j] == y[t - n + 1:t]:
                f.add(y[j])
    return f


def _reference_step(x, ls, cum, fin, htok, hpar, B, K, V, t, cons):
    """numpy restatement of one constrained step on logits x [R, V] (fp32): the candidates of a live row are its
    allowed tokens at fp32(cum + fp32(fp32(x - max x) - ls)), ls [R] the row's log-sum-exp *as the unconstrained
    kernel computed it*; a finished row carries <end> at cum; per image the K best, ties to the smaller q V + v.
    -> tok, par, cum_out, fin_out, the smallest gap between consecutive scores among each image's K + 1 best, and
    per survivor the rank of its granule by raw granule max within its row (0 = the largest)."""
    sup, nmin, n, nea = cons
    tok, par, out, fo, gap, granks = [], [], [], [], np.inf, []
    for b in range(B):
        c = []
        for k in range(K):
            r = b * K + k
            if fin[r]:
                c.append((np.float32(cum[r]), k * V + END, True))
                continue
            f = _forbidden(_own_tokens(htok, hpar, b, k, K, t), t, V, sup, nmin, n, nea)
            s = (cum[r] + ((x[r] - x[r].max()) - ls[r]).astype(np.float32)).astype(np.float32)
            c += [(s[v], k * V + v, False) for v in np.argsort(-s, kind="stable")[:K + len(f) + 1] if v not in f]
        c.sort(key=lambda e: (-float(e[0]), e[1]))
        gap = min(gap, min(float(c[i][0]) - float(c[i + 1][0]) for i in range(K)))
        for s, flat, carried in c[:K]:
            q, v = divmod(flat, V)
            tok.append(v), par.append(b * K + q), out.append(s), fo.append(int(carried or v == END))
            gmax = np.pad(x[b * K + q], (0, -V % 32), constant_values=-np.inf).reshape(-1, 32).max(1)
            granks.append(-1 if carried else int((gmax > gmax[v // 32]).sum()))
    return np.array(tok), np.array(par, np.int32), np.array(out, np.float32), np.array(fo, np.int32), gap, granks


@pytest.mark.parametrize("V,K", [(3001, 3), (3001, 8), (100, 3), (100, 8)])
def test_threshold_repair_on_hand_built_logits(V, K, gpu_device):
    """k_beam_select3c alone (aa_beam_select_step: k_gsumm, then one selection launch) on logits built so that the
    constraints hit the granule maxima the top-K search rests on.  Five images of K rows at step t = 3, every
    value gap inside a row >= 0.1:

    0  the K columns with the largest values, one per granule, are suppressed; the K best allowed columns lie in
       K other granules (V = 3001: granules ranked K+1 .. 2K by raw max; V = 100 has four granules in all) --
       the unrepaired threshold would keep only the first K granules;
    1  suppressed tokens at column 0 and column V - 1, the row's two largest;
    2  <end> is the row's arg-max and forbidden: by ``min_length`` in the first call, by ``no_end_after`` (the
       rows' last token) in the second;
    3  row 0's arg-max completes a repeated bigram, and the row's own tokens (A, B, A) are found only by following
       ``hist_par`` through slots 2 -> 1 -> 0 (the tokens at the row's own slot forbid nothing); the other rows'
       histories are random;
    4  everything at once on random values, one row finished (its <end> is carried whatever the rules say).

    Compared with a numpy restatement on the same arrays: tok, par and fin_out equal, and cum_out equal bit for
    bit to fp32(cum + fp32(fp32(x - max) - ls)) with ls the row's log-sum-exp read off an *unconstrained* call on
    the same logits (K = 1, cum = 0: its survivor is the row's arg-max at 0 - ls) -- the constrained kernel's
    log-sum-exp is the unconstrained one's.  The inputs are checked first: no near-tie (score gaps > 1e-3), and
    image 0's survivors lie in granules that the K-th largest raw granule max excludes.  Checked once against a
    build that gives forbidden columns key 0 but takes the threshold from the unmodified granule maxima: this
    test fails there at V = 3001 for both K (image 0 keeps tokens of its first K granules); V = 100 cannot show it
    -- with four granules and K = 3 or 8 the unrepaired threshold already admits the granules that matter -- and
    covers the few-granule path of the repair instead."""
    dev = gpu_device
    rng = np.random.default_rng(V * 10 + K)
    B, t, Vp = 5, 3, -(-V // 128) * 128
    R = B * K
    NG = -(-V // 32)
    x = np.stack([0.1 * rng.permutation(V) for _ in range(R)]).astype(np.float32)
    top = np.float32(0.1 * V + 10)
    pool = [c for c in range(3, V - 1) if c % 32 not in (0, 31)]
    # suppressed columns: one per granule, granules spread over the vocabulary; the allowed runners-up elsewhere
    gs = rng.permutation(np.arange(1, NG - 1))
    forb = [int(g) * 32 + 5 + i for i, g in enumerate(gs[:K] if NG - 2 >= K else np.resize(gs, K))]
    good = [int(g) * 32 + 17 - i for i, g in enumerate(gs[K:2 * K] if NG - 2 >= 2 * K else np.resize(gs[::-1], K))]
    A, Bt, C, D = [c for c in pool if c not in forb and c not in good and c > 40][:4] if V > 100 else (90, 91, 92, 93)
    assert len({0, V - 1, END, A, Bt, C, D, *forb, *good}) == 7 + 2 * K
    htok = rng.choice([A, Bt, C, D], size=(t, R)).astype(np.int32)
    hpar = rng.integers(0, K, size=(t, R)).astype(np.int32)
    for k in range(K):
        r = 0 * K + k      # image 0: suppressed maxima, the best allowed columns in other granules
        x[r, forb] = top + 20 + 0.1 * rng.permutation(K)
        x[r, good] = top + 10 + 0.1 * rng.permutation(K)
        r = 1 * K + k      # image 1: columns 0 and V - 1
        x[r, [0, V - 1]] = top + 20 + np.float32([0.3, 0.0] if k % 2 else [0.0, 0.3])
        r = 2 * K + k      # image 2: <end> on top; the rows' last token is A
        x[r, END] = top + 20
        htok[t - 1, r] = A
        r = 3 * K + k      # image 3: Bt on top of every row (row 0's history is set below)
        x[r, Bt] = top + 20
        r = 4 * K + k      # image 4: a bit of everything
        cols = [0, V - 1, END, A, Bt, C, D] + forb[:2] + good[:2]
        x[r, cols] = top + 5 + 0.1 * rng.permutation(len(cols))
    # image 3, row 0: its own tokens are (A, Bt, A) through slots 2 -> 1 -> 0; the tokens at its own slot,
    # (D, C, A), forbid nothing
    r0 = 3 * K
    htok[2, r0], hpar[2, r0] = A, 1
    htok[1, r0 + 1], hpar[1, r0 + 1] = Bt, 2
    htok[0, r0 + 2] = A
    htok[1, r0], htok[0, r0], htok[0, r0 + 1] = C, D, D
    cum = (-rng.uniform(0.5, 6.0, size=R)).astype(np.float32)
    cum[r0] = -0.1                     # the image's best row: unconstrained, (row 0, Bt) survives
    fin = np.zeros(R, np.int32)
    fin[4 * K + K - 1] = 1
    cum[4 * K + K - 1] = -0.2          # the finished row's carried <end> is the image's best candidate
    assert float(np.diff(np.sort(x, axis=1), axis=1).min()) >= 0.09
    xp = np.zeros((R, Vp), np.float32)   # padding columns at 0: above every negative... they take no part
    xp[:, :V] = x
    d = {"logits": torch.from_numpy(xp).to(dev), "cum": torch.from_numpy(cum).to(dev), "fin": torch.from_numpy(fin).to(dev),
         "htok": torch.from_numpy(htok).to(dev), "hpar": torch.from_numpy(hpar).to(dev)}
    # the unconstrained log-sum-exp of every row: K = 1, cum = 0, step 0
    zero = torch.zeros(R, dtype=torch.float32, device=dev)
    tok1, _, lse1, _ = _select_step(dev, R, 1, V, Vp, 0, d["logits"], zero, torch.zeros_like(d["fin"]), None, None)
    assert np.array_equal(tok1, x.argmax(1))
    ls = -lse1
    want_ls = np.log(np.exp(x.astype(np.float64) - x.max(1, keepdims=True)).sum(1))
    assert float(np.abs(ls - want_ls).max()) < 1e-5
    # the unconstrained step itself against the restatement (nothing forbidden)
    for label, cons in (("unconstrained", None),
                        ("min_length", (tuple(forb) + (0, V - 1), t + 1, 2, ())),
                        ("no_end_after", (tuple(forb) + (0, V - 1, 0), 0, 2, (A, A)))):
        got = _select_step(dev, B, K, V, Vp, t, d["logits"], d["cum"], d["fin"], d["htok"], d["hpar"], cons)
        tok, par, out, fo, gap, granks = _reference_step(x, ls, cum, fin, htok, hpar, B, K, V, t, cons or ((), 0, 0, ()))
        assert gap > 1e-3, f"{label}: hand-built scores too close to call ({gap})"
        if cons is not None:
            # the inputs do what they are there for
            if NG - 2 >= 2 * K:
                assert all(g >= K for g in granks[:K]), granks[:K]      # image 0: outside the raw top-K granules
            assert not set(tok[:K]) & set(forb) and not set(tok[K:2 * K]) & {0, V - 1}
            assert END not in tok[2 * K:3 * K]
            assert not any(v == Bt and q == r0 for v, q in zip(tok[3 * K:4 * K], par[3 * K:4 * K]))
            assert fo[4 * K:].sum() >= 1 and END in tok[4 * K:]          # the finished row's carried <end>
        else:
            assert set(tok[2 * K:3 * K]) >= {END}
            assert any(v == Bt and q == r0 for v, q in zip(tok[3 * K:4 * K], par[3 * K:4 * K]))
        assert np.array_equal(got[0], tok), (label, got[0], tok)
        assert np.array_equal(got[1], par), label
        assert np.array_equal(got[2].view(np.uint32), out.view(np.uint32)), (label, got[2], out)
        assert np.array_equal(got[3], fo), label


def test_beam_size_one_is_the_constrained_greedy_decode(gpu_device):
    """K = 1 with suppress_ids and no_repeat_ngram = 2 (both block something: asserted) equals the oracle."""
    b = dc.BEAM["h768_k3"]
    kw = {"suppress_ids": (1622,), "no_repeat_ngram": 2}
    feats = torch.from_numpy(dc.features(b))
    o = BeamConsOracle(dc.state(b)).beam_search_cons(feats, b.T, 1, **kw)
    d = BeamConsOracle(dc.state(b), dtype=torch.float64).beam_search_cons(feats.double(), b.T, 1, **kw)
    assert o["sel_margin"] > 4 * SCORE_TOL and torch.equal(o["seqs"], d["seqs"])
    assert o["blocked"]["suppress"] > 0 and o["blocked"]["ngram"] > 0
    m = model_for(b, gpu_device)
    failures = []
    for mode, mkw in MODES:
        got = [x.cpu() for x in m.beam_search(feats.to(gpu_device), b.T, 1, **mkw, **kw, return_details=True)]
        _compare(f"h768_k3 K=1 {mode}", b, got, o, d, failures)
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("mode,kw", MODES)
def test_batch_invariance(mode, kw, gpu_device):
    """Images 60..66 of the 67 of h256_ragged (rows 180..200: across the last 64-row boundary) alone equal the
    same images in the full batch, bit for bit, under every constraint of the case."""
    case = cases.CONS["h256_ragged"]
    b = case.beam
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    big = m.beam_search(feats, b.T, b.K, **kw, **cases.kwargs(case), return_details=True)
    small = m.beam_search(feats[60:67].contiguous(), b.T, b.K, **kw, **cases.kwargs(case), return_details=True)
    for n, x, y in zip(NAMES, big, small):
        assert torch.equal(x[60:67], y), n


def test_finished_beams_are_carried_unchanged(gpu_device):
    """h256_k3 with all four constraints, no_repeat_ngram = 1 among them: beams finish from step 2 on and are
    carried as <end> to the last step -- tokens the unigram rule would forbid a live hypothesis -- at the score
    they finished with (the oracle's, which never applies a rule to a finished beam)."""
    b = dc.BEAM["h256_k3"]
    kw = {"suppress_ids": (1587,), "min_length": 2, "no_repeat_ngram": 1, "no_end_after": (1006,)}
    feats = torch.from_numpy(dc.features(b))
    o = BeamConsOracle(dc.state(b)).beam_search_cons(feats, b.T, b.K, **kw)
    d = BeamConsOracle(dc.state(b), dtype=torch.float64).beam_search_cons(feats.double(), b.T, b.K, **kw)
    assert o["sel_margin"] > 4 * SCORE_TOL and o["rank_margin"] > 4 * SCORE_TOL and torch.equal(o["seqs"], d["seqs"])
    assert all(v > 0 for v in o["blocked"].values()), o["blocked"]
    assert int(((o["seqs"] == END).sum(2) > 1).sum()) >= b.B      # <end> repeated: only a carried beam can
    m = model_for(b, gpu_device)
    failures = []
    for mode, mkw in MODES:
        got = [x.cpu() for x in m.beam_search(feats.to(gpu_device), b.T, b.K, **mkw, **kw, return_details=True)]
        _compare(f"h256_k3 finished {mode}", b, got, o, d, failures)
        seqs, lengths = got[3], got[5].long()
        after = torch.arange(b.T).view(1, 1, -1) >= lengths.unsqueeze(2)
        assert bool((seqs[after] == END).all()) and bool((lengths >= 3).all()), mode
    assert not failures, "; ".join(failures)


def test_argument_errors_leave_the_process_usable(gpu_device):
    b = dc.BEAM["h256_v37"]
    m = model_for(b, gpu_device)
    feats = torch.from_numpy(dc.features(b)).to(gpu_device)
    kw = {"suppress_ids": (16,), "min_length": 3, "no_repeat_ngram": 2}
    before = m.beam_search(feats, b.T, b.K, **kw)
    for bad in ({"suppress_ids": (37,)}, {"suppress_ids": (END,)}, {"min_length": -1}, {"no_repeat_ngram": -2},
                {"no_end_after": (-1,)}, {"suppress_ids": tuple(range(3, 36)), "no_repeat_ngram": 1},
                {"end_id": -1, "min_length": 1}):
        with pytest.raises(ValueError):
            m.beam_search(feats, b.T, b.K, **bad)
    # the C entry point's own refusals, on a real model and real buffers
    lib = _lib.load()
    ws = torch.empty(lib.aa_beam_workspace_bytes(m._c_dims(), b.B, b.T, b.K), dtype=torch.uint8, device=gpu_device)
    ids = torch.tensor([16], dtype=torch.int32, device=gpu_device)
    for c in (_lib.BeamConstraints(ids.data_ptr(), 65, 0, 0, None, 0), _lib.BeamConstraints(ids.data_ptr(), 1, -1, 0, None, 0),
              _lib.BeamConstraints(ids.data_ptr(), 33, 0, 1, None, 0)):
        with torch.cuda.device(gpu_device):
            rc = lib.aa_beam_decode_cx(m._model_struct(), feats.data_ptr(), b.B, b.T, b.K, END, None, None, None, None,
                                       None, ws.data_ptr(), ws.numel(), 0, _lib.stream_handle(), None, None, ctypes.byref(c))
        assert rc == -3
    after = m.beam_search(feats, b.T, b.K, **kw)
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    plain = m.beam_search(feats, b.T, b.K)
    assert bool((plain[3] >= 0).all()) and bool(torch.isfinite(plain[4]).all())
