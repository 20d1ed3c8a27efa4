"""Measured errors of the training step against the CPU oracle's autograd (tools only; GPU): the figures
the tolerances in tests/test_gpu_configs.py, tests/test_gpu_train.py and tests/test_gpu_train_dims.py
are set from or quoted beside.

Default: the config-5 step (B = 128, T = 18), bf16 and fp32 GEMMs; the train.py closure (three
zero_grad / forward / CE / backward / clip / Adam steps, bf16 GEMMs) against the same closure on the
oracle; and decoder(...) on whole captions (T = 12) against the oracle's Decoder.forward.

    python tools/train_tolerances.py > profiles/r06_tolerances.txt

``--hidden / --embed / --vocab`` run the config-5 step at another model size (the closure and the
decoder sections run at the default size only); ``--dtype float64`` evaluates the oracle in double.
``--cases all`` (or a list, ``A,C``) runs the cases of tests/train_cases.py instead, fp32 and bf16,
against their float64 reference, with a worst-per-case summary:

    python tools/train_tolerances.py --cases all > profiles/train_dims_errors.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from adaptive_amd import Config, Encoder2Decoder, synth  # noqa: E402
from test_gpu_configs import _config5_batch, _gpu_loss  # noqa: E402


def _batch(vocab, B=128, T=18, seed=0):
    """_config5_batch with the tokens drawn below ``vocab`` (the same batch at the default vocabulary)."""
    if vocab == 10123:
        return _config5_batch(B, T, seed)
    rng = np.random.default_rng(seed)
    lengths = sorted(rng.integers(T // 2, T + 1, size=B).tolist(), reverse=True)
    lengths[0] = T
    caps = rng.integers(2, vocab, size=(B, T + 1)).astype(np.int64)
    caps[:, 0] = 1
    return caps, lengths


def main(hidden, embed, vocab, dtype):
    from oracle.adaptive_oracle import TrainOracle
    dev = torch.device("cuda", 0)
    default = (hidden, embed, vocab) == (512, 256, 10123)
    dims = synth.Dims(embed=embed, hidden=hidden, vocab=vocab)
    cf = Config(adaptive_word_embed_size=embed, adaptive_lstm_hidden_size=hidden, vocab_length=vocab)
    caps, lengths = _batch(vocab)
    state = synth.make_weights(123, dims, bias_noise=0.02)
    feats = synth.make_features(128, seed=0)
    print(f"config-5 step B=128 T=18 hidden={hidden} embed={embed} vocab={vocab}, oracle in {dtype}")
    oracle = TrainOracle(state, dtype=dtype)
    loss, packed = oracle.loss(torch.from_numpy(feats).to(dtype), torch.from_numpy(caps), lengths)
    loss.backward()
    rscores = packed[0].detach().double().numpy()
    rgrads = {k: v.grad.detach().double().numpy() for k, v in oracle.w.items()}
    for bf16 in (True, False):
        m = Encoder2Decoder(cf).to(dev).load_synthetic(123, bias_noise=0.02)
        m.train_bf16 = bf16
        l, p = _gpu_loss(m, torch.from_numpy(feats).to(dev), torch.from_numpy(caps).to(dev), lengths)
        got = p[0].detach().cpu().double().numpy()
        l.backward()
        print(f"bf16={bf16}: scores rel-Frobenius {np.linalg.norm(got - rscores) / np.linalg.norm(rscores):.3e}, "
              f"max abs {np.abs(got - rscores).max():.3e}; loss rel {abs(l.item() - loss.item()) / abs(loss.item()):.3e}")
        worst = (0.0, "")
        for k, prm in m.named_parameters():
            g, r = prm.grad.detach().cpu().double().numpy(), rgrads[k]
            rel = np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30)
            ent = np.abs(g - r).max() / max(np.abs(r).max(), 1e-30)
            print(f"   {k:48s} rel-Frobenius {rel:.3e}  max-entry/max {ent:.3e}")
            worst = max(worst, (rel, k))
        print(f"   worst gradient rel-Frobenius {worst[0]:.3e} ({worst[1]})")
    if default:
        closure(dev, caps, lengths, feats)
        decoder_whole_captions(dev)


def cases(names):
    """The cases of tests/train_cases.py through the product path, fp32 and bf16, against float64."""
    import train_cases as tc
    from test_gpu_train_dims import f64, gpu_step, gradient_errors, rel_fro
    dev = torch.device("cuda", 0)
    for name in names:
        case = tc.CASES[name]
        rloss, rscores, rgrads, rdfeats = tc.reference(name)
        print(f"case {name}: H={case.H} E={case.E} V={case.V} B={case.B} T={case.T} rows={case.total} ({case.reaches})")
        for bf16 in (False, True):
            loss, scores, grads, dfeats = gpu_step(name, dev, bf16)
            got = f64(scores)
            print(f" {'bf16' if bf16 else 'fp32'}: scores max abs {np.abs(got - rscores).max():.3e} rel-Frobenius "
                  f"{rel_fro(got, rscores):.3e}; loss rel {abs(loss - rloss) / abs(rloss):.3e}")
            worst = [(0.0, ""), (0.0, ""), (0.0, "")]
            for k, e in gradient_errors(name, grads, dfeats).items():
                if not np.any(rgrads.get(k, rdfeats)):
                    print(f"   {k:48s} reference exactly 0; largest |entry| {float(np.abs(f64(grads[k])).max()):.3e}")
                    continue
                print(f"   {k:48s} rel-Frobenius {e[0]:.3e}  max-entry/max {e[1]:.3e}  masked max-entry/max {e[2]:.3e}")
                worst = [(x, k) if x > w[0] else w for w, x in zip(worst, e)]
            print(f"   worst: rel-Frobenius {worst[0][0]:.3e} ({worst[0][1]}), max-entry/max {worst[1][0]:.3e} "
                  f"({worst[1][1]}), masked max-entry/max {worst[2][0]:.3e} ({worst[2][1] or 'none masked'})")


def closure(dev, caps, lengths, feats):
    """test_config5_adam_clip_closure_vs_oracle's three steps: per-step loss and clip-norm errors."""
    from oracle.adaptive_oracle import TrainOracle
    oracle = TrainOracle(synth.make_weights(123, bias_noise=0.02))
    o_opt = torch.optim.Adam(list(oracle.w.values()), lr=1e-3)
    o_lstm = [oracle.w["decoder.LSTM." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    model = Encoder2Decoder(Config()).to(dev).load_synthetic(123, bias_noise=0.02)
    model.train_bf16 = True
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    f, c = torch.from_numpy(feats).to(dev), torch.from_numpy(caps).to(dev)
    of, oc = torch.from_numpy(feats), torch.from_numpy(caps)
    for i in range(3):
        model.zero_grad()
        opt.zero_grad()
        loss, _ = _gpu_loss(model, f, c, lengths)
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(model.decoder.LSTM.parameters(), 5.0)
        opt.step()
        o_opt.zero_grad()
        rloss, _ = oracle.loss(of, oc, lengths)
        rloss.backward()
        rnorm = torch.nn.utils.clip_grad_norm_(o_lstm, 5.0)
        o_opt.step()
        print(f"closure step {i}: loss rel {abs(loss.item() - rloss.item()) / abs(rloss.item()):.3e}, "
              f"clip-norm rel {abs(norm.item() - rnorm.item()) / rnorm.item():.3e}")


def decoder_whole_captions(dev):
    """test_decoder_whole_captions_vs_oracle: max abs errors of scores, alpha, beta, h, c."""
    from oracle.adaptive_oracle import OracleModel
    B, T = 9, 12
    m = Encoder2Decoder(Config()).to(dev).load_synthetic(31, bias_noise=0.01)
    feats = torch.from_numpy(synth.make_features(B, seed=5)).to(dev)
    V, v_g, (h0, c0) = m.encoder(feats)
    rng = np.random.default_rng(3)
    caps = torch.from_numpy(rng.integers(0, 10123, size=(B, T)).astype(np.int64))
    caps[:, 0] = 1
    states = (h0.transpose(0, 1), c0.transpose(0, 1))
    sc, al, be, (h, c) = m.decoder(V, v_g, caps.to(dev), states)
    o = OracleModel(synth.make_weights(31, bias_noise=0.01))
    with torch.no_grad():
        osc, oal, obe, (oh, oc) = o.decoder(V.cpu(), v_g.cpu(), caps, (states[0].cpu().contiguous(),
                                                                     states[1].cpu().contiguous()))
    for name, x, y in (("scores", sc, osc), ("alpha", al, oal), ("beta", be, obe), ("h", h, oh), ("c", c, oc)):
        print(f"decoder T={T}: {name} max abs {float((x.cpu() - y).abs().max()):.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hidden", type=int, default=512, choices=(256, 512, 768, 1024))
    ap.add_argument("--embed", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=10123)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float64"), help="precision of the CPU oracle")
    ap.add_argument("--cases", default=None, help="'all' or a comma-separated list of tests/train_cases.py ids")
    a = ap.parse_args()
    if a.cases:
        import train_cases
        cases(list(train_cases.CASES) if a.cases == "all" else a.cases.split(","))
    else:
        main(a.hidden, a.embed, a.vocab, getattr(torch, a.dtype))
