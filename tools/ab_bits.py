#!/usr/bin/env python3
"""Bitwise A/B of two library builds on one decode (GPU box): run once per build with AA_LIB_PATH
set, dumping the outputs; then compare the dumps.
    AA_LIB_PATH=a.so python tools/ab_bits.py dump gpurun_out/a.npz [--beam K] [--batch B]
    AA_LIB_PATH=b.so python tools/ab_bits.py dump gpurun_out/b.npz ...
    (--train bf16|fp32 --batch 128 --T 18: one training step's scores and gradients instead, with
     dL/dfeats, the whole-caption decoder outputs and a forward_sampled(sampler_gate=True) step;
     --dims E,H,V --lengths 4,3,3,1,1 [--const-caps]: another model size and other caption lengths)
    python tools/ab_bits.py cmp gpurun_out/a.npz gpurun_out/b.npz"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def dump_train(path, batch, T, dtype, dims=None, lengths=None, const_caps=False):
    """One teacher-forced forward + CE + backward (bench_train's batch, or captions of the given
    lengths for a model of the given size): scores, loss, every gradient and dL/dfeats; then the
    whole-caption decoder's outputs and one forward_sampled(sampler_gate=True) step's."""
    import torch
    import torch.nn.functional as F
    from torch.nn.utils.rnn import pack_padded_sequence
    from bench_train import make_batch
    from adaptive_amd import Config, Encoder2Decoder
    from adaptive_amd.adaptive_attention import synthetic_features
    dev = torch.device("cuda", 0)
    cf = Config()
    if dims:
        E, H, V = dims
        cf = Config(adaptive_word_embed_size=E, adaptive_lstm_hidden_size=H, vocab_length=V)
    m = Encoder2Decoder(cf).to(dev).load_synthetic(123)
    if lengths:
        batch, T = len(lengths), lengths[0]
        caps_np = np.random.default_rng(5).integers(0, m.dims.vocab, size=(batch, T + 2)).astype(np.int64)
        caps_np[:, 0] = 1
        if const_caps:
            caps_np[:] = 1
    else:
        caps_np, lengths = make_batch(batch, T)
    m.train_bf16 = dtype == "bf16"
    m.train_aux_stream = os.environ.get("AB_ONE_STREAM") != "1"  # bitwise A/B of the two-stream calls
    feats = synthetic_features(batch, dev, seed=0).requires_grad_(True)
    caps = torch.from_numpy(caps_np).to(dev)

    def grads(prefix):
        got = {prefix + n: p_.grad.cpu().numpy() for n, p_ in m.named_parameters() if p_.grad is not None}
        got[prefix + "dfeats"] = feats.grad.cpu().numpy()
        m.zero_grad(set_to_none=True)
        feats.grad = None
        return got

    packed = m(feats, caps, lengths)
    loss = F.cross_entropy(packed[0], pack_padded_sequence(caps[:, 1:], lengths, batch_first=True)[0])
    loss.backward()
    torch.cuda.synchronize()
    out = {"scores": packed[0].detach().cpu().numpy(), "loss": loss.detach().cpu().numpy()}
    out.update(grads("grad."))
    with torch.no_grad():  # aa_decoder_forward over the whole captions
        Vf, vg, states = m.encoder(feats)
        sc, al, be, (h, c) = m.decoder(Vf, vg, caps[:, :T], states)
    for n, x in (("scores", sc), ("alpha", al), ("beta", be), ("h", h), ("c", c)):
        out["decoder." + n] = x.cpu().numpy()
    # AA_TRAIN_SENTINEL_H0: the captions' own tokens as the "samples", every one at full length
    sampled = m.forward_sampled(feats, caps[:, 1:T + 1].contiguous(), sampler_gate=True)
    sampled.square().mean().backward()
    torch.cuda.synchronize()
    out["sampled.scores"] = sampled.detach().cpu().numpy()
    out.update(grads("sampled.grad."))
    np.savez(path, **out)
    print("dumped", path, len(out), "arrays")


def dump(path, beam, batch, T, fast):
    import torch
    from adaptive_amd import Config, Encoder2Decoder
    from adaptive_amd.adaptive_attention import synthetic_features
    m = Encoder2Decoder(Config()).to("cuda:0")
    m.load_synthetic(123)
    feats = synthetic_features(batch, "cuda:0", seed=0)
    if beam:
        out = m.beam_search(feats, max_len=T, beam_size=beam, fast=fast)
        names = ("ids", "alpha", "beta", "seqs", "scores")
    else:
        out = m.sampler(feats, max_len=T)
        names = ("ids", "alpha", "beta")
    torch.cuda.synchronize()
    np.savez(path, **{n: o.cpu().numpy() for n, o in zip(names, out)})
    print("dumped", path, {n: o.shape for n, o in zip(names, out)})


def cmp(a, b):
    x, y = np.load(a), np.load(b)
    ok = True
    for n in x.files:
        same = x[n].tobytes() == y[n].tobytes()
        ok &= same
        print(n, "bit-identical" if same else f"DIFFERS (max |d| {np.abs(x[n].astype(np.float64) - y[n]).max():.3g})")
    print("ALL BIT-IDENTICAL" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("dump", "cmp"))
    ap.add_argument("files", nargs="+")
    ap.add_argument("--beam", type=int, default=0)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--fast", action="store_true")
    ap.add_argument("--train", choices=("bf16", "fp32"), default=None, help="dump a training step instead")
    ap.add_argument("--dims", default=None, help="--train: E,H,V of the model (default: Config())")
    ap.add_argument("--lengths", default=None, help="--train: caption lengths, sorted descending (sets batch and T)")
    ap.add_argument("--const-caps", action="store_true", help="--train with --lengths: every token 1")
    a = ap.parse_args()
    if a.mode == "dump" and a.train:
        ints = lambda v: tuple(map(int, v.split(","))) if v else None
        dump_train(a.files[0], a.batch, a.T, a.train, ints(a.dims), ints(a.lengths), a.const_caps)
    elif a.mode == "dump":
        dump(a.files[0], a.beam, a.batch, a.T, a.fast)
    else:
        sys.exit(cmp(*a.files))
