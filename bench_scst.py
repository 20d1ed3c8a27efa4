#!/usr/bin/env python3
"""Self-critical training step benchmark: one full step of Encoder2Decoder at B = 128 images, N = 5
sampled captions each, T = 20, on 1 MI355X, against the synthetic corpus of bench_cider.py:

    sample(num_samples=N) -> greedy sampler -> CiderD rewards -> forward_sampled (HIP, all R = B N rows
    at length T) -> policy_gradient_loss (HIP) -> backward (HIP) -> clip_grad_norm_(LSTM, 5) -> Adam

Prints ONE JSON line:
* steps/s of the public path (``self_critical_loss`` + backward + clip + Adam; wall clock over ``--steps``
  steps after ``--warmup``), bf16 GEMMs in the training forward / backward by default (``--dtype fp32``);
* a per-phase breakdown from HIP events (median over the steps) of the same step written out phase by
  phase: repack (the decode weights packed again after the previous Adam update), sample, greedy, reward,
  forward, loss forward + backward, train backward, clip + Adam;
* the loss kernels beside the same loss written in torch ops (mask by cumsum, log_softmax, gather,
  weighted mean, autograd) on the same tensors in this process, for three inputs: the step's own draws
  ("model"), caption-like ids (references with 30 % of the tokens redrawn, <end>-padded, advantages the
  CIDEr-D difference of two such rows: "captions") and nothing skipped (no <end>, no zero advantage:
  "dense"); with the share of rows the kernels skipped in each.

The synthetic weights draw near-uniform tokens, so the model's own draws score ~0 against the corpus and
most advantages are exactly 0: the "model" row shows the kernels' best case, "captions" what a trained
policy's draws look like, "dense" the worst case.

    python bench_scst.py [--steps 100] [--warmup 5] [--batch 128] [--num-samples 5] [--T 20] [--dtype bf16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from adaptive_amd import Config, Encoder2Decoder  # noqa: E402
from adaptive_amd.adaptive_attention import synthetic_features  # noqa: E402
from adaptive_amd.cider import CiderD  # noqa: E402
from adaptive_amd.optim import Adam, clip_grad_norm_, policy_gradient_loss  # noqa: E402
from bench_cider import END, make_corpus, make_rows  # noqa: E402

PHASES = ("repack", "sample", "greedy", "reward", "forward", "loss_fwd_bwd", "train_backward", "clip_adam")


def torch_loss(scores, ids, adv, end_id, tau):
    """The same loss in torch ops (what a user without the kernels would write)."""
    R, T = ids.shape
    is_end = (ids == end_id).to(torch.int64)
    live = (is_end.cumsum(1) - is_end) == 0
    lsm = F.log_softmax(scores / tau, dim=1).view(T, R, -1).transpose(0, 1)
    logp = lsm.gather(2, ids.unsqueeze(2)).squeeze(2)
    return -(adv.unsqueeze(1) * logp * live).sum() / live.sum()


def skipped_share(ids, adv, end_id):
    is_end = (ids == end_id).to(torch.int64)
    live = (is_end.cumsum(1) - is_end) == 0
    return float((~live | (adv == 0).unsqueeze(1)).float().mean().item())


def timed(fn, iters, warmup=3):
    """Median ms of ``fn()`` over ``iters`` calls, each between its own pair of HIP events."""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def loss_pair(scores, ids, adv, end_id, tau, iters):
    """(HIP ms, torch ms, |difference of the two losses|, skipped share) of loss forward + backward."""
    adv32 = adv.float()
    out = {}

    def hip():
        x = scores.detach().requires_grad_(True)
        loss = policy_gradient_loss(x, ids, adv32, end_id, tau)
        loss.backward()
        out["hip"] = loss.detach()

    def ref():
        x = scores.detach().requires_grad_(True)
        loss = torch_loss(x, ids, adv32, end_id, tau)
        loss.backward()
        out["torch"] = loss.detach()

    h, t = timed(hip, iters), timed(ref, iters)
    return {"hip_ms": h, "torch_ms": t, "torch_over_hip": t / h,
            "loss_abs_diff": abs(float(out["hip"]) - float(out["torch"])),
            "rows_skipped_share": skipped_share(ids, adv32, end_id)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--num-samples", type=int, default=5)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--refs", type=int, default=5)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--loss-iters", type=int, default=50)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, N, T, tau = args.batch, args.num_samples, args.T, args.temperature
    R = B * N
    rng = np.random.default_rng(0)
    corpus = make_corpus(rng, args.images, args.refs)
    images = rng.choice(args.images, size=B, replace=False)
    scorer = CiderD(corpus, end_id=END).to(dev)
    idx = torch.from_numpy(images.astype(np.int32)).to(dev)
    model = Encoder2Decoder(Config()).to(dev).load_synthetic(123)
    model.train_bf16 = args.dtype == "bf16"
    feats = synthetic_features(B, dev, seed=0)
    opt = Adam(model.parameters(), lr=1e-5)
    lstm = list(model.decoder.LSTM.parameters())

    def public_step(seed):
        model.zero_grad()
        loss, info = model.self_critical_loss(feats, scorer, idx, num_samples=N, max_len=T, temperature=tau, seed=seed)
        loss.backward()
        clip_grad_norm_(lstm, 5.0)
        opt.step()
        return loss, info

    for s in range(args.warmup):
        public_step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = []
    for s in range(args.steps):
        th = time.perf_counter()
        loss, info = public_step(args.warmup + s)
        host.append(time.perf_counter() - th)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0

    # the same step phase by phase, an event at every boundary
    per = {k: [] for k in PHASES}
    marks = []
    for s in range(args.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
        model.zero_grad()
        ev[0].record()
        model._model_struct()  # the decode weights, packed again after the previous step's Adam update
        ev[1].record()
        with torch.no_grad():
            sid, slogp, _, _ = model.sample(feats, T, tau, 1000 + s, num_samples=N)
            ev[2].record()
            gid = model.sampler(feats, T)[0]
            ev[3].record()
            adv = scorer.self_critical(sid, gid, N, idx)
        ev[4].record()
        scores = model.forward_sampled(feats, sid, N, sampler_gate=True)
        ev[5].record()
        x = scores.detach().requires_grad_(True)
        policy_gradient_loss(x, sid, adv, END, tau).backward()
        ev[6].record()
        scores.backward(x.grad)
        ev[7].record()
        clip_grad_norm_(lstm, 5.0)
        opt.step()
        ev[8].record()
        marks.append(ev)
    torch.cuda.synchronize()
    for ev in marks:
        for i, k in enumerate(PHASES):
            per[k].append(ev[i].elapsed_time(ev[i + 1]))
    phases = {k: float(np.median(v)) for k, v in per.items()}

    # the loss kernels beside torch ops, on the last step's scores
    scores = scores.detach()
    V = scores.size(1)
    rows = torch.from_numpy(make_rows(rng, corpus, np.repeat(images, N), T)).to(dev)
    other = torch.from_numpy(make_rows(rng, corpus, np.repeat(images, N), T)).to(dev)
    ridx = idx.repeat_interleave(N)
    adv_rows = scorer.score(rows, ridx) - scorer.score(other, ridx)
    dense_ids = torch.randint(3, V, (R, T), device=dev)
    dense_adv = torch.randn(R, device=dev, dtype=torch.float64) + 3.0
    losses = {"model": loss_pair(scores, sid, adv, END, tau, args.loss_iters),
              "captions": loss_pair(scores, rows, adv_rows, END, tau, args.loss_iters),
              "dense": loss_pair(scores, dense_ids, dense_adv, END, tau, args.loss_iters)}

    is_end = (sid == END).to(torch.int64)
    live = (is_end.cumsum(1) - is_end) == 0
    res = {"metric": f"self-critical steps/s (sample + greedy + CIDEr-D + fwd + loss + bwd + clip + Adam) at B={B}, "
                     f"N={N}, T={T}",
           "value": args.steps / el, "unit": "steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": 1e3 * el / args.steps, "host_ms_per_step": 1e3 * float(np.median(host[:10])),
           "host_note": "median host time of the first 10 timed steps' Python calls, which return before their kernels "
                        "run; later steps also wait for room in the device queue once the host is ahead",
           "captions_per_s": R * args.steps / el, "higher_is_better": True, "dtype": args.dtype,
           "data": f"synthetic: U[0,1) post-trunk features, random-init weights, {args.images} images x {args.refs} "
                   "references of 8..16 Zipf tokens (bench_cider.make_corpus, numpy seed 0)",
           "config": {"workload": "Encoder2Decoder.self_critical_loss + backward + clip_grad_norm_(LSTM, 5) + optim.Adam",
                      "batch": B, "num_samples": N, "T": T, "rows": R, "vocab": V, "temperature": tau,
                      "train_gemm": args.dtype},
           "phases_ms": phases, "phases_sum_ms": float(sum(phases.values())),
           "phases_note": "median over the steps of HIP-event intervals around each phase of the step written out "
                          "by hand (the same calls as self_critical_loss)",
           "loss_forward_backward": losses,
           "loss_note": "policy_gradient_loss forward + backward (HIP) beside the same loss in torch ops, median of "
                        f"{args.loss_iters} event-timed calls each on the same [T R, V] scores; model = this step's own "
                        "draws, captions = references with 30 % redrawn and the CIDEr-D difference of two such rows, "
                        "dense = no <end> and no zero advantage",
           "model_draws": {"live_share": float(live.float().mean().item()),
                           "advantage_nonzero_share": float((adv != 0).float().mean().item()),
                           "reward_sample_mean": float(info.reward_sample.mean().item()),
                           "reward_greedy_mean": float(info.reward_greedy.mean().item())},
           "final_loss": float(loss.item())}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
