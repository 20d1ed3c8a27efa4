#!/usr/bin/env python3
"""Sampling-decode benchmark: B=512 images, max_len 20 on 1 MI355X through Encoder2Decoder.sample
(C-ABI aa_sample_decode: seeded Gumbel-max draws over the exact fp32 logits).

Synthetic post-trunk features U[0,1) and the portable random-init weights (adaptive_amd.synth), inputs
resident in HBM.  Prints ONE JSON line: captions/s of ``sample`` (median of the timed regions); in the
same process, as the yardstick, ``beam_search(..., beam_size=1, end_id=-1)`` at the same shape (the
same three launches per step with k_beam_select3 in k_sample_select's place), the two interleaved
region by region; and, from traced passes, the median launch duration of k_sample_select (an event
pair handed to each step's launch) and of the beam's vocab stage k_vexact.

    python bench_sample.py [--steps 10] [--warmup 3] [--regions 5] [--batch 512] [--T 20] [--temperature 1.0]
                           [--top-k K] [--top-p P] [--num-samples N]

With any of ``--top-k`` / ``--top-p`` / ``--num-samples`` a third region, ``sample`` with those options, is
interleaved with the two and reported under ``"options"`` (captions/s counts the B*N drawn captions; the
selection launch's median from its own traced passes); with ``--num-samples N > 1`` a fourth, the same
options on ``images.repeat_interleave(N)`` -- what N draws per image cost without the shared encoder
pass.  Without them the output is what it was.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from adaptive_amd import Config, Encoder2Decoder  # noqa: E402
from adaptive_amd.adaptive_attention import synthetic_features  # noqa: E402
from adaptive_amd.hip_events import EventArray  # noqa: E402

HBM_PEAK = 8.0e12  # B/s (MI355X_MICROARCH.md)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
            "launches": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="decode calls per timed region")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=None, help="also time sample(top_k=K)")
    ap.add_argument("--top-p", type=float, default=None, help="also time sample(top_p=P)")
    ap.add_argument("--num-samples", type=int, default=None, help="also time sample(num_samples=N)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, K, tau = args.batch, args.T, args.steps, args.temperature
    model = Encoder2Decoder(Config()).to(dev).load_synthetic(123)
    feats = synthetic_features(B, dev, seed=0)

    def run_sample():
        return model.sample(feats, T, temperature=tau, seed=0)

    def run_beam1():
        return model.beam_search(feats, T, 1, end_id=-1)

    runs = [("sample", run_sample), ("beam1", run_beam1)]
    opt = None
    if args.top_k is not None or args.top_p is not None or args.num_samples is not None:
        opt = {"top_k": args.top_k or 0, "top_p": 1.0 if args.top_p is None else args.top_p,
               "num_samples": args.num_samples or 1}
        runs.append(("options", lambda: model.sample(feats, T, temperature=tau, seed=0, **opt)))
        if opt["num_samples"] > 1:
            rep = feats.repeat_interleave(opt["num_samples"], 0)
            runs.append(("repeat", lambda: model.sample(rep, T, temperature=tau, seed=0, top_k=opt["top_k"],
                                                        top_p=opt["top_p"])))
    for _ in range(args.warmup):
        out = run_sample()
        for _, fn in runs[1:]:
            fn()
    torch.cuda.synchronize()
    regions = {name: [] for name, _ in runs}
    for _ in range(args.regions):  # interleaved: all see the same clocks and the same neighbours
        for name, fn in runs:
            t0 = time.perf_counter()
            for _ in range(K):
                fn()
            torch.cuda.synchronize()
            regions[name].append(time.perf_counter() - t0)
    el = {k: float(np.median(v)) for k, v in regions.items()}
    # traced passes: the same calls with an event pair per step
    sel, vex = [], []
    for _ in range(K):
        ev = EventArray(2 * T)
        model.sample(feats, T, temperature=tau, seed=0, select_events=ev.ptr)
        torch.cuda.synchronize()
        sel += ev.pair_durations_ms()
        ev.close()
        ev = EventArray(2 * T)
        model.beam_search(feats, T, 1, end_id=-1, vocab_events=ev.ptr)
        torch.cuda.synchronize()
        vex += ev.pair_durations_ms()
        ev.close()
    osel = []
    for _ in range(K if opt else 0):
        ev = EventArray(2 * T)
        model.sample(feats, T, temperature=tau, seed=0, select_events=ev.ptr, **opt)
        torch.cuda.synchronize()
        osel += ev.pair_durations_ms()
        ev.close()
    Vn = model.dims.vocab
    Vp = (Vn + 127) // 128 * 128
    sel_ms = float(np.median(sel))
    # k_sample_select's traffic: one read of the row's V logits (written just before by k_vexact, so served
    # by L2 / the Infinity Cache rather than HBM) and 20 bytes of results per row
    bytes_moved = B * (Vn * 4 + 20)
    roofline = {"kernel": "k_sample_select", "bound": "issue (ALU: per element one splitmix64, two logf, one expf, "
                "one division)", "bytes_per_launch": bytes_moved, "achieved_GBps": bytes_moved / (sel_ms * 1e-3) / 1e9,
                "hbm_peak_GBps": HBM_PEAK / 1e9, "frac_of_hbm_peak": bytes_moved / (sel_ms * 1e-3) / HBM_PEAK,
                "elements_per_launch": B * Vn, "elements_per_us": B * Vn / (sel_ms * 1e3), "padded_pitch": Vp}
    value = B * K / el["sample"]
    beam1 = B * K / el["beam1"]
    res = {"metric": f"captions/sec (sample, temperature={tau}, max_len={T}) at B={B}", "value": value,
           "unit": "captions/s", "n_gpus": 1, "steps": K, "warmup": args.warmup, "regions_s": regions["sample"],
           "reported": "median region", "ms_per_step": 1e3 * el["sample"] / K, "higher_is_better": True, "dtype": "fp32",
           "data": "synthetic: U[0,1) post-trunk features, random-init weights (adaptive_amd.synth seed 123)",
           "config": {"workload": f"Encoder2Decoder.sample B={B} max_len={T} temperature={tau} seed=0", "batch": B,
                      "T": T, "temperature": tau},
           "beam1": {"value": beam1, "unit": "captions/s", "ms_per_step": 1e3 * el["beam1"] / K,
                     "regions_s": regions["beam1"],
                     "workload": f"Encoder2Decoder.beam_search B={B} beam=1 max_len={T} end_id=-1 (same process)"},
           "sample_over_beam1": value / beam1,
           "kernels": {"k_sample_select": stats(sel), "k_vexact(beam1)": stats(vex)}, "roofline": roofline,
           "ids_checksum": int(out[0].sum().item()), "logp_mean": float(out[1].mean().item())}
    if opt:
        n = opt["num_samples"]
        o = {**opt, "value": B * n * K / el["options"], "unit": "captions/s (B * num_samples per call)",
             "ms_per_step": 1e3 * el["options"] / K, "regions_s": regions["options"],
             "over_sample": el["sample"] * n / el["options"], "selection_launch": stats(osel),
             # (the same B rows in both launches only without num_samples)
             "selection_over_k_sample_select": float(np.median(osel)) / sel_ms if n == 1 else None}
        if "repeat" in el:
            o["repeat_interleave"] = {"value": B * n * K / el["repeat"], "ms_per_step": 1e3 * el["repeat"] / K,
                                      "regions_s": regions["repeat"]}
            o["over_repeat_interleave"] = el["repeat"] / el["options"]
        res["options"] = o
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
