#!/usr/bin/env python3
"""Baseline-model benchmark: B=512 images, max_len 20 on 1 MI355X through
adaptive_amd.baseline_attention.Encoder2Decoder.sampler (AA_DECODE_BASELINE, the no-sentinel kernels).

Synthetic post-trunk features U[0,1) and the portable random-init weights (adaptive_amd.synth, minus
the sentinel's three tensors), inputs resident in HBM.  Prints ONE JSON line: captions/s of ``sampler``
(median of the timed regions) and, from one more traced pass, the median launch durations of k_lstm
(steps >= 1: GEMM + cell + the previous step's rescoring), k_atten and the vocab screen
(aa_trace events: the dispatches' own begin / end timestamps).

``--adaptive`` measures the adaptive model the same way, for a side-by-side in one session.

    python bench_baseline.py [--steps 10] [--warmup 3] [--regions 5] [--batch 512] [--T 20] [--adaptive]
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

from adaptive_amd import _lib  # noqa: E402
from adaptive_amd.adaptive_attention import synthetic_features  # noqa: E402
from adaptive_amd.hip_events import EventArray  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="sampler calls per timed region")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--adaptive", action="store_true", help="the adaptive model instead (comparison run)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, K = args.batch, args.T, args.steps
    if args.adaptive:
        from adaptive_amd import Config, Encoder2Decoder
        name = "adaptive_attention"
    else:
        from adaptive_amd.baseline_attention import Config, Encoder2Decoder
        name = "baseline_attention"
    model = Encoder2Decoder(Config()).to(dev).load_synthetic(123)
    feats = synthetic_features(B, dev, seed=0)
    for _ in range(args.warmup):
        out = model.sampler(feats, max_len=T)
    torch.cuda.synchronize()
    regions = []
    for _ in range(args.regions):
        t0 = time.perf_counter()
        for _ in range(K):
            out = model.sampler(feats, max_len=T)
        torch.cuda.synchronize()
        regions.append(time.perf_counter() - t0)
    el = float(np.median(regions))
    # traced pass: the same calls with an event pair handed to every step's launches
    per = {"k_lstm(step0)": [], "k_lstm": [], "k_atten": [], "k_vscreen": []}
    for _ in range(K):
        ev = {k: EventArray(2 * T) for k in ("lstm", "atten", "screen", "rescore")}
        ev["encoder"] = EventArray(2 * _lib.TRACE_ENCODER_KERNELS)
        tr = _lib.Trace(ev["encoder"].ptr, ev["lstm"].ptr, ev["atten"].ptr, ev["screen"].ptr, ev["rescore"].ptr, None)
        model.sampler(feats, max_len=T, trace=tr)
        torch.cuda.synchronize()
        lstm = ev["lstm"].pair_durations_ms()
        per["k_lstm(step0)"].append(lstm[0])
        per["k_lstm"] += lstm[1:]
        per["k_atten"] += ev["atten"].pair_durations_ms()
        per["k_vscreen"] += ev["screen"].pair_durations_ms()
    kernels = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                   "launches": len(v)} for k, v in per.items()}
    res = {"metric": f"captions/sec ({name} greedy, max_len={T}) at B={B}", "value": B * K / el,
           "unit": "captions/s", "n_gpus": 1, "steps": K, "warmup": args.warmup, "regions_s": regions,
           "reported": "median region", "ms_per_step": 1e3 * el / K, "higher_is_better": True, "dtype": "fp32",
           "model": name,
           "data": "synthetic: U[0,1) post-trunk features, random-init weights (adaptive_amd.synth seed 123)",
           "config": {"workload": f"{name}.Encoder2Decoder.sampler B={B} max_len={T}", "batch": B, "T": T},
           "kernels": kernels, "ids_checksum": int(out[0].sum().item())}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
