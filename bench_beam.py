#!/usr/bin/env python3
"""Beam-search benchmark (BASELINE.json config 4): B=512 images, beam 3,
max_len 20 on 1 MI355X through Encoder2Decoder.beam_search (C-ABI aa_beam_decode).

Synthetic post-trunk features U[0,1) and the portable random-init weights (adaptive_amd.synth),
inputs resident in HBM.  Prints ONE JSON line: captions/s (one caption = the best beam of one image,
all K beams decoded), ms per batch, and the CPU restatement (oracle BeamOracle) timed on a bounded
sample on this host.

    python bench_beam.py [--steps 10] [--warmup 2] [--batch 512] [--beam 3] [--T 20] [--no-cpu-baseline]

--groups G / --diversity L / --length-penalty A (any of them given): the line is that of the grouped
decode (aa_beam_decode_ex: k_beam_select3<true>, k_beam_final_ex), and its "ab" entry compares it with the
plain call (aa_beam_decode) at the same beam width in this process: --regions alternating regions of
--steps calls each, the median region of either, and their ratio.

--suppress N / --min-length M / --no-repeat-ngram n / --no-end-after N (any of them given): the line is that
of the constrained decode (aa_beam_decode_cx: k_beam_select3c) with the other options as given, and its "cons"
entry compares it with the same call without constraints in this process, as "ab" does.  The suppressed ids
are the N most frequent non-<end> tokens of a warm-up decode, the no-end-after ids the most frequent ones
after those.
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

from adaptive_amd import Config, Encoder2Decoder, synth  # noqa: E402
from adaptive_amd.adaptive_attention import synthetic_features  # noqa: E402
from adaptive_amd.hip_events import EventArray  # noqa: E402

PEAK_FP32 = 157.3e12       # MI355X dense fp32 MFMA (MI355X_MICROARCH.md)
PEAK_X3 = 2.5e15 / 6       # fp32-accurate bf16x3 GEMM: six bf16 MFMA products per fp32 product


def cpu_baseline(K, T, sample, budget_s):
    from oracle.adaptive_oracle import BeamOracle  # test / baseline infrastructure only
    from bench import available_cpus  # every CPU this process may use (affinity capped by the cgroup quota)
    threads = available_cpus()["usable"]
    torch.set_num_threads(threads)
    m = BeamOracle(synth.make_weights(123))
    feats = torch.from_numpy(synth.make_features(sample, seed=0))
    times = []
    t_end = time.perf_counter() + budget_s
    while len(times) < 2 or (time.perf_counter() < t_end and len(times) < 5):
        t0 = time.perf_counter()
        m.beam_search(feats, T, K)
        times.append(time.perf_counter() - t0)
    med = float(np.median(times))
    return {"value": sample / med, "unit": "captions/s", "cores": threads, "kind": "port",
            "sample": f"oracle/adaptive_oracle.py BeamOracle (PyTorch-CPU fp32, the reference decoder step) on "
                      f"{sample} images, beam {K}, max_len {T}; median of {len(times)} runs "
                      f"({', '.join(f'{t:.2f}' for t in times)} s); {threads} threads"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--beam", type=int, default=3)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--cpu-sample", type=int, default=64)
    ap.add_argument("--cpu-budget", type=float, default=15.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--fast", action="store_true", help="opt-in bf16x3 logits (AA_BEAM_FAST) instead of the exact "
                    "fp32 default")
    ap.add_argument("--groups", type=int, default=None, help="diverse beam search: G groups of beam / G slots")
    ap.add_argument("--diversity", type=float, default=None, help="Hamming diversity penalty per earlier group's pick")
    ap.add_argument("--length-penalty", type=float, default=None, help="rank the final beams by score / len^A")
    ap.add_argument("--regions", type=int, default=5, help="grouped / constrained decode: alternating regions per "
                    "side of the A/B")
    ap.add_argument("--suppress", type=int, default=0, help="suppress the N most frequent tokens of a warm-up decode")
    ap.add_argument("--min-length", type=int, default=0, help="no <end> before this many tokens")
    ap.add_argument("--no-repeat-ngram", type=int, default=0, help="no n-gram twice in a hypothesis")
    ap.add_argument("--no-end-after", type=int, default=0, help="no <end> right after the next N most frequent tokens")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, K, T = args.batch, args.beam, args.T
    grouped = not (args.groups is None and args.diversity is None and args.length_penalty is None)
    # the grouped decode goes through aa_beam_decode_ex whatever the values (return_details forces it)
    div = ({"groups": args.groups or 1, "diversity": args.diversity or 0.0, "length_penalty": args.length_penalty or 0.0,
            "return_details": True} if grouped else {})
    model = Encoder2Decoder(Config()).to(dev).load_synthetic(123)
    feats = synthetic_features(B, dev, seed=0)

    def region(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            o = model.beam_search(feats, T, K, fast=args.fast, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, o

    for _ in range(args.warmup):
        model.beam_search(feats, T, K, fast=args.fast, **div)
    el, out = region(div)
    ab = cons = None
    if args.suppress or args.min_length or args.no_repeat_ngram or args.no_end_after:
        seqs = out[3].flatten()
        ids, counts = torch.unique(seqs[seqs != 2], return_counts=True)
        freq = ids[torch.argsort(counts, descending=True, stable=True)].tolist()
        ckw = {"suppress_ids": tuple(freq[:args.suppress]), "min_length": args.min_length,
               "no_repeat_ngram": args.no_repeat_ngram,
               "no_end_after": tuple(freq[args.suppress:args.suppress + args.no_end_after])}
        for _ in range(args.warmup):
            out = model.beam_search(feats, T, K, fast=args.fast, **div, **ckw)
        free_s, cons_s = [], []
        for _ in range(max(1, args.regions)):
            free_s.append(region(div)[0])
            cons_s.append(region({**div, **ckw})[0])
        mf, mc = float(np.median(free_s)), float(np.median(cons_s))
        sel = "k_beam_select3c<true>" if grouped else "k_beam_select3c<false>"
        cons = {"regions": len(cons_s), "calls_per_region": args.steps, **ckw,
                "unconstrained": {"ms_per_call": 1e3 * mf / args.steps, "captions_per_s": B * args.steps / mf,
                                  "region_ms": [1e3 * x for x in free_s]},
                "constrained": {"path": f"aa_beam_decode_cx ({sel})", "ms_per_call": 1e3 * mc / args.steps,
                                "captions_per_s": B * args.steps / mc, "region_ms": [1e3 * x for x in cons_s]},
                "constrained_over_unconstrained_time": mc / mf}
        div = {**div, **ckw}
        el = mc
    if grouped and not cons:
        for _ in range(args.warmup):
            model.beam_search(feats, T, K, fast=args.fast)
        plain_s, div_s = [], []
        for _ in range(max(1, args.regions)):
            plain_s.append(region({})[0])
            div_s.append(region(div)[0])
        mp, md = float(np.median(plain_s)), float(np.median(div_s))
        ab = {"regions": len(div_s), "calls_per_region": args.steps,
              "plain": {"path": "aa_beam_decode (k_beam_select3<false>, k_beam_final)", "ms_per_call": 1e3 * mp / args.steps,
                        "captions_per_s": B * args.steps / mp, "region_ms": [1e3 * x for x in plain_s]},
              "grouped": {"path": "aa_beam_decode_ex (k_beam_select3<true>, k_beam_final_ex)",
                          "ms_per_call": 1e3 * md / args.steps, "captions_per_s": B * args.steps / md,
                          "region_ms": [1e3 * x for x in div_s]},
              "grouped_over_plain_time": md / mp}
        el = md
    # traced pass (the same calls again): HIP events on the launch stream around every step's vocab
    # stage -- the dominant kernel (k_vexact: exact fp32 logits + granule summaries; fast mode:
    # k_vbeam5 / k_vbeam4) -- for its average launch duration
    evs = [EventArray(2 * T) for _ in range(args.steps)]
    for ev in evs:
        model.beam_search(feats, T, K, fast=args.fast, vocab_events=ev.ptr, **div)
    torch.cuda.synchronize()
    durs = [d for ev in evs for d in ev.pair_durations_ms()]
    avg_ms = float(np.mean(durs))
    Vn, H = model.dims.vocab, model.dims.hidden
    flops = 2.0 * B * K * Vn * H  # algorithmic: the [B K, H] x [H, V] logits GEMM of one step
    peak = PEAK_X3 if args.fast else PEAK_FP32
    kname = "k_vbeam5" if args.fast else "k_vexact"
    traffic = None
    try:
        with open(os.path.join(ROOT, "profiles", "traffic_beam.json")) as f:
            traffic = json.load(f).get(kname, {}).get("hbm_bytes_per_launch")
    except Exception:
        pass
    roofline = {"kernel": kname, "bound": "mfma", "achieved": flops / (avg_ms * 1e-3) / 1e12, "peak": peak / 1e12,
                "unit": "TFLOP/s", "frac": flops / (avg_ms * 1e-3) / peak, "traffic": traffic,
                "avg_launch_ms": avg_ms, "launches_timed": len(durs), "algorithmic_flops_per_launch": flops,
                "note": ("bf16x3 GEMM priced at bf16 peak / 6" if args.fast else
                         "exact fp32 GEMM on v_mfma_f32_32x32x2f32, priced at the fp32 MFMA peak") +
                        "; the launch also writes the per-granule (max, sum exp) summaries"}
    res = {"metric": f"captions/sec (beam {K}, max_len={T}) at B={B}", "value": B * args.steps / el,
           "unit": "captions/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": 1e3 * el / args.steps, "higher_is_better": True, "dtype": "fp32",
           "data": "synthetic: U[0,1) post-trunk features, random-init weights (adaptive_amd.synth seed 123)",
           "config": {"workload": f"Encoder2Decoder.beam_search B={B} beam={K} max_len={T}", "batch": B,
                      "beam": K, "T": T, "rows": B * K,
                      "vocab_kernel": "bf16x3 k_vbeam5 (256x256)"
                      if args.fast else "exact fp32: k_vexact (fused fp32 MFMA logits + granule summaries)",
                      "mode": "fast (opt-in bf16x3)" if args.fast else "exact (default)",
                      **({k: div[k] for k in ("groups", "diversity", "length_penalty")} if grouped else {})},
           "best_score_mean": float(out[4][:, 0].mean().item()), "roofline": roofline, "cpu_baseline": None}
    if ab:
        res["ab"] = ab
    if cons:
        res["cons"] = cons
    if not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(K, T, args.cpu_sample, args.cpu_budget)
        res["speedup_vs_cpu"] = res["value"] / res["cpu_baseline"]["value"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
