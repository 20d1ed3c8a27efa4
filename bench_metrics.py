#!/usr/bin/env python3
"""BLEU / ROUGE-L scoring benchmark: R = B * N captions of max_len T scored on 1 MI355X through
CaptionMetrics.score (C-ABI aa_metrics_score: one k_metrics launch), on bench_cider.py's workload -- a
synthetic corpus of 5,000 images x 5 references, B = 512 images, N = 5 captions each.

Prints ONE JSON line and writes it to ``--out`` (default profiles/b512_n5_metrics_bench.json): ms per
``score`` call (HIP events around regions of ``--steps`` calls, the median region after warm-up); in the same
process ms per ``CiderD.score`` call on the same rows (k_cider, the kernel this one sits beside) and per
``corpus_score`` call (score + aa_bleu_corpus + the means); the CPU oracle (tests/metrics_oracle.py) on the
same rows, on this host; the host corpus build time; and the largest differences between device and oracle.
``--sample-ms`` takes the ms per ``sample(num_samples=N)`` call that bench_sample.py printed in the same
session and reports the scoring as a share of it.

    python bench_metrics.py [--steps 200] [--warmup 20] [--regions 9] [--batch 512] [--num-samples 5] [--T 20]
                            [--images 5000] [--refs 5] [--sample-ms MS] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from adaptive_amd.cider import CiderD  # noqa: E402
from adaptive_amd.metrics import CaptionMetrics  # noqa: E402
from bench_cider import END, VOCAB, make_corpus, make_rows  # noqa: E402  (the same workload)
from metrics_oracle import MetricsOracle  # noqa: E402  (checker and CPU yardstick)


def timed(fn, steps, warmup, regions):
    """Seconds per region of `steps` calls: the median of `regions` regions between HIP events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="score calls per timed region")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--num-samples", type=int, default=5)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--refs", type=int, default=5)
    ap.add_argument("--sample-ms", type=float, default=None,
                    help="ms per sample(num_samples=N) call from bench_sample.py in the same session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "b512_n5_metrics_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, N, T, K = args.batch, args.num_samples, args.T, args.steps
    R = B * N
    rng = np.random.default_rng(0)
    corpus = make_corpus(rng, args.images, args.refs)
    image_index = np.repeat(rng.choice(args.images, size=B, replace=False), N)  # image-major, as sample(num_samples=N)
    rows = make_rows(rng, corpus, image_index, T)

    t0 = time.perf_counter()
    scorer = CaptionMetrics(corpus, end_id=END)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    scorer.to(dev)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    cider = CiderD(corpus, end_id=END).to(dev)
    ids = torch.from_numpy(rows).to(dev)
    idx = torch.from_numpy(image_index.astype(np.int32)).to(dev)

    el, regions = timed(lambda: scorer.score(ids, idx), K, args.warmup, args.regions)
    el_cider, regions_cider = timed(lambda: cider.score(ids, idx), K, args.warmup, args.regions)
    el_table, regions_table = timed(lambda: scorer.corpus_score(ids, idx), K, args.warmup, args.regions)
    got = scorer.score(ids, idx)
    table = {k: v.item() for k, v in scorer.corpus_score(ids, idx, cider=cider).items()}

    t0 = time.perf_counter()
    oracle = MetricsOracle(corpus, end_id=END)
    oracle_build_s = time.perf_counter() - t0
    hyps = list(rows)
    t0 = time.perf_counter()
    want_stats, want_bleu, want_rouge = (oracle.stats(hyps, image_index), oracle.bleu(hyps, image_index),
                                         oracle.rouge(hyps, image_index))
    cpu_s = time.perf_counter() - t0
    want_table = oracle.corpus(hyps, image_index)

    res = {"metric": f"captions/sec (CaptionMetrics.score, max_len={T}) at R={R} (B={B} x N={N})", "value": R * K / el,
           "unit": "captions/s", "n_gpus": 1, "steps": K, "warmup": args.warmup, "regions_s": regions,
           "reported": "median region (HIP events around the region's calls)", "ms_per_call": 1e3 * el / K,
           "higher_is_better": True, "dtype": "int32 statistics, fp64 scores",
           "data": f"synthetic: {args.images} images x {args.refs} references of 8..16 Zipf tokens over {VOCAB} words "
                   "(numpy seed 0); hypotheses are references with 30 % of the tokens redrawn (bench_cider.py's)",
           "config": {"workload": f"CaptionMetrics.score R={R} T={T}: BLEU-1..4 statistics and scores, ROUGE-L",
                      "batch": B, "num_samples": N, "T": T, "images": args.images, "refs_per_image": args.refs},
           "cider_same_rows": {"ms_per_call": 1e3 * el_cider / K, "regions_s": regions_cider,
                               "what": "CiderD.score (k_cider) on the same rows, same process"},
           "metrics_over_cider": el / el_cider,
           "corpus_score": {"ms_per_call": 1e3 * el_table / K, "regions_s": regions_table,
                            "what": "score + aa_bleu_corpus + the ROUGE-L mean and the dict's slices"},
           "corpus": {"host_build_s": build_s, "upload_s": upload_s, "clip_entries": int(scorer.clip_keys.size),
                      "reference_tokens": int(scorer.ref_tok.size),
                      "device_bytes": int(scorer.clip_keys.size * 12 + scorer.ref_tok.size * 2 + scorer.refs * 8
                                          + scorer.images * 8)},
           "cpu_oracle": {"value": R / cpu_s, "unit": "captions/s", "seconds": cpu_s, "build_s": oracle_build_s,
                          "what": "tests/metrics_oracle.py stats + bleu + rouge on the same rows, one thread of this host"},
           "device_over_cpu_oracle": (R * K / el) / (R / cpu_s),
           "stats_equal_oracle": bool(np.array_equal(got.stats.cpu().numpy(), want_stats)),
           "max_abs_diff_vs_oracle": {"bleu": float(np.max(np.abs(got.bleu.cpu().numpy() - want_bleu))),
                                      "rouge_l": float(np.max(np.abs(got.rouge_l.cpu().numpy() - want_rouge))),
                                      "table": float(max(abs(table[k] - want_table[k]) for k in want_table))},
           "table": table}
    if args.sample_ms is not None:
        res["share_of_sample"] = {"sample_ms_per_call": args.sample_ms, "metrics": 1e3 * el / K / args.sample_ms,
                                  "what": f"ms per score call over ms per sample(num_samples={N}) call "
                                          "(bench_sample.py, same session)"}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
