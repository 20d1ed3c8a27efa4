#!/usr/bin/env python3
"""CIDEr-D scoring benchmark: R = B * N captions of max_len T scored on 1 MI355X through CiderD.score
(C-ABI aa_cider_score: one k_cider launch), against a synthetic corpus of 5,000 images x 5 references.

The workload is the reward of one self-critical step: B = 512 images, N = 5 sampled captions each, every
caption scored against its image's references with document frequencies from the whole corpus.  Tokens are
Zipf-distributed over a 10,000-word vocabulary (a few words in most images, most words in few, as in
captions); a hypothesis is one of its image's references with some tokens redrawn, so n-grams do overlap.

Prints ONE JSON line: captions/s of ``score`` (HIP events around regions of ``--steps`` calls, the median
region after warm-up); in the same process the CPU oracle (tests/cider_oracle.py) on the same rows, on this
host; the host corpus build time; and the largest difference between the two sets of scores.

    python bench_cider.py [--steps 200] [--warmup 20] [--regions 9] [--batch 512] [--num-samples 5] [--T 20]
                          [--images 5000] [--refs 5]
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
from cider_oracle import CiderOracle  # noqa: E402  (checker and CPU yardstick)

END, VOCAB = 2, 10000


def zipf_tokens(rng, n):
    """n tokens in [3, 3 + VOCAB): rank r with probability ~ 1 / r."""
    p = 1.0 / np.arange(1, VOCAB + 1)
    return 3 + rng.choice(VOCAB, size=n, p=p / p.sum())


def make_corpus(rng, images, refs):
    lens = rng.integers(8, 17, size=images * refs)
    tok = zipf_tokens(rng, int(lens.sum()))
    caps = np.split(tok, np.cumsum(lens)[:-1])
    return [[caps[i * refs + j].tolist() for j in range(refs)] for i in range(images)]


def make_rows(rng, corpus, image_index, T):
    rows = np.full((len(image_index), T), END, dtype=np.int64)
    for r, i in enumerate(image_index):
        cap = np.array(corpus[i][int(rng.integers(len(corpus[i])))][:T])
        redraw = rng.random(cap.size) < 0.3
        cap[redraw] = zipf_tokens(rng, int(redraw.sum()))
        rows[r, :cap.size] = cap
    return rows


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
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, N, T, K = args.batch, args.num_samples, args.T, args.steps
    R = B * N
    rng = np.random.default_rng(0)
    corpus = make_corpus(rng, args.images, args.refs)
    image_index = np.repeat(rng.choice(args.images, size=B, replace=False), N)  # image-major, as sample(num_samples=N)
    rows = make_rows(rng, corpus, image_index, T)

    t0 = time.perf_counter()
    scorer = CiderD(corpus, end_id=END)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    scorer.to(dev)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    ids = torch.from_numpy(rows).to(dev)
    idx = torch.from_numpy(image_index.astype(np.int32)).to(dev)

    for _ in range(args.warmup):
        out = scorer.score(ids, idx)
    torch.cuda.synchronize()
    regions = []
    for _ in range(args.regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(K):
            out = scorer.score(ids, idx)
        b.record()
        b.synchronize()
        regions.append(a.elapsed_time(b) * 1e-3)
    el = float(np.median(regions))
    got = out.cpu().numpy()

    t0 = time.perf_counter()
    oracle = CiderOracle(corpus, end_id=END)
    oracle_build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = oracle.score(list(rows), image_index)
    cpu_s = time.perf_counter() - t0

    entries = int(scorer.ref_ptr[-1])
    res = {"metric": f"captions/sec (CiderD.score, max_len={T}) at R={R} (B={B} x N={N})", "value": R * K / el,
           "unit": "captions/s", "n_gpus": 1, "steps": K, "warmup": args.warmup, "regions_s": regions,
           "reported": "median region (HIP events around the region's calls)", "ms_per_call": 1e3 * el / K,
           "higher_is_better": True, "dtype": "fp64",
           "data": f"synthetic: {args.images} images x {args.refs} references of 8..16 Zipf tokens over {VOCAB} words "
                   "(numpy seed 0); hypotheses are references with 30 % of the tokens redrawn",
           "config": {"workload": f"CiderD.score R={R} T={T}, df from the references themselves", "batch": B,
                      "num_samples": N, "T": T, "images": args.images, "refs_per_image": args.refs},
           "corpus": {"host_build_s": build_s, "upload_s": upload_s, "ngram_entries": entries,
                      "table_slots": int(scorer.tab_keys.size), "distinct_ngrams": int(np.count_nonzero(scorer.tab_keys)),
                      "device_bytes": int(entries * 12 + scorer.tab_keys.size * 16 + scorer.refs * 40)},
           "cpu_oracle": {"value": R / cpu_s, "unit": "captions/s", "seconds": cpu_s, "build_s": oracle_build_s,
                          "what": "tests/cider_oracle.py CiderOracle.score on the same rows, one thread of this host"},
           "device_over_cpu_oracle": (R * K / el) / (R / cpu_s),
           "max_abs_diff_vs_oracle": float(np.max(np.abs(got - want))), "score_mean": float(got.mean()),
           "rows_scoring_above_zero": int((got > 0).sum())}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
