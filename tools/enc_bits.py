#!/usr/bin/env python3
"""Bitwise A/B of the encoder tail's V and a_g between two library builds (GPU box).

    python tools/enc_bits.py a.so b.so [--batches 1,3,67,512] [--hidden 512,256] [--time N]

Each build runs in a child process of its own (one HIP runtime and one library per process), which
encodes the seeded feature batches through the default path and through the forced bf16x3 body and
prints the sha256 of every output; the parent compares the digests.  --time N also times N encoder
tails at the largest batch in each child (device events around Encoder2Decoder._encode: k_enc_v4,
the heads, VWv and x_g), after N / 2 warm-up calls.  Exit status 0: every output bit-identical."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def child(batches, hidden, ntime):
    import numpy as np
    import torch
    from adaptive_amd import Config, Encoder2Decoder, _lib
    from adaptive_amd.adaptive_attention import synthetic_features
    dev = torch.device("cuda", 0)
    out = {}
    for H in hidden:
        m = Encoder2Decoder(Config(adaptive_lstm_hidden_size=H)).to(dev).load_synthetic(123)
        for B in batches:
            feats = synthetic_features(B, dev, seed=3)
            for forced in (False, True):
                m.decode_extra_flags = _lib.DECODE_ENC_BF16X3 if forced else 0
                V, _, _, a_g, _ = m._encode(feats)
                torch.cuda.synchronize()
                for name, x in (("V", V), ("a_g", a_g)):
                    key = f"H{H} B{B} {'bf16x3' if forced else 'default'} {name}"
                    out[key] = hashlib.sha256(np.ascontiguousarray(x.cpu().numpy()).tobytes()).hexdigest()
            m.decode_extra_flags = 0
        if ntime:
            feats = synthetic_features(max(batches), dev, seed=0)
            for _ in range(max(1, ntime // 2)):
                m._encode(feats)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ntime)]
            for a, b in ev:
                a.record()
                m._encode(feats)
                b.record()
            torch.cuda.synchronize()
            us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
            out[f"H{H} B{max(batches)} encoder tail us (min, median, max)"] = [us[0], us[len(us) // 2], us[-1]]
    print("ENC_BITS " + json.dumps(out), flush=True)


def run_child(lib, args):
    env = dict(os.environ, AA_LIB_PATH=os.path.abspath(lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batches", args.batches, "--hidden", args.hidden,
           "--time", str(args.time)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"{lib}: child exited {r.returncode}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ENC_BITS ")][-1]
    return json.loads(line[len("ENC_BITS "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--batches", default="1,3,67,512")
    ap.add_argument("--hidden", default="512,256")
    ap.add_argument("--time", type=int, default=0)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    ints = lambda v: [int(x) for x in v.split(",")]
    if args.child:
        child(ints(args.batches), ints(args.hidden), args.time)
        return 0
    if len(args.libs) != 2:
        ap.error("two library paths")
    a, b = (run_child(lib, args) for lib in args.libs)
    ok = True
    for k in list(a) + [k for k in b if k not in a]:
        if isinstance(a.get(k, b.get(k)), list):
            print(f"{k}: {args.libs[0]} {a.get(k)}  {args.libs[1]} {b.get(k)}")
            continue
        same = k in a and k in b and a[k] == b[k]
        ok &= same
        print(k, "bit-identical" if same else "DIFFERS")
    print("ALL BIT-IDENTICAL" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
