"""Generate the baseline model's golden vectors by running the REAL reference
``baseline_attention.Encoder2Decoder.sampler`` on CPU.

Run where the reference tree is present (it is not on the GPU box):

    python tests/golden/make_golden_baseline.py [case ...]

The reference is driven as in ``make_golden.py``: ``torchvision`` stubbed so that ``resnet_conv`` is an
empty ``nn.Sequential`` (identity trunk, ``images`` = post-trunk features [B,2048,7,7]); weights =
``adaptive_amd.synth.make_weights`` minus the three sentinel tensors, loaded strictly.  The baseline
sampler transposes its states itself (``baseline_attention.py:251-252``), so nothing is patched.

A case whose smallest top-2 logit margin is below ``MIN_MARGIN`` is refused: the GPU tests compare its
ids for exact equality, and a fixture that fragile would make them depend on rounding.

Writes ``base_*.npz`` and ``manifest_baseline.json`` (data only; inputs are regenerated from seeds,
their sha256 recorded).
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from adaptive_amd import synth  # noqa: E402

MIN_MARGIN = 5e-5
ABSENT = ("decoder.adaptive.sentinel.affine_x.weight", "decoder.adaptive.sentinel.affine_h.weight",
          "decoder.adaptive.atten.affine_s.weight")
T = 20
CASES = [
    # name, weight seed, bias_noise, feature seed, B, what to keep
    ("base_b4", 123, 0.0, 0, 4, "full"),
    ("base_biased_b16", 99, 0.02, 5, 16, "t0"),
    ("base_b67", 123, 0.0, 0, 67, "alpha"),
    ("base_b130", 11, 0.02, 9, 130, "alpha_s4"),
]


def load_reference():
    sys.path.insert(0, HERE)
    import make_golden  # the torchvision stub and the reference tree's location
    make_golden.load_reference()
    from code_src.models import baseline_attention  # noqa: E402
    return baseline_attention


class Cf:
    base_word_embed_size = 256
    base_lstm_hidden_size = 512
    vocab_length = 10123


def baseline_weights(seed, bias_noise=0.0):
    return {k: v for k, v in synth.make_weights(seed, bias_noise=bias_noise).items() if k not in ABSENT}


def build(ba, state):
    torch.manual_seed(0)
    m = ba.Encoder2Decoder(Cf())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m.eval()
    return m


def run(m, feats):
    """sampler() plus the per-step logits captured by wrapping decoder.forward."""
    logs = []
    dec_forward = m.decoder.forward

    def dec_spy(*a, **k):
        out = dec_forward(*a, **k)
        logs.append(out[0].detach().clone())
        return out

    m.decoder.forward = dec_spy
    with torch.no_grad():
        ids, alpha = m.sampler(torch.from_numpy(feats), max_len=T)
    m.decoder.forward = dec_forward
    scores = torch.cat(logs, dim=1)  # [B,T,V]
    top2 = scores.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]).numpy()
    return ids.numpy(), alpha.numpy(), scores.numpy(), margin


def main(only=None):
    torch.set_num_threads(8)
    ba = load_reference()
    path = os.path.join(HERE, "manifest_baseline.json")
    manifest = {"reference": "wzn0828/Adaptive code_src/models/baseline_attention.py Encoder2Decoder.sampler",
                "torch": torch.__version__, "T": T, "min_margin_required": MIN_MARGIN, "cases": {}}
    if only:  # regenerate some cases only; the manifest keeps the others' entries
        with open(path) as f:
            manifest["cases"] = json.load(f)["cases"]
    for name, wseed, noise, fseed, B, keep in CASES:
        if only and name not in only:
            continue
        state = baseline_weights(wseed, noise)
        feats = synth.make_features(B, seed=fseed)
        ids, alpha, scores, margin = run(build(ba, state), feats)
        if float(margin.min()) < MIN_MARGIN:
            raise SystemExit(f"{name}: min top-2 margin {margin.min():.3e} < {MIN_MARGIN:.0e}: too fragile a fixture "
                             "for exact id comparison; choose other seeds")
        out = {"ids": ids.astype(np.int16), "margin": margin.astype(np.float32)}
        if keep == "alpha_s4":  # alpha of every 4th row
            out["alpha_s4"] = alpha[::4].astype(np.float32)
        else:
            out["alpha"] = alpha.astype(np.float32)
        if keep in ("full", "t0"):
            out["scores_t0"] = scores[:, 0].astype(np.float32)  # step-0 logits of every row
        if keep == "full":
            out["scores_r01_t01"] = scores[:2, :2].astype(np.float32)  # rows 0,1 at steps 0,1
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
        manifest["cases"][name] = {
            "weight_seed": wseed, "bias_noise": noise, "feature_seed": fseed, "B": B,
            "weights_sha256": synth.digest(state), "features_sha256": synth.digest({"f": feats})["f"],
            "min_margin": float(margin.min()), "distinct_tokens": int(len(np.unique(ids))),
        }
        print(name, manifest["cases"][name]["min_margin"], manifest["cases"][name]["distinct_tokens"], flush=True)
    m = build(ba, baseline_weights(123))
    manifest["state_dict"] = {k: list(v.shape) for k, v in m.state_dict().items()}
    with open(path, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:])  # optional case names
