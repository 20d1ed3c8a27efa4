"""Drop-in ``Encoder2Decoder`` for the baseline spatial-attention model (the reference's default
``cf.atten_model_name = 'baseline_attention'``), executed by the no-sentinel MI355X HIP kernels.

The baseline model is the adaptive one minus the visual sentinel (code_src/models/baseline_attention.py):
alpha is a 49-way softmax, ``c_hat = c_t``, ``scores = mlp(c_t + h)``; there is no beta, no ``Sentinel``
module and no ``atten.affine_s`` (:66-128).  Public surface:

* ``Encoder2Decoder(cf)``                 — baseline_attention.py:198-204 (``cf.base_word_embed_size``,
  ``cf.base_lstm_hidden_size``, ``cf.vocab_length``)
* ``.sampler(images, max_len=30)``       — :233-280  -> (ids, alpha)
* ``.encoder(images)``                    — AttentiveCNN.forward, :36-62
* ``.decoder(V, v_g, captions, states)`` — Decoder.forward with one-token captions, :148-194
  -> (scores, alpha, states)
* ``DecodePlan(model, B, T)``             — replays return (ids, alpha)
* the 18 state-dict keys of the reference's baseline model.

The class reuses ``adaptive_attention.Encoder2Decoder`` (encoder tail, packing, workspace, trunk,
``fp32_encoder``, ``exact_vocab``); the packed weights carry NULL for the three absent parameters and
every decode passes ``AA_DECODE_BASELINE``.  Only ``cf.base_lstm_hidden_size == 512`` decodes (the
library returns its dims error otherwise).  Not built yet, each raising ``NotImplementedError`` before
any GPU work: ``forward`` (training), ``beam_search``, ``sample``, multi-token ``decoder(...)``, ``device_parallel``,
``distributed_sampler`` / ``sharded_sampler``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch.nn import init

from . import _lib
from . import adaptive_attention as _A
from .adaptive_attention import ATT, AttentiveCNN, DecodePlan  # noqa: F401  (same encoder, same plan class)

# the adaptive model's parameters minus the sentinel's
ABSENT_KEYS = ("decoder.adaptive.sentinel.affine_x.weight", "decoder.adaptive.sentinel.affine_h.weight",
               "decoder.adaptive.atten.affine_s.weight")
WEIGHT_FIELDS = [(f, k) for f, k in _lib.WEIGHT_FIELDS if k not in ABSENT_KEYS]


class Config:
    """The three ``cf`` attributes the baseline model reads (baseline_attention.py:203-204)."""

    def __init__(self, base_word_embed_size: int = 256, base_lstm_hidden_size: int = 512, vocab_length: int = 10123):
        self.base_word_embed_size = base_word_embed_size
        self.base_lstm_hidden_size = base_lstm_hidden_size
        self.vocab_length = vocab_length
        self.atten_model_name = "baseline_attention"


class _AsAdaptive:
    """``cf`` as the shared base class reads it (the base_* sizes under the adaptive_* names)."""

    def __init__(self, cf):
        self.adaptive_word_embed_size = cf.base_word_embed_size
        self.adaptive_lstm_hidden_size = cf.base_lstm_hidden_size
        self.vocab_length = cf.vocab_length


def _xavier_normal(nonlinearity, *mods):  # model_utils.xavier_normal
    gain = init.calculate_gain(nonlinearity)
    for m in mods:
        init.xavier_normal_(m.weight, gain)
        if m.bias is not None:
            m.bias.data.fill_(0)


class Atten(nn.Module):
    """Parameter holder of baseline_attention.py:66-76."""

    def __init__(self, hidden_size: int):
        super().__init__()
        self.affine_v = nn.Linear(hidden_size, ATT, bias=False)
        self.affine_g = nn.Linear(hidden_size, ATT, bias=False)
        self.affine_h = nn.Linear(ATT, 1, bias=False)
        self.dropout = nn.Dropout(0)
        _xavier_normal("tanh", self.affine_v, self.affine_g)
        _A._kaiming(init.kaiming_normal_, "relu", 0, self.affine_h)


class AdaptiveBlock(nn.Module):
    """Parameter holder of baseline_attention.py:100-114."""

    def __init__(self, hidden_size: int, vocab_size: int):
        super().__init__()
        self.atten = Atten(hidden_size)
        self.mlp = nn.Linear(hidden_size, vocab_size)
        self.dropout = nn.Dropout(0)
        _A._kaiming(init.kaiming_normal_, "relu", 0, self.mlp)


class Decoder(_A.Decoder):
    """Decoder (baseline_attention.py:132-194); ``forward`` is the shared dispatch to the owner."""

    def __init__(self, embed_size: int, vocab_size: int, hidden_size: int):
        nn.Module.__init__(self)
        self.embed = nn.Embedding(vocab_size, embed_size)
        self.LSTM = nn.LSTM(embed_size * 2, hidden_size, 1, batch_first=True)
        self.adaptive = AdaptiveBlock(hidden_size, vocab_size)
        _A._lstm_init(self.LSTM)
        self._owner = None


def _unsupported(what: str):
    return NotImplementedError(f"adaptive_amd: the baseline_attention model does not support {what} yet "
                               "(greedy sampler, one-token decoder steps and DecodePlan only)")


class Encoder2Decoder(_A.Encoder2Decoder):
    """baseline_attention.Encoder2Decoder on the no-sentinel MI355X kernels."""

    _weight_fields = WEIGHT_FIELDS

    def __init__(self, cf, trunk: bool = False):
        super().__init__(_AsAdaptive(cf), trunk=trunk)
        d = self.dims
        self.decoder = Decoder(d.embed, d.vocab, d.hidden)  # replaces the adaptive decoder (sentinel and all)
        object.__setattr__(self.decoder, "_owner", self)

    # ---- weights -------------------------------------------------------------------------------
    def load_synthetic(self, seed: int = 123, bias_noise: float = 0.0) -> "Encoder2Decoder":
        """The counter-based synthetic weights of the adaptive model minus the three sentinel tensors."""
        from .synth import make_weights
        dev = next(self.parameters()).device
        full = {k: torch.from_numpy(v).to(dev) for k, v in make_weights(seed, self.dims, bias_noise=bias_noise).items()
                if k not in ABSENT_KEYS}
        if self.has_trunk:
            full.update({"encoder.resnet_conv." + k: v for k, v in self.encoder.resnet_conv.state_dict().items()})
        self.load_state_dict(full, strict=True)
        return self

    def _decode_flags(self) -> int:
        return super()._decode_flags() | _lib.DECODE_BASELINE

    # ---- Encoder2Decoder.sampler (baseline_attention.py:233-280) --------------------------------
    @torch.no_grad()
    def sampler(self, images: torch.Tensor, max_len: int = 30, trace: Optional[_lib.Trace] = None,
                exact_vocab: bool = False):
        """Greedy decode -> (ids [B,max_len] int64, alpha [B,max_len,49]); ``exact_vocab`` and ``trace``
        as for the adaptive model's sampler.  This device only."""
        if self.device_parallel:
            raise _unsupported("device_parallel")
        if self.distributed_sampler:
            raise _unsupported("distributed_sampler")
        return self._sampler_local(images, max_len, trace, exact_vocab)

    @torch.no_grad()
    def _sampler_local(self, images, max_len, trace=None, exact_vocab=False):
        images = self._check_images(self.features(images))
        B, T, dev = images.size(0), int(max_len), images.device
        ids = torch.empty(B, T, dtype=torch.int64, device=dev)
        alpha = torch.empty(B, T, ATT, dtype=torch.float32, device=dev)
        self._decode_into(images, T, ids, alpha, None, trace=trace, exact_vocab=exact_vocab)
        return ids, alpha

    # ---- Decoder.forward, one token (baseline_attention.py:148-194) -------------------------------
    @torch.no_grad()
    def _decode_step(self, V, v_g, captions, states):
        """One-token captions [B,1] -> scores [B,1,V], alpha [B,1,49], (h, c) [1,B,H]
        (aa_baseline_decode_step)."""
        d = self.dims
        if captions.dim() != 2:
            raise ValueError(f"captions must be [B, T] token ids, got {tuple(captions.shape)}")
        if states is None:
            raise ValueError("states (h, c) are required")
        if captions.size(1) != 1:
            raise _unsupported("multi-token decoder(...) (teacher-forced captions)")
        B, dev = V.size(0), V.device
        h, c = states
        h = h.reshape(B, d.hidden).contiguous()
        c = c.reshape(B, d.hidden).contiguous()
        tokens = captions.reshape(B).to(torch.int64).contiguous()
        if B and (int(tokens.min()) < 0 or int(tokens.max()) >= d.vocab):
            raise IndexError("index out of range in self (embedding)")  # nn.Embedding's error
        model = self._model_struct()
        lib = _lib.load()
        V = V.contiguous()
        v_g = v_g.contiguous()
        h_out = torch.empty(1, B, d.hidden, device=dev)
        c_out = torch.empty(1, B, d.hidden, device=dev)
        scores = torch.empty(B, 1, d.vocab, device=dev)
        tok_out = torch.empty(B, dtype=torch.int64, device=dev)
        alpha = torch.empty(B, 1, ATT, device=dev)
        ws = self._workspace(lib.aa_step_workspace_bytes(self._c_dims(), B), dev)
        with torch.cuda.device(dev):
            rc = lib.aa_baseline_decode_step(model, B, tokens.data_ptr(), V.data_ptr(), None, v_g.data_ptr(),
                                             h.data_ptr(), c.data_ptr(), h_out.data_ptr(), c_out.data_ptr(),
                                             scores.data_ptr(), tok_out.data_ptr(), alpha.data_ptr(), _lib.ptr(ws),
                                             ws.numel() if ws is not None else 0, _lib.stream_handle())
        _lib.check(rc, "baseline_decode_step")
        self._last_tokens = tok_out
        return scores, alpha, (h_out, c_out)

    # ---- not built for the baseline model: none of these may run sentinel code ------------------
    def forward(self, images, captions, lengths):
        raise _unsupported("forward (teacher-forced training)")

    def beam_search(self, *args, **kwargs):
        raise _unsupported("beam_search")

    def sample(self, *args, **kwargs):
        raise _unsupported("sample")

    def sharded_sampler(self, *args, **kwargs):
        raise _unsupported("sharded_sampler")
