"""adaptive_amd — MI355X-native greedy decode of the adaptive-attention captioner.

The hot path of wzn0828/Adaptive (``Encoder2Decoder.sampler``, code_src/models/adaptive_attention.py)
rebuilt as hand-written gfx950 HIP kernels behind a C-ABI (include/adaptive_amd.h), bound here with
ctypes and wrapped in a drop-in ``Encoder2Decoder`` module.  The reference's other shipped decoder,
the baseline spatial-attention model (code_src/models/baseline_attention.py), is
``adaptive_amd.baseline_attention.Encoder2Decoder``; ``get_model(cf)`` picks between them as the
reference's model factory does.
"""
from .synth import Dims, make_features, make_weights  # noqa: F401

__all__ = ["Dims", "make_features", "make_weights", "Encoder2Decoder", "Config", "DecodePlan", "get_model",
           "CiderD", "CaptionMetrics"]


def get_model(cf):
    """The model ``cf.atten_model_name`` names (code_src/models/model_factory.py:7-12).
    ``'rnn_attention'`` is not built (the reference's own constructor call for it fails)."""
    name = cf.atten_model_name
    if name == "baseline_attention":
        from . import baseline_attention
        return baseline_attention.Encoder2Decoder(cf)
    if name == "adaptive_attention":
        from . import adaptive_attention
        return adaptive_attention.Encoder2Decoder(cf)
    if name == "rnn_attention":
        raise NotImplementedError("adaptive_amd: atten_model_name 'rnn_attention' is not supported")
    raise ValueError(f"adaptive_amd: unknown atten_model_name {name!r}")


def __getattr__(name):  # lazy: importing the package must not require torch/HIP
    if name in ("Encoder2Decoder", "Config", "synthetic_features", "DecodePlan"):
        from . import adaptive_attention
        return getattr(adaptive_attention, name)
    if name == "CiderD":
        from .cider import CiderD
        return CiderD
    if name == "CaptionMetrics":
        from .metrics import CaptionMetrics
        return CaptionMetrics
    if name == "baseline_attention":
        import importlib
        return importlib.import_module(".baseline_attention", __name__)
    raise AttributeError(name)
