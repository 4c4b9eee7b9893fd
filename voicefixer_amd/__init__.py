"""voicefixer_amd -- the VoiceFixer restore / vocoder inference path on AMD MI355X (gfx950).

Same public surface as ``voicefixer`` for this path::

    from voicefixer_amd import VoiceFixer, Vocoder
"""
from .api import LoudnessMeter, RestoreSession, StreamPlanner, VoiceFixer, Vocoder, loudness_report, measure_loudness, measure_true_peak, quantize, limit, level  # noqa: F401
from .loudness import channel_weights  # noqa: F401

__all__ = ["VoiceFixer", "Vocoder", "measure_loudness", "measure_true_peak", "loudness_report", "RestoreSession",
           "StreamPlanner", "channel_weights", "quantize", "limit", "level", "LoudnessMeter"]
