"""pvamd — host-side mirror of the reference's PhaseVocoder interface over libpv.so
(the MI355X HIP phase-vocoder hot path).  See DESIGN.md and include/pv.h."""
from ._lib import PVError, frame_count, lib  # noqa: F401
from .vocoder import (CHROMATIC, MAJOR, PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT,  # noqa: F401
                      PhaseVocoder, pitch_correction, rate_map, timemap_split)
from .realtime import RealTimeVocoder, interval_ratios  # noqa: F401
from .harmonizer import Harmonizer  # noqa: F401
from .resample import Resampler  # noqa: F401
from .varresample import VarResampler, pitch_map_plan, ratio_steps  # noqa: F401

__all__ = ["PhaseVocoder", "PVError", "TIME_SHIFT", "PITCH_SHIFT", "REF_COMPAT", "STANDARD", "RealTimeVocoder", "Harmonizer",
           "Resampler", "VarResampler", "frame_count", "lib", "pitch_map_plan", "rate_map", "ratio_steps",
           "timemap_split", "pitch_correction", "MAJOR", "CHROMATIC", "interval_ratios"]
