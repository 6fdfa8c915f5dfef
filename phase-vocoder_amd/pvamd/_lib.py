"""ctypes binding of libpv.so (include/pv.h).  Loads the in-tree build and fails loudly
if it is missing: there is no CPU fallback in the product path."""
from __future__ import annotations

import ctypes
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(_PKG, "..", ".."))
LIB_PATH = os.environ.get("PV_LIB_PATH") or os.path.join(_PKG, "..", "build", "libpv.so")
HEADER = os.path.join(ROOT, "include", "pv.h")

PV_OK, PV_ERR_ARG, PV_ERR_UNSUPPORTED, PV_ERR_HIP, PV_ERR_NOMEM = range(5)
PV_TIME_SHIFT, PV_PITCH_SHIFT = ord("t"), ord("p")
PV_MODE_REF_COMPAT, PV_MODE_STANDARD = 0, 1
PV_WINDOW_DEFAULT, PV_WINDOW_HAMMING_REF, PV_WINDOW_HANN_REF = 0, 1, 2
PV_SPEC_NATURAL, PV_SPEC_PACKED = 0, 1
PV_TRANSIENT_OFF, PV_TRANSIENT_FLAGS, PV_TRANSIENT_DETECT = 0, 1, 2
PV_TRANSIENT_DEFAULT_THRESHOLD = 0.3  # include/pv.h
PV_PITCH_TRACK_DEFAULT_KAPPA = 0.9  # include/pv.h
ABI_VERSION = 5  # PV_ABI_VERSION of include/pv.h (pv_config / pv_info lead with it)


class PVError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{msg} (status {status})")
        self.status = status


class pv_config(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int), ("n_samps", ctypes.c_int), ("hop_div", ctypes.c_int), ("effect", ctypes.c_int),
                ("scale", ctypes.c_float), ("mode", ctypes.c_int), ("max_channels", ctypes.c_int),
                ("max_frames", ctypes.c_int), ("device", ctypes.c_int), ("window", ctypes.c_int),
                ("nan_faithful", ctypes.c_int), ("spec_layout", ctypes.c_int),
                ("tables_external", ctypes.c_int)]


class pv_info(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int), ("n_samps", ctypes.c_int), ("hop", ctypes.c_int), ("out_hop", ctypes.c_int),
                ("spec_bins", ctypes.c_int), ("spec_stride", ctypes.c_int),
                ("frames_per_run", ctypes.c_int), ("mode", ctypes.c_int), ("effect", ctypes.c_int),
                ("scale", ctypes.c_float), ("single_launch", ctypes.c_int),
                ("single_launch_frames", ctypes.c_int),
                ("lane_constants", ctypes.c_int), ("spec_layout", ctypes.c_int)]


class pv_pitch_correct(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int), ("a4", ctypes.c_double), ("scale_mask", ctypes.c_uint),
                ("strength_min", ctypes.c_double), ("retune", ctypes.c_double)]


def config(n_samps, hop_div, effect, scale, mode, max_channels, max_frames, device=0, window=PV_WINDOW_DEFAULT,
           nan_faithful=0, spec_layout=PV_SPEC_NATURAL, tables_external=0) -> pv_config:
    """A pv_config for this ABI (abi_version filled in)."""
    return pv_config(ABI_VERSION, int(n_samps), int(hop_div), int(effect), float(scale), int(mode),
                     int(max_channels), int(max_frames), int(device), int(window), int(nan_faithful),
                     int(spec_layout), int(tables_external))


def new_info() -> pv_info:
    """A pv_info for pv_get_info (abi_version filled in)."""
    i = pv_info()
    i.abi_version = ABI_VERSION
    return i


_lib = None
CSRC = os.path.join(ROOT, "phase-vocoder_amd", "csrc")


def sources_sha() -> str:
    """sha256[:16] of the library's sources as the Makefile computes it (SHA_FILES: every
    *.hip *.hpp *.h *.cpp in csrc/ and the Makefile in byte order, then include/pv.h)"""
    import hashlib
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".h", ".cpp")) or f == "Makefile")
    h = hashlib.sha256()
    for p in [os.path.join(CSRC, f) for f in names] + [HEADER]:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def declared_symbols() -> list[str]:
    """Function names declared in include/pv.h (the ABI contract)."""
    txt = open(HEADER).read()
    return sorted(set(m.group(2) for m in re.finditer(r"^\s*((?:[\w\s\*]+?))\b(pv_\w+)\s*\(", txt, flags=re.M)
                      if "static" not in m.group(1)))  # static inline helpers are not exported


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PVError(-1, f"libpv.so not built at {LIB_PATH}: run `make -C phase-vocoder_amd/csrc` "
                          "(no CPU fallback exists)")
    L = ctypes.CDLL(os.path.abspath(LIB_PATH))
    vp, ll, i, f = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_float
    # a library built from other sources than this tree's (a stale build shipped with the
    # tree, or a leftover) is refused: `make` rebuilds it
    L.pv_sources_sha.restype = ctypes.c_char_p
    built, tree = L.pv_sources_sha().decode(), sources_sha()
    if built != tree:
        raise PVError(-1, f"{LIB_PATH} was built from sources {built}, the tree's are {tree}: "
                          "rebuild with `make -C phase-vocoder_amd/csrc`")
    L.pv_abi_version.restype = i
    if hasattr(L, "pv_contract_version"):  # (A/B builds of older revisions lack it)
        L.pv_contract_version.restype = i
    if hasattr(L, "pv_diagnostic_build"):
        L.pv_diagnostic_build.restype = i
    L.pv_status_string.argtypes = [i]
    L.pv_status_string.restype = ctypes.c_char_p
    L.pv_last_error.restype = ctypes.c_char_p
    L.pv_create.argtypes = [ctypes.POINTER(pv_config), ctypes.POINTER(vp)]
    L.pv_create.restype = i
    L.pv_destroy.argtypes = [vp]
    L.pv_destroy.restype = None
    L.pv_get_info.argtypes = [vp, ctypes.POINTER(pv_info)]
    L.pv_get_info.restype = i
    L.pv_frame_count.argtypes = [ll, i]
    L.pv_frame_count.restype = i
    L.pv_output_length.argtypes = [vp, i]
    L.pv_output_length.restype = ll
    L.pv_analysis.argtypes = [vp, vp, ll, ll, i, i, vp, ll, vp]
    L.pv_analysis.restype = i
    L.pv_resynthesis.argtypes = [vp, vp, ll, i, i, vp, ll, vp, ll, vp]
    L.pv_resynthesis.restype = i
    L.pv_segment_summary_words.argtypes = [vp]
    L.pv_segment_summary_words.restype = i
    L.pv_segment_summary.argtypes = [vp, vp, ll, i, i, vp, vp]
    L.pv_segment_summary.restype = i
    L.pv_segment_resynthesis.argtypes = [vp, vp, ll, i, i, ll, vp, i, vp, ll, vp]
    L.pv_segment_resynthesis.restype = i
    L.pv_process.argtypes = [vp, vp, ll, ll, i, i, vp, ll, vp, ll, vp]
    L.pv_process.restype = i
    L.pv_reserve_spectrum.argtypes = [vp]
    L.pv_reserve_spectrum.restype = i
    L.pv_resident_min_channels.argtypes = [vp]
    L.pv_resident_min_channels.restype = i
    L.pv_set_phase_lock.argtypes = [vp, i]
    L.pv_set_phase_lock.restype = i
    L.pv_get_phase_lock.argtypes = [vp]
    L.pv_get_phase_lock.restype = i
    L.pv_set_formant.argtypes = [vp, i]
    L.pv_set_formant.restype = i
    L.pv_get_formant.argtypes = [vp]
    L.pv_get_formant.restype = i
    L.pv_spectral_envelope.argtypes = [vp, vp, ll, i, i, i, vp, ll, vp]
    L.pv_spectral_envelope.restype = i
    L.pv_export_tables.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), vp]
    L.pv_export_tables.restype = i
    L.pv_import_tables.argtypes = [vp, vp, ctypes.c_size_t, vp]
    L.pv_import_tables.restype = i
    L.pv_set_window.argtypes = [vp, vp, vp]
    L.pv_set_window.restype = i
    L.pv_test_overlap_add.argtypes = [vp, vp, vp, vp, i, i, vp]
    L.pv_test_overlap_add.restype = i
    L.pv_profile_enable.argtypes = [vp, i]
    L.pv_profile_enable.restype = i
    L.pv_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_int), i]
    L.pv_profile_read.restype = i
    L.pv_profile_reset.argtypes = [vp]
    L.pv_profile_reset.restype = None
    L.pv_rt_create.argtypes = [ctypes.POINTER(pv_config), i, ctypes.POINTER(vp)]
    L.pv_rt_create.restype = i
    L.pv_rt_destroy.argtypes = [vp]
    L.pv_rt_destroy.restype = None
    L.pv_rt_reset.argtypes = [vp, vp]
    L.pv_rt_reset.restype = i
    L.pv_rt_push.argtypes = [vp, vp, ll, i, vp, ll, vp, ll, vp]
    L.pv_rt_push.restype = i
    L.pv_rt_capture.argtypes = [vp, i]
    L.pv_rt_capture.restype = i
    fpp = ctypes.POINTER(ctypes.POINTER(ctypes.c_float))
    L.pv_rt_host_buffers.argtypes = [vp, fpp, fpp]
    L.pv_rt_host_buffers.restype = i
    L.pv_rt_callback.argtypes = [vp, vp, vp]
    L.pv_rt_callback.restype = i
    L.pv_rt_set_phase_lock.argtypes = [vp, i]
    L.pv_rt_set_phase_lock.restype = i
    L.pv_rt_get_phase_lock.argtypes = [vp]
    L.pv_rt_get_phase_lock.restype = i
    L.pv_rt_pitch_reserve.argtypes = [vp, i, i]
    L.pv_rt_pitch_reserve.restype = i
    L.pv_rt_pitch_latency.argtypes = [vp]
    L.pv_rt_pitch_latency.restype = i
    L.pv_rt_pitch_push.argtypes = [vp, vp, ll, i, vp, ll, vp, ll, vp]
    L.pv_rt_pitch_push.restype = i
    L.pv_rt_pitchmap_reserve.argtypes = [vp, i, i, f, f]
    L.pv_rt_pitchmap_reserve.restype = i
    L.pv_rt_pitchmap_latency.argtypes = [vp]
    L.pv_rt_pitchmap_latency.restype = i
    L.pv_rt_pitchmap_push.argtypes = [vp, vp, ll, i, vp, ll, vp, ll, vp, ll, vp]
    L.pv_rt_pitchmap_push.restype = i
    L.pv_rt_pitchmap_host_ratios.argtypes = [vp, fpp]
    L.pv_rt_pitchmap_host_ratios.restype = i
    L.pv_rt_harmonizer_max_voices.argtypes = [i]
    L.pv_rt_harmonizer_max_voices.restype = i
    L.pv_rt_harmonizer_reserve.argtypes = [vp, i, i, i, f, f]
    L.pv_rt_harmonizer_reserve.restype = i
    L.pv_rt_harmonizer_voices.argtypes = [vp]
    L.pv_rt_harmonizer_voices.restype = i
    L.pv_rt_harmonizer_latency.argtypes = [vp]
    L.pv_rt_harmonizer_latency.restype = i
    L.pv_rt_harmonizer_push.argtypes = [vp, vp, ll, i, vp, vp, ll, vp, ll, vp, ll, vp, ll, vp]
    L.pv_rt_harmonizer_push.restype = i
    L.pv_rt_harmonizer_host_controls.argtypes = [vp, fpp, fpp]
    L.pv_rt_harmonizer_host_controls.restype = i
    L.pv_fft_c2c.argtypes = [vp, vp, i, i, i, vp]
    L.pv_fft_c2c.restype = i
    L.pv_harmonizer_create.argtypes = [ctypes.POINTER(pv_config), ctypes.POINTER(ctypes.c_float), i,
                                       ctypes.POINTER(vp)]
    L.pv_harmonizer_create.restype = i
    L.pv_harmonizer_destroy.argtypes = [vp]
    L.pv_harmonizer_destroy.restype = None
    L.pv_harmonize.argtypes = [vp, vp, ll, ll, i, i, vp, ll, vp, ll, ll, ctypes.POINTER(ctypes.c_float),
                               vp, ll, vp]
    L.pv_harmonize.restype = i
    L.pv_harmonizer_set_formant.argtypes = [vp, i]
    L.pv_harmonizer_set_formant.restype = i
    L.pv_resampler_create.argtypes = [i, i, i, i, ctypes.POINTER(vp)]
    L.pv_resampler_create.restype = i
    L.pv_resampler_destroy.argtypes = [vp]
    L.pv_resampler_destroy.restype = None
    L.pv_resample_length.argtypes = [vp, ll]
    L.pv_resample_length.restype = ll
    L.pv_resample.argtypes = [vp, vp, ll, ll, i, vp, ll, vp]
    L.pv_resample.restype = i
    L.pv_pitch_reserve.argtypes = [vp, i]
    L.pv_pitch_reserve.restype = i
    L.pv_pitch_output_length.argtypes = [vp, i]
    L.pv_pitch_output_length.restype = ll
    L.pv_pitch_process.argtypes = [vp, vp, ll, ll, i, i, vp, ll, vp, ll, vp]
    L.pv_pitch_process.restype = i
    L.pv_pitch_set_formant.argtypes = [vp, i]
    L.pv_pitch_set_formant.restype = i
    L.pv_pitch_get_formant.argtypes = [vp]
    L.pv_pitch_get_formant.restype = i
    L.pv_transient_reserve.argtypes = [vp]
    L.pv_transient_reserve.restype = i
    L.pv_set_transient.argtypes = [vp, i, f]
    L.pv_set_transient.restype = i
    L.pv_get_transient.argtypes = [vp]
    L.pv_get_transient.restype = i
    L.pv_transient_set_flags.argtypes = [vp, vp, ll, i, i, vp]
    L.pv_transient_set_flags.restype = i
    L.pv_transient_get_flags.argtypes = [vp, vp, ll, i, i, vp]
    L.pv_transient_get_flags.restype = i
    L.pv_onset_strength.argtypes = [vp, vp, ll, i, i, vp, ll, vp]
    L.pv_onset_strength.restype = i
    L.pv_timemap_split.argtypes = [vp, i, vp, vp]
    L.pv_timemap_split.restype = i
    L.pv_timemap_set.argtypes = [vp, vp, i]
    L.pv_timemap_set.restype = i
    L.pv_timemap_frames.argtypes = [vp]
    L.pv_timemap_frames.restype = i
    L.pv_timemap_set_channels.argtypes = [vp, vp, ll, vp, i, i]
    L.pv_timemap_set_channels.restype = i
    L.pv_timemap_channels.argtypes = [vp]
    L.pv_timemap_channels.restype = i
    L.pv_timemap_process.argtypes = [vp, vp, ll, ll, i, i, vp, ll, vp, ll, vp]
    L.pv_timemap_process.restype = i
    L.pv_varresampler_create.argtypes = [i, i, i, i, ctypes.POINTER(vp)]
    L.pv_varresampler_create.restype = i
    L.pv_varresampler_destroy.argtypes = [vp]
    L.pv_varresampler_destroy.restype = None
    L.pv_varresample_steps.argtypes = [vp, i, vp]
    L.pv_varresample_steps.restype = i
    L.pv_varresampler_set_map.argtypes = [vp, ll, vp, i]
    L.pv_varresampler_set_map.restype = i
    L.pv_varresampler_set_maps.argtypes = [vp, i, vp, vp, ll, i]
    L.pv_varresampler_set_maps.restype = i
    L.pv_varresample_map_channels.argtypes = [vp]
    L.pv_varresample_map_channels.restype = i
    L.pv_varresample_length.argtypes = [vp]
    L.pv_varresample_length.restype = ll
    L.pv_varresample.argtypes = [vp, vp, ll, ll, i, vp, ll, ll, vp]
    L.pv_varresample.restype = i
    L.pv_pitchmap_plan.argtypes = [i, i, vp, vp, i, vp, i, ctypes.POINTER(i), vp, i, ctypes.POINTER(i)]
    L.pv_pitchmap_plan.restype = i
    L.pv_pitchmap_set.argtypes = [vp, vp, vp, i, i]
    L.pv_pitchmap_set.restype = i
    L.pv_pitchmap_set_channels.argtypes = [vp, vp, ll, vp, ll, i, i, i]
    L.pv_pitchmap_set_channels.restype = i
    L.pv_pitchmap_output_length.argtypes = [vp]
    L.pv_pitchmap_output_length.restype = ll
    L.pv_pitchmap_process.argtypes = [vp, vp, ll, ll, i, i, vp, ll, vp, ll, vp]
    L.pv_pitchmap_process.restype = i
    L.pv_pitch_track.argtypes = [vp, vp, ll, i, i, i, i, f, vp, ll, vp]
    L.pv_pitch_track.restype = i
    L.pv_pitch_correct_plan.argtypes = [vp, i, vp, i, ctypes.POINTER(pv_pitch_correct), vp]
    L.pv_pitch_correct_plan.restype = i
    _lib = L
    return L


def check(status: int, what: str = "pv call"):
    if status != PV_OK:
        L = lib()
        raise PVError(status, f"{what}: {L.pv_status_string(status).decode()}: "
                              f"{L.pv_last_error().decode()}")


def frame_count(n_samples: int, hop: int) -> int:
    return lib().pv_frame_count(int(n_samples), int(hop))


def diagnostic_build() -> bool:
    """True when the loaded libpv was built with PV_DIAGNOSTIC_BUILD (timing-only ablations
    or instrumentation: not the product)."""
    L = lib()
    return bool(L.pv_diagnostic_build()) if hasattr(L, "pv_diagnostic_build") else False
