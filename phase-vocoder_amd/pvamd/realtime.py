"""Real-time ring-buffer mode over libpv's pv_rt_* (include/pv.h), BASELINE config 5.

The reference sketches this path only: an RtAudio `callback` (src/main.cpp:45-59) copies
each input buffer into `PhaseVocoder::curr_input` and runs a per-callback `analysis()`
that looks back at `prev_input` / `prev_mag_phase` / `prev_output`
(src/phaseVocoder.h:16-31, README.md:46-50).  `RealTimeVocoder` keeps that shape: state
lives on the device between callbacks, one callback is one hipGraph replay
(`capture` + `callback`), or one `push` on a caller's stream.

A time-stretch vocoder can also shift the pitch live: `set_phase_lock` turns identity phase
locking on, `reserve_pitch` adds the streaming resampler, and `pitch_push` (or the captured
callback) then takes nframes*hopSize samples and gives nframes*hopSize shifted ones,
`pitch_latency` output samples late.

A vocoder at scale 1 can follow a pitch ratio that changes from frame to frame:
`reserve_pitch_map` sets the preset and the ratio range, `pitch_map_push` (or the captured
callback, `callback(x, ratios)`) takes one ratio per channel and frame beside the samples, and
the stream comes out `pitch_map_latency` samples late.

The same vocoder can play a chord under its input: `reserve_harmonizer` sets the number of voices,
`harmonize_push` (or the captured callback, `callback(x, ratios, gains)`) takes one ratio and one
gain per channel, voice and frame and gives the gain-weighted mix of the voices (and each voice on
its own when asked), `harmonizer_latency` samples late.  `interval_ratios` turns semitones into
ratios.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .vocoder import PITCH_SHIFT, TIME_SHIFT, _ptr, _torch  # noqa: F401


def interval_ratios(semitones) -> np.ndarray:
    """fp32 pitch ratios 2^(s/12) of intervals in semitones (a scalar or an array)"""
    return np.exp2(np.asarray(semitones, dtype=np.float64) / 12.0).astype(np.float32)


class RealTimeVocoder:
    def __init__(self, samples: int, effect: str = PITCH_SHIFT, scaleFactor: float = 1.0,
                 hop: int = 4, *, channels: int = 1, device: int = 0, phase_lock: bool = False):
        eff = effect if isinstance(effect, int) else ord(effect)
        cfg = _lib.config(samples, hop, eff, scaleFactor, _lib.PV_MODE_STANDARD, channels, 1, device)
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.pv_rt_create(ctypes.byref(cfg), int(channels), ctypes.byref(h)), "pv_rt_create")
        self._h = h
        self.device = int(device)
        self.channels = int(channels)
        self.nSamps = int(samples)
        self.hopSize = int(samples) // int(hop)
        self.outHopSize = int(float(scaleFactor) * self.hopSize) if chr(eff) == TIME_SHIFT else self.hopSize
        self.spec_bins = self.nSamps // 2 + 1
        self.spec_stride = (self.spec_bins + 7) & ~7
        self._graph_frames = 0
        self._pitch = False
        self.host_ratios = None
        self.host_gains = None
        if phase_lock:
            self.set_phase_lock(True)

    def close(self):
        if getattr(self, "_h", None):
            self._L.pv_rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream=None):
        if stream is not None:
            return ctypes.c_void_p(int(stream))
        torch = _torch()
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, stream=None):
        _lib.check(self._L.pv_rt_reset(self._h, self._stream(stream)), "pv_rt_reset")

    def push(self, x, out=None, spec=None, stream=None):
        """x: [C, nframes*hop] CUDA float32 -> out [C, nframes*outHop] (device, async)."""
        torch = _torch()
        x = x.unsqueeze(0) if x.dim() == 1 else x
        C, n = x.shape
        assert C == self.channels and n % self.hopSize == 0 and x.stride(-1) == 1
        nf = n // self.hopSize
        if out is None:
            out = torch.empty((C, nf * self.outHopSize), dtype=torch.float32, device=x.device)
        lds = 0 if spec is None else spec.stride(0) // 2
        _lib.check(self._L.pv_rt_push(self._h, _ptr(x), x.stride(0), nf, _ptr(out), out.stride(0),
                                      _ptr(spec), lds, self._stream(stream)), "pv_rt_push")
        return out

    # ---------------------------------------------------------- locked stretch, pitch shift
    def set_phase_lock(self, lock: bool = True):
        """pv_rt_set_phase_lock: identity phase locking of the time stretch (time-stretch
        vocoders only; before `capture`)."""
        _lib.check(self._L.pv_rt_set_phase_lock(self._h, 1 if lock else 0), "pv_rt_set_phase_lock")

    @property
    def phase_lock(self) -> bool:
        return bool(self._L.pv_rt_get_phase_lock(self._h))

    def reserve_pitch(self, quality: int = 0, max_frames: int = 1):
        """pv_rt_pitch_reserve: the streaming resampler of `pitch_push` (quality 0 fast, 1 best)
        for pushes of up to max_frames frames; time-stretch vocoders only, before `capture`."""
        _lib.check(self._L.pv_rt_pitch_reserve(self._h, int(quality), int(max_frames)), "pv_rt_pitch_reserve")
        self._pitch = True

    @property
    def pitch_latency(self) -> int:
        """output samples by which `pitch_push`'s stream is delayed (0 before `reserve_pitch`)"""
        return int(self._L.pv_rt_pitch_latency(self._h))

    def pitch_push(self, x, out=None, spec=None, stream=None):
        """x: [C, nframes*hop] CUDA float32 -> out [C, nframes*hop], shifted in pitch by
        outHop / hop (device, async)."""
        torch = _torch()
        x = x.unsqueeze(0) if x.dim() == 1 else x
        C, n = x.shape
        assert C == self.channels and n % self.hopSize == 0 and x.stride(-1) == 1
        nf = n // self.hopSize
        if out is None:
            out = torch.empty((C, n), dtype=torch.float32, device=x.device)
        lds = 0 if spec is None else spec.stride(0) // 2
        _lib.check(self._L.pv_rt_pitch_push(self._h, _ptr(x), x.stride(0), nf, _ptr(out), out.stride(0),
                                            _ptr(spec), lds, self._stream(stream)), "pv_rt_pitch_push")
        return out

    # ---------------------------------------------------------- pitch map
    def reserve_pitch_map(self, quality: int = 0, max_frames: int = 1, *, ratio_min: float = 0.5,
                          ratio_max: float = 2.0):
        """pv_rt_pitchmap_reserve: the state of `pitch_map_push` for pushes of up to max_frames
        frames and pitch ratios in [ratio_min, ratio_max] (inside [1/4, 4]; a ratio outside the
        range is clamped to it).  The range sets the latency.  Scale-1 time-stretch vocoders only,
        before `capture`."""
        _lib.check(self._L.pv_rt_pitchmap_reserve(self._h, int(quality), int(max_frames), float(ratio_min),
                                                  float(ratio_max)), "pv_rt_pitchmap_reserve")
        self._pitch = True

    @property
    def pitch_map_latency(self) -> int:
        """output samples by which `pitch_map_push`'s stream is delayed (0 before `reserve_pitch_map`)"""
        return int(self._L.pv_rt_pitchmap_latency(self._h))

    def pitch_map_push(self, x, ratios=None, out=None, spec=None, stream=None):
        """x: [C, nframes*hop] CUDA float32, ratios: [C, nframes] CUDA float32 (None: 1) -> out
        [C, nframes*hop]: the stream shifted in pitch by each frame's ratio (device, async)."""
        torch = _torch()
        x = x.unsqueeze(0) if x.dim() == 1 else x
        C, n = x.shape
        assert C == self.channels and n % self.hopSize == 0 and x.stride(-1) == 1
        nf = n // self.hopSize
        ldr = 0
        if ratios is not None:
            ratios = ratios.unsqueeze(0) if ratios.dim() == 1 else ratios
            assert ratios.shape == (C, nf) and ratios.dtype == torch.float32 and ratios.stride(-1) == 1
            ldr = ratios.stride(0)
        if out is None:
            out = torch.empty((C, n), dtype=torch.float32, device=x.device)
        lds = 0 if spec is None else spec.stride(0) // 2
        _lib.check(self._L.pv_rt_pitchmap_push(self._h, _ptr(x), x.stride(0), nf, _ptr(ratios), ldr, _ptr(out),
                                               out.stride(0), _ptr(spec), lds, self._stream(stream)),
                   "pv_rt_pitchmap_push")
        return out

    # ---------------------------------------------------------- harmoniser
    def reserve_harmonizer(self, voices: int, quality: int = 0, max_frames: int = 1, *, ratio_min: float = 0.5,
                           ratio_max: float = 2.0):
        """pv_rt_harmonizer_reserve: the state of `harmonize_push` for `voices` voices per channel
        (at most pv_rt_harmonizer_max_voices: 8, or 4 at 2048 samples), pushes of up to max_frames
        frames and pitch ratios in [ratio_min, ratio_max] (as `reserve_pitch_map`).  Scale-1
        time-stretch vocoders only, before `capture`."""
        _lib.check(self._L.pv_rt_harmonizer_reserve(self._h, int(voices), int(quality), int(max_frames),
                                                    float(ratio_min), float(ratio_max)), "pv_rt_harmonizer_reserve")
        self._pitch = True

    @property
    def harmonizer_voices(self) -> int:
        """voices per channel of `harmonize_push` (0 before `reserve_harmonizer`)"""
        return int(self._L.pv_rt_harmonizer_voices(self._h))

    @property
    def harmonizer_latency(self) -> int:
        """output samples by which `harmonize_push`'s streams are delayed (0 before `reserve_harmonizer`)"""
        return int(self._L.pv_rt_harmonizer_latency(self._h))

    def harmonize_push(self, x, ratios=None, gains=None, out=None, voices=False, spec=None, stream=None):
        """x: [C, nframes*hop] CUDA float32, ratios and gains: [C, V, nframes] CUDA float32 (None: 1,
        and 1/V) -> mix [C, nframes*hop], the gain-weighted sum of the V voices, each the stream
        shifted in pitch by its frames' ratios; with voices=True (or a [V, C, nframes*hop] tensor
        to write) -> (mix, voices [V, C, nframes*hop]) (device, async)."""
        torch = _torch()
        x = x.unsqueeze(0) if x.dim() == 1 else x
        C, n = x.shape
        assert C == self.channels and n % self.hopSize == 0 and x.stride(-1) == 1
        nf = n // self.hopSize
        V = self.harmonizer_voices
        ld_ctl = nf
        for t in (ratios, gains):
            if t is not None:
                assert t.shape == (C, V, nf) and t.dtype == torch.float32 and t.is_contiguous()
        if out is None:
            out = torch.empty((C, n), dtype=torch.float32, device=x.device)
        vo = None
        if voices is True:
            vo = torch.empty((max(V, 1), C, n), dtype=torch.float32, device=x.device)
        elif voices is not False and voices is not None:
            vo = voices
            assert vo.shape == (V, C, n) and vo.dtype == torch.float32 and vo.stride(-1) == 1
            assert vo.stride(0) == C * vo.stride(1)
        lds = 0 if spec is None else spec.stride(0) // 2
        _lib.check(self._L.pv_rt_harmonizer_push(self._h, _ptr(x), x.stride(0), nf, _ptr(ratios), _ptr(gains), ld_ctl,
                                                 _ptr(out), out.stride(0), _ptr(vo), 0 if vo is None else vo.stride(1),
                                                 _ptr(spec), lds, self._stream(stream)), "pv_rt_harmonizer_push")
        return out if vo is None else (out, vo)

    # ---------------------------------------------------------- captured callback
    def capture(self, nframes: int = 1):
        _lib.check(self._L.pv_rt_capture(self._h, int(nframes)), "pv_rt_capture")
        self._graph_frames = int(nframes)
        fi = ctypes.POINTER(ctypes.c_float)()
        fo = ctypes.POINTER(ctypes.c_float)()
        _lib.check(self._L.pv_rt_host_buffers(self._h, ctypes.byref(fi), ctypes.byref(fo)),
                   "pv_rt_host_buffers")
        # (after reserve_pitch the callback is pitch_push: nframes * hop samples out)
        ni, no = nframes * self.hopSize, nframes * (self.hopSize if self._pitch else self.outHopSize)
        # zero-copy numpy views of the pinned callback buffers
        self.host_in = np.ctypeslib.as_array(fi, shape=(self.channels, ni))
        self.host_out = np.ctypeslib.as_array(fo, shape=(self.channels, no))
        # after reserve_pitch_map: the pinned ratios the callback reads, [C, nframes], all 1
        self.host_ratios = None
        fr = ctypes.POINTER(ctypes.c_float)()
        if self._L.pv_rt_pitchmap_host_ratios(self._h, ctypes.byref(fr)) == _lib.PV_OK:
            self.host_ratios = np.ctypeslib.as_array(fr, shape=(self.channels, nframes))
        # after reserve_harmonizer: the pinned ratios and gains, [C, V, nframes], all 1 and all 1/V
        self.host_gains = None
        fg = ctypes.POINTER(ctypes.c_float)()
        if self._L.pv_rt_harmonizer_host_controls(self._h, ctypes.byref(fr), ctypes.byref(fg)) == _lib.PV_OK:
            shape = (self.channels, self.harmonizer_voices, nframes)
            self.host_ratios = np.ctypeslib.as_array(fr, shape=shape)
            self.host_gains = np.ctypeslib.as_array(fg, shape=shape)

    def callback(self, x: np.ndarray | None = None, ratios: np.ndarray | None = None,
                 gains: np.ndarray | None = None) -> np.ndarray:
        """One synchronous callback: x (host [C, nframes*hop], or None when host_in was
        filled in place) -> host_out view [C, nframes*outHop] ([C, nframes*hop] after
        `reserve_pitch`, `reserve_pitch_map` or `reserve_harmonizer`, whose callback gives the mix).
        ratios (host [C, nframes] after `reserve_pitch_map`, [C, V, nframes] after
        `reserve_harmonizer`): written into host_ratios, which keeps them for the callbacks after;
        gains (host [C, V, nframes], after `reserve_harmonizer`): into host_gains likewise."""
        if ratios is not None:
            if self.host_ratios is None:
                raise _lib.PVError(_lib.PV_ERR_ARG, "callback(ratios=...): the captured callback is not pitch_map_push "
                                                    "or harmonize_push")
            self.host_ratios[...] = np.asarray(ratios, dtype=np.float32).reshape(self.host_ratios.shape)
        if gains is not None:
            if self.host_gains is None:
                raise _lib.PVError(_lib.PV_ERR_ARG, "callback(gains=...): the captured callback is not harmonize_push")
            self.host_gains[...] = np.asarray(gains, dtype=np.float32).reshape(self.host_gains.shape)
        src = None
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            src = x.ctypes.data_as(ctypes.c_void_p)
        _lib.check(self._L.pv_rt_callback(self._h, src, None), "pv_rt_callback")
        return self.host_out
