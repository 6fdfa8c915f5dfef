"""Python mirror of the reference's `PhaseVocoder` / `CudaPhase` surface over libpv.

Same names, argument meaning and (optionally) the print-and-exit error behaviour of the
reference, so parity tests read like src/main.cpp:
  PhaseVocoder(samples, effect, scaleFactor, hop)      src/phaseVocoder.h:79-116
  .nSamps .hopSize .outHopSize .timeScale .imp          src/phaseVocoder.h:16-31
  .analysis_CUFFT(input, output, fft, intermediary)     src/phaseVocoder.cpp:25-33
  .resynthesis_CUFFT(backFrame, frontFrame, output)     src/phaseVocoder.cpp:60-76
plus the batched entry points the MI355X design is built around (analysis / resynthesis /
process over channels x frames).  Tensors are torch CUDA tensors (device memory and the
current stream are the only things torch provides here).
"""
from __future__ import annotations

import ctypes
import sys

import numpy as np

from . import _lib
from ._lib import PV_MODE_REF_COMPAT, PV_MODE_STANDARD, PVError

TIME_SHIFT = "t"  # phaseVocoder.h:6
PITCH_SHIFT = "p"  # phaseVocoder.h:7
REF_COMPAT = "ref_compat"
STANDARD = "standard"


def _torch():
    import torch  # plumbing only: device memory + streams

    return torch


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def rate_map(frames: int, rate: float) -> np.ndarray:
    """The time map of a constant playback rate over `frames` analysed frames: positions 0, rate,
    2 rate, .. up to frames - 1 (float64), for `PhaseVocoder.set_time_map`.  rate < 1 stretches."""
    return np.arange(0, frames - 1 + 1e-9, rate).astype(np.float64)


def timemap_split(pos):
    """pv_timemap_split (pure host, no GPU): positions -> (floor as int32, fraction as float32).
    Raises PVError on a position that is not finite, negative or >= 2^30."""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1)
    idx = np.empty(pos.size, dtype=np.int32)
    frac = np.empty(pos.size, dtype=np.float32)
    vp = ctypes.c_void_p
    _lib.check(_lib.lib().pv_timemap_split(pos.ctypes.data_as(vp), int(pos.size), idx.ctypes.data_as(vp),
                                           frac.ctypes.data_as(vp)), "pv_timemap_split")
    return idx, frac


CHROMATIC = 0xFFF  # every pitch class (bit i: class i, 0 = C)
MAJOR = 0xAB5      # C D E F G A B


def pitch_correction(track, a4: float, scale=CHROMATIC, strength_min: float = 0.5, retune: float = 1.0,
                     pos=None) -> np.ndarray:
    """pv_pitch_correct_plan (pure host, no GPU): the {f0, strength} track of one voice
    ([frames, 2], numpy or a tensor, `PhaseVocoder.pitch_track`'s row) -> the pitch ratios
    (float64) that snap it to the scale, one per output frame, for `PhaseVocoder.set_pitch_map`.
    A [channels, frames, 2] track (`pitch_track`'s whole result) gives [channels, n] ratios, one
    plan per row, for `set_pitch_map`'s 2-D form; pos is then one row for all voices or one per voice.
    a4: the frequency of A4 in cycles per sample (440 / sample rate); scale: a 12-bit mask (bit i
    = pitch class i is allowed, 0 = C; `MAJOR`, `CHROMATIC`) or an iterable of pitch classes;
    frames with a strength below strength_min hold the last correction; retune in (0, 1]: 1 snaps
    at once, less glides there; pos: the analysis position of every output frame (None: frame u
    for output u)."""
    if hasattr(track, "detach"):
        track = track.detach().cpu().numpy()
    tr = np.ascontiguousarray(track, dtype=np.float32)
    if tr.ndim == 3 and tr.shape[2] == 2:
        if pos is not None:
            pos = np.asarray(pos, dtype=np.float64)
            if pos.ndim == 2 and pos.shape[0] != tr.shape[0]:
                raise ValueError("pos must be one row for all voices or one per voice")
        rows = [pitch_correction(tr[c], a4, scale, strength_min, retune,
                                 None if pos is None else (pos[c] if pos.ndim == 2 else pos))
                for c in range(tr.shape[0])]
        return np.stack(rows) if rows else np.empty((0, 0), dtype=np.float64)
    if tr.ndim != 2 or tr.shape[1] != 2:
        raise ValueError("track must be [frames, 2]: one voice's {f0, strength}, or [channels, frames, 2]")
    if isinstance(scale, (int, np.integer)):
        mask = int(scale)
    else:
        mask = 0
        for pc in scale:
            if not 0 <= int(pc) < 12:
                raise ValueError("a pitch class must be in 0 .. 11 (0 = C)")
            mask |= 1 << int(pc)
    if not 0 <= mask < 2 ** 32:
        raise ValueError("scale mask out of range")
    vp = ctypes.c_void_p
    if pos is None:
        n, pp = tr.shape[0], None
    else:
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1)
        n, pp = int(pos.size), pos.ctypes.data_as(vp)
    cfg = _lib.pv_pitch_correct(_lib.ABI_VERSION, float(a4), mask, float(strength_min), float(retune))
    ratio = np.empty(max(n, 1), dtype=np.float64)
    _lib.check(_lib.lib().pv_pitch_correct_plan(tr.ctypes.data_as(vp), int(tr.shape[0]), pp, n, ctypes.byref(cfg),
                                                ratio.ctypes.data_as(vp)), "pv_pitch_correct_plan")
    return ratio[:n]


class PhaseVocoder:
    """`class PhaseVocoder` (src/phaseVocoder.h:9-139) on the MI355X HIP path."""

    def __init__(self, samples: int, effect: str = TIME_SHIFT, scaleFactor: float = 1.0,
                 hop: int = 2, *, mode: str = REF_COMPAT, max_channels: int = 1,
                 max_frames: int = 4096, device: int = 0, exit_on_error: bool = False,
                 window: int = _lib.PV_WINDOW_DEFAULT, nan_faithful: bool = False,
                 spec_layout: int = _lib.PV_SPEC_NATURAL, tables_external: bool = False,
                 phase_lock: bool = False, formant: int = 0, pitch_formant: int = 0,
                 transients: str = "off", transient_threshold: float = 0.0):
        """window: PV_WINDOW_DEFAULT (the mode's), PV_WINDOW_HAMMING_REF or
        PV_WINDOW_HANN_REF (the 1-argument constructor's, phaseVocoder.h:64-66; see
        `single_arg`); nan_faithful: REF_COMPAT atanf(0/0) = NaN (kernel.cu:101-109);
        spec_layout: PV_SPEC_NATURAL or PV_SPEC_PACKED (STANDARD: bin N/2 folded into slot 0,
        see `unpack_spec`); tables_external: build no tables — `import_tables` (or
        pvamd.dist.broadcast_tables) must load them before any compute call; phase_lock:
        identity phase locking (STANDARD time stretch only, see `set_phase_lock`); formant:
        lifter order of the formant-preserving pitch shift (STANDARD pitch shift only, see
        `set_formant`; 0 = off); pitch_formant: lifter order of the formant preservation of
        `pitch_process` (STANDARD time stretch only, see `set_pitch_formant`; 0 = off);
        transients / transient_threshold: the transient phase reset (STANDARD time stretch only,
        see `set_transients`)."""
        self.exit_on_error = exit_on_error
        eff = effect if isinstance(effect, int) else ord(effect)
        m = PV_MODE_REF_COMPAT if mode == REF_COMPAT else PV_MODE_STANDARD
        cfg = _lib.config(samples, hop, eff, scaleFactor, m, max_channels, max_frames, device, window,
                          1 if nan_faithful else 0, spec_layout, 1 if tables_external else 0)
        self.window = int(window)
        h = ctypes.c_void_p()
        self._L = _lib.lib()
        self._call(self._L.pv_create(ctypes.byref(cfg), ctypes.byref(h)), "pv_create")
        self._h = h
        info = self._read_info()
        self.device = int(device)
        self.mode = mode
        self.effect = chr(eff)
        # field names of phaseVocoder.h
        self.nSamps = info.n_samps
        self.N = info.n_samps
        self.hopSize = info.hop
        self.outHopSize = info.out_hop
        self.timeScale = float(scaleFactor) if self.effect == TIME_SHIFT else 1.0
        self.spec_bins = info.spec_bins
        self.spec_stride = info.spec_stride
        self.frames_per_run = info.frames_per_run
        self.lane_constants = info.lane_constants
        self.spec_layout = info.spec_layout
        # channels from which process(spec=None) takes the channel-resident launch (0: never)
        self.resident_min_channels = int(self._L.pv_resident_min_channels(self._h))
        if phase_lock:
            self.set_phase_lock(True)
        if formant:
            self.set_formant(formant)
        if pitch_formant:
            self.set_pitch_formant(pitch_formant)
        if transients != "off":
            self.set_transients(transients, transient_threshold)

    def _read_info(self):
        info = _lib.new_info()
        self._call(self._L.pv_get_info(self._h, ctypes.byref(info)), "pv_get_info")
        self.info = info
        # 0 split path, 1 single q = 1 launch (pv_fused.hip)
        self.single_launch = info.single_launch
        self.single_launch_frames = info.single_launch_frames
        return info

    def set_phase_lock(self, lock: bool = True):
        """pv_set_phase_lock: identity phase locking of the STANDARD time stretch — every bin
        takes the phase advance of the nearest magnitude peak of its frame, which keeps the
        bins of one partial coherent (no "phasiness").  Applies to the calls made after it;
        a single-launch handle runs the split path while locking is on."""
        self._call(self._L.pv_set_phase_lock(self._h, 1 if lock else 0), "pv_set_phase_lock")
        self._read_info()

    @property
    def phase_lock(self) -> bool:
        return bool(self._L.pv_get_phase_lock(self._h))

    _TRANSIENT_MODES = {"off": _lib.PV_TRANSIENT_OFF, "flags": _lib.PV_TRANSIENT_FLAGS,
                        "detect": _lib.PV_TRANSIENT_DETECT}

    def set_transients(self, mode: str = "detect", threshold: float = 0.0):
        """pv_set_transient: the transient phase reset of the STANDARD time stretch — a flagged
        frame is put down with its analysis phases (an attack keeps its shape instead of
        smearing over a window) and the frames after it keep the offset that made it so.
        "off"; "flags": the frames given to `set_transient_flags`; "detect": the frames the
        onset detector flags in every `process` call (threshold in (0, 1), 0 = the default).
        Composes with `set_phase_lock`.  Applies to the calls made after it (`process`,
        `pitch_process`); a single-launch handle runs the split path while it is on."""
        if mode not in self._TRANSIENT_MODES:
            raise ValueError(f"transients must be one of {sorted(self._TRANSIENT_MODES)}")
        self._call(self._L.pv_set_transient(self._h, self._TRANSIENT_MODES[mode], float(threshold)),
                   "pv_set_transient")
        self._read_info()

    @property
    def transients(self) -> str:
        m = int(self._L.pv_get_transient(self._h))
        return {v: k for k, v in self._TRANSIENT_MODES.items()}[m]

    def reserve_transients(self):
        """pv_transient_reserve: allocate (once, zeroed) the handle's flags, onset strengths and
        reset offsets, so that the calls that use them can be captured into a graph."""
        self._call(self._L.pv_transient_reserve(self._h), "pv_transient_reserve")

    def set_transient_flags(self, flags, stream=None):
        """pv_transient_set_flags: flags [C, frames] (or [frames]), nonzero = the frame is a
        transient (any CUDA tensor; compared with 0).  Frame 0 is never flagged."""
        torch = _torch()
        f = self._as2d(flags)
        f = (f != 0).to(torch.uint8).contiguous()
        self._call(self._L.pv_transient_set_flags(self._h, _ptr(f), f.stride(0), f.shape[0], f.shape[1],
                                                  self._stream(stream)), "pv_transient_set_flags")

    def transient_flags(self, channels: int, frames: int, stream=None):
        """pv_transient_get_flags: the handle's flags [channels, frames] uint8 — the caller's, or
        in "detect" mode those of the last `process` call."""
        torch = _torch()
        f = torch.zeros((channels, frames), dtype=torch.uint8, device=f"cuda:{self.device}")
        self._call(self._L.pv_transient_get_flags(self._h, _ptr(f), f.stride(0), channels, frames,
                                                  self._stream(stream)), "pv_transient_get_flags")
        return f

    def onset_strength(self, spec, frames: int | None = None, stream=None):
        """pv_onset_strength: spec [C, frames, spec_stride, 2] of a STANDARD handle -> [C, frames,
        2] float32 {rise, tot}: the summed positive magnitude increments of every frame over the
        frame before it, and the frame's summed magnitudes."""
        torch = _torch()
        C = spec.shape[0]
        frames = spec.shape[1] if frames is None else frames
        dst = torch.zeros((C, frames, 2), dtype=torch.float32, device=spec.device)
        self._call(self._L.pv_onset_strength(self._h, _ptr(spec), spec.stride(0) // 2, C, frames, _ptr(dst),
                                             dst.stride(0) // 2, self._stream(stream)), "pv_onset_strength")
        return dst

    def set_formant(self, order: int):
        """pv_set_formant: formant-preserving STANDARD pitch shift — the frame's cepstral
        envelope (quefrencies up to `order`, 1 .. N/4) is divided out of the source bins and put
        back at the target bins, so the formants stay where the input has them.  0 turns it
        off.  Applies to the calls made after it; the first call allocates the handle's
        envelope rows, and a single-launch handle runs the split path while it is on."""
        self._call(self._L.pv_set_formant(self._h, int(order)), "pv_set_formant")
        self._read_info()

    @property
    def formant(self) -> int:
        return int(self._L.pv_get_formant(self._h))

    def spectral_envelope(self, spec, order: int, frames: int | None = None, stream=None):
        """pv_spectral_envelope: spec [C, frames, spec_stride, 2] of a STANDARD handle -> the
        frames' log envelopes le [C, frames, N/2 + 1] float32 (natural log of the magnitude
        envelope; a view of rows padded to N/2 + 8)."""
        torch = _torch()
        C = spec.shape[0]
        frames = spec.shape[1] if frames is None else frames
        B = self.nSamps // 2 + 1
        env = torch.zeros((C, frames, B + 7), dtype=torch.float32, device=spec.device)
        self._call(self._L.pv_spectral_envelope(self._h, _ptr(spec), spec.stride(0) // 2, C, frames,
                                                int(order), _ptr(env), env.stride(0), self._stream(stream)),
                   "pv_spectral_envelope")
        return env[..., :B]

    @classmethod
    def single_arg(cls, samples: int, **kw):
        """`PhaseVocoder(int samples)` (src/phaseVocoder.h:46-78): hop = samples/2,
        timeScale 1, periodic Hann window 0.5f*(1 - cosf(2 pi i/N))."""
        return cls(samples, TIME_SHIFT, 1.0, 2, mode=REF_COMPAT,
                   window=_lib.PV_WINDOW_HANN_REF, **kw)

    def set_window(self, win, stream=None):
        """REF_COMPAT: use the caller's window (CUDA float32 tensor of nSamps) for the
        analysis and the resynthesis, as CudaPhase::*_CUFFT's `win` (kernel.cu:301, :406)."""
        assert win.is_cuda and win.numel() == self.nSamps and win.is_contiguous()
        self._call(self._L.pv_set_window(self._h, _ptr(win), self._stream(stream)), "pv_set_window")

    # -------------------------------------------------------------- plumbing
    def _call(self, status, what):
        if status != _lib.PV_OK:
            if self.exit_on_error:  # the reference's checkCUDAError_ (io.cpp:115-124)
                L = _lib.lib()
                print(f"Cuda error: {what}: {L.pv_last_error().decode()}.", file=sys.stderr)
                sys.exit(1)
            _lib.check(status, what)

    def _stream(self, stream=None):
        if stream is not None:
            return ctypes.c_void_p(int(stream))
        torch = _torch()
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            self._L.pv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def imp(self) -> np.ndarray:
        """Analysis window (phaseVocoder.h:16 `imp`), host copy."""
        from .tables import analysis_window
        return analysis_window(self.nSamps, self.mode, self.window)

    # -------------------------------------------------------------- geometry
    def num_frames(self, n_samples: int) -> int:
        return _lib.frame_count(n_samples, self.hopSize)

    def output_length(self, frames: int) -> int:
        return int(self._L.pv_output_length(self._h, int(frames)))

    def alloc_spec(self, channels: int, frames: int):
        torch = _torch()
        return torch.zeros((channels, frames, self.spec_stride, 2), dtype=torch.float32,
                           device=f"cuda:{self.device}")

    def unpack_spec(self, spec):
        """Spectrum rows of this handle -> natural {mag, phase} bins 0 .. N/2, as a
        [..., N/2 + 1, 2] float32 tensor (a copy).  PV_SPEC_PACKED rows carry bins 0 and N/2
        in slot 0 as sign-coded magnitudes (include/pv.h pv_unpack_bins): exact."""
        torch = _torch()
        B = self.nSamps // 2 + 1
        if self.spec_layout != _lib.PV_SPEC_PACKED:
            return spec[..., :B, :].clone()
        L = self.nSamps // 2
        out = torch.empty(spec.shape[:-2] + (B, 2), dtype=spec.dtype, device=spec.device)
        out[..., 1:L, :] = spec[..., 1:L, :]
        s0 = spec[..., 0, :]
        pi = torch.tensor(float(np.float32(np.pi)), dtype=spec.dtype, device=spec.device)
        zero = torch.zeros((), dtype=spec.dtype, device=spec.device)
        for dst, src in ((0, s0[..., 0]), (L, s0[..., 1])):
            out[..., dst, 0] = src.abs()
            out[..., dst, 1] = torch.where(torch.signbit(src), pi, zero)
        return out

    def alloc_out(self, channels: int, frames: int):
        torch = _torch()
        return torch.empty((channels, self.output_length(frames)), dtype=torch.float32,
                           device=f"cuda:{self.device}")

    # -------------------------------------------------------------- batched API
    @staticmethod
    def _as2d(x):
        return x.unsqueeze(0) if x.dim() == 1 else x

    def analysis(self, x, frames: int | None = None, n_samples: int | None = None, spec=None,
                 stream=None):
        """x: [C, n] (or [n]) float32 CUDA -> spec [C, frames, spec_stride, 2]."""
        x = self._as2d(x)
        assert x.is_cuda and x.dtype.is_floating_point and x.stride(-1) == 1
        C, n = x.shape
        n_samples = n if n_samples is None else n_samples
        frames = self.num_frames(n_samples) if frames is None else frames
        if spec is None:
            spec = self.alloc_spec(C, frames)
        self._call(self._L.pv_analysis(self._h, _ptr(x), x.stride(0), n_samples, C, frames,
                                       _ptr(spec), spec.stride(0) // 2, self._stream(stream)),
                   "pv_analysis")
        return spec

    def resynthesis(self, spec, frames: int | None = None, out=None, ola_in=None, stream=None):
        """spec [C, frames, spec_stride, 2] -> out [C, frames*outHop + N - outHop]."""
        C = spec.shape[0]
        frames = spec.shape[1] if frames is None else frames
        if out is None:
            out = self.alloc_out(C, frames)
        ld_ola = 0 if ola_in is None else self._as2d(ola_in).stride(0)
        self._call(self._L.pv_resynthesis(self._h, _ptr(spec), spec.stride(0) // 2, C, frames,
                                          _ptr(ola_in), ld_ola, _ptr(out), out.stride(0),
                                          self._stream(stream)), "pv_resynthesis")
        return out

    # -------------------------------------------------------------- stream segments
    def segment_summary(self, spec, frames: int | None = None, stream=None):
        """pv_segment_summary: spec [C, frames, spec_stride, 2] of one segment of a longer
        stream -> summary [C, words] int32 (device)."""
        torch = _torch()
        C = spec.shape[0]
        frames = spec.shape[1] if frames is None else frames
        words = self._L.pv_segment_summary_words(self._h)
        summary = torch.empty((C, words), dtype=torch.int32, device=spec.device)
        self._call(self._L.pv_segment_summary(self._h, _ptr(spec), spec.stride(0) // 2, C, frames,
                                              _ptr(summary), self._stream(stream)), "pv_segment_summary")
        return summary

    def segment_resynthesis(self, spec, frame0: int, summaries=None, frames: int | None = None, out=None,
                            stream=None):
        """pv_segment_resynthesis: the segment starting at stream frame `frame0`, after the
        earlier segments' summaries [s, C, words] (None or empty for the first segment) ->
        its own overlap-add [C, frames*outHop + N - outHop]."""
        C = spec.shape[0]
        frames = spec.shape[1] if frames is None else frames
        if out is None:
            out = self.alloc_out(C, frames)
        seg = 0 if summaries is None else int(summaries.shape[0])
        if seg:
            assert summaries.is_contiguous() and summaries.dtype == _torch().int32
        self._call(self._L.pv_segment_resynthesis(self._h, _ptr(spec), spec.stride(0) // 2, C, frames,
                                                  int(frame0), _ptr(summaries) if seg else None, seg,
                                                  _ptr(out), out.stride(0), self._stream(stream)),
                   "pv_segment_resynthesis")
        return out

    def process(self, x, frames: int | None = None, n_samples: int | None = None, spec=None,
                out=None, stream=None, spectrum: bool = True):
        """analysis -> processing -> resynthesis; returns (out, spec).  spectrum=False: the
        caller gets no spectrum (spec is None) — the single launch keeps the rows on chip, the
        split path uses the handle's own buffer; for pitch > 1 the bins no output bin reads
        are then not analysed (same output bits)."""
        x = self._as2d(x)
        C, n = x.shape
        n_samples = n if n_samples is None else n_samples
        frames = self.num_frames(n_samples) if frames is None else frames
        if not spectrum and spec is not None:
            raise ValueError("spectrum=False with a spec buffer")
        if spectrum and spec is None:
            spec = self.alloc_spec(C, frames)
        if out is None:
            out = self.alloc_out(C, frames)
        self._call(self._L.pv_process(self._h, _ptr(x), x.stride(0), n_samples, C, frames,
                                      _ptr(spec) if spec is not None else None,
                                      spec.stride(0) // 2 if spec is not None else 0, _ptr(out),
                                      out.stride(0), self._stream(stream)), "pv_process")
        return out, spec

    # -------------------------------------------------------------- time-map stretch
    def set_time_map(self, positions, counts=None):
        """pv_timemap_set: output frame u of `time_map_process` is built at the fractional
        analysis position positions[u] (frames, float64; finite, >= 0; need not be monotonic:
        a freeze, a scrub and a reverse are maps; see `rate_map`).  One map for all channels;
        at most max_frames entries.  STANDARD time-stretch handles at scale 1.  None clears it.
        A 2-D [channels, n_out] array is a map per channel (pv_timemap_set_channels): channel c
        of `time_map_process` uses row c, of which counts[c] entries count (None: all n_out); its
        output past output_length(counts[c]) is zero."""
        if positions is None:
            self._call(self._L.pv_timemap_set(self._h, None, 0), "pv_timemap_set")
            return
        if np.ndim(positions) == 2:
            pos = np.ascontiguousarray(positions, dtype=np.float64)
            vp = ctypes.c_void_p
            cnt = None
            if counts is not None:
                cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
                if cnt.size != pos.shape[0]:
                    raise ValueError("counts must have one entry per channel")
            self._call(self._L.pv_timemap_set_channels(self._h, pos.ctypes.data_as(vp), int(pos.shape[1]),
                                                       None if cnt is None else cnt.ctypes.data_as(vp),
                                                       int(pos.shape[0]), int(pos.shape[1])), "pv_timemap_set_channels")
            return
        if counts is not None:
            raise ValueError("counts go with a [channels, n_out] map")
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        self._call(self._L.pv_timemap_set(self._h, pos.ctypes.data_as(ctypes.c_void_p), int(pos.size)),
                   "pv_timemap_set")

    @property
    def time_map_frames(self) -> int:
        return int(self._L.pv_timemap_frames(self._h))

    @property
    def time_map_channels(self) -> int:
        """pv_timemap_channels: the channels of a map per channel; 0 without a map or with the shared one"""
        return int(self._L.pv_timemap_channels(self._h))

    def time_map_process(self, x, frames: int | None = None, n_samples: int | None = None, spec=None,
                         out=None, stream=None, spectrum: bool = True):
        """pv_timemap_process: analysis of x's `frames` frames, then the handle's time map ->
        (out [C, output_length(time_map_frames)], spec), as `process` does (spectrum=False: the
        handle's own rows)."""
        x = self._as2d(x)
        C, n = x.shape
        n_samples = n if n_samples is None else n_samples
        frames = self.num_frames(n_samples) if frames is None else frames
        if not spectrum and spec is not None:
            raise ValueError("spectrum=False with a spec buffer")
        if spectrum and spec is None:
            spec = self.alloc_spec(C, frames)
        if out is None:
            out = self.alloc_out(C, self.time_map_frames)
        self._call(self._L.pv_timemap_process(self._h, _ptr(x), x.stride(0), n_samples, C, frames,
                                              _ptr(spec) if spec is not None else None,
                                              spec.stride(0) // 2 if spec is not None else 0, _ptr(out),
                                              out.stride(0), self._stream(stream)), "pv_timemap_process")
        return out, spec

    # -------------------------------------------------------------- pitch map
    def set_pitch_map(self, positions, ratios=None, quality: int = 0):
        """pv_pitchmap_set: final output frame u of `pitch_map_process` sounds at the analysis
        position positions[u] (the tempo curve, as `set_time_map`'s) with its pitch moved by
        ratios[u] (1/4 .. 4): a glide, a vibrato, a correction curve, tempo and pitch varying
        independently.  It installs the time map of the stretch (`time_map_frames` then reads its
        length) and the handle's variable-rate resampler (quality 0 fast, 1 best).  One map for
        all channels; a setup call.  positions=None clears it; so does a later `set_time_map`.
        2-D [channels, n] positions and ratios are a pitch map per channel
        (pv_pitchmap_set_channels): one plan per row, n final frames for every channel."""
        if positions is None:
            self._call(self._L.pv_pitchmap_set(self._h, None, None, 0, 0), "pv_pitchmap_set")
            return
        if np.ndim(positions) == 2 or np.ndim(ratios) == 2:
            pos = np.ascontiguousarray(positions, dtype=np.float64)
            rat = np.ascontiguousarray(ratios, dtype=np.float64)
            if pos.ndim != 2 or pos.shape != rat.shape:
                raise ValueError("positions and ratios must both be [channels, n]")
            vp = ctypes.c_void_p
            self._call(self._L.pv_pitchmap_set_channels(self._h, pos.ctypes.data_as(vp), int(pos.shape[1]),
                                                        rat.ctypes.data_as(vp), int(rat.shape[1]), int(pos.shape[0]),
                                                        int(pos.shape[1]), int(quality)), "pv_pitchmap_set_channels")
            return
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        rat = np.ascontiguousarray(ratios, dtype=np.float64).reshape(-1)
        if pos.size != rat.size:
            raise ValueError("positions and ratios must have one entry per output frame each")
        vp = ctypes.c_void_p
        self._call(self._L.pv_pitchmap_set(self._h, pos.ctypes.data_as(vp), rat.ctypes.data_as(vp), int(pos.size),
                                           int(quality)), "pv_pitchmap_set")

    @property
    def pitch_map_output_length(self) -> int:
        return int(self._L.pv_pitchmap_output_length(self._h))

    def pitch_map_process(self, x, frames: int | None = None, n_samples: int | None = None, spec=None,
                          out=None, stream=None, spectrum: bool = True):
        """pv_pitchmap_process: `time_map_process` with the pitch map's stretch map into the
        handle's scratch rows, then the variable-rate resampling -> (out [C,
        pitch_map_output_length], spec), as `process` does."""
        torch = _torch()
        x = self._as2d(x)
        C, n = x.shape
        n_samples = n if n_samples is None else n_samples
        frames = self.num_frames(n_samples) if frames is None else frames
        if not spectrum and spec is not None:
            raise ValueError("spectrum=False with a spec buffer")
        if spectrum and spec is None:
            spec = self.alloc_spec(C, frames)
        if out is None:
            out = torch.empty((C, self.pitch_map_output_length), dtype=torch.float32, device=f"cuda:{self.device}")
        self._call(self._L.pv_pitchmap_process(self._h, _ptr(x), x.stride(0), n_samples, C, frames,
                                               _ptr(spec) if spec is not None else None,
                                               spec.stride(0) // 2 if spec is not None else 0, _ptr(out),
                                               out.stride(0), self._stream(stream)), "pv_pitchmap_process")
        return out, spec

    # -------------------------------------------------------------- pitch tracker
    def pitch_track(self, spec, fmin: float | None = None, fmax: float | None = None, kappa: float = 0.0,
                    frames: int | None = None, stream=None, *, tau_min: int | None = None,
                    tau_max: int | None = None):
        """pv_pitch_track: spec [C, frames, spec_stride, 2] of a STANDARD handle -> [C, frames, 2]
        float32 {f0, strength}: the fundamental frequency of every frame in cycles per sample
        (0: none found) and the height of its autocorrelation peak (about 1 for a clean voice,
        below 0.5 for noise: the caller's to threshold; see `pitch_correction`).  The search
        range is fmin .. fmax in cycles per sample, as the lags ceil(1 / fmax) .. floor(1 / fmin),
        or the lags themselves (tau_min=, tau_max=); they must lie in [2, N/2 - 1], and periods
        up to N/4 are the recommended range.  kappa in (0, 1] (0: the default 0.9): how close to
        the highest peak an earlier one must come to be taken for the period."""
        torch = _torch()
        if tau_min is None:
            if fmax is None or not fmax > 0:
                raise PVError(_lib.PV_ERR_ARG, "pitch_track: fmax (cycles per sample) must be > 0, or give tau_min")
            tau_min = int(np.ceil(1.0 / fmax))
        if tau_max is None:
            if fmin is None or not fmin > 0:
                raise PVError(_lib.PV_ERR_ARG, "pitch_track: fmin (cycles per sample) must be > 0, or give tau_max")
            tau_max = int(min(np.floor(1.0 / fmin), 2 ** 30))
        C = spec.shape[0]
        frames = spec.shape[1] if frames is None else frames
        dst = torch.zeros((C, frames, 2), dtype=torch.float32, device=spec.device)
        self._call(self._L.pv_pitch_track(self._h, _ptr(spec), spec.stride(0) // 2, C, frames, int(tau_min),
                                          int(tau_max), float(kappa), _ptr(dst), dst.stride(0) // 2,
                                          self._stream(stream)), "pv_pitch_track")
        return dst

    # -------------------------------------------------------------- pitch shift by resampling
    def reserve_pitch(self, quality: int = 0):
        """pv_pitch_reserve: build the handle's resampler (ratio outHopSize / hopSize; quality 0
        fast, 1 best) and allocate the scratch rows of `pitch_process`.  STANDARD time-stretch
        handles; a setup call (not capturable)."""
        self._call(self._L.pv_pitch_reserve(self._h, int(quality)), "pv_pitch_reserve")

    def set_pitch_formant(self, order: int):
        """pv_pitch_set_formant: formant preservation for `pitch_process` — every frame of the
        time stretch is scaled by its cepstral envelope (quefrencies up to `order`, 1 .. N/4) read
        at the position the resampling will move the bin to, so that after the resampling the
        formants lie where the input has them.  Composes with `set_phase_lock`.  0 turns it off.
        Applies to the calls made after it (`process`, `resynthesis` and the stream segments
        included: `pitch_process` is `process`, then the resampling); the first call allocates the
        handle's envelope rows, and a single-launch handle runs the split path while it is on.
        For harmonic-rich signals: a lone sinusoid has no formants — its envelope is the partial
        itself, and the warp attenuates it."""
        self._call(self._L.pv_pitch_set_formant(self._h, int(order)), "pv_pitch_set_formant")
        self._read_info()

    @property
    def pitch_formant(self) -> int:
        return int(self._L.pv_pitch_get_formant(self._h))

    def pitch_output_length(self, frames: int) -> int:
        return int(self._L.pv_pitch_output_length(self._h, int(frames)))

    def pitch_process(self, x, frames: int | None = None, n_samples: int | None = None, spec=None,
                      out=None, stream=None, spectrum: bool = True):
        """pv_pitch_process: `process` (the time stretch, phase locking and `set_pitch_formant`
        included) into the
        handle's scratch rows, then the resampling by outHopSize / hopSize: the input's duration,
        its pitch moved by that ratio.  Returns (out [C, pitch_output_length(frames)], spec), as
        `process` does."""
        torch = _torch()
        x = self._as2d(x)
        C, n = x.shape
        n_samples = n if n_samples is None else n_samples
        frames = self.num_frames(n_samples) if frames is None else frames
        if not spectrum and spec is not None:
            raise ValueError("spectrum=False with a spec buffer")
        if spectrum and spec is None:
            spec = self.alloc_spec(C, frames)
        if out is None:
            out = torch.empty((C, self.pitch_output_length(frames)), dtype=torch.float32,
                              device=f"cuda:{self.device}")
        self._call(self._L.pv_pitch_process(self._h, _ptr(x), x.stride(0), n_samples, C, frames,
                                            _ptr(spec) if spec is not None else None,
                                            spec.stride(0) // 2 if spec is not None else 0, _ptr(out),
                                            out.stride(0), self._stream(stream)), "pv_pitch_process")
        return out, spec

    def reserve_spectrum(self):
        """Allocate (once, zeroed) the handle's own spectrum rows that process(spectrum=False)
        uses on the split path, so that such calls can be captured into a graph."""
        self._call(self._L.pv_reserve_spectrum(self._h), "pv_reserve_spectrum")

    # -------------------------------------------------------------- reference per-frame API
    def analysis_CUFFT(self, input, output, fft=None, intermediary=None):
        """PhaseVocoder::analysis_CUFFT (phaseVocoder.cpp:25-33): one frame of nSamps
        samples starting at `input` -> `output` (2N float2 in REF_COMPAT).  `fft` and
        `intermediary` are accepted for signature parity and unused (as in the reference
        the cuFFT path never touches `fft`; the window product stays on chip here)."""
        self._call(self._L.pv_analysis(self._h, _ptr(input), self.nSamps, self.nSamps, 1, 1,
                                       _ptr(output), self.spec_stride, self._stream()),
                   "analysis_CUFFT")

    def resynthesis_CUFFT(self, backFrame, frontFrame, output):
        """PhaseVocoder::resynthesis_CUFFT (phaseVocoder.cpp:60-76): output[0..N) =
        frame(frontFrame) + backFrame[outHop..N) shifted to the front (cudaOverlapAdd,
        kernel.cu:111-119)."""
        ola = backFrame[self.outHopSize:]
        self._call(self._L.pv_resynthesis(self._h, _ptr(frontFrame), self.spec_stride, 1, 1,
                                          _ptr(ola), self.nSamps, _ptr(output), self.nSamps,
                                          self._stream()), "resynthesis_CUFFT")

    # -------------------------------------------------------------- shared tables
    def tables_bytes(self) -> int:
        """Size of this handle's table blob (pv_export_tables with no destination)."""
        n = ctypes.c_size_t()
        self._call(self._L.pv_export_tables(self._h, None, 0, ctypes.byref(n), None), "pv_export_tables")
        return int(n.value)

    def export_tables(self):
        """Constant tables as one uint8 CUDA tensor (header + windows + twiddles + ...)."""
        torch = _torch()
        n = ctypes.c_size_t()
        self._call(self._L.pv_export_tables(self._h, None, 0, ctypes.byref(n), None), "pv_export_tables")
        blob = torch.zeros(n.value, dtype=torch.uint8, device=f"cuda:{self.device}")
        self._call(self._L.pv_export_tables(self._h, _ptr(blob), n.value, ctypes.byref(n),
                                            self._stream()), "pv_export_tables")
        return blob

    def import_tables(self, blob):
        self._call(self._L.pv_import_tables(self._h, _ptr(blob), blob.numel(), self._stream()),
                   "pv_import_tables")

    # -------------------------------------------------------------- profiling (bench.py)
    def profile(self, enable=True):
        """enable: False/0 off, True/1 every launch, k > 1 every k-th call's launches."""
        k = int(enable) if not isinstance(enable, bool) else (1 if enable else 0)
        self._call(self._L.pv_profile_enable(self._h, k), "pv_profile_enable")

    def profile_read(self) -> dict:
        cap = 8
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_double * cap)()
        cnt = (ctypes.c_int * cap)()
        n = self._L.pv_profile_read(self._h, names, ms, cnt, cap)
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n)}

    def profile_reset(self):
        self._L.pv_profile_reset(self._h)
