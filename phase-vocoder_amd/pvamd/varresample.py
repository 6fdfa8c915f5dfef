"""Variable-rate band-limited resampler over libpv's pv_varresample (include/pv.h "variable-rate
resampler"): the ratio is constant within a block of `block` output samples and may change from
block to block; one launch over channels x output tiles.  Also the host-only helpers of the pitch
map (`ratio_steps`, `pitch_map_plan`)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .vocoder import _ptr, _torch

_vp = ctypes.c_void_p


def ratio_steps(ratios) -> np.ndarray:
    """pv_varresample_steps (pure host, no GPU): ratios in [1/4, 4] -> steps llrint(ratio 2^32) as
    int64, in units of 2^-32 input samples per output sample."""
    r = np.ascontiguousarray(ratios, dtype=np.float64).reshape(-1)
    step = np.empty(r.size, dtype=np.int64)
    _lib.check(_lib.lib().pv_varresample_steps(r.ctypes.data_as(_vp), int(r.size), step.ctypes.data_as(_vp)),
               "pv_varresample_steps")
    return step


def pitch_map_plan(N: int, hop: int, positions, ratios):
    """pv_pitchmap_plan (pure host, no GPU): per final output frame a position and a pitch ratio
    -> (pos_s float64 [n_s], the time map of the stretch; steps int64 [ceil((n hop + N - hop) /
    hop)], the resampler's map in blocks of hop)."""
    pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
    rat = np.ascontiguousarray(ratios, dtype=np.float64).reshape(-1)
    if pos.size != rat.size:
        raise ValueError("positions and ratios must have one entry per output frame each")
    n = int(pos.size)
    cap_s, cap_b = 4 * n + 2, n + (int(N) + int(hop) - 1) // max(int(hop), 1) + 1
    pos_s = np.empty(cap_s, dtype=np.float64)
    step = np.empty(cap_b, dtype=np.int64)
    n_s, n_b = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().pv_pitchmap_plan(int(N), int(hop), pos.ctypes.data_as(_vp), rat.ctypes.data_as(_vp), n,
                                           pos_s.ctypes.data_as(_vp), cap_s, ctypes.byref(n_s),
                                           step.ctypes.data_as(_vp), cap_b, ctypes.byref(n_b)), "pv_pitchmap_plan")
    return pos_s[:n_s.value].copy(), step[:n_b.value].copy()


class VarResampler:
    """Output sample m of block b = m // block reads the input at T_b + (m - b block) d_b, with
    T_0 = start, T_{b+1} = T_b + block d_b (units of 2^-32 samples): a ratio > 1 raises the pitch.
    quality: 0 fast (Z = 16), 1 best (Z = 64)."""

    def __init__(self, block: int, quality: int = 0, max_blocks: int = 4096, device: int = 0):
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.pv_varresampler_create(int(quality), int(block), int(max_blocks), int(device),
                                                  ctypes.byref(h)), "pv_varresampler_create")
        self._h = h
        self.block, self.quality, self.max_blocks, self.device = int(block), int(quality), int(max_blocks), int(device)

    def set_map(self, steps_or_ratios, start: int = 0):
        """pv_varresampler_set_map: one entry per block; an integer array holds steps (2^32 = ratio
        1), a floating one ratios (converted by `ratio_steps`).  start: the first output's input
        position in units of 2^-32 samples.  A setup call (not capturable).
        A 2-D [channels, blocks] array is a map per channel (pv_varresampler_set_maps): row c
        and start[c] (a scalar start: the same for every channel) for channel c of a call."""
        a = np.asarray(steps_or_ratios)
        if a.ndim == 2:
            C, nb = a.shape
            step = (ratio_steps(a).reshape(C, nb) if a.dtype.kind == "f"
                    else np.ascontiguousarray(a, dtype=np.int64))
            st = np.ascontiguousarray(np.broadcast_to(np.asarray(start, dtype=np.int64), (C,)))
            _lib.check(self._L.pv_varresampler_set_maps(self._h, int(C), st.ctypes.data_as(_vp),
                                                        step.ctypes.data_as(_vp), int(nb), int(nb)),
                       "pv_varresampler_set_maps")
            return
        step = ratio_steps(a) if a.dtype.kind == "f" else np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        _lib.check(self._L.pv_varresampler_set_map(self._h, int(start), step.ctypes.data_as(_vp), int(step.size)),
                   "pv_varresampler_set_map")

    @property
    def map_channels(self) -> int:
        """pv_varresample_map_channels: the channels of maps per channel; 0 without a map or with the shared one"""
        return int(self._L.pv_varresample_map_channels(self._h))

    @property
    def length(self) -> int:
        """output samples of the map: blocks * block (0 without a map)"""
        return int(self._L.pv_varresample_length(self._h))

    def __call__(self, x, n_out: int | None = None, out=None, stream=None):
        """x: [C, n] (or [n]) float32 CUDA, rows contiguous -> [C, n_out] (or [n_out]); n_out
        defaults to `length`."""
        torch = _torch()
        x2 = x.unsqueeze(0) if x.dim() == 1 else x
        assert x2.is_cuda and x2.dtype == torch.float32 and (x2.shape[-1] == 0 or x2.stride(-1) == 1)
        C, n = x2.shape
        n_out = self.length if n_out is None else int(n_out)
        if out is None:
            out = torch.empty((C, n_out), dtype=torch.float32, device=x2.device)
            if x.dim() == 1:
                out = out[0]
        o2 = out.unsqueeze(0) if out.dim() == 1 else out
        assert o2.is_cuda and o2.dtype == torch.float32 and o2.shape[0] == C and o2.shape[-1] >= n_out
        s = ctypes.c_void_p(int(stream) if stream is not None
                            else torch.cuda.current_stream(x2.device).cuda_stream)
        _lib.check(self._L.pv_varresample(self._h, _ptr(x2), x2.stride(0), n, C, _ptr(o2), o2.stride(0), n_out, s),
                   "pv_varresample")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.pv_varresampler_destroy(self._h)
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
