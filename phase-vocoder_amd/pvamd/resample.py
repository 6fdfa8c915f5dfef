"""Standalone band-limited resampler over libpv's pv_resample (include/pv.h "resampler"): a
Kaiser-windowed sinc in polyphase form, ratio p/q (reduced; 1/4 .. 4), one launch over
channels x output tiles."""
from __future__ import annotations

import ctypes

from . import _lib
from .vocoder import _ptr, _torch


class Resampler:
    """Output sample m reads the input at m * p / q: p/q > 1 raises the pitch and shortens the
    signal.  quality: 0 fast (Z = 16), 1 best (Z = 64)."""

    def __init__(self, p: int, q: int, quality: int = 0, device: int = 0):
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.pv_resampler_create(int(p), int(q), int(quality), int(device), ctypes.byref(h)),
                   "pv_resampler_create")
        self._h = h
        self.p, self.q, self.quality, self.device = int(p), int(q), int(quality), int(device)

    def length(self, n: int) -> int:
        """output samples for n input samples: ceil(n q / p)"""
        return int(self._L.pv_resample_length(self._h, int(n)))

    def __call__(self, x, out=None, stream=None):
        """x: [C, n] (or [n]) float32 CUDA, rows contiguous -> [C, length(n)] (or [length(n)])."""
        torch = _torch()
        x2 = x.unsqueeze(0) if x.dim() == 1 else x
        assert x2.is_cuda and x2.dtype == torch.float32 and (x2.shape[-1] == 0 or x2.stride(-1) == 1)
        C, n = x2.shape
        if out is None:
            out = torch.empty((C, self.length(n)), dtype=torch.float32, device=x2.device)
            if x.dim() == 1:
                out = out[0]
        o2 = out.unsqueeze(0) if out.dim() == 1 else out
        assert o2.is_cuda and o2.dtype == torch.float32 and o2.shape[0] == C and o2.shape[-1] >= self.length(n)
        s = ctypes.c_void_p(int(stream) if stream is not None
                            else torch.cuda.current_stream(x2.device).cuda_stream)
        _lib.check(self._L.pv_resample(self._h, _ptr(x2), x2.stride(0), n, C, _ptr(o2), o2.stride(0), s),
                   "pv_resample")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.pv_resampler_destroy(self._h)
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
