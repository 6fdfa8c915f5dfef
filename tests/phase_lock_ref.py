"""fp64 reference of the STANDARD time stretch with identity phase locking (DESIGN.md §3.6,
include/pv.h pv_set_phase_lock), restated in numpy from what the oracle exports: the
bit-exact analysis rows, the expected advance, the contract's unwrap decision per bin and
frame, and the textbook phase recurrence exactly as the oracle's std_process writes it.  With
lock=False it reproduces pvref.std_process (tests/test_phase_lock_ref.py), which is what
makes it a yardstick for lock=True.

Locked frame: bin k is a peak iff mag[k] > mag[k'] (strict, on the fp32 magnitudes) for every
k' in {k-2, k-1, k+1, k+2} inside [0, N/2]; own(k) is the nearest peak (the lower one on a
tie; k itself if the frame has none); Y[k] = mag[k] exp(i (phi[k] + acc[own] - phi[own])).
"""
import numpy as np

import pvref
from ref_cache import array, memo

TWO_PI = 2.0 * np.pi


def peaks(mag):
    """bool [B]: strict local maxima over the neighbours at distance 1 and 2 (fp32 compares;
    a NaN compares false; out-of-range neighbours are ignored)."""
    mag = np.asarray(mag, np.float32)
    B = mag.shape[0]
    pk = np.ones(B, bool)
    with np.errstate(invalid="ignore"):
        for d in (1, 2):
            pk[:B - d] &= mag[:B - d] > mag[d:]
            pk[d:] &= mag[d:] > mag[:B - d]
        pk &= mag == mag  # a lone NaN bin (B <= 1) is no peak either
    return pk


def owners(pk):
    """int [B]: the nearest peak of every bin, the lower one on a tie; the bin itself if
    there is no peak."""
    B = pk.shape[0]
    k = np.arange(B)
    idx = np.flatnonzero(pk)
    if idx.size == 0:
        return k
    hi_pos = np.searchsorted(idx, k, side="left")          # first peak >= k
    lo = idx[np.clip(hi_pos - 1, 0, idx.size - 1)]
    hi = idx[np.clip(hi_pos, 0, idx.size - 1)]
    exact = (hi_pos < idx.size) & (hi == k)
    no_lo = hi_pos == 0
    no_hi = hi_pos >= idx.size
    dlo = np.where(no_lo, B + 1, k - lo)
    dhi = np.where(no_hi, B + 1, hi - k)
    own = np.where(dlo <= dhi, lo, hi)
    return np.where(exact, k, own)


def std_process_lock(x, N, hop_div, scale, lock, frames=None):
    """Time stretch of one channel (float32 samples) -> float64 output, as
    pvref.std_process(x, N, hop_div, ord('t'), scale) with optional identity locking."""
    x = np.ascontiguousarray(x, np.float32)
    hop = N // hop_div
    if frames is None:
        frames = pvref.num_frames(x.shape[0], hop)
    hs = pvref.out_hop(N, hop_div, ord("t"), scale)
    B = N // 2 + 1
    mag, ph = pvref.std_analysis(x, N, hop, frames)
    ek, jk = pvref.expected_advance(N, hop)
    i = np.arange(N, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(TWO_PI * i / N)
    g = w * (hs / np.sum(w * w))  # (np.fft.irfft carries the 1 / N)
    wk = TWO_PI * np.arange(B, dtype=np.float64) / N
    out = np.zeros(frames * hs + (N - hs), np.float64)
    acc = np.zeros(B, np.float64)
    prev = np.zeros(B, np.float32)
    for t in range(frames):
        p32 = ph[t]
        m = np.array([pvref.unwrap_count(p32[k], prev[k], ek[k]) for k in range(B)], np.float64)
        p64 = p32.astype(np.float64)
        delta = (p64 - prev.astype(np.float64) - wk * hop) + TWO_PI * (m + jk)
        omega = wk + delta / hop
        prev = p32
        acc = np.fmod(acc + hs * omega, TWO_PI)
        if lock:
            own = owners(peaks(mag[t]))
            phase = p64 + (acc - p64)[own]
        else:
            phase = acc
        Y = mag[t].astype(np.float64) * np.exp(1j * phase)
        out[t * hs:t * hs + N] += np.fft.irfft(Y, N) * g
    return out


@memo(x=array(np.float32), scale=float, lock=bool)
def cached(x, N, hop_div, scale, lock, frames=None):
    """std_process_lock, computed once per (input, configuration) and shared read-only."""
    return std_process_lock(x, N, hop_div, scale, lock, frames)


def chirp(n=6144, f0=0.03, f1=0.11, amp=0.5):
    """linear chirp, f0 -> f1 cycles/sample over n samples"""
    t = np.arange(n, dtype=np.float64)
    return (amp * np.sin(TWO_PI * (f0 * t + 0.5 * (f1 - f0) / n * t * t))).astype(np.float32)


def mean_envelope(y, N):
    """mean magnitude of the FFT-built analytic signal, 2N samples dropped at each end"""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    Y = np.fft.fft(y)
    h = np.zeros(n)
    h[0] = 1.0
    if n % 2 == 0:
        h[n // 2] = 1.0
        h[1:n // 2] = 2.0
    else:
        h[1:(n + 1) // 2] = 2.0
    env = np.abs(np.fft.ifft(Y * h))
    return float(np.mean(env[2 * N:n - 2 * N]))
