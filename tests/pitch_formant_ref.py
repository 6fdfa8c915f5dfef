"""fp64 reference of the STANDARD time stretch with the envelope warp (DESIGN.md §3.10,
include/pv.h pv_pitch_set_formant): formant preservation for the pitch shift by time stretch
and resampling.  Written like phase_lock_ref.std_process_lock, from what the oracle exports
(the bit-exact analysis rows, the expected advance, the contract's unwrap decision, the phase
recurrence), with formant_ref.log_envelope for the envelope.  With order = 0 it reproduces
std_process_lock (tests/test_pitch_formant_ref.py), which is what makes it a yardstick for
order > 0.

Frame with order > 0: le = log_envelope(mag); bin k reads it at k out_hop / hop in exact
integers: a = k out_hop, i_k = a div hop, r_k = a mod hop, and {L, 0} from the first bin with
i_k >= L on; lw[k] = le[i_k] + (r_k / hop) (le[min(i_k + 1, L)] - le[i_k]);
|Y[k]| = mag[k] exp(lw[k] - le[k]); the phase is the stretch's, unlocked or locked, and the
peaks and owners are those of the unscaled magnitudes.
"""
import numpy as np

import pvref
from formant_ref import log_envelope
from phase_lock_ref import owners, peaks
from ref_cache import array, memo

TWO_PI = 2.0 * np.pi


def warp_map(N, hop, out_hop):
    """(i_k int64 [B], r_k int64 [B]) of the bins k = 0 .. N/2"""
    L = N // 2
    a = np.arange(L + 1, dtype=np.int64) * int(out_hop)
    i, r = a // int(hop), a % int(hop)
    over = i >= L
    return np.where(over, L, i), np.where(over, 0, r)


def warp_gain(le, N, hop, out_hop):
    """exp(lw - le) of the envelope rows le [..., N/2 + 1]"""
    L = N // 2
    i, r = warp_map(N, hop, out_hop)
    lo = le[..., i]
    hi = le[..., np.minimum(i + 1, L)]
    with np.errstate(invalid="ignore", over="ignore"):
        lw = lo + (r.astype(np.float64) / hop) * (hi - lo)
        return np.exp(lw - le)


def std_process_warp(x, N, hop_div, scale, lock, order, frames=None):
    """Time stretch of one channel (float32 samples) -> float64 output, as
    phase_lock_ref.std_process_lock(x, N, hop_div, scale, lock) with the envelope warp of
    `order` (0: none)."""
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
    gain = warp_gain(log_envelope(mag, N, order), N, hop, hs) if order > 0 else None
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
            own = owners(peaks(mag[t]))  # decided on the row's own magnitudes
            phase = p64 + (acc - p64)[own]
        else:
            phase = acc
        with np.errstate(invalid="ignore", over="ignore"):
            m64 = mag[t].astype(np.float64)
            if gain is not None:
                m64 = m64 * gain[t]
            Y = m64 * np.exp(1j * phase)
            out[t * hs:t * hs + N] += np.fft.irfft(Y, N) * g
    return out


@memo(x=array(np.float32), scale=float, lock=bool, order=int)
def cached(x, N, hop_div, scale, lock, order, frames=None):
    """std_process_warp, computed once per (input, configuration) and shared read-only."""
    return std_process_warp(x, N, hop_div, scale, lock, order, frames)
