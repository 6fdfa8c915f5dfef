"""fp64 reference of the transient phase reset of the STANDARD time stretch (DESIGN.md §3.11,
include/pv.h pv_set_transient), restated in numpy from what the oracle exports — the bit-exact
analysis rows, the expected advance, the contract's unwrap decision per bin and frame — on the
recurrence of tests/phase_lock_ref.py.  With no frame flagged it reproduces that reference, lock
off and lock on (tests/test_transient_ref.py), which is what makes it a yardstick for the flagged
frames.

Reset: a flagged frame t0 is put down with its analysis phases; the frames after it, up to the
next flagged frame, add theta[k] = (phi(t0)[k] - closed(t0)[k]) mod 2 pi to the plain stretch's
phase closed(t)[k].  Locked: the peak's output phase includes its theta, the locking is
otherwise unchanged.

Detector: rise[t] = sum_k max(0, mag_t[k] - mag_{t-1}[k]) (mag_{-1} = 0), tot[t] = sum_k mag_t[k]
(a NaN magnitude adds 0 to both); flag[t] = t >= 1 and rise[t] > thr tot[t] and rise[t] >
rise[t-1] and rise[t] >= rise[t+1] (rise[frames] = 0).
"""
import numpy as np

import pvref
from phase_lock_ref import owners, peaks
from ref_cache import array, memo

TWO_PI = 2.0 * np.pi
DEFAULT_THRESHOLD = 0.3  # PV_TRANSIENT_DEFAULT_THRESHOLD (include/pv.h)


def std_process_reset(x, N, hop_div, scale, lock, flags, frames=None, spectra=None):
    """Time stretch of one channel (float32 samples) with the frames flagged in `flags`
    (truthy per frame; frame 0's is ignored; None = none) reset -> float64 output.  spectra: a
    list that receives every frame's (synthesised Y, analysis X), complex128 [N/2 + 1]."""
    x = np.ascontiguousarray(x, np.float32)
    hop = N // hop_div
    if frames is None:
        frames = pvref.num_frames(x.shape[0], hop)
    fl = np.zeros(frames, bool)
    if flags is not None:
        f = np.asarray(flags).astype(bool)[:frames]
        fl[:f.shape[0]] = f
    if frames:
        fl[0] = False
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
    theta = np.zeros(B, np.float64)
    prev = np.zeros(B, np.float32)
    for t in range(frames):
        p32 = ph[t]
        m = np.array([pvref.unwrap_count(p32[k], prev[k], ek[k]) for k in range(B)], np.float64)
        p64 = p32.astype(np.float64)
        delta = (p64 - prev.astype(np.float64) - wk * hop) + TWO_PI * (m + jk)
        omega = wk + delta / hop
        prev = p32
        acc = np.fmod(acc + hs * omega, TWO_PI)
        if fl[t]:
            theta = np.fmod(p64 - acc, TWO_PI)
        ps = acc + theta
        if lock:
            own = owners(peaks(mag[t]))
            phase = p64 + (ps - p64)[own]
        else:
            phase = ps
        Y = mag[t].astype(np.float64) * np.exp(1j * phase)
        if spectra is not None:
            spectra.append((Y, mag[t].astype(np.float64) * np.exp(1j * p64)))
        out[t * hs:t * hs + N] += np.fft.irfft(Y, N) * g
    return out


@memo(x=array(np.float32), scale=float, lock=bool, flags=lambda f: (np.asarray(f) != 0).astype(np.uint8))
def cached(x, N, hop_div, scale, lock, flags, frames=None):
    """std_process_reset, computed once per (input, configuration, flags) and shared read-only."""
    return std_process_reset(x, N, hop_div, scale, lock, flags, frames)


# ---------------------------------------------------------------- detector
def strengths(mag):
    """mag [frames, B] (fp32 magnitudes) -> (rise, tot), float64 [frames]"""
    m = np.asarray(mag, np.float64)
    prev = np.vstack([np.zeros((1, m.shape[1])), m[:-1]])
    rise = np.sum(np.fmax(m - prev, 0.0), axis=1)
    tot = np.sum(np.fmax(m, 0.0), axis=1)
    return rise, tot


def _neighbours(rise):
    before = np.concatenate([[0.0], rise[:-1]])
    after = np.concatenate([rise[1:], [0.0]])
    return before, after


def pick(rise, tot, thr=DEFAULT_THRESHOLD):
    """flags (bool [frames]) of the detector's rule"""
    before, after = _neighbours(rise)
    fl = (rise > thr * tot) & (rise > before) & (rise >= after)
    if fl.shape[0]:
        fl[0] = False
    return fl


def clear(rise, tot, thr=DEFAULT_THRESHOLD, rel=1e-4):
    """bool [frames]: every one of the three comparisons of the frame clears its threshold by
    the relative margin `rel` (of the larger operand), so fp32 sums in another order decide the
    same way"""
    before, after = _neighbours(rise)

    def ok(a, b):
        return np.abs(a - b) > rel * np.maximum(np.abs(a), np.abs(b))
    return ok(rise, thr * tot) & ok(rise, before) & ok(rise, after)


def bursts(n, seed, amp=0.02, f=0.031, noise=0.0):
    """clicks and tone bursts over a quiet tone (seeded): the detector's test input; noise:
    amplitude of a uniform noise floor"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = amp * np.sin(TWO_PI * f * t + rng.uniform(0, TWO_PI))
    if noise:
        x += np.random.default_rng(seed + 1000003).uniform(-noise, noise, n)
    pos = 300
    while pos < n - 200:
        if rng.uniform() < 0.5:
            x[pos] += rng.uniform(0.4, 0.9) * rng.choice([-1.0, 1.0])
        else:
            ln = int(rng.integers(150, 500))
            seg = slice(pos, min(n, pos + ln))
            k = np.arange(seg.stop - seg.start)
            x[seg] += rng.uniform(0.2, 0.5) * np.sin(TWO_PI * rng.uniform(0.05, 0.2) * k) * np.exp(-k / (0.4 * ln))
        pos += int(rng.integers(700, 1500))
    return x.astype(np.float32)


# ---------------------------------------------------------------- the quality figure
def clicks(n=8000, period=1536, first=700, amp=0.8, tone=0.05, f=0.02):
    """single-sample clicks of amplitude `amp` every `period` samples over a `tone`-amplitude
    sine; returns (x float32, click positions)"""
    t = np.arange(n, dtype=np.float64)
    x = tone * np.sin(TWO_PI * f * t)
    pos = np.arange(first, n - 2 * 256, period)
    x[pos] += amp
    return x.astype(np.float32), pos


def click_frames(pos, N, hop):
    """the frame whose centre (t hop + N/2) is nearest each click"""
    return np.maximum(np.rint((pos - N / 2) / hop).astype(int), 0)


def click_flags(pos, N, hop, frames):
    fl = np.zeros(frames, np.uint8)
    fl[click_frames(pos, N, hop)] = 1
    return fl


def compactness(y, pos, N, hop, hs):
    """per click: energy within +-N/8 of its output position (t0 hs + its offset in frame t0)
    over the energy within +-N, averaged over the clicks"""
    y = np.asarray(y, np.float64)
    vals = []
    for p, t0 in zip(pos, click_frames(pos, N, hop)):
        o = int(t0 * hs + (p - t0 * hop))
        a = np.sum(y[max(o - N // 8, 0):o + N // 8 + 1] ** 2)
        b = np.sum(y[max(o - N, 0):o + N + 1] ** 2)
        vals.append(a / b)
    return float(np.mean(vals))
