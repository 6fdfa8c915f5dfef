"""fp64 reference of the formant-preserving STANDARD pitch shift (DESIGN.md §3.7,
include/pv.h pv_set_formant), restated in numpy from what the oracle exports: the bit-exact
analysis rows, the expected advance, the contract's unwrap decision per bin and frame, the
floor(beta k + 0.5) bin map with beta the fp32 scale, and the phase recurrence exactly as the
oracle's std_process writes it.  With order = 0 it reproduces pvref.std_process(..., 'p', beta)
(tests/test_formant_ref.py), which is what makes it a yardstick for order > 0.

Frame with order > 0: lg = ln max(mag, 2^-30) (a NaN magnitude gives the floor), evenly
extended to N points; c = irfft(lg), zeroed where min(n, N - n) > order; le = Re rfft(c);
|Y[k']| = exp(le[k']) * sum over the sources k of k' of mag[k] exp(-le[k]).
"""
import functools

import numpy as np

import pvref
from ref_cache import array, memo

TWO_PI = 2.0 * np.pi
FLOOR = 2.0 ** -30


def log_envelope(mag, N, order):
    """le [..., N/2 + 1] float64 of the fp32 magnitude rows mag [..., N/2 + 1]."""
    m = np.asarray(mag, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        lg = np.log(np.where(m >= FLOOR, m, FLOOR))  # maxNum: NaN -> the floor
    with np.errstate(invalid="ignore"):
        c = np.fft.irfft(lg, N, axis=-1)
        n = np.arange(N)
        c = np.where(np.minimum(n, N - n) <= order, c, 0.0)
        return np.fft.rfft(c, axis=-1).real


def pitch_map(N, beta):
    """{first source, count} of every output bin: k' = floor(beta k + 0.5)"""
    B = N // 2 + 1
    first = np.full(B, -1, np.int64)
    cnt = np.zeros(B, np.int64)
    for k in range(B):
        kp = int(np.floor(beta * k + 0.5))
        if kp < 0 or kp >= B:
            continue
        if first[kp] < 0:
            first[kp] = k
        cnt[kp] += 1
    return first, cnt


def std_process_formant(x, N, hop_div, scale, order, frames=None):
    """Pitch shift of one channel (float32 samples) -> float64 output, as
    pvref.std_process(x, N, hop_div, ord('p'), scale) with the formant envelope of `order`
    (0: none)."""
    x = np.ascontiguousarray(x, np.float32)
    hop = N // hop_div
    if frames is None:
        frames = pvref.num_frames(x.shape[0], hop)
    beta = float(np.float32(scale))
    B = N // 2 + 1
    mag, ph = pvref.std_analysis(x, N, hop, frames)
    ek, jk = pvref.expected_advance(N, hop)
    i = np.arange(N, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(TWO_PI * i / N)
    g = w * (hop / np.sum(w * w))  # (np.fft.irfft carries the 1 / N)
    wk = TWO_PI * np.arange(B, dtype=np.float64) / N
    first, cnt = pitch_map(N, beta)
    has = cnt > 0
    src = np.where(has, first, 0)
    le = log_envelope(mag, N, order) if order > 0 else np.zeros(mag.shape, np.float64)
    out = np.zeros(frames * hop + (N - hop), np.float64)
    acc = np.zeros(B, np.float64)
    prev = np.zeros(B, np.float32)
    for t in range(frames):
        p32 = ph[t]
        m = np.array([pvref.unwrap_count(p32[k], prev[k], ek[k]) for k in range(B)], np.float64)
        p64 = p32.astype(np.float64)
        delta = (p64 - prev.astype(np.float64) - wk * hop) + TWO_PI * (m + jk)
        omega = wk + delta / hop
        prev = p32
        acc = np.where(has, np.fmod(acc + hop * beta * omega[src], TWO_PI), acc)
        with np.errstate(invalid="ignore", over="ignore"):
            white = mag[t].astype(np.float64) * np.exp(-le[t])
            msum = np.zeros(B, np.float64)
            for q in range(int(cnt.max())):  # source order, as the oracle
                msum += np.where(q < cnt, white[np.minimum(src + q, B - 1)], 0.0)
            Y = np.where(has, msum * np.exp(le[t]) * np.exp(1j * acc), 0.0)
            out[t * hop:t * hop + N] += np.fft.irfft(Y, N) * g
    return out


@memo(x=array(np.float32), scale=float, order=int)
def cached(x, N, hop_div, scale, order, frames=None):
    """std_process_formant, computed once per (input, configuration) and shared read-only."""
    return std_process_formant(x, N, hop_div, scale, order, frames)


# ---------------------------------------------------------------- the formant property
F0 = 0.004        # cycles/sample
FORMANT = 0.09    # the resonance
WIDTH = 0.006
INPUT_PEAK = 0.0894  # formant_peak(voice()): the harmonics nearest the resonance are 0.088, 0.092


@functools.lru_cache(maxsize=None)
def voice(n=16000, lead=3000, seed=5):
    """harmonics of F0 under one resonance (amplitude 1 / (1 + ((f - FORMANT) / WIDTH)^2)),
    peak amplitude 0.5, uniform noise 1e-3; the first `lead` samples are zero (frames that
    sit on the 2^-30 floor)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros(n)
    for h in range(1, int(0.5 / F0)):
        f = h * F0
        x += np.sin(TWO_PI * f * t + rng.uniform(0, TWO_PI)) / (1.0 + ((f - FORMANT) / WIDTH) ** 2)
    x *= 0.5 / np.max(np.abs(x))
    x += rng.uniform(-1e-3, 1e-3, n)
    x[:lead] = 0.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def formant_peak(y, start=4000, nfft=2048, lo=0.02, hi=0.3, smooth=0.012):
    """frequency (cycles/sample) of the peak of the harmonic-smoothed long-term spectrum: mean
    power of nfft-point Hann frames from sample `start` on, box-smoothed over `smooth`
    cycles/sample (three harmonics of F0), searched over [lo, hi]."""
    y = np.asarray(y, np.float64)[start:]
    w = 0.5 - 0.5 * np.cos(TWO_PI * np.arange(nfft) / nfft)
    nf = (y.shape[0] - nfft) // (nfft // 4) + 1
    P = np.zeros(nfft // 2 + 1)
    for j in range(nf):
        P += np.abs(np.fft.rfft(y[j * (nfft // 4):j * (nfft // 4) + nfft] * w)) ** 2
    k = max(1, int(round(smooth * nfft)))
    Ps = np.convolve(P, np.ones(k) / k, mode="same")
    f = np.arange(nfft // 2 + 1) / nfft
    sel = (f >= lo) & (f <= hi)
    return float(f[sel][np.argmax(Ps[sel])])
