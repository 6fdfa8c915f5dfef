"""fp64 reference of the real-time pitch map (include/pv.h pv_rt_pitchmap_push),
restated in numpy from the oracle's bit-exact analysis rows and the pieces the offline references
are made of: timemap_ref.phase_turns / scan / lerp32, phase_lock_ref's peaks and owners,
varresample_ref.block_filter / kernel.

A stream of T pushed frames (T hop samples, one fp32 ratio per frame), per channel:
  rows      row t = analysis frame t of the stream prefixed with N - hop zeros; P(t) = phase_turns
  steps     r' = min(max(r_t, ratio_min), ratio_max), a NaN reading as ratio_min; d = int(r' 2^32);
            frame 0's ratio is ignored, d_{t-1} = d for t >= 1; Sigma_0 = 0, Sigma_{b+1} = Sigma_b + hop d_b
  stretch   frame v at t_v = v hop 2^32 lies in span b, Sigma_b <= t_v < Sigma_{b+1}: position (b, a),
            a = float32(float64(t_v - Sigma_b) / float64(hop d_b)) — fed as (i, a), not through
            timemap_ref.split, which would round b + a
  output    block b, sample j at Sigma_b + j d_b through the filter of a block with step d_b; no copy
            shortcut at ratio 1
  latency   G = ceil(W_max 2^32 / (hop d_min)); pushed frame t emits block t - 1 - G, zeros below 0
"""
import functools

import numpy as np

import pvref
import timemap_ref as tm
import varresample_ref as vr
from phase_lock_ref import owners, peaks
from ref_cache import array, memo

ONE = vr.ONE
TWO_PI = 2.0 * np.pi


# ---------------------------------------------------------------- integers
def step_of(r, ratio_min, ratio_max):
    """the step of one pushed ratio (any float): clamped in fp32, then the exact integer"""
    r = np.float32(r)
    lo, hi = np.float32(ratio_min), np.float32(ratio_max)
    r = lo if np.isnan(r) else min(max(r, lo), hi)
    return int(np.float64(r) * 4294967296.0)  # exact: an fp32 >= 1/4 is a multiple of 2^-26


def steps_of(ratios, ratio_min, ratio_max):
    """ratios [T] of the pushed frames -> d_0 .. d_{T-2} (frame 0's ratio is ignored)"""
    return [step_of(r, ratio_min, ratio_max) for r in np.asarray(ratios).reshape(-1)[1:]]


def plan(hop, quality, ratio_min, ratio_max, max_nframes=1):
    """pvtab::rt_pitchmap_plan: dict of d_min, d_max, W_max, G, latency, K, row_len, ring_cap"""
    d_min, d_max = step_of(ratio_min, ratio_min, ratio_max), step_of(ratio_max, ratio_min, ratio_max)
    _, W_max = vr.block_filter(d_max, quality)
    den = hop * d_min
    G = -(-(W_max << 32) // den)
    K = (W_max + 3) & ~3
    span = -(-((G + max_nframes) * hop * d_max) // ONE)
    return dict(d_min=d_min, d_max=d_max, W_max=W_max, G=G, latency=(G + 1) * hop, K=K,
                row_len=(K + span + hop + 4 + 3) & ~3, ring_cap=G + max_nframes)


def knots(steps, hop):
    return vr.knots(0, steps, hop)


def stretched_frames(steps, hop):
    """[(b, off, span)] of every stretched frame below Sigma_{len(steps)}, in order"""
    S = knots(steps, hop)
    unit = hop * ONE
    out, b = [], 0
    for v in range(-(-S[-1] // unit)):
        t = v * unit
        while t >= S[b + 1]:
            b += 1
        out.append((b, t - S[b], S[b + 1] - S[b]))
    return out


def final_below(steps, hop, t):
    """after the callback of pushed frame t (t >= 1) the scratch row holds the stretched stream
    below this sample: the start of the first stretched frame at or beyond Sigma_t"""
    S = knots(steps[:t], hop)
    unit = hop * ONE
    return -(-S[t] // unit) * hop


def guaranteed_below(steps, hop, t):
    """... of which ceil(Sigma_t / 2^32) is what holds wherever the stretched frames fall: every
    stretched frame with t_v < Sigma_t has been added.  G is derived from this bound."""
    return -(-knots(steps[:t], hop)[t] // ONE)


def block_reach(steps, hop, quality, b):
    """the highest stretched sample block b reads"""
    S = knots(steps[:b], hop)
    _, W = vr.block_filter(steps[b], quality)
    return ((S[b] + (hop - 1) * steps[b]) >> 32) + W


def least_slack(steps, hop, quality, G, below=guaranteed_below):
    """min over the blocks b emitted with latency G (at the callback of frame b + 1 + G) of
    below(b + 1 + G) - 1 - reach: negative when some block reads a sample that is not final yet"""
    T = len(steps) + 1
    return min(below(steps, hop, b + 1 + G) - 1 - block_reach(steps, hop, quality, b)
               for b in range(0, T - 1 - G))


# ---------------------------------------------------------------- the stream
def stretch(x, N, hop_div, steps, lock):
    """The stretched stream S of one channel (float32 samples, T hop of them, T = len(steps) + 1):
    float64, nv hop + N - hop samples of which the first nv hop are final."""
    x = np.ascontiguousarray(x, np.float32)
    hop = N // hop_div
    T = len(steps) + 1
    assert x.shape[0] == T * hop
    xp = np.concatenate([np.zeros(N - hop, np.float32), x])
    mag, ph = pvref.std_analysis(xp, N, hop, T)
    P = tm.phase_turns(ph)
    fr = stretched_frames(steps, hop)
    idx = np.array([b for b, _, _ in fr], np.int64)
    Phi = tm.scan(P, idx)  # Phi(0) = P(0); += P(b + 1) - P(b) after every frame of span b
    i = np.arange(N, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(TWO_PI * i / N)
    g = w * (hop / np.sum(w * w))
    out = np.zeros(len(fr) * hop + (N - hop), np.float64)
    for v, (b, off, span) in enumerate(fr):
        a = np.float32(np.float64(off) / np.float64(span))
        m = tm.lerp32(a, mag[b], mag[b + 1])
        if lock:
            own = owners(peaks(m))
            Psi = (P[b] + ((Phi[v] - P[b]) & tm.MASK)[own]) & tm.MASK
        else:
            Psi = Phi[v]
        signed = np.where(Psi >= 2 ** 31, Psi - 2 ** 32, Psi).astype(np.float64)
        Y = m.astype(np.float64) * np.exp(1j * (TWO_PI * signed / 2.0 ** 32))
        out[v * hop:v * hop + N] += np.fft.irfft(Y, N) * g
    return out


def resample_blocks(S, steps, hop, quality, nblocks):
    """y of blocks 0 .. nblocks - 1 (S reads as 0 below sample 0; nothing at or above len(S) may be
    read): every block through its filter, ratio 1 included"""
    Sg = knots(steps, hop)
    y = np.zeros(nblocks * hop, np.float64)
    for b in range(nblocks):
        d = steps[b]
        t = [Sg[b] + j * d for j in range(hop)]
        i = np.array([v >> 32 for v in t], np.int64)
        f = np.array([v & (ONE - 1) for v in t], np.float64) / 4294967296.0
        Sq, W = vr.block_filter(d, quality)
        assert i[-1] + W < len(S)
        for j in range(-W + 1, W + 1):
            idx = i + j
            xv = np.where(idx >= 0, S[np.clip(idx, 0, None)], 0.0)
            y[b * hop:(b + 1) * hop] += xv * vr.kernel(j - f, Sq, quality)
    return y


def stream(x, N, hop_div, ratios, lock, quality=0, ratio_min=0.5, ratio_max=2.0):
    """The emitted stream of one channel: x [T hop] float32 and ratios [T] -> float64 [T hop]"""
    hop = N // hop_div
    ratios = np.asarray(ratios, np.float32).reshape(-1)
    T = ratios.shape[0]
    steps = steps_of(ratios, ratio_min, ratio_max)
    G = plan(hop, quality, ratio_min, ratio_max)["G"]
    out = np.zeros(T * hop, np.float64)
    nb = T - 1 - G
    if nb > 0:
        S = stretch(x, N, hop_div, steps, lock)
        out[(G + 1) * hop:] = resample_blocks(S, steps, hop, quality, nb)
    return out


@memo(x=array(np.float32), ratios=array(np.float32), lock=bool)
def cached(x, N, hop_div, ratios, lock, quality=0, ratio_min=0.5, ratio_max=2.0):
    """stream, computed once per (input, configuration, ratios) and shared read-only."""
    return stream(x, N, hop_div, ratios, lock, quality, ratio_min, ratio_max)


# ---------------------------------------------------------------- ratio sequences (fp32-exact)
def constant(T, r):
    return np.full(T, r, np.float32)


def glide(T, r0, r1):
    return vr.glide(T, r0, r1).astype(np.float32)


def vibrato(T, depth=0.06, period=23.0, phase=0.0):
    return (1.0 + depth * np.sin(TWO_PI * np.arange(T) / period + phase)).astype(np.float32)


def alternating(T, r0, r1):
    return np.where(np.arange(T) % 2 == 0, r0, r1).astype(np.float32)


def spikes(T, r0, r1, period):
    """r1 once per `period` frames, r0 otherwise: the widest filter followed by the shortest spans"""
    return np.where(np.arange(T) % period == 1, r1, r0).astype(np.float32)


# ---------------------------------------------------------------- live correction
LIVE_RANGE = (0.84, 1.19)  # +-3 semitones
LIVE_BEFORE, LIVE_AFTER = 34.99, 1.90  # median cents off the scale, measured on this reference


def live_correction(x, N, hop_div, a4, mask, lags, quality=0, lock=True, track_rows=None):
    """The live loop of one voice on the CPU: the ratio pushed with frame b + 1 is the causal
    correction (retune 1) of the track of rows 0 .. b.  -> (ratios float32 [T], stream)"""
    import pitchtrack_ref as pr
    hop = N // hop_div
    T = len(x) // hop
    x = np.ascontiguousarray(x[:T * hop], np.float32)
    xp = np.concatenate([np.zeros(N - hop, np.float32), x])
    mag, _ = pvref.std_analysis(xp, N, hop, T)
    r = pr.track(mag, N, lags[0], lags[1])
    trk = np.stack([r["f0"], r["strength"]], 1)
    c = pr.correction(trk, a4, mask, 0.5, 1.0)  # causal: c[b] = correction(trk[:b + 1])[-1]
    ratios = np.ones(T, np.float32)
    ratios[1:] = c[:-1].astype(np.float32)
    return ratios, stream(x, N, hop_div, ratios, lock, quality, *LIVE_RANGE)


@functools.lru_cache(maxsize=None)
def live_reference():
    """DESIGN.md §3.14's voice (pitchtrack_ref.e2e_input: N = 1024, hop 256, C major, retune 1,
    locked) corrected live on this reference -> (median cents off the scale before, after): the
    track of the stream's own rows, and of the oracle's rows of the emitted stream behind its latency"""
    import pitchtrack_ref as pr
    N, hop_div = pr.E2E_N, pr.E2E_HOP_DIV
    hop = N // hop_div
    x = pr.e2e_input()
    lags = pr.e2e_lags()
    ratios, y = live_correction(x, N, hop_div, pr.E2E_A4, pr.MAJOR, lags)
    T = len(ratios)
    xp = np.concatenate([np.zeros(N - hop, np.float32), x[:T * hop]])
    mag, _ = pvref.std_analysis(xp, N, hop, T)
    r = pr.track(mag, N, *lags)
    before = pr.median_cents(r["f0"], r["strength"])
    out = np.asarray(y[plan(hop, 0, *LIVE_RANGE)["latency"]:], np.float32)
    frames = pvref.num_frames(len(out), hop)
    mag2, _ = pvref.std_analysis(out, N, hop, frames)
    r2 = pr.track(mag2, N, *lags)
    return before, pr.median_cents(r2["f0"], r2["strength"])
