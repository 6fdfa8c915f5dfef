"""fp64 reference of the real-time harmoniser (include/pv.h pv_rt_harmonizer_push):
per voice the real-time pitch map's stream (tests/rt_pitchmap_ref.py, shared through its memo), the
gain ramp and the sum, as defined there.

One channel, V voices, T pushed frames (T hop samples; ratios and gains [V, T] float32):
  voice   y_v = rt_pitchmap_ref.stream(x, ratios[v]): blocks 0 .. T - 2 - G behind (G + 1) hop zeros
  gain    the gain pushed with frame t >= 1 belongs to block b = t - 1, as the step does; a NaN reads
          as 0; frame 0's is ignored.  g(j) = g_prev + (j + 1) / hop (g_b - g_prev), g_prev = g_{b-1},
          g_{-1} = g_0
  mix     sum over v of g_v(j) y_v[j]
"""
import numpy as np

import rt_pitchmap_ref as rm


def block_gains(gains):
    """gains [T] of the pushed frames -> g_0 .. g_{T-2} float64 (fp32 values; a NaN reads as 0)"""
    g = np.asarray(gains, np.float32).reshape(-1)[1:].astype(np.float64)
    return np.where(np.isnan(g), 0.0, g)


def ramp32(gains, hop):
    """the definition's own fp32 ramp: [T - 1, hop] float32,
    g(j) = fmaf((float)(j + 1) * (1.0f / (float)hop), g_b - g_prev, g_prev)"""
    g = block_gains(gains).astype(np.float32)
    prev = np.concatenate([g[:1], g[:-1]])
    fr = (np.arange(1, hop + 1, dtype=np.float32) * (np.float32(1.0) / np.float32(hop))).astype(np.float32)
    diff = (g - prev).astype(np.float32)
    return fma32(fr[None, :], diff[:, None], prev[:, None])


def fma32(a, b, c):
    """fmaf on float32 arrays, one rounding: the product is exact in fp64; the fp64 sum is rounded
    to odd (TwoSum gives its error), after which the rounding to fp32 is that of the exact sum"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.int64)
    fix = (e != 0.0) & ((bits & 1) == 0)
    away = (e > 0.0) == (s > 0.0)  # the exact sum lies further from zero than s
    bits += np.where(fix, np.where(away, 1, -1), 0)
    return bits.view(np.float64).astype(np.float32)


def ramp64(gains, hop):
    """the ramp in fp64 from the fp32 gains: [T - 1, hop]"""
    g = block_gains(gains)
    prev = np.concatenate([g[:1], g[:-1]])
    fr = np.arange(1, hop + 1, dtype=np.float64) / hop
    return prev[:, None] + fr[None, :] * (g - prev)[:, None]


def gain_stream(gains, hop, G, ramp=ramp64):
    """the gain of every emitted sample: [T hop]; 0 over the (G + 1) hop samples of latency, then
    blocks 0 .. T - 2 - G"""
    T = np.asarray(gains).reshape(-1).shape[0]
    out = np.zeros(T * hop, np.float64)
    nb = T - 1 - G
    if nb > 0:
        out[(G + 1) * hop:] = ramp(gains, hop)[:nb].reshape(-1)
    return out


def prev_stream(gains, hop, G):
    """g_prev of every emitted sample, laid out as gain_stream: [T hop] float64"""
    g = block_gains(gains)
    prev = np.concatenate([g[:1], g[:-1]])
    return gain_stream(gains, hop, G, ramp=lambda _g, h: np.repeat(prev[:, None], h, axis=1))


def voices(x, N, hop_div, ratios, lock, quality=0, ratio_min=0.5, ratio_max=2.0):
    """[V, T hop] float64: every voice's own stream (read-only views of the shared memo)"""
    return np.stack([rm.cached(x, N, hop_div, np.asarray(r, np.float32), lock, quality, ratio_min, ratio_max)
                     for r in np.asarray(ratios, np.float32)])


def stream(x, N, hop_div, ratios, gains, lock, quality=0, ratio_min=0.5, ratio_max=2.0):
    """x [T hop] float32, ratios and gains [V, T] -> (mix [T hop], voices [V, T hop]) float64"""
    hop = N // hop_div
    ys = voices(x, N, hop_div, ratios, lock, quality, ratio_min, ratio_max)
    G = rm.plan(hop, quality, ratio_min, ratio_max)["G"]
    mix = np.zeros(ys.shape[1], np.float64)
    for y, g in zip(ys, np.asarray(gains, np.float32)):
        mix += gain_stream(g, hop, G) * y
    return mix, ys


# ---------------------------------------------------------------- the chord
CHORD_N, CHORD_HOP_DIV, CHORD_T = 1024, 4, 64
CHORD_FREQ, CHORD_AMP = 0.05, 0.5
CHORD_SEMITONES = (0, 4, 7)
CHORD_GAINS = (0.5, 0.3, 0.2)
CHORD_SEG = 8192
CHORD_BIN_TOL, CHORD_AMP_FLOOR = 0.02, 0.98  # §3.13's bound for a tone


def chord_input():
    hop = CHORD_N // CHORD_HOP_DIV
    return (CHORD_AMP * np.sin(2.0 * np.pi * CHORD_FREQ * np.arange(CHORD_T * hop))).astype(np.float32)


def chord_controls():
    """ratios and gains [3, T] float32"""
    r = np.exp2(np.asarray(CHORD_SEMITONES, np.float64) / 12.0).astype(np.float32)
    return (np.tile(r[:, None], (1, CHORD_T)).astype(np.float32),
            np.tile(np.asarray(CHORD_GAINS, np.float32)[:, None], (1, CHORD_T)).astype(np.float32))


def tone_peak(seg, f0):
    """(frequency in cycles / sample, amplitude) of the sinusoid nearest f0 in a Hann-windowed
    segment: the maximum of the windowed DTFT's magnitude within half an analysis bin of f0 (golden
    section on |X(f)|; the Hann window's coherent gain is 1/2)"""
    n = len(seg)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
    xs = np.asarray(seg, np.float64) * w
    t = np.arange(n)

    def mag(f):
        return abs(np.sum(xs * np.exp(-2j * np.pi * f * t)))

    half = 0.5 / CHORD_N
    grid = np.linspace(f0 - half, f0 + half, 65)
    k = int(np.argmax([mag(f) for f in grid]))
    lo, hi = grid[max(k - 1, 0)], grid[min(k + 1, len(grid) - 1)]
    phi = (np.sqrt(5.0) - 1.0) / 2.0
    a, b = hi - phi * (hi - lo), lo + phi * (hi - lo)
    fa, fb = mag(a), mag(b)
    for _ in range(60):
        if fa < fb:
            lo, a, fa = a, b, fb
            b = lo + phi * (hi - lo)
            fb = mag(b)
        else:
            hi, b, fb = b, a, fa
            a = hi - phi * (hi - lo)
            fa = mag(a)
    f = 0.5 * (lo + hi)
    return f, mag(f) / (0.5 * np.sum(w))


def chord_peaks(mix, latency):
    """[(offset from 0.05 ratio in analysis bins (1 / N), amplitude / (gain 0.5))] of the three
    voices in the mix's segment of CHORD_SEG samples starting 2 N after the latency"""
    r, _ = chord_controls()
    seg = np.asarray(mix, np.float64)[latency + 2 * CHORD_N:latency + 2 * CHORD_N + CHORD_SEG]
    assert len(seg) == CHORD_SEG
    out = []
    for v, g in enumerate(CHORD_GAINS):
        f0 = CHORD_FREQ * float(r[v, 0])
        f, a = tone_peak(seg, f0)
        out.append(((f - f0) * CHORD_N, a / (g * CHORD_AMP)))
    return out
