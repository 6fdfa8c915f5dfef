"""fp64 reference of the variable-rate resampler and of the pitch map built on it (include/pv.h
"variable-rate resampler" and "pitch map"), restated in numpy.

The output is cut into blocks of B samples.  Positions are 64-bit integers in units of 2^-32 input
samples: T_0 = start, T_{b+1} = T_b + B d_b; output m = b B + j reads the input at
t_m = T_b + j d_b, i_m = t_m >> 32, fq_m = t_m & 0xffffffff.  Per block, with the presets of
resample_ref: Sq_b = the largest even integer <= rolloff min(1, 2^32 / d_b) 2^32 (fp64),
s_b = Sq_b / 2^32, W_b = ceil(Z / s_b) and
  y[m] = sum_{j = -W_b+1}^{W_b} x[i_m + j] h_b(j - fq_m / 2^32),
  h_b(tau) = s_b sinc(s_b tau) I0(beta sqrt(1 - u^2)) / I0(beta), u = s_b tau / Z, 0 for |u| >= 1,
x = 0 outside [0, n_in).  Every step 2^32 and a start without a fraction: the shifted copy.

The pitch map: per final output frame u < n a position pos[u] (the tempo curve) and a pitch ratio
ratio[u]; `plan` gives the time map pos_s of the stretch and the steps of the resampling that
follows it, `pitchmap_process` is timemap_ref.timemap_process(pos_s), then `varresample`.
"""
import math

import numpy as np

from ref_cache import array, memo
from resample_ref import PRESETS

ONE = 1 << 32
STEP_MIN, STEP_MAX = 1 << 30, 1 << 34


def ratio_steps(ratio):
    """pv_varresample_steps: d = rint(ratio 2^32) as Python integers"""
    r = np.asarray(ratio, np.float64).reshape(-1)
    if r.size < 1 or not np.all(np.isfinite(r)) or np.any(r < 0.25) or np.any(r > 4.0):
        raise ValueError("ratios must be finite and in [1/4, 4]")
    return [int(v) for v in np.rint(r * 4294967296.0)]


def knots(start, steps, B):
    """T_0 .. T_nblocks as Python integers"""
    T = [int(start)]
    for d in steps:
        T.append(T[-1] + int(B) * int(d))
    return T


def block_filter(d, quality):
    """(Sq, W) of a block with step d"""
    Z, rolloff, _ = PRESETS[quality]
    v = rolloff * min(1.0, 4294967296.0 / float(d)) * 4294967296.0
    Sq = int(math.floor(v)) & ~1
    return Sq, int(math.ceil(Z / (Sq / 4294967296.0)))


def kernel(tau, Sq, quality):
    """h_b(tau) of a block whose cutoff is Sq / 2^32"""
    Z, _, beta = PRESETS[quality]
    s = Sq / 4294967296.0
    tau = np.asarray(tau, np.float64)
    u = s * tau / Z
    inside = np.abs(u) < 1.0
    win = np.i0(beta * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(beta)
    return np.where(inside, s * np.sinc(s * tau) * win, 0.0)


def varresample(x, steps, B, start=0, quality=0, n_out=None):
    """x [..., n_in] -> float64 [..., n_out] (n_out <= len(steps) B, the default)"""
    x = np.asarray(x, np.float64)
    steps = [int(d) for d in steps]
    if any(d < STEP_MIN or d > STEP_MAX for d in steps) or start < 0:
        raise ValueError("a step outside [2^30, 2^34] or a negative start")
    length = len(steps) * B
    n_out = length if n_out is None else int(n_out)
    assert 0 <= n_out <= length
    n_in = x.shape[-1]
    y = np.zeros(x.shape[:-1] + (n_out,), np.float64)
    if all(d == ONE for d in steps) and start % ONE == 0:
        s0 = start // ONE
        k = max(0, min(n_out, n_in - s0))
        y[..., :k] = x[..., s0:s0 + k]
        return y
    T = knots(start, steps, B)
    for b, d in enumerate(steps):
        m0 = b * B
        if m0 >= n_out:
            break
        nj = min(B, n_out - m0)
        t = [T[b] + j * d for j in range(nj)]
        i = np.array([v >> 32 for v in t], np.int64)
        f = np.array([v & (ONE - 1) for v in t], np.float64) / 4294967296.0
        Sq, W = block_filter(d, quality)
        for j in range(-W + 1, W + 1):
            idx = i + j
            ok = (idx >= 0) & (idx < n_in)
            xv = np.where(ok, x[..., np.clip(idx, 0, max(n_in - 1, 0))], 0.0) if n_in else 0.0
            y[..., m0:m0 + nj] += xv * kernel(j - f, Sq, quality)
    return y


# ---------------------------------------------------------------- the pitch map's plan
def plan(N, hop, pos, ratio):
    """pv_pitchmap_plan: (pos_s float64 [n_s], steps as Python integers [nb])"""
    pos = np.asarray(pos, np.float64).reshape(-1)
    ratio = np.asarray(ratio, np.float64).reshape(-1)
    n = pos.size
    if n < 1 or ratio.size != n or n * hop >= 1 << 28:
        raise ValueError("bad map length")
    if not np.all(np.isfinite(pos)) or np.any(pos < 0) or np.any(pos >= 2.0 ** 30):
        raise ValueError("positions must be finite, >= 0 and < 2^30")
    d = ratio_steps(ratio)
    L = n * hop + N - hop
    nb = -(-L // hop)
    steps = d + [d[-1]] * (nb - n)
    S = knots(0, d, hop)  # Sigma_0 .. Sigma_n
    unit = hop * ONE
    n_s = max(1, -(-S[n] // unit))
    pos_s = np.empty(n_s, np.float64)
    b = 0
    for v in range(n_s):
        t = v * unit
        while b < n - 1 and t >= S[b + 1]:
            b += 1
        w = float(t - S[b]) / float(S[b + 1] - S[b])
        p0, p1 = pos[b], pos[min(b + 1, n - 1)]
        pos_s[v] = p0 + w * (p1 - p0)
    return pos_s, steps


def pitchmap_process(x, N, hop_div, pos_s, steps, lock, frames=None, quality=0, n=None):
    """One channel: the time-map stretch at pos_s, then the variable-rate resampling by `steps` in
    blocks of hop, cut to the n hop + N - hop samples of the final output (n: final frames;
    default: every block)."""
    import timemap_ref as tm
    hop = N // hop_div
    mid = tm.cached(x, N, hop_div, pos_s, lock, frames)
    n_out = len(steps) * hop if n is None else n * hop + N - hop
    return varresample(mid, steps, hop, 0, quality, n_out)


@memo(x=array(np.float32), pos_s=array(np.float64), steps=array(np.int64), lock=bool)
def cached(x, N, hop_div, pos_s, steps, lock, frames=None, quality=0, n=None):
    """pitchmap_process, computed once per (input, configuration, plan) and shared read-only."""
    return pitchmap_process(x, N, hop_div, pos_s, steps, lock, frames, quality, n)


# ---------------------------------------------------------------- maps
def glide(n, r0, r1):
    """a geometric glide of the ratio from r0 (first entry) to r1 (last entry)"""
    if n == 1:
        return np.array([r0], np.float64)
    return (r0 * (r1 / r0) ** (np.arange(n) / (n - 1.0))).astype(np.float64)


def vibrato(n, depth=0.06, period=23.0):
    """a ratio swinging by +-depth around 1"""
    return (1.0 + depth * np.sin(2.0 * np.pi * np.arange(n) / period)).astype(np.float64)
