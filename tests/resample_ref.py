"""fp64 reference of the band-limited polyphase resampler (include/pv.h "resampler", DESIGN.md
§3.8), restated in numpy.

P/Q is reduced by its gcd.  Output m sits at input position m P / Q: i_m = floor(m P / Q),
r_m = (m P) mod Q (exact integers), n_out = ceil(n_in Q / P).  With s = rolloff min(1, Q/P),
W = ceil(Z / s) and h(tau) = s sinc(s tau) I0(beta sqrt(1 - u^2)) / I0(beta), u = s tau / Z
(0 for |u| >= 1):  y[m] = sum_{j = -W+1}^{W} x[i_m + j] h(j - r_m / Q), x = 0 outside [0, n_in).
Ratio 1 is a copy.
"""
import math

import numpy as np

# quality -> (Z, rolloff, Kaiser beta)
PRESETS = {0: (16, 0.85, 8.555504641634386), 1: (64, 0.9475937167399596, 14.769656459379492)}


def reduce_ratio(p, q):
    g = math.gcd(int(p), int(q))
    return int(p) // g, int(q) // g


def half_width(p, q, quality=0):
    """W of the reduced ratio p/q"""
    P, Q = reduce_ratio(p, q)
    Z, rolloff, _ = PRESETS[quality]
    return int(math.ceil(Z / (rolloff * min(1.0, Q / P))))


def out_length(p, q, n_in):
    P, Q = reduce_ratio(p, q)
    return 0 if n_in <= 0 else (int(n_in) * Q + P - 1) // P


def kernel(tau, p, q, quality=0):
    """h(tau) for the reduced ratio p/q, float64 array in, float64 out"""
    P, Q = reduce_ratio(p, q)
    Z, rolloff, beta = PRESETS[quality]
    s = rolloff * min(1.0, Q / P)
    tau = np.asarray(tau, np.float64)
    u = s * tau / Z
    inside = np.abs(u) < 1.0
    win = np.i0(beta * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(beta)
    return np.where(inside, s * np.sinc(s * tau) * win, 0.0)


def resample(x, p, q, quality=0):
    """x [..., n_in] -> float64 [..., n_out]"""
    x = np.asarray(x, np.float64)
    P, Q = reduce_ratio(p, q)
    if P == Q:
        return x.copy()
    n_in = x.shape[-1]
    n_out = out_length(P, Q, n_in)
    W = half_width(P, Q, quality)
    m = np.arange(n_out, dtype=np.int64)
    i = (m * P) // Q
    frac = ((m * P) % Q).astype(np.float64) / Q
    xp = np.concatenate([np.zeros(x.shape[:-1] + (W,)), x, np.zeros(x.shape[:-1] + (W + 1,))], axis=-1)
    y = np.zeros(x.shape[:-1] + (n_out,), np.float64)
    for j in range(-W + 1, W + 1):
        y += xp[..., i + j + W] * kernel(j - frac, P, Q, quality)
    return y
