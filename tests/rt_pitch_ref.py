"""fp64 reference of the real-time pitch shift's streaming resampler (include/pv.h
pv_rt_pitch_push), built on tests/resample_ref.py.

S[n], n >= 0, is the stretched stream (0 for n < 0), P/Q = out_hop / hop reduced.  For every
integer m, negative included, y[m] = sum_{j = -W+1}^{W} S[i_m + j] h(j - r_m / Q) with
i_m = floor(m P / Q) and r_m = m P mod Q; the emitted stream is z[m'] = y[m' - D], m' >= 0,
D = floor(W Q / P).  Prefixing S with a P zeros moves y by exactly a Q outputs and leaves every
phase as it is, so the offline resampler gives y at negative m too.
"""
import numpy as np

import resample_ref as rr
from phase_lock_ref import chirp, std_process_lock


def latency(hs, hop, quality=0):
    """D = floor(W Q / P) output samples (0 at ratio 1)"""
    P, Q = rr.reduce_ratio(hs, hop)
    if P == Q:
        return 0
    return (rr.half_width(P, Q, quality) * Q) // P


def stream_reference(S, hs, hop, quality=0):
    """S [..., n] stretched samples -> float64 z [..., >= floor(n Q / P)]: the stream a
    pv_rt_pitch_push sequence emits.  z[m'] is final (what an endless S would give) for
    m' < floor(n / hs) * hop."""
    S = np.asarray(S, np.float64)
    P, Q = rr.reduce_ratio(hs, hop)
    D = latency(hs, hop, quality)
    a = -(-D // Q)  # any a with a Q >= D
    xp = np.concatenate([np.zeros(S.shape[:-1] + (a * P,)), S], axis=-1)
    return rr.resample(xp, P, Q, quality)[..., a * Q - D:]


# mean_envelope (phase_lock_ref) of the fp64 real-time streams of the 0.5-amplitude chirp shifted
# by 1.5 at N = 256, hop 64 (rt_chirp_reference: 96 callbacks, 3:2 fast preset, latency 19);
# tests/test_rt_pitch_ref.py recomputes them, tests/test_gpu_rt_pitch.py holds the GPU to them.
# The offline figures are 0.484 and 0.338.
RT_CHIRP_LOCKED = 0.48356
RT_CHIRP_UNLOCKED = 0.34609


def rt_chirp_reference(lock, N=256, hop_div=4, scale=1.5):
    """the stream pv_rt_pitch_push emits for phase_lock_ref.chirp(), one frame per hop"""
    hop = N // hop_div
    hs = int(scale * hop)
    x = chirp()
    K = len(x) // hop
    xp = np.concatenate([np.zeros(N - hop, np.float32), x[:K * hop]])
    S = std_process_lock(xp, N, hop_div, scale, lock, frames=K)[:K * hs]
    return stream_reference(S, hs, hop, 0)[:K * hop]
