"""fp64 reference of the time-map stretch (include/pv.h pv_timemap_process),
restated in numpy from the oracle's bit-exact analysis rows (pvref.std_analysis).  Output frame
u is built at the analysis position pos[u] = i_u + a_u with the synthesis hop equal to the
analysis hop:

  P(i)      = ((uint32)(int32) rint(fp32(phi(i) * (1/2pi)) * 2^31)) << 1    a fraction of a turn
  Phi(0)    = P(i_0),  Phi(u+1) = Phi(u) + Delta(i_u)                        modulo 2^32
  Delta(i)  = P(i+1) - P(i) for i + 1 < frames,  Delta(frames-1) = 0
  m(u)      = fmaf(a_u, mag(i_u+1) - mag(i_u), mag(i_u)) in fp32; row `frames` is magnitude 0
  Psi       = Phi(u), or locked: P(i_u) + (Phi(u) - P(i_u))[own], peaks / owners on m(u)
  Y         = m(u) exp(2 pi i Psi / 2^32)

With the identity map it reproduces pvref.std_process at scale 1 (tests/test_timemap_ref.py),
which is what makes it a yardstick for the other maps.
"""
import numpy as np

import pvref
from phase_lock_ref import owners, peaks
from ref_cache import array, memo

TWO_PI = 2.0 * np.pi
INV_2PI = np.float32(float.fromhex("0x1.45f306p-3"))  # kInv2Pi (pv_device.hpp)
MASK = np.int64(0xFFFFFFFF)


def split(pos):
    """positions -> (floor as int64, fraction as float32): pv_timemap_split's definition"""
    pos = np.asarray(pos, np.float64).reshape(-1)
    if pos.size < 1 or not np.all(np.isfinite(pos)) or np.any(pos < 0) or np.any(pos >= 2.0 ** 30):
        raise ValueError("positions must be finite, >= 0 and < 2^30")
    fl = np.floor(pos)
    return fl.astype(np.int64), (pos - fl).astype(np.float32)


def phase_turns(ph):
    """fp32 phases -> P as int64 in [0, 2^32)"""
    t = np.asarray(ph, np.float32) * INV_2PI              # one fp32 multiply
    r = np.rint(t.astype(np.float64) * 2.0 ** 31)          # exact scaling, ties to even
    return (r.astype(np.int64) << 1) & MASK


def deltas(P):
    """P [frames, B] -> Delta [frames, B]: P(i+1) - P(i) modulo 2^32, 0 for the last row"""
    D = np.zeros_like(P)
    D[:-1] = (P[1:] - P[:-1]) & MASK
    return D


def scan(P, idx, run=None):
    """Phi [n_out, B] of the map's frames.  run=None: the sequential sum.  run=F: per-run sums of
    Delta(i_u), an exclusive scan of them from P(i_0) (the carries), then each run from its carry —
    the kernels' order (k_map_sum, k_map_carry, k_synthesis)."""
    D = deltas(P)
    n = idx.shape[0]
    Phi = np.zeros((n, P.shape[1]), np.int64)
    if run is None:
        acc = P[idx[0]].copy()
        for u in range(n):
            Phi[u] = acc
            acc = (acc + D[idx[u]]) & MASK
        return Phi
    nruns = (n + run - 1) // run
    sums = [np.sum(D[idx[r * run:(r + 1) * run]], axis=0) & MASK for r in range(nruns)]
    carry = P[idx[0]].copy()
    for r in range(nruns):
        acc = carry.copy()
        for u in range(r * run, min(n, (r + 1) * run)):
            Phi[u] = acc
            acc = (acc + D[idx[u]]) & MASK
        carry = (carry + sums[r]) & MASK
    return Phi


def lerp32(a, m0, m1):
    """fmaf(a, m1 - m0, m0) in fp32: the fp32 difference, the exact product in float64, one add,
    then the rounding to fp32"""
    d = (np.asarray(m1, np.float32) - np.asarray(m0, np.float32)).astype(np.float64)
    return (np.float64(np.float32(a)) * d + np.asarray(m0, np.float32).astype(np.float64)).astype(np.float32)


def output_phases(mag, P, pos, lock, run=None):
    """(m [n_out, B] fp32, Psi [n_out, B] int64 in [0, 2^32)) of every output frame"""
    idx, frac = split(pos)
    frames, B = P.shape
    if idx.max() > frames - 1:
        raise ValueError("the map reads past the last analysed frame")
    Phi = scan(P, idx, run)
    zero = np.zeros(B, np.float32)
    m = np.empty((idx.shape[0], B), np.float32)
    Psi = np.empty((idx.shape[0], B), np.int64)
    for u, (i, a) in enumerate(zip(idx, frac)):
        m[u] = lerp32(a, mag[i], mag[i + 1] if i + 1 < frames else zero)
        if lock:
            own = owners(peaks(m[u]))
            Psi[u] = (P[i] + ((Phi[u] - P[i]) & MASK)[own]) & MASK
        else:
            Psi[u] = Phi[u]
    return m, Psi


def timemap_process(x, N, hop_div, pos, lock, frames=None):
    """The time-map stretch of one channel (float32 samples) -> float64 output of
    n_out * hop + N - hop samples."""
    x = np.ascontiguousarray(x, np.float32)
    hop = N // hop_div
    if frames is None:
        frames = pvref.num_frames(x.shape[0], hop)
    mag, ph = pvref.std_analysis(x, N, hop, frames)
    m, Psi = output_phases(mag, phase_turns(ph), pos, lock)
    n_out = m.shape[0]
    i = np.arange(N, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(TWO_PI * i / N)
    g = w * (hop / np.sum(w * w))  # (np.fft.irfft carries the 1 / N)
    out = np.zeros(n_out * hop + (N - hop), np.float64)
    signed = np.where(Psi >= 2 ** 31, Psi - 2 ** 32, Psi).astype(np.float64)  # (int32)Psi
    for u in range(n_out):
        Y = m[u].astype(np.float64) * np.exp(1j * (TWO_PI * signed[u] / 2.0 ** 32))
        out[u * hop:u * hop + N] += np.fft.irfft(Y, N) * g
    return out


@memo(x=array(np.float32), pos=array(np.float64), lock=bool)
def cached(x, N, hop_div, pos, lock, frames=None):
    """timemap_process, computed once per (input, configuration, map) and shared read-only."""
    return timemap_process(x, N, hop_div, pos, lock, frames)


# ---------------------------------------------------------------- maps
def rate_map(frames, rate):
    """pvamd.rate_map's definition"""
    return np.arange(0, frames - 1 + 1e-9, rate).astype(np.float64)


def ramp_map(frames, r0, r1):
    """a tempo curve: the playback rate goes linearly with the position from r0 at frame 0 to r1
    at frame frames - 1; pos[0] = 0, pos[u+1] = pos[u] + rate(pos[u]), while pos <= frames - 1"""
    last = float(frames - 1)
    pos = [0.0]
    while True:
        nxt = pos[-1] + r0 + (r1 - r0) * pos[-1] / last
        if nxt > last:
            break
        pos.append(nxt)
    return np.array(pos, np.float64)


def scrub_map():
    """a fractional start, a freeze, a reverse, and the last of 60 rows three times"""
    fwd = np.arange(20) + 0.5
    freeze = np.full(10, 20.0)
    back = np.arange(19.25, 5.0 - 1e-9, -0.75)
    return np.concatenate([fwd, freeze, back, [59.0, 59.0, 59.0]]).astype(np.float64)
