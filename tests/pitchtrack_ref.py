"""fp64 reference of the pitch tracker and of the correction planner (DESIGN.md §3.14,
include/pv.h pv_pitch_track / pv_pitch_correct_plan), restated in numpy from what the oracle
exports: the analysis rows' fp32 magnitudes (pvref.std_analysis, the GPU's bit for bit).

Frame: mx = max mag (NaN counts as 0); s = 2^-exponent(mx) from mx's fp32 bits; P = (mag s)^2;
r = irfft(P, N); rho[n] = r[n] / (r[0] g[n]), g[n] = 2/3 + cos(2 pi n / N) / 3; candidates are the
lags of [tau_min, tau_max] with rho[n] > rho[n-1], rho[n] >= rho[n+1], rho[n] > 0; the pick is
the smallest candidate with rho >= kappa top; a parabola through its neighbours gives
{1 / (tau + d), strength}.  `track` also returns the margins by which the pick was decided
(`clear`), and takes dtype=np.float32 to run the same steps in fp32 (the restatement that sizes
the GPU test's tolerance).
"""
import functools

import numpy as np

TWO_PI = 2.0 * np.pi
KAPPA = 0.9           # PV_PITCH_TRACK_DEFAULT_KAPPA
CLEAR_MARGIN = 1e-3   # of top: a comparison that holds or fails by less is not clear
# The tolerance of tests/test_gpu_pitchtrack.py on frames with equal lags: ten times the worst
# error of the fp32 restatement (track(..., dtype=np.float32)) against the fp64 reference over the
# parity cases' rows (measured, tests/test_pitchtrack_ref.py: f0 9.9e-8 relative, strength 1.7e-7
# absolute)
F0_TOL = 1.0e-6
STRENGTH_TOL = 1.7e-6


def _scale(mx32):
    """s = 2^-e, e the exponent of the fp32 mx from its bits, taken as at most 126"""
    b = (np.asarray(mx32, np.float32).view(np.uint32) >> 23).astype(np.int64)  # (the sign is 0)
    sbe = np.maximum(254 - b, 1)
    return (sbe.astype(np.uint32) << 23).view(np.float32)


def normalised_autocorrelation(mag, N, dtype=np.float64):
    """rho [frames, N/2 + 1] of the fp32 magnitude rows mag [frames, N/2 + 1], and `ok`
    [frames]: False where the frame's result is {0, 0} (no magnitude, a non-finite maximum, or
    r[0] not above 0; rho is 0 there)."""
    m32 = np.asarray(mag, np.float32)
    L = N // 2
    assert m32.ndim == 2 and m32.shape[1] == L + 1
    with np.errstate(invalid="ignore", over="ignore"):
        clean = np.where(m32 >= 0, m32, np.float32(0))  # maxNum against 0: NaN -> 0
        mx = clean.max(axis=1)
        ok = (mx > 0) & np.isfinite(mx)
        s = _scale(np.where(ok, mx, np.float32(1)))
        a = np.where(ok[:, None], clean * s[:, None], np.float32(0)).astype(dtype)  # (exact in fp32)
        P = a * a
        r = np.fft.irfft(P, N, axis=1)[:, :L + 1]
        assert r.dtype == dtype
        ok &= r[:, 0] > 0
        n = np.arange(L + 1)
        g = (dtype(2) + np.cos(dtype(TWO_PI) * n.astype(dtype) / dtype(N))) / dtype(3)
        r0 = np.where(ok, r[:, 0], dtype(1))
        rho = np.where(ok[:, None], r / (r0[:, None] * g[None, :]), dtype(0))
    return rho.astype(dtype), ok


def track(mag, N, tau_min, tau_max, kappa=KAPPA, dtype=np.float64):
    """-> dict of per-frame arrays: f0, strength (dtype), tau (int, 0: no pick), top, and clear
    (bool): every comparison that decided the pick held, or failed, by CLEAR_MARGIN top —
    the kappa top test of every candidate up to and including the chosen one, and the
    local-maximum tests of every lag at or below the chosen one whose rho reaches
    (kappa - CLEAR_MARGIN) top.  A frame without a pick is clear iff it has no magnitude."""
    L = N // 2
    assert 2 <= tau_min <= tau_max <= L - 1 and 0 < kappa <= 1
    rho, ok = normalised_autocorrelation(mag, N, dtype)
    T = rho.shape[0]
    f0 = np.zeros(T, dtype)
    strength = np.zeros(T, dtype)
    tau = np.zeros(T, np.int64)
    top = np.zeros(T, dtype)
    clear = np.zeros(T, bool)
    kap = dtype(kappa)
    lags = np.arange(tau_min, tau_max + 1)
    for t in range(T):
        if not ok[t]:
            m = np.asarray(mag[t], np.float32)
            clear[t] = not np.any(m > 0)
            continue
        x = rho[t]
        here, before, after = x[lags], x[lags - 1], x[lags + 1]
        cand = (here > before) & (here >= after) & (here > 0)
        if not cand.any():
            continue
        tp = here[cand].max()
        top[t] = tp
        q = cand & (here >= kap * tp)
        j = int(np.argmax(q))  # the first one
        n = int(lags[j])
        tau[t] = n
        a, b, c = x[n - 1], x[n], x[n + 1]
        d = (a - c) / (dtype(2) * (a - dtype(2) * b + c))
        f0[t] = dtype(1) / (dtype(n) + d)
        strength[t] = b - (a - c) * d / dtype(4)
        # ---- the margins (fp64 whatever dtype is)
        h, bf, af = (v[:j + 1].astype(np.float64) for v in (here, before, after))
        tp64, k64, mg = float(tp), float(kappa), CLEAR_MARGIN * float(tp)
        is_max = (h >= bf + mg) & (h >= af + mg) & (h >= mg)
        not_max = (h <= bf - mg) | (h <= af - mg) | (h <= -mg)
        near = h >= (k64 - CLEAR_MARGIN) * tp64
        good = np.all(~near | is_max | not_max)
        cj = cand[:j + 1]
        good &= bool(np.all(h[:j][cj[:j]] <= k64 * tp64 - mg))
        good &= bool(h[j] >= k64 * tp64 + mg)
        clear[t] = good
    return {"f0": f0, "strength": strength, "tau": tau, "top": top, "clear": clear}


def lag_of(f0):
    """the integer lag behind an f0 (|d| <= 1/2): round(1 / f0), 0 where f0 is 0 or not finite"""
    f0 = np.asarray(f0, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(np.isfinite(f0) & (f0 > 0), 1.0 / f0, 0.0)
    return np.floor(p + 0.5).astype(np.int64)


# ---------------------------------------------------------------- the planner
CHROMATIC = 0xFFF
MAJOR = 0xAB5


def correction(trk, a4, mask, strength_min=0.5, retune=1.0, pos=None):
    """pv_pitch_correct_plan: track [frames, 2] {f0, strength} -> ratio float64 [n]"""
    trk = np.asarray(trk, np.float32).astype(np.float64)
    frames = trk.shape[0]
    if frames < 1 or not (a4 > 0 and np.isfinite(a4)) or not 0 < mask < 4096 or np.isnan(strength_min) \
            or not 0 < retune <= 1:
        raise ValueError("bad argument")
    pos = np.arange(frames, dtype=np.float64) if pos is None else np.asarray(pos, np.float64).reshape(-1)
    if pos.size < 1 or not np.all(np.isfinite(pos)):
        raise ValueError("bad positions")
    ratio = np.empty(pos.size, np.float64)
    s = 0.0
    for u in range(pos.size):
        t = int(min(max(np.floor(pos[u] + 0.5), 0.0), frames - 1.0))
        f0, st = trk[t]
        c = s
        if np.isfinite(f0) and f0 > 0 and st >= strength_min:
            note = 69.0 + 12.0 * np.log2(f0 / a4)
            if np.isfinite(note):
                lo, hi = int(np.floor(note)), int(np.ceil(note))
                while not (mask >> (lo % 12)) & 1:
                    lo -= 1
                while not (mask >> (hi % 12)) & 1:
                    hi += 1
                target = lo if note - lo <= hi - note else hi
                c = (target - note) / 12.0
        s = s + retune * (c - s)
        ratio[u] = min(4.0, max(0.25, 2.0 ** s))
    return ratio


def cents_off_scale(f0, a4, mask):
    """distance of every f0 > 0 to the nearest allowed semitone, in cents (NaN where f0 <= 0)"""
    f0 = np.asarray(f0, np.float64)
    out = np.full(f0.shape, np.nan)
    for i, f in enumerate(f0):
        if np.isfinite(f) and f > 0:
            note = 69.0 + 12.0 * np.log2(f / a4)
            lo, hi = int(np.floor(note)), int(np.ceil(note))
            while not (mask >> (lo % 12)) & 1:
                lo -= 1
            while not (mask >> (hi % 12)) & 1:
                hi += 1
            out[i] = 100.0 * min(note - lo, hi - note)
    return out


# ---------------------------------------------------------------- signals
HARMONICS = 12


def voice(n, f0, seed, noise=0.0, vibrato_cents=0.0, vibrato_period=4000.0, glide_octaves=0.0):
    """12 harmonics (amplitudes 1 / h, random phases) of a fundamental f0 (cycles per sample)
    that swings by +-vibrato_cents with the given period in samples and glides up by
    glide_octaves over the signal; peak 0.5; Gaussian noise of the given deviation added.
    -> (x float32, the instantaneous f0 per sample float64)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f = f0 * 2.0 ** (vibrato_cents / 1200.0 * np.sin(TWO_PI * t / vibrato_period) + glide_octaves * t / n)
    ph = TWO_PI * np.concatenate([[0.0], np.cumsum(f)[:-1]])
    x = np.zeros(n)
    for h in range(1, HARMONICS + 1):
        x += np.sin(h * ph + rng.uniform(0, TWO_PI)) / h
    x *= 0.5 / np.max(np.abs(x))
    if noise:
        x += rng.normal(0.0, noise, n)
    return x.astype(np.float32), f


def white(n, seed):
    """full-scale uniform white noise"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def frame_f0(f, N, hop, frames):
    """the true f0 of every frame: the instantaneous f0 at the frame's centre"""
    idx = np.minimum(np.arange(frames) * hop + N // 2, len(f) - 1)
    return f[idx]


# ---- the three channels of the GPU parity test (tests/test_gpu_pitchtrack.py) and of the CPU
# test that sizes its tolerance: a voice with vibrato, the same with noise 0.05, white noise
PARITY_F0 = 0.023     # a period of 43.5 samples: inside [8, N/4] at every N
PARITY_FRAMES = 45
PARITY_SIZES = (256, 512, 1024, 2048)


def parity_ranges(N):
    return ((8, N // 4), (2, N // 2 - 1))


@functools.lru_cache(maxsize=None)
def parity_inputs(N):
    hop = N // 4
    n = PARITY_FRAMES * hop + 13  # not a multiple of the hop
    v, _ = voice(n, PARITY_F0, 11, vibrato_cents=50.0, vibrato_period=9.3 * N)
    vn, _ = voice(n, PARITY_F0, 11, noise=0.05, vibrato_cents=50.0, vibrato_period=9.3 * N)
    xs = np.stack([v, vn, white(n, 12 + N)])
    xs.setflags(write=False)
    return xs


# ---- the end-to-end correction (tests/test_pitchtrack_ref.py, tests/test_gpu_pitchtrack.py):
# a voice held 35 cents under E4 of A4 = 440 Hz at 44.1 kHz, +-15 cents of slow vibrato
E2E_N, E2E_HOP_DIV, E2E_FRAMES = 1024, 4, 62
E2E_A4 = 440.0 / 44100.0
E2E_NOTE = 64         # E4, in C major
E2E_OFF_CENTS = -35.0
E2E_RANGE = (0.004, 0.02)  # fmin, fmax: lags 50 .. 250
E2E_EDGE = 6          # frames left out at either end: 50 frames, one period of the vibrato, remain


@functools.lru_cache(maxsize=None)
def e2e_input():
    hop = E2E_N // E2E_HOP_DIV
    n = E2E_FRAMES * hop + 13
    f0 = E2E_A4 * 2.0 ** ((E2E_NOTE - 69 + E2E_OFF_CENTS / 100.0) / 12.0)
    x, _ = voice(n, f0, 21, vibrato_cents=15.0, vibrato_period=50.0 * hop)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """the whole loop on the CPU: the oracle's rows -> track -> correction(retune = 1) ->
    tests/varresample_ref.py's plan and pitchmap_process (phase lock on) -> the oracle's rows of
    the output -> track.  -> (median cents before, median cents after)"""
    import pvref
    import varresample_ref as vr
    N, hop = E2E_N, E2E_N // E2E_HOP_DIV
    x = e2e_input()
    frames = pvref.num_frames(x.shape[0], hop)
    assert frames == E2E_FRAMES
    lo, hi = e2e_lags()
    mag, _ = pvref.std_analysis(x, N, hop, frames)
    r = track(mag, N, lo, hi)
    before = median_cents(r["f0"], r["strength"])
    ratio = correction(np.stack([r["f0"], r["strength"]], 1), E2E_A4, MAJOR, 0.5, 1.0)
    pos_s, steps = vr.plan(N, hop, np.arange(frames, dtype=np.float64), ratio)
    y = np.asarray(vr.pitchmap_process(x, N, E2E_HOP_DIV, pos_s, steps, True, frames, 0, frames), np.float32)
    mag2, _ = pvref.std_analysis(y, N, hop, frames)
    r2 = track(mag2, N, lo, hi)
    return before, median_cents(r2["f0"], r2["strength"])


def e2e_lags():
    return int(np.ceil(1.0 / E2E_RANGE[1])), int(np.floor(1.0 / E2E_RANGE[0]))


def median_cents(f0, strength, strength_min=0.5):
    """median distance to the C-major scale, in cents, over the voiced frames away from the ends"""
    f0, strength = np.asarray(f0, np.float64), np.asarray(strength, np.float64)
    sel = slice(E2E_EDGE, len(f0) - E2E_EDGE)
    c = cents_off_scale(f0[sel], E2E_A4, MAJOR)
    v = (f0[sel] > 0) & (strength[sel] >= strength_min)
    assert v.sum() >= (len(f0) - 2 * E2E_EDGE) // 2
    return float(np.median(c[v]))
