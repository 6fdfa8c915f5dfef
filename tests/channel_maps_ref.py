"""Per-channel references of the maps set per channel (a helper: no tests in
here): channel c of a batched call is what the single-map references give that channel with its
own map — tests/timemap_ref.py, tests/varresample_ref.py — followed, for a time map that ends
before the longest one, by exact zeros up to the common row length.  Also the three voices of the
batched correction (tests/test_gpu_channel_maps.py) and their CPU chains (tests/pitchtrack_ref.py).
"""
import functools

import numpy as np

import pitchtrack_ref as pr
import timemap_ref as tm
import varresample_ref as vr


def padded_rows(rows, fill=np.nan):
    """rows of different lengths -> ([C, max len] float64 filled with `fill` past a row's end,
    counts int32): pv_timemap_set_channels' pos and counts"""
    counts = np.array([len(r) for r in rows], np.int32)
    out = np.full((len(rows), int(counts.max())), fill, np.float64)
    for c, r in enumerate(rows):
        out[c, :len(r)] = r
    return out, counts


def timemap_channels(xs, N, hop_div, pos, counts, lock, frames=None):
    """[C, n_out * hop + N - hop] float64: channel c is timemap_ref's stretch of xs[c] at
    pos[c][:counts[c]], then zeros (counts=None: every entry of the row counts)"""
    pos = np.asarray(pos, np.float64)
    C, n_out = pos.shape
    hop = N // hop_div
    out = np.zeros((C, n_out * hop + N - hop), np.float64)
    for c in range(C):
        n_c = n_out if counts is None else int(counts[c])
        ref = tm.cached(xs[c], N, hop_div, pos[c, :n_c], lock, frames)
        assert ref.shape[0] == n_c * hop + N - hop
        out[c, :ref.shape[0]] = ref
    return out


def varresample_channels(xs, steps, B, starts, quality=0, n_out=None):
    """[C, n_out] float64: channel c is varresample_ref's resampling of xs[c] by steps[c] from
    starts[c]"""
    return np.stack([vr.varresample(xs[c], [int(d) for d in steps[c]], B, int(starts[c]), quality, n_out)
                     for c in range(len(steps))])


def pitchmap_channels(xs, N, hop_div, plans, lock, frames, quality, n):
    """[C, n * hop + N - hop] float64: channel c is varresample_ref's composition with its own
    plan (pos_s, steps) = plans[c]"""
    return np.stack([vr.cached(xs[c], N, hop_div, plans[c][0], plans[c][1], lock, frames, quality, n)
                     for c in range(len(plans))])


# ---- three voices corrected in one call: the voice of the single-voice end-to-end test 35 cents
# under E4, one 30 cents over it (both with that test's +-15 cents of vibrato), and a steady one on E4
VOICES = ((-35.0, 15.0), (30.0, 15.0), (0.0, 0.0))  # (cents off E4, vibrato cents)
IN_TUNE = 2


@functools.lru_cache(maxsize=None)
def voices_input():
    hop = pr.E2E_N // pr.E2E_HOP_DIV
    n = pr.E2E_FRAMES * hop + 13
    rows = []
    for off, vib in VOICES:
        f0 = pr.E2E_A4 * 2.0 ** ((pr.E2E_NOTE - 69 + off / 100.0) / 12.0)
        x, _ = pr.voice(n, f0, 21, vibrato_cents=vib, vibrato_period=50.0 * hop)
        rows.append(x)
    xs = np.stack(rows)
    xs.setflags(write=False)
    assert np.array_equal(xs[0], pr.e2e_input())
    return xs


@functools.lru_cache(maxsize=None)
def voice_reference(c):
    """pitchtrack_ref.e2e_reference's chain for voice c -> (median cents before, after, the
    reference's ratios [frames], the cents off the scale its track reads per frame)"""
    import pvref
    N, hop = pr.E2E_N, pr.E2E_N // pr.E2E_HOP_DIV
    x = voices_input()[c]
    frames = pr.E2E_FRAMES
    lo, hi = pr.e2e_lags()
    mag, _ = pvref.std_analysis(x, N, hop, frames)
    r = pr.track(mag, N, lo, hi)
    before = pr.median_cents(r["f0"], r["strength"])
    ratio = pr.correction(np.stack([r["f0"], r["strength"]], 1), pr.E2E_A4, pr.MAJOR, 0.5, 1.0)
    pos_s, steps = vr.plan(N, hop, np.arange(frames, dtype=np.float64), ratio)
    y = np.asarray(vr.pitchmap_process(x, N, pr.E2E_HOP_DIV, pos_s, steps, True, frames, 0, frames), np.float32)
    mag2, _ = pvref.std_analysis(y, N, hop, frames)
    r2 = pr.track(mag2, N, lo, hi)
    return before, pr.median_cents(r2["f0"], r2["strength"]), ratio, pr.cents_off_scale(r["f0"], pr.E2E_A4, pr.MAJOR)
