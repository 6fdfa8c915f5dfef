"""The real-time harmoniser on the GPU (pv_rt_harmonizer_reserve / pv_rt_harmonizer_push; DESIGN.md
§3.17): every voice against the real-time pitch map's own kernels bit for bit, the mix against its
definition, both against tests/rt_harmonizer_ref.py's fp64 streams, their independence of how the
stream is cut into pushes, of the other channels and voices and of the captured callback, the
clamps, the reset, the refusals and a live chord.  3 channels; 1, 3 and 8 voices (4 at 2048
samples): wave 0 alone, a partly filled workgroup, the 512-thread one.  Every ratio and gain is an
fp32 value."""
import ctypes

import numpy as np
import pytest

import pvref
import rt_harmonizer_ref as rh
import rt_pitchmap_ref as rm
from gpu_helpers import RMS_TOL, status_of, to_dev
from pvamd import PITCH_SHIFT, TIME_SHIFT, RealTimeVocoder, _lib, interval_ratios
from signals import rms, synth
from test_gpu_rt_pitchmap import cuts_of

pytestmark = pytest.mark.gpu

C = 3
WIDE = (0.25, 4.0)
MID = (0.5, 2.0)
GEOMETRIES = [(256, 4, 40), (512, 3, 40), (1024, 4, 40), (2048, 4, 24)]  # N, hop_div, frames (hop 170 at 512)
U = 2.0 ** -24


def signal(n, seed, channels=C):
    return np.stack([synth(n, seed + 13 * c) for c in range(channels)])


def programme(k, T, c, v):
    """the ratio programme number k of voice v of channel c: in one pushed frame the voices of a
    channel have spans of 0, 1 and 4 stretched frames (under [1/4, 4])"""
    k %= 5
    if k == 0:
        return rm.constant(T, 1.0)
    if k == 1:
        return rm.alternating(T, 0.25, 4.0)
    if k == 2:
        return rm.glide(T, 0.5, 2.0)
    if k == 3:
        return rm.vibrato(T, 0.06, 23.0, 1.3 * c + 0.7 * v)
    return rm.alternating(T, 4.0, 0.25)


def programmes(V, T, channels=C, first=0):
    """[channels, V, T] float32 ratios: voice v runs programme first + v"""
    return np.stack([np.stack([programme(first + v, T, c, v) for v in range(V)]) for c in range(channels)])


def constant_gains(V, T, channels=C):
    g = np.array([1.0 / (v + 2.0) for v in range(V)], np.float32)
    return np.tile(g[None, :, None], (channels, 1, T)).astype(np.float32)


def changing_gains(V, T, channels=C, seed=3):
    """another gain at every frame; about a fifth are zeros, and every voice has a NaN"""
    rng = np.random.default_rng(seed + 10 * V)
    g = rng.uniform(-0.25, 1.0, (channels, V, T)).astype(np.float32)
    g[rng.uniform(size=g.shape) < 0.2] = 0.0
    for c in range(channels):
        for v in range(V):
            g[c, v, 3 + (5 * c + 3 * v) % (T - 4)] = np.nan
    return g


def make(N, hop_div, V, lock, rng=MID, quality=0, max_frames=4, channels=C):
    rt = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div, channels=channels, phase_lock=lock)
    rt.reserve_harmonizer(V, quality, max_frames, ratio_min=rng[0], ratio_max=rng[1])
    return rt


def run(rt, xs, ratios, gains, per_push, voices=True, spec=None, phases=None):
    """xs [C, T hop], ratios and gains [C, V, T] (None: no argument) -> (mix [C, T hop], voices
    [V, C, T hop] or None)"""
    hop = rt.hopSize
    xd = to_dev(xs)
    rd = None if ratios is None else to_dev(np.asarray(ratios, np.float32))
    gd = None if gains is None else to_dev(np.asarray(gains, np.float32))
    mixes, vos, t = [], [], 0
    for nf in cuts_of(xs.shape[1] // hop, per_push):
        r = None if rd is None else rd[:, :, t:t + nf].contiguous()
        g = None if gd is None else gd[:, :, t:t + nf].contiguous()
        s = None if spec is None else spec[:, :nf]
        got = rt.harmonize_push(xd[:, t * hop:(t + nf) * hop].contiguous(), r, g, voices=voices, spec=s)
        if voices:
            mixes.append(got[0].cpu().numpy())
            vos.append(got[1].cpu().numpy())
        else:
            mixes.append(got.cpu().numpy())
        if phases is not None:
            phases.append(spec.cpu().numpy()[:, :nf, :rt.spec_bins, 1].copy())
        t += nf
    return np.concatenate(mixes, axis=1), (np.concatenate(vos, axis=2) if voices else None)


def pitch_map_stream(N, hop_div, lock, rng, xs, ratios, per_push, quality=0):
    """the yardstick: a single-voice vocoder's pitch_map_push of xs with ratios [C, T]"""
    rt = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div, channels=xs.shape[0], phase_lock=lock)
    rt.reserve_pitch_map(quality, 4, ratio_min=rng[0], ratio_max=rng[1])
    hop = rt.hopSize
    xd, rd = to_dev(xs), to_dev(np.ascontiguousarray(ratios, np.float32))
    outs, t = [], 0
    for nf in cuts_of(xs.shape[1] // hop, per_push):
        outs.append(rt.pitch_map_push(xd[:, t * hop:(t + nf) * hop].contiguous(), rd[:, t:t + nf].contiguous()).cpu().numpy())
        t += nf
    return np.concatenate(outs, axis=1)


def voice_counts(N):
    return (1, 3, 4) if N == 2048 else (1, 3, 8)


def mix_bound(vo, gains, hop, G):
    """(the fp64 sum of g_v(j) voices_v[j] with the definition's fp32 ramp, the bound on the
    distance of the kernel's mix from it): test_voices_and_mix's docstring has the derivation"""
    V, Cn, n = vo.shape
    want, mag, rterm = np.zeros((Cn, n)), np.zeros((Cn, n)), np.zeros((Cn, n))
    for c in range(Cn):
        for v in range(V):
            g = rh.gain_stream(gains[c, v], hop, G, ramp=rh.ramp32)
            y = vo[v, c].astype(np.float64)
            want[c] += g * y
            mag[c] += np.abs(g * y)
            rterm[c] += np.abs((rh.gain_stream(gains[c, v], hop, G) - rh.prev_stream(gains[c, v], hop, G)) * y)
    return want, V * U * mag + V * U * rterm


# ------------------------------------------------------------------ 1, 2: the voices and the mix
@pytest.mark.parametrize("rng", [WIDE, MID], ids=["wide", "mid"])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,T,V", [(N, hd, T, V) for N, hd, T in GEOMETRIES for V in voice_counts(N)])
def test_voices_and_mix(cuda, N, hop_div, T, V, lock, rng):
    """Every voice is the existing shifter bit for bit: voices[v][c] equals the stream a separate
    vocoder's pitch_map_push gives for the same input and voice v's ratios (same range, preset and
    lock; pushed in other chunks, which that stream does not depend on), and the returned rows'
    phases are the oracle's.  Under [1/4, 4] the gains change at every frame (zeros and a NaN among
    them), under [1/2, 2] they are constant.

    The mix against its definition, per sample j: with g_v(j) the definition's fp32 ramp
    (rt_harmonizer_ref.ramp32: fmaf to the bit) and S = sum_v g_v(j) voices_v[j] in fp64,
        |mix - S| <= V 2^-24 sum_v |g_v(j) voices_v[j]| + V 2^-24 sum_v |r_v(j) voices_v[j]|,
    r_v(j) = (j + 1) / hop (g_b - g_prev) the ramp term.  The kernel's mix is V fmaf in a row, each
    one rounding of a partial sum no larger than sum_v |g_v voices_v|: relative 2^-24 each, V of
    them, the first term.  The second allows the restated ramp one rounding for its fmaf and one for
    its product (j + 1) (1 / hop) per voice, were it off by either; it is 0 where the gain does not
    change, and there the first term alone must hold."""
    import torch
    hop = N // hop_div
    G = rm.plan(hop, 0, *rng)["G"]
    rt = make(N, hop_div, V, lock, rng)
    assert rt.harmonizer_voices == V and rt.harmonizer_latency == (G + 1) * hop and T - 1 - G >= 8
    xs = signal(T * hop, 7100 + N)
    ratios = programmes(V, T)
    gains = changing_gains(V, T) if rng is WIDE else constant_gains(V, T)
    spec = torch.zeros((C, 4, rt.spec_stride, 2), dtype=torch.float32, device="cuda")
    phases = []
    mix, vo = run(rt, xs, ratios, gains, (3, 1, 4), True, spec, phases)
    assert mix.shape == (C, T * hop) and vo.shape == (V, C, T * hop)
    assert np.isfinite(mix).all() and np.isfinite(vo).all()
    assert not mix[:, :(G + 1) * hop].any() and not vo[:, :, :(G + 1) * hop].any() and mix[:, (G + 1) * hop:].any()
    for v in range(V):
        want = pitch_map_stream(N, hop_div, lock, rng, xs, ratios[:, v], 4)
        assert want.any() and np.array_equal(vo[v], want), f"voice {v} is not the pitch map's stream"
    gph = np.concatenate(phases, axis=1)
    for c in range(C):
        xp = np.concatenate([np.zeros(N - hop, np.float32), xs[c]])
        _, ph = pvref.std_analysis(xp, N, hop, T)
        assert np.array_equal(gph[c].view(np.uint32), ph.view(np.uint32)), f"channel {c}: phases differ"
    want, bound = mix_bound(vo, gains, hop, G)
    err = np.abs(mix.astype(np.float64) - want)
    live = bound > 0
    worst = float(np.max(err[live] / bound[live])) if live.any() else 0.0
    print(f"N={N} hop {hop} V={V} lock {lock} range {rng}: worst |mix - sum| / bound {worst:.3f}, "
          f"largest |mix - sum| {float(err.max()):.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("N,hop_div,T,V", [(256, 4, 40, 3), (256, 4, 40, 8), (512, 3, 40, 3), (1024, 4, 40, 3),
                                            (2048, 4, 24, 4)])
def test_one_hot_gains_give_the_voice(cuda, N, hop_div, T, V):
    hop = N // hop_div
    xs = signal(T * hop, 7200 + N)
    ratios = programmes(V, T)
    for v in range(V):
        gains = np.zeros((C, V, T), np.float32)
        gains[:, v] = 1.0
        mix, vo = run(make(N, hop_div, V, True, WIDE), xs, ratios, gains, 4)
        assert vo[v].any() and np.array_equal(mix, vo[v]), f"voice {v}"


# ------------------------------------------------------------------ 3: the fp64 reference
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,T,V", [(256, 4, 40, 3), (256, 4, 40, 8), (512, 3, 40, 3), (1024, 4, 40, 3),
                                            (2048, 4, 24, 4)])
def test_streams_match_reference(cuda, N, hop_div, T, V, lock):
    """RMS_TOL against rt_harmonizer_ref's mix and voices, per channel, under [1/4, 4] with gains
    that change at every frame"""
    hop = N // hop_div
    xs = signal(T * hop, 7100 + N)
    ratios = programmes(V, T)
    gains = changing_gains(V, T)
    mix, vo = run(make(N, hop_div, V, lock, WIDE), xs, ratios, gains, 4)
    for c in range(C):
        rmix, rvo = rh.stream(xs[c], N, hop_div, ratios[c], gains[c], lock, 0, *WIDE)
        em = rms(mix[c], rmix)
        ev = [rms(vo[v, c], rvo[v]) for v in range(V)]
        print(f"N={N} hop {hop} V={V} lock {lock} channel {c}: mix rms {em:.3e}, voices rms up to {max(ev):.3e}")
        assert rmix.any() and em <= RMS_TOL and max(ev) <= RMS_TOL


# ------------------------------------------------------------------ 4: bit-identical
@pytest.mark.parametrize("N,T,V,rng", [(256, 48, 8, WIDE), (256, 48, 3, MID), (2048, 24, 4, WIDE)])
def test_streams_do_not_depend_on_the_chunking(cuda, N, T, V, rng):
    hop_div = 4
    xs = signal(T * (N // hop_div), 881)
    ratios = programmes(V, T)
    gains = changing_gains(V, T)
    got = [run(make(N, hop_div, V, True, rng), xs, ratios, gains, pp) for pp in (1, 4, (3, 1, 2))]
    assert got[0][0].any()
    for mix, vo in got[1:]:
        assert np.array_equal(mix, got[0][0]) and np.array_equal(vo, got[0][1])


def test_a_channel_alone_equals_its_row_of_the_batch(cuda):
    N, hop_div, T, V = 512, 4, 30, 3
    xs = signal(T * (N // hop_div), 78)
    ratios, gains = programmes(V, T), changing_gains(V, T)
    mix, vo = run(make(N, hop_div, V, True, WIDE), xs, ratios, gains, 2)
    for c in (0, 2):
        m1, v1 = run(make(N, hop_div, V, True, WIDE, channels=1), xs[c:c + 1], ratios[c:c + 1], gains[c:c + 1], 2)
        assert m1.any() and np.array_equal(m1[0], mix[c]) and np.array_equal(v1[:, 0], vo[:, c])


def test_a_voice_does_not_depend_on_the_other_voices(cuda):
    """voice 1 of a 3-voice handle is voice 5 of an 8-voice handle whose other voices run other programmes"""
    N, hop_div, T = 256, 4, 40
    xs = signal(T * (N // hop_div), 79)
    r3, g3 = programmes(3, T), changing_gains(3, T)
    _, vo3 = run(make(N, hop_div, 3, True, WIDE), xs, r3, g3, 3)
    r8, g8 = programmes(8, T, first=2), changing_gains(8, T, seed=11)
    r8[:, 5] = r3[:, 1]
    _, vo8 = run(make(N, hop_div, 8, True, WIDE), xs, r8, g8, 3)
    assert vo3[1].any() and np.array_equal(vo8[5], vo3[1])
    assert not np.array_equal(vo8[4], vo3[0])


def test_mix_with_and_without_the_voices(cuda):
    N, hop_div, T, V = 512, 3, 30, 3
    xs = signal(T * (N // hop_div), 80)
    ratios, gains = programmes(V, T), changing_gains(V, T)
    a, _ = run(make(N, hop_div, V, True, WIDE), xs, ratios, gains, 3, voices=True)
    b, none = run(make(N, hop_div, V, True, WIDE), xs, ratios, gains, 3, voices=False)
    assert none is None and a.any() and np.array_equal(a, b)


# ------------------------------------------------------------------ 5: the captured callback
@pytest.mark.parametrize("launch", ["direct", "graph"])
def test_callback_with_pinned_controls_equals_push(cuda, monkeypatch, launch):
    """the captured callback reads its ratios and gains from the pinned buffers at replay time"""
    import torch
    monkeypatch.setenv("PV_RT_LAUNCH", launch)
    N, hop_div, T, nf, V = 256, 4, 30, 2, 3
    hop = N // hop_div
    xs = signal(T * hop, 311)
    ratios, gains = programmes(V, T), changing_gains(V, T)
    a, b = make(N, hop_div, V, True, WIDE, max_frames=nf), make(N, hop_div, V, True, WIDE, max_frames=nf)
    b.capture(nf)
    assert b.host_in.shape == (C, nf * hop) and b.host_out.shape == (C, nf * hop)
    assert b.host_ratios.shape == (C, V, nf) and (b.host_ratios == 1.0).all()
    assert b.host_gains.shape == (C, V, nf) and (b.host_gains == np.float32(1.0) / np.float32(V)).all()
    ga, _ = run(a, xs, ratios, gains, nf, voices=False)
    n = nf * hop
    gb = []
    for j in range(T // nf):
        r, g = ratios[:, :, j * nf:(j + 1) * nf], gains[:, :, j * nf:(j + 1) * nf]
        if j % 2:  # through the arguments, or written in place
            gb.append(b.callback(xs[:, j * n:(j + 1) * n], r, g).copy())
        else:
            b.host_ratios[...] = r
            b.host_gains[...] = g
            gb.append(b.callback(xs[:, j * n:(j + 1) * n]).copy())
    gb = np.concatenate(gb, axis=1)
    assert ga.any() and np.array_equal(ga, gb)
    # without controls the callback keeps the last ones; ratios of 1 and gains of 1 / V are the NULL arguments'
    torch.cuda.synchronize()
    b.reset()
    a.reset()
    torch.cuda.synchronize()
    b.host_ratios[...] = 1.0
    b.host_gains[...] = np.float32(1.0) / np.float32(V)
    again = np.concatenate([b.callback(xs[:, j * n:(j + 1) * n]).copy() for j in range(6)], axis=1)
    want, _ = run(a, xs[:, :6 * n], None, None, nf, voices=False)
    assert want.any() and np.array_equal(again, want)


# ------------------------------------------------------------------ 6: clamps
def test_wild_controls_are_clamped(cuda):
    N, hop_div, T, V = 256, 4, 30, 3
    xs = signal(T * (N // hop_div), 4243)
    wild = programmes(V, T, first=2)
    wild[:, :, 3::5] = 7.5
    wild[:, 1, 4::7] = 0.01
    wild[:, 2, 6::9] = np.nan
    wild[1, 0, 10] = np.inf
    wild[2, 1, 11] = -np.inf
    wild[0, 2, 12] = -1.0
    tame = np.where(np.isnan(wild), MID[0], np.clip(wild, MID[0], MID[1])).astype(np.float32)
    gains = changing_gains(V, T)
    assert np.isnan(gains).any()
    zeroed = np.where(np.isnan(gains), 0.0, gains).astype(np.float32)
    a = run(make(N, hop_div, V, True), xs, wild, gains, 3)
    b = run(make(N, hop_div, V, True), xs, tame, zeroed, 3)
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and a[0].any()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ 7: reset and coexistence
def test_reset_and_the_other_pushes(cuda):
    import torch
    N, hop_div, T, V = 256, 4, 12, 3
    hop = N // hop_div
    xs = signal(T * hop, 98)
    xd = to_dev(xs)
    ratios, gains = programmes(V, T), changing_gains(V, T)

    def each(fn):
        return np.concatenate([fn(xd[:, j * hop:(j + 1) * hop].contiguous()).cpu().numpy() for j in range(T)], 1)

    for lock in (False, True):
        used = make(N, hop_div, V, lock, WIDE)
        first = run(used, xs, ratios, gains, 4)
        run(used, xs[:, :5 * hop], ratios[:, :, :5], gains[:, :, :5], 1)
        torch.cuda.synchronize()
        used.reset()
        again = run(used, xs, ratios, gains, 4)
        assert first[0].any() and np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
        # push, pitch_push and pitch_map_push on the handle equal a fresh handle's
        fresh = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div, channels=C, phase_lock=lock)
        used.reset()
        want, got = each(fresh.push), each(used.push)
        assert want.any() and np.array_equal(got, want)
        used.reserve_pitch(0, max_frames=4)
        fresh.reserve_pitch(0, max_frames=4)
        used.reset()
        fresh.reset()
        torch.cuda.synchronize()
        assert np.array_equal(each(used.pitch_push), each(fresh.pitch_push))
        used.reserve_pitch_map(0, 4, ratio_min=WIDE[0], ratio_max=WIDE[1])
        used.reset()
        torch.cuda.synchronize()
        rd = to_dev(ratios[:, 2].copy())
        got = np.concatenate([used.pitch_map_push(xd[:, j * hop:(j + 1) * hop].contiguous(), rd[:, j:j + 1].contiguous())
                              .cpu().numpy() for j in range(T)], 1)
        assert np.array_equal(got, pitch_map_stream(N, hop_div, lock, WIDE, xs, ratios[:, 2], 1))
        # and the harmoniser once more, its state untouched by what ran in between but the reset
        used.reset()
        torch.cuda.synchronize()
        again = run(used, xs, ratios, gains, 4)
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


def test_the_later_reserve_decides_what_is_captured(cuda):
    N, hop_div, V = 256, 4, 3
    hop = N // hop_div
    rt = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div)
    rt.reserve_pitch_map(0, 1)
    rt.reserve_harmonizer(V, 0, 1)
    rt.capture(1)
    assert rt.host_ratios.shape == (1, V, 1) and rt.host_gains.shape == (1, V, 1)
    fr = ctypes.POINTER(ctypes.c_float)()
    assert rt._L.pv_rt_pitchmap_host_ratios(rt._h, ctypes.byref(fr)) == _lib.PV_ERR_ARG
    assert rt.callback(np.zeros((1, hop), np.float32), np.ones((1, V, 1), np.float32),
                       np.ones((1, V, 1), np.float32)).shape == (1, hop)
    rt2 = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div)
    rt2.reserve_harmonizer(V, 0, 1)
    rt2.reserve_pitch_map(0, 1)
    rt2.capture(1)
    assert rt2.host_ratios.shape == (1, 1) and rt2.host_gains is None
    fg = ctypes.POINTER(ctypes.c_float)()
    assert rt2._L.pv_rt_harmonizer_host_controls(rt2._h, ctypes.byref(fr), ctypes.byref(fg)) == _lib.PV_ERR_ARG
    assert len(rt2._L.pv_last_error()) > 0
    assert status_of(lambda: rt2.callback(np.zeros((1, hop), np.float32), None, np.ones((1, V, 1), np.float32))) == _lib.PV_ERR_ARG
    rt3 = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div)
    rt3.reserve_harmonizer(V, 0, 1)
    rt3.reserve_pitch(0, max_frames=1)
    rt3.capture(1)
    assert rt3.host_ratios is None and rt3.host_gains is None


# ------------------------------------------------------------------ 8: refusals
def test_refusals(cuda):
    import torch
    N, hop_div = 256, 4
    hop = N // hop_div
    x = torch.zeros((1, 2 * hop), dtype=torch.float32, device="cuda")
    # a PV_PITCH_SHIFT handle, out_hop != hop, hop < 16
    assert status_of(lambda: RealTimeVocoder(N, PITCH_SHIFT, 1.5, hop_div).reserve_harmonizer(3)) == _lib.PV_ERR_UNSUPPORTED
    assert status_of(lambda: RealTimeVocoder(N, TIME_SHIFT, 1.5, hop_div).reserve_harmonizer(3)) == _lib.PV_ERR_UNSUPPORTED
    assert status_of(lambda: RealTimeVocoder(N, TIME_SHIFT, 1.0, 32).reserve_harmonizer(3)) == _lib.PV_ERR_UNSUPPORTED
    rt = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div)
    assert rt.harmonizer_latency == 0 and rt.harmonizer_voices == 0
    # push before a successful reserve
    assert status_of(lambda: rt.harmonize_push(x)) == _lib.PV_ERR_ARG
    # voices 0 and 9; 5 at 2048 samples
    assert status_of(lambda: rt.reserve_harmonizer(0)) == _lib.PV_ERR_ARG
    assert status_of(lambda: rt.reserve_harmonizer(9)) == _lib.PV_ERR_ARG
    assert status_of(lambda: rt.reserve_harmonizer(-1)) == _lib.PV_ERR_ARG
    big = RealTimeVocoder(2048, TIME_SHIFT, 1.0, 4)
    assert status_of(lambda: big.reserve_harmonizer(5)) == _lib.PV_ERR_ARG
    assert status_of(lambda: big.reserve_harmonizer(4)) == _lib.PV_OK and big.harmonizer_voices == 4
    # bad quality, max_nframes <= 0, bad ranges
    for quality, mx, lo, hi in ((2, 1, 0.5, 2.0), (-1, 1, 0.5, 2.0), (0, 0, 0.5, 2.0), (0, -3, 0.5, 2.0),
                                (0, 1, 0.2, 2.0), (0, 1, 0.5, 4.5), (0, 1, 2.0, 0.5), (0, 1, float("nan"), 2.0),
                                (0, 1, 0.5, float("nan"))):
        assert status_of(lambda: rt.reserve_harmonizer(3, quality, mx, ratio_min=lo, ratio_max=hi)) == _lib.PV_ERR_ARG
    # G > 64: hop 16, best preset, [1/4, 4] needs 68 callbacks
    small = RealTimeVocoder(N, TIME_SHIFT, 1.0, 16)
    assert status_of(lambda: small.reserve_harmonizer(2, 1, 1, ratio_min=0.25, ratio_max=4.0)) == _lib.PV_ERR_ARG
    # after the refused reserves the feature is off and push still works
    assert rt.harmonizer_latency == 0 and rt.harmonizer_voices == 0
    assert status_of(lambda: rt.harmonize_push(x)) == _lib.PV_ERR_ARG
    assert rt.push(x).shape == (1, 2 * hop)
    rt.reset()
    # more frames than reserved, in a push and in a capture
    rt.reserve_harmonizer(3, 0, 1, ratio_min=0.84, ratio_max=1.19)
    assert rt.harmonizer_latency == 2 * hop and rt.harmonizer_voices == 3
    assert status_of(lambda: rt.harmonize_push(x)) == _lib.PV_ERR_ARG
    assert status_of(lambda: rt.capture(2)) == _lib.PV_ERR_ARG
    assert rt.harmonize_push(x[:, :hop]).shape == (1, hop)
    mix, vo = rt.harmonize_push(x[:, :hop], voices=True)
    assert mix.shape == (1, hop) and vo.shape == (3, 1, hop)
    # the pinned controls exist only behind a captured harmoniser callback
    fr, fg = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_float)()
    assert rt._L.pv_rt_harmonizer_host_controls(rt._h, ctypes.byref(fr), ctypes.byref(fg)) == _lib.PV_ERR_ARG
    assert len(rt._L.pv_last_error()) > 0
    # the setup call comes before pv_rt_capture
    rt.capture(1)
    assert rt._L.pv_rt_harmonizer_host_controls(rt._h, ctypes.byref(fr), ctypes.byref(fg)) == _lib.PV_OK
    assert status_of(lambda: rt.reserve_harmonizer(3, 0, 1)) == _lib.PV_ERR_ARG
    assert rt.callback(np.zeros((1, hop), np.float32)).shape == (1, hop)


def test_reserve_out_of_memory_leaves_the_feature_off(cuda):
    """scratch rows of 256 channels x 8 voices x 4e6 frames x 64 samples x ratio 2 cannot be
    allocated; the rows are the first allocation, so nothing else is taken before it fails"""
    import torch
    rt = RealTimeVocoder(256, TIME_SHIFT, 1.0, 4, channels=256)
    assert status_of(lambda: rt.reserve_harmonizer(8, 0, max_frames=4_000_000)) == _lib.PV_ERR_NOMEM
    assert rt.harmonizer_latency == 0 and rt.harmonizer_voices == 0
    x = torch.zeros((256, 64), dtype=torch.float32, device="cuda")
    assert status_of(lambda: rt.harmonize_push(x)) == _lib.PV_ERR_ARG
    assert rt.push(x).shape == (256, 64)


# ------------------------------------------------------------------ 9: the chord
def test_a_live_chord(cuda):
    """tests/test_rt_harmonizer_ref.py's chord through the GPU: the mix's three peaks within 0.02
    analysis bin of 0.05 ratio at no less than 0.98 of gain 0.5, the CPU test's own bounds, and
    beside the reference's figures"""
    x = rh.chord_input()
    ratios, gains = rh.chord_controls()
    assert np.array_equal(ratios[:, 0], interval_ratios(rh.CHORD_SEMITONES))
    rt = make(rh.CHORD_N, rh.CHORD_HOP_DIV, 3, True, MID, channels=1)
    mix, _ = run(rt, x[None], ratios[None], gains[None], 4, voices=False)
    ref, _ = rh.stream(x, rh.CHORD_N, rh.CHORD_HOP_DIV, ratios, gains, True)
    got, want = rh.chord_peaks(mix[0], rt.harmonizer_latency), rh.chord_peaks(ref, rt.harmonizer_latency)
    for v, ((df, a), (rdf, ra)) in enumerate(zip(got, want)):
        print(f"voice {v}: {df:+.4f} bin, {a:.4f} of its amplitude (reference {rdf:+.4f}, {ra:.4f})")
        assert abs(df) <= rh.CHORD_BIN_TOL and a >= rh.CHORD_AMP_FLOOR
