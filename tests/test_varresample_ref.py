"""Variable-rate resampler and pitch map, CPU side: the numpy reference (tests/varresample_ref.py)
pinned to the polyphase reference by constant maps, the integer facts the design rests on, the
host-only entry points and the refusals that need no GPU through ctypes, and the quality of the
composed reference (a glide lands on pitch, at full amplitude, whatever the tempo)."""
import ctypes

import numpy as np
import pytest

import pvref
import resample_ref as rr
import timemap_ref as tm
import varresample_ref as vr
import pvamd
from pvamd import _lib
from signals import rms


# ------------------------------------------------------------------ pinned to resample_ref
@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("p,q", [(3, 2), (3, 4), (1, 4), (4, 1), (5, 8)])
def test_constant_map_is_the_polyphase_reference(p, q, quality):
    """steps 2^32 P / Q (exact), start 0: only the even-integer quantisation of s differs"""
    x = np.random.default_rng(100 * p + q).standard_normal(3000)
    B = 64
    n_out = rr.out_length(p, q, len(x))
    d = (vr.ONE * p) // q
    assert d * q == vr.ONE * p
    steps = [d] * (-(-n_out // B))
    got = vr.varresample(x, steps, B, 0, quality, n_out)
    ref = rr.resample(x, p, q, quality)
    assert got.shape == ref.shape
    err, worst = rms(got, ref), float(np.max(np.abs(got - ref)))
    print(f"{p}:{q} quality {quality}: rms {err:.3g} max {worst:.3g}")
    assert err <= 1e-7 and worst <= 1e-7
    assert vr.block_filter(d, quality)[1] == rr.half_width(p, q, quality)


def test_all_ones_map_is_the_shifted_copy():
    x = np.random.default_rng(5).standard_normal(500)
    y = vr.varresample(x, [vr.ONE] * 10, 64, 7 * vr.ONE)
    assert np.array_equal(y[:493], x[7:]) and not y[493:].any()
    # a fraction in the start goes through the filter: a tone in the passband comes out as it is
    # up to the passband ripple (the fast preset's stopband is below -80 dB), noise does not
    s = np.sin(2.0 * np.pi * 0.05 * np.arange(500))
    z = vr.varresample(s, [vr.ONE] * 10, 64, 7 * vr.ONE + 1)
    assert not np.array_equal(z[:493], s[7:]) and np.max(np.abs(z[50:400] - s[57:407])) < 1e-3
    assert rms(vr.varresample(x, [vr.ONE] * 10, 64, 7 * vr.ONE + 1)[50:400], x[57:407]) > 0.1


# ------------------------------------------------------------------ integer facts
def test_steps_and_knots_are_exact_integers():
    rng = np.random.default_rng(2)
    ratios = np.concatenate([[0.25, 4.0, 1.0, 1.5, 2.0 ** -0.5], rng.uniform(0.25, 4.0, 200)])
    steps = pvamd.ratio_steps(ratios)
    assert steps.dtype == np.int64
    assert list(steps) == vr.ratio_steps(ratios) == [int(v) for v in np.rint(ratios * 2.0 ** 32)]
    assert steps[0] == 1 << 30 and steps[1] == 1 << 34 and steps[2] == 1 << 32
    # knots up to the 2^62 the host accepts: the 64-bit sums are the big-integer sums
    B = 4096
    big = [1 << 34] * ((1 << 16) - 1)
    T = vr.knots(12345, big, B)
    assert T[-1] < 1 << 62
    assert np.array_equal(np.array(T[1:], np.int64), 12345 + np.cumsum(np.array(big, np.int64) * B))
    for d, quality in ((1 << 32, 0), (1 << 34, 1), (1 << 30, 0), (6442450944, 1)):
        Sq, W = vr.block_filter(d, quality)
        Z, rolloff, _ = rr.PRESETS[quality]
        assert Sq % 2 == 0 and 0 <= rolloff * min(1.0, 2.0 ** 32 / d) * 2.0 ** 32 - Sq < 2
        assert W == int(np.ceil(Z / (Sq / 2.0 ** 32)))


PLAN_CASES = [
    (256, 64, 199, 1.0, ("glide", 1.0, 1.5)),
    (256, 64, 199, 0.73, ("glide", 1.0, 1.5)),
    (512, 170, 60, 0.73, ("vibrato",)),
    (1024, 256, 60, 1.37, ("glide", 1.5, 0.75)),
    (1024, 256, 1, 1.0, ("glide", 0.25, 0.25)),
    (256, 16, 7, 1.0, ("glide", 4.0, 4.0)),
]


def plan_inputs(frames, rate, shape):
    pos = tm.rate_map(frames, rate)
    ratio = vr.glide(len(pos), shape[1], shape[2]) if shape[0] == "glide" else vr.vibrato(len(pos))
    return pos, ratio


@pytest.mark.parametrize("N,hop,frames,rate,shape", PLAN_CASES)
def test_plan_is_the_restatement(N, hop, frames, rate, shape):
    pos, ratio = plan_inputs(frames, rate, shape)
    pos_s, steps = pvamd.pitch_map_plan(N, hop, pos, ratio)
    ref_pos, ref_steps = vr.plan(N, hop, pos, ratio)
    n = len(pos)
    assert len(steps) == -(-(n * hop + N - hop) // hop) and list(steps) == ref_steps
    assert list(steps[n:]) == [steps[n - 1]] * (len(steps) - n)
    assert len(pos_s) == len(ref_pos) == max(1, -(-sum(ref_steps[:n]) * hop // (hop << 32)))
    assert np.max(np.abs(pos_s - ref_pos)) <= 1e-9
    assert pos_s.min() >= pos.min() and pos_s.max() <= pos.max()


def test_plan_at_ratio_one_returns_the_positions():
    pos = tm.rate_map(60, 0.73)
    pos_s, steps = pvamd.pitch_map_plan(1024, 256, pos, np.ones(len(pos)))
    assert np.array_equal(pos_s, pos) and set(steps) == {1 << 32}


# ------------------------------------------------------------------ ABI without a GPU
def test_symbols_and_refusals_without_a_gpu():
    L = _lib.lib()
    for s in ("pv_varresampler_create", "pv_varresampler_destroy", "pv_varresample_steps", "pv_varresampler_set_map",
              "pv_varresample_length", "pv_varresample", "pv_pitchmap_plan", "pv_pitchmap_set",
              "pv_pitchmap_output_length", "pv_pitchmap_process"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4
    vp = ctypes.c_void_p
    # pv_varresample_steps
    one = (ctypes.c_double * 1)(1.5)
    st = (ctypes.c_longlong * 1)()
    assert L.pv_varresample_steps(one, 1, st) == _lib.PV_OK and st[0] == 3 << 31
    assert L.pv_varresample_steps(None, 1, st) == _lib.PV_ERR_ARG
    assert L.pv_varresample_steps(one, 1, None) == _lib.PV_ERR_ARG
    assert L.pv_varresample_steps(one, 0, st) == _lib.PV_ERR_ARG
    assert L.pv_varresample_steps(one, -3, st) == _lib.PV_ERR_ARG
    assert b"pv_varresample_steps" in L.pv_last_error()
    for bad in (0.2499, 4.0001, 0.0, -1.0, np.nan, np.inf):
        with pytest.raises(pvamd.PVError) as e:
            pvamd.ratio_steps([1.0, bad])
        assert e.value.status == _lib.PV_ERR_ARG
    # pv_varresampler_create: the arguments are refused before any device call
    h = vp()
    for quality, block, max_blocks in ((2, 64, 8), (-1, 64, 8), (0, 15, 8), (0, 4097, 8), (0, 64, 0), (0, 64, -1),
                                       (0, 4096, 1 << 19)):
        assert L.pv_varresampler_create(quality, block, max_blocks, 0, ctypes.byref(h)) == _lib.PV_ERR_ARG
        assert L.pv_last_error() and not h.value
    assert L.pv_varresampler_create(0, 64, 8, 0, None) == _lib.PV_ERR_ARG
    # NULL objects
    L.pv_varresampler_destroy(None)
    assert L.pv_varresampler_set_map(None, 0, st, 1) == _lib.PV_ERR_ARG
    assert L.pv_varresample_length(None) == 0
    assert L.pv_varresample(None, None, 0, 0, 1, None, 0, 0, None) == _lib.PV_ERR_ARG
    assert b"null" in L.pv_last_error()
    assert L.pv_pitchmap_set(None, one, one, 1, 0) == _lib.PV_ERR_ARG
    assert L.pv_pitchmap_set(None, None, None, 0, 0) == _lib.PV_ERR_ARG
    assert L.pv_pitchmap_output_length(None) == 0
    assert L.pv_pitchmap_process(None, None, 0, 0, 1, 1, None, 0, None, 0, None) == _lib.PV_ERR_ARG


def test_plan_refusals():
    L = _lib.lib()
    pos, ratio = np.arange(8, dtype=np.float64), np.ones(8)
    pvamd.pitch_map_plan(256, 64, pos, ratio)
    for bad_pos in ([-0.5], [np.nan], [2.0 ** 30]):
        with pytest.raises(pvamd.PVError) as e:
            pvamd.pitch_map_plan(256, 64, bad_pos, [1.0])
        assert e.value.status == _lib.PV_ERR_ARG
    for bad_ratio in ([0.2], [4.5], [0.0], [-1.0], [np.nan]):
        with pytest.raises(pvamd.PVError) as e:
            pvamd.pitch_map_plan(256, 64, [0.0], bad_ratio)
        assert e.value.status == _lib.PV_ERR_ARG
    vp = ctypes.c_void_p
    p, r = pos.ctypes.data_as(vp), ratio.ctypes.data_as(vp)
    ps, stp = np.empty(64), np.empty(64, np.int64)
    ns, nb = ctypes.c_int(), ctypes.c_int()
    args = lambda **k: [k.get("N", 256), k.get("hop", 64), k.get("p", p), k.get("r", r), k.get("n", 8),  # noqa: E731
                        k.get("ps", ps.ctypes.data_as(vp)), k.get("cap_s", 64), k.get("ns", ctypes.byref(ns)),
                        k.get("stp", stp.ctypes.data_as(vp)), k.get("cap_b", 64), k.get("nb", ctypes.byref(nb))]
    assert L.pv_pitchmap_plan(*args()) == _lib.PV_OK and ns.value == 8 and nb.value == 11
    for k in (dict(p=None), dict(r=None), dict(ps=None), dict(stp=None), dict(ns=None), dict(nb=None), dict(n=0),
              dict(n=-1), dict(cap_s=7), dict(cap_b=10), dict(hop=0), dict(hop=257)):
        assert L.pv_pitchmap_plan(*args(**k)) == _lib.PV_ERR_ARG, k
        assert b"pv_pitchmap_plan" in L.pv_last_error()


# ------------------------------------------------------------------ quality of the composed reference
def frame_peak(y, N):
    """(frequency in analysis bins, amplitude) of the strongest partial of one frame: periodic
    Hann window, 4N zero-padded FFT, parabolic interpolation of the log magnitude"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    X = np.abs(np.fft.rfft(y * w, 4 * N))
    k = int(np.argmax(X[1:-1])) + 1
    a, b, c = np.log(X[k - 1]), np.log(X[k]), np.log(X[k + 1])
    delta = 0.5 * (a - c) / (a - 2.0 * b + c)
    peak = np.exp(b - 0.25 * (a - c) * delta)
    return (k + delta) / 4.0, 2.0 * peak / np.sum(w)


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("rate", [1.0, 0.73])
def test_a_glide_lands_on_pitch_at_full_amplitude(rate, lock):
    N, hop_div = 256, 4
    hop = N // hop_div
    x = (0.5 * np.sin(2.0 * np.pi * 0.05 * np.arange(12800))).astype(np.float32)
    frames = pvref.num_frames(len(x), hop)
    pos = tm.rate_map(frames, rate)
    n = len(pos)
    ratio = vr.glide(n, 1.0, 1.5)
    pos_s, steps = vr.plan(N, hop, pos, ratio)
    y = vr.pitchmap_process(x, N, hop_div, pos_s, steps, lock, frames, 0, n)
    assert len(y) == n * hop + N - hop == {1.0: 12928, 0.73: 17600}[rate]
    worst_f, least_a = 0.0, 1.0
    for u in range(4, n - 4):
        f, a = frame_peak(y[u * hop:u * hop + N], N)
        centre = u + N / (2.0 * hop)
        want = 0.05 * N * 1.5 ** (centre / (n - 1.0))
        worst_f, least_a = max(worst_f, abs(f - want)), min(least_a, a)
    print(f"rate {rate} lock {lock}: {n} frames, worst peak offset {worst_f:.4f} bin, least amplitude {least_a:.4f}")
    assert worst_f <= 0.1
    assert least_a >= 0.45
