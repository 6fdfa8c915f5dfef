"""Maps set per channel on the GPU: pv_timemap_set_channels,
pv_varresampler_set_maps and pv_pitchmap_set_channels against the fp64 references with every
channel's own map (tests/channel_maps_ref.py), and bit for bit against the shared-map calls of
each channel alone.  The shapes of test_gpu_timemap / test_gpu_varresample: 3 channels, 60 analysed
frames, max_frames 128, runs of 8 frames (one case of 16); n_in = 5003 for the resampler alone."""
import ctypes
import functools

import numpy as np
import pytest

import channel_maps_ref as cm
import pitchtrack_ref as pr
import timemap_ref as tm
import varresample_ref as vr
from gpu_helpers import (MAP_INPUTS, RMS_TOL, SENTINEL, channel_errors, make_vocoder, padded_input, run_padded,
                         status_of, stretch_inputs, to_dev, to_dev_copy, wide)
from pvamd import (MAJOR, PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, PhaseVocoder, VarResampler, _lib,
                   pitch_correction, pitch_map_plan, rate_map)
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 3
FRAMES = MAP_INPUTS["frames"]
MAX_FRAMES = 128
GEOMETRIES = [(256, 4), (512, 3), (1024, 4)]
ONE = 1 << 32

inputs = functools.partial(stretch_inputs, **MAP_INPUTS, channels=C)  # (the stretch's references are shared)

# three maps of different lengths in one call: 60, 81 and 53 output frames
TIME_ROWS = [np.arange(FRAMES, dtype=np.float64), rate_map(FRAMES, 0.73), tm.scrub_map()]


def make(monkeypatch, N, hop_div, F=8, **kw):
    pv = make_vocoder(monkeypatch, N, hop_div, TIME_SHIFT, 1.0, F, max_frames=MAX_FRAMES, channels=C, **kw)
    assert pv.outHopSize == pv.hopSize
    return pv


# ---------------------------------------------------------------- 1. the time map against the reference
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div", GEOMETRIES)
def test_time_map_parity(cuda, monkeypatch, N, hop_div, lock):
    import torch
    xs = inputs(N, hop_div)
    pos, counts = cm.padded_rows(TIME_ROWS)  # (NaN past a row's count: those entries are not read)
    assert counts.tolist() == [60, 81, 53]
    n_out = pos.shape[1]
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    assert pv.time_map_channels == 0
    pv.set_time_map(pos, counts)
    assert pv.time_map_frames == n_out and pv.time_map_channels == C
    olen = pv.output_length(n_out)
    xbuf = padded_input(xs, 38)
    obuf = torch.full((C, olen + 5), SENTINEL, dtype=torch.float32, device="cuda")
    out, spec = pv.time_map_process(xbuf[:, :xs.shape[1]], out=obuf[:, :olen])
    assert (obuf[:, olen:] == SENTINEL).all() and spec.shape[1] == FRAMES
    ref = cm.timemap_channels(xs, N, hop_div, pos, counts, lock, FRAMES)
    errs = channel_errors(out, lambda c: ref[c], C)
    print(f"N={N} hop_div={hop_div} lock={lock} maps of {counts.tolist()} frames: rms "
          + ", ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= RMS_TOL
    for c in range(C):
        assert not out[c, pv.output_length(int(counts[c])):].any(), f"channel {c}: samples past its own length"
    again, _ = pv.time_map_process(to_dev(xs))  # contiguous rows, an aligned output: the same bits
    assert torch.equal(again, out)


# ---------------------------------------------------------------- 2. a channel does not see its neighbours
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,layout,spectrum,F", [
    (1024, 4, _lib.PV_SPEC_NATURAL, True, 8), (1024, 4, _lib.PV_SPEC_NATURAL, False, 8),
    (1024, 4, _lib.PV_SPEC_PACKED, True, 8), (1024, 4, _lib.PV_SPEC_PACKED, False, 8),
    (1024, 4, _lib.PV_SPEC_NATURAL, True, 16), (512, 3, _lib.PV_SPEC_NATURAL, True, 8),
    (256, 4, _lib.PV_SPEC_PACKED, False, 8)])
def test_a_channel_is_its_own_shared_map_call(cuda, monkeypatch, N, hop_div, layout, spectrum, F, lock):
    import torch
    xd = to_dev(inputs(N, hop_div))
    pos, counts = cm.padded_rows(TIME_ROWS)
    pv = make(monkeypatch, N, hop_div, F, phase_lock=lock, spec_layout=layout)
    pv.set_time_map(pos, counts)
    batch, _ = pv.time_map_process(xd, spectrum=spectrum)
    for c in range(C):
        n_c = int(counts[c])
        pv.set_time_map(pos[c, :n_c])
        assert pv.time_map_channels == 0 and pv.time_map_frames == n_c
        alone, _ = pv.time_map_process(xd[c:c + 1].contiguous(), spectrum=spectrum)
        assert alone.shape[1] == pv.output_length(n_c)
        assert torch.equal(alone[0], batch[c, :alone.shape[1]]), f"channel {c}"


# ---------------------------------------------------------------- 3. the shared path is a special case
@pytest.mark.parametrize("lock", [False, True])
def test_the_same_map_for_every_channel_is_the_shared_map(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xd = to_dev(inputs(N, hop_div))
    pos = TIME_ROWS[1]
    fresh = make(monkeypatch, N, hop_div, phase_lock=lock)
    want_own, want_own_spec = fresh.process(xd)
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    pv.set_time_map(pos)
    want, want_spec = pv.time_map_process(xd)
    pv.set_time_map(np.stack([pos] * C))
    assert pv.time_map_channels == C and pv.time_map_frames == len(pos)
    got, got_spec = pv.time_map_process(xd)
    assert torch.equal(got, want) and torch.equal(got_spec, want_spec)
    # fewer channels than the map has: the first ones
    two, _ = pv.time_map_process(xd[:2].contiguous())
    assert torch.equal(two, want[:2])
    pv.set_time_map(pos)
    assert pv.time_map_channels == 0
    again, _ = pv.time_map_process(xd)
    assert torch.equal(again, want)
    own, own_spec = pv.process(xd)  # a following pv_process is unchanged
    assert torch.equal(own, want_own) and torch.equal(own_spec, want_own_spec)
    pv.set_time_map(np.stack([pos] * C))
    pv.set_time_map(None)
    assert pv.time_map_channels == 0 and pv.time_map_frames == 0


# ---------------------------------------------------------------- 4. the variable-rate resampler alone
N_IN = 5003
PAD = 38


@functools.lru_cache(maxsize=None)
def resampler_signal():
    xs = np.stack([synth(N_IN, 4400 + 13 * c) for c in range(C)])
    xs.setflags(write=False)
    return xs


def resampler_maps(B):
    """per channel {const 3/2, glide, vibrato with a fractional start}, the same blocks for all"""
    nb = -(-3300 // B)
    steps = np.array([[ONE * 3 // 2] * nb, vr.ratio_steps(vr.glide(nb, 0.5, 2.0)), vr.ratio_steps(vr.vibrato(nb))],
                     np.int64)
    return steps, np.array([0, 0, 5 * ONE + 0x9e3779b9], np.int64)


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("B", [64, 170])
def test_resampler_maps_per_channel(cuda, B, quality):
    import torch
    xs = resampler_signal()
    xd = to_dev_copy(xs)
    steps, starts = resampler_maps(B)
    nb = steps.shape[1]
    rs = VarResampler(B, quality, max_blocks=nb + 3)
    assert rs.map_channels == 0
    rs.set_map(steps, starts)
    assert rs.map_channels == C and rs.length == nb * B
    n_out = rs.length - 7
    assert n_out % B and n_out % 1024 and n_out > 3 * 1024
    g = run_padded(rs, xs, PAD, n_out)
    ref = cm.varresample_channels(xs, steps, B, starts, quality, n_out)
    for c in range(C):
        err = rms(g[c], ref[c])
        print(f"B={B} quality {quality} channel {c} ({n_out} outputs): rms {err:.3e}")
        assert err <= RMS_TOL
    batch = rs(xd, n_out=n_out)
    assert np.array_equal(batch.cpu().numpy(), g)
    for c in range(C):  # each channel is the shared-map run of that channel alone
        rs.set_map(steps[c], int(starts[c]))
        assert rs.map_channels == 0
        assert torch.equal(rs(xd[c].contiguous(), n_out=n_out), batch[c]), f"channel {c}"
    # a channel of all-ones steps beside two filtered ones: the shifted copy, bit for bit
    mixed = steps.copy()
    mixed[0] = ONE
    rs.set_map(mixed, np.array([7 * ONE, 0, starts[2]], np.int64))
    g2 = run_padded(rs, xs, PAD, n_out)
    assert np.array_equal(g2[0], xs[0, 7:7 + n_out]) and np.array_equal(g2[1:], g[1:])
    # ... and past the input's end it reads zeros
    long_rs = VarResampler(B, quality, max_blocks=-(-N_IN // B) + 2)
    nl = long_rs.max_blocks
    lsteps = np.stack([np.full(nl, ONE, np.int64), np.full(nl, ONE * 3 // 2, np.int64)])
    long_rs.set_map(lsteps, np.array([7 * ONE, 0], np.int64))
    g3 = run_padded(long_rs, xs[:2], PAD, long_rs.length - 7)
    assert np.array_equal(g3[0, :N_IN - 7], xs[0, 7:]) and not g3[0, N_IN - 7:].any()
    # all three channels all-ones: the copy, a shift per channel
    rs.set_map(np.full((C, nb), ONE, np.int64), np.array([0, 7 * ONE, 3 * ONE], np.int64))
    assert rs.map_channels == C
    g4 = run_padded(rs, xs, PAD, n_out)
    for c, sh in enumerate((0, 7, 3)):
        assert np.array_equal(g4[c], xs[c, sh:sh + n_out]), f"channel {c}"
    # a fraction in one start: that channel goes through the filter, the others stay copies
    rs.set_map(np.full((C, nb), ONE, np.int64), np.array([0, 7 * ONE + 1, 3 * ONE], np.int64))
    g5 = run_padded(rs, xs, PAD, n_out)
    assert np.array_equal(g5[0], g4[0]) and np.array_equal(g5[2], g4[2]) and not np.array_equal(g5[1], g4[1])
    assert rms(g5[1], vr.varresample(xs[1], [ONE] * nb, B, 7 * ONE + 1, quality, n_out)) <= RMS_TOL


def test_resampler_map_refusals(cuda):
    import torch
    L = _lib.lib()
    rs = VarResampler(64, 0, max_blocks=8)
    ok = np.full((2, 8), ONE * 3 // 2, np.int64)
    for steps, starts in ((np.zeros((2, 0), np.int64), [0, 0]), (np.full((2, 9), ONE, np.int64), [0, 0]),
                          (np.array([[ONE] * 8, [ONE] * 7 + [(1 << 30) - 1]], np.int64), [0, 0]),
                          (ok, [0, -1]), (ok, [0, (1 << 62) - 10])):
        assert status_of(lambda: rs.set_map(steps, np.array(starts, np.int64))) == _lib.PV_ERR_ARG
        assert rs.length == 0 and rs.map_channels == 0
    assert b"channel 1" in L.pv_last_error()
    st = (ctypes.c_longlong * 2)(0, 0)
    assert L.pv_varresampler_set_maps(rs._h, 2, None, ok.ctypes.data_as(ctypes.c_void_p), 8, 8) == _lib.PV_ERR_ARG
    assert L.pv_varresampler_set_maps(rs._h, 2, st, None, 8, 8) == _lib.PV_ERR_ARG
    assert L.pv_varresampler_set_maps(rs._h, 0, st, ok.ctypes.data_as(ctypes.c_void_p), 8, 8) == _lib.PV_ERR_ARG
    assert L.pv_varresampler_set_maps(rs._h, 2, st, ok.ctypes.data_as(ctypes.c_void_p), 7, 8) == _lib.PV_ERR_ARG
    rs.set_map(ok, 0)
    # a failed set leaves the maps as they were; more channels than the maps are refused
    assert status_of(lambda: rs.set_map(ok, np.array([0, -1], np.int64))) == _lib.PV_ERR_ARG
    assert rs.map_channels == 2 and rs.length == 512
    x = torch.zeros((3, 1000), device="cuda")
    assert status_of(lambda: rs(x)) == _lib.PV_ERR_ARG
    assert rs(x[:2].contiguous()).shape == (2, 512) and rs(x[0].contiguous()).shape == (512,)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. the pitch map
def pitch_rows():
    """per channel {identity + glide 1 -> 1.5, rate 0.73 + vibrato, rate 1.37 + ratio 1 throughout}
    over the n = 44 final frames the shortest of the three position curves has (every channel of a
    call has the same n): the stretches are 55, 45 and 44 frames long"""
    fast = rate_map(FRAMES, 1.37)
    n = len(fast)
    pos = np.stack([np.arange(n, dtype=np.float64), rate_map(FRAMES, 0.73)[:n], fast])
    ratio = np.stack([vr.glide(n, 1.0, 1.5), vr.vibrato(n), np.ones(n)])
    return pos, ratio


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div", GEOMETRIES)
def test_pitch_map_per_channel(cuda, monkeypatch, N, hop_div, lock):
    import torch
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    pos, ratio = pitch_rows()
    n = pos.shape[1]
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    hop = pv.hopSize
    pv.set_pitch_map(pos, ratio)
    # the reference takes the library's plan per channel (tests/test_varresample_ref.py has checked it)
    plans = [pitch_map_plan(N, hop, pos[c], ratio[c]) for c in range(C)]
    n_s = [len(p[0]) for p in plans]
    assert len(set(n_s)) > 1 and n_s[2] == n
    assert pv.time_map_frames == max(n_s) and pv.time_map_channels == C
    assert pv.pitch_map_output_length == pv.output_length(n)
    out, spec = pv.pitch_map_process(xd)
    assert out.shape == (C, n * hop + N - hop) and spec.shape[1] == FRAMES
    ref = cm.pitchmap_channels(xs, N, hop_div, plans, lock, FRAMES, 0, n)
    errs = channel_errors(out, lambda c: ref[c], C)
    print(f"N={N} hop_div={hop_div} lock={lock} ({n} frames, stretches {n_s}): rms "
          + ", ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= RMS_TOL
    for c in range(C):  # each channel is its own shared-map pitch_map_process
        pv.set_pitch_map(pos[c], ratio[c])
        assert pv.time_map_channels == 0 and pv.time_map_frames == n_s[c]
        alone, _ = pv.pitch_map_process(xd[c:c + 1].contiguous())
        assert torch.equal(alone[0], out[c]), f"channel {c}"
    pv.set_time_map(pos[2])  # the channel at ratio 1 is the time-map stretch of its positions
    plain, _ = pv.time_map_process(xd[2:3].contiguous())
    assert pv.pitch_map_output_length == 0 and torch.equal(plain[0], out[2])
    pv.set_pitch_map(pos, ratio)
    pv.set_pitch_map(None)
    assert pv.pitch_map_output_length == 0 and pv.time_map_frames == 0 and pv.time_map_channels == 0


# ---------------------------------------------------------------- 6. graph capture and refusals
@pytest.mark.parametrize("lock", [False, True])
def test_pitch_map_per_channel_in_a_graph(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xd = to_dev(inputs(N, hop_div))
    pos, ratio = pitch_rows()
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    pv.reserve_spectrum()
    pv.set_pitch_map(pos, ratio)
    ref, none = pv.pitch_map_process(xd, spectrum=False)
    assert none is None
    out = torch.zeros_like(ref)
    L = _lib.lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        st = L.pv_pitchmap_process(pv._h, xd.data_ptr(), xd.stride(0), xd.shape[1], C, FRAMES, None, 0,
                                   out.data_ptr(), out.stride(0), ctypes.c_void_p(s.cuda_stream))
        g.capture_end()
    assert st == _lib.PV_OK
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        out.zero_()


def test_channel_map_refusals(cuda):
    import torch
    L = _lib.lib()
    vp = ctypes.c_void_p
    pos = np.stack([np.arange(8, dtype=np.float64)] * 3)
    ratio = np.full((3, 8), 1.25)
    x = to_dev(np.stack([synth(16 * 256 + 13, 3 + c) for c in range(3)]))
    # REF_COMPAT, PV_PITCH_SHIFT and out_hop != hop handles
    for effect, mode, scale in ((TIME_SHIFT, REF_COMPAT, 1.0), (PITCH_SHIFT, STANDARD, 1.5), (TIME_SHIFT, STANDARD, 1.5)):
        pv = PhaseVocoder(1024, effect, scale, 4, mode=mode, max_frames=16, max_channels=3)
        assert status_of(lambda: pv.set_time_map(pos)) == _lib.PV_ERR_UNSUPPORTED
        assert status_of(lambda: pv.set_pitch_map(pos, ratio)) == _lib.PV_ERR_UNSUPPORTED
        assert L.pv_last_error() and pv.time_map_channels == 0 and pv.time_map_frames == 0
    pv = PhaseVocoder(1024, TIME_SHIFT, 1.0, 4, mode=STANDARD, max_frames=16, max_channels=3)
    assert pv.num_frames(x.shape[1]) == 16
    p = pos.ctypes.data_as(vp)
    r = ratio.ctypes.data_as(vp)

    def untouched():
        return pv.time_map_channels == 0 and pv.time_map_frames == 0 and pv.pitch_map_output_length == 0

    # null pointers; channels outside [1, max_channels]; n_out outside [1, max_frames]
    assert L.pv_timemap_set_channels(pv._h, None, 8, None, 3, 8) == _lib.PV_ERR_ARG and L.pv_last_error()
    assert L.pv_pitchmap_set_channels(pv._h, None, 8, r, 8, 3, 8, 0) == _lib.PV_ERR_ARG and L.pv_last_error()
    assert L.pv_pitchmap_set_channels(pv._h, p, 8, None, 8, 3, 8, 0) == _lib.PV_ERR_ARG and L.pv_last_error()
    for ch in (0, -1, 4):
        assert L.pv_timemap_set_channels(pv._h, p, 8, None, ch, 8) == _lib.PV_ERR_ARG and L.pv_last_error()
        assert L.pv_pitchmap_set_channels(pv._h, p, 8, r, 8, ch, 8, 0) == _lib.PV_ERR_ARG and L.pv_last_error()
    assert status_of(lambda: pv.set_time_map(np.zeros((3, 17)))) == _lib.PV_ERR_ARG
    assert status_of(lambda: pv.set_pitch_map(np.zeros((3, 17)), np.ones((3, 17)))) == _lib.PV_ERR_ARG
    assert L.pv_timemap_set_channels(pv._h, p, 8, None, 3, 0) == _lib.PV_ERR_ARG
    assert L.pv_pitchmap_set_channels(pv._h, p, 8, r, 8, 3, 8, 2) == _lib.PV_ERR_ARG  # quality
    # counts outside [1, n_out]
    for bad in ([8, 0, 8], [8, 8, 9]):
        assert status_of(lambda: pv.set_time_map(pos, bad)) == _lib.PV_ERR_ARG
        assert b"channel" in L.pv_last_error()
    # ld_pos < n_out with more than one channel (one channel: the stride is not read)
    assert L.pv_timemap_set_channels(pv._h, p, 7, None, 3, 8) == _lib.PV_ERR_ARG and L.pv_last_error()
    assert L.pv_pitchmap_set_channels(pv._h, p, 7, r, 8, 3, 8, 0) == _lib.PV_ERR_ARG and L.pv_last_error()
    assert L.pv_pitchmap_set_channels(pv._h, p, 8, r, 7, 3, 8, 0) == _lib.PV_ERR_ARG and L.pv_last_error()
    # a bad position or ratio in a channel other than 0
    for bad in (-1.0, np.nan, np.inf):
        q = pos.copy()
        q[1, 5] = bad
        assert status_of(lambda: pv.set_time_map(q)) == _lib.PV_ERR_ARG and b"channel 1" in L.pv_last_error()
        assert status_of(lambda: pv.set_pitch_map(q, ratio)) == _lib.PV_ERR_ARG and b"channel 1" in L.pv_last_error()
    for bad in (0.2, 4.5, np.nan):
        q = ratio.copy()
        q[2, 0] = bad
        assert status_of(lambda: pv.set_pitch_map(pos, q)) == _lib.PV_ERR_ARG and b"channel 2" in L.pv_last_error()
    # a channel whose stretch needs more than max_frames (8 frames at 2.5: 20)
    q = ratio.copy()
    q[1] = 2.5
    assert status_of(lambda: pv.set_pitch_map(pos, q)) == _lib.PV_ERR_ARG and b"channel 1" in L.pv_last_error()
    assert untouched()
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG  # process before a successful set
    # process with more channels than the map has
    pv.set_time_map(pos[:2])
    assert pv.time_map_channels == 2
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG and L.pv_last_error()
    pv.time_map_process(x[:2].contiguous())
    pv.set_pitch_map(pos[:2], ratio[:2])
    assert pv.time_map_channels == 2 and pv.time_map_frames == 10
    assert status_of(lambda: pv.pitch_map_process(x)) == _lib.PV_ERR_ARG
    pv.pitch_map_process(x[:2].contiguous())
    # a failed set leaves the maps as they were
    assert status_of(lambda: pv.set_pitch_map(pos, q)) == _lib.PV_ERR_ARG
    assert pv.time_map_channels == 2 and pv.pitch_map_output_length == pv.output_length(8)
    # a map that reads past the analysed frames in channel 2 only
    q = pos.copy()
    q[2, 3] = 9.5
    pv.set_time_map(q)
    pv.time_map_process(x, frames=10)
    assert status_of(lambda: pv.time_map_process(x, frames=9)) == _lib.PV_ERR_ARG
    pv.time_map_process(x[:2].contiguous(), frames=8)  # channels 0 and 1 read rows 0 .. 7
    pv.set_time_map(q, [8, 8, 3])                       # ... and channel 2's counted frames too
    pv.time_map_process(x, frames=8)
    assert status_of(lambda: pv.time_map_process(x, frames=7)) == _lib.PV_ERR_ARG
    # the transient mode or the envelope warp on
    pv.set_pitch_map(pos, ratio)
    pv.set_transients("flags")
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG
    assert status_of(lambda: pv.pitch_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_transients("off")
    pv.set_pitch_formant(30)
    assert status_of(lambda: pv.pitch_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_pitch_formant(0)
    pv.pitch_map_process(x)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. three voices corrected in one call
def test_three_voices_corrected_in_one_call(cuda, monkeypatch):
    """One analysis, one pitch_track, pitch_correction on the [3, frames, 2] track, one
    set_pitch_map(2-D), one pitch_map_process (phase lock on), and the output tracked again.  Per
    voice what test_gpu_pitchtrack's end-to-end test asserts for its single voice, with its margin
    1200 log2(1 + 2 F0_TOL) = 0.0035 cents: the median distance to the C-major scale before and
    after against the CPU chain of the same voice (tests/channel_maps_ref.py).  The in-tune voice's
    ratios are 1 where voiced, as far as a track can say: within the distance from the scale that
    the reference's own track reads for that steady voice (0.007 cents at most), plus the margin.
    (Measured on an MI355X: DESIGN.md §3.15.)"""
    N, hop = pr.E2E_N, pr.E2E_N // pr.E2E_HOP_DIV
    xs = cm.voices_input()
    frames = pr.E2E_FRAMES
    tol = 1200.0 * np.log2(1.0 + 2.0 * pr.F0_TOL)
    pv = make_vocoder(monkeypatch, N, pr.E2E_HOP_DIV, TIME_SHIFT, 1.0, 8, max_frames=4 * frames, channels=3,
                      phase_lock=True)
    assert pv.num_frames(xs.shape[1]) == frames
    xd = wide(xs)
    fmin, fmax = pr.E2E_RANGE
    trk = pv.pitch_track(pv.analysis(xd), fmin, fmax).cpu().numpy()
    assert trk.shape == (3, frames, 2)
    ratio = pitch_correction(trk, pr.E2E_A4, MAJOR, strength_min=0.5, retune=1.0)
    assert ratio.shape == (3, frames)
    pv.set_pitch_map(np.stack([np.arange(frames, dtype=np.float64)] * 3), ratio)
    assert pv.time_map_channels == 3
    out, _ = pv.pitch_map_process(xd)
    assert out.shape == (3, frames * hop + N - hop)
    trk2 = pv.pitch_track(pv.analysis(out, frames=frames), fmin, fmax).cpu().numpy()
    for c in range(3):
        ref_before, ref_after, _, ref_cents = cm.voice_reference(c)
        before = pr.median_cents(trk[c, :, 0], trk[c, :, 1])
        after = pr.median_cents(trk2[c, :, 0], trk2[c, :, 1])
        print(f"voice {c}: median cents off the scale before {before:.4f} (reference {ref_before:.4f}), "
              f"after {after:.4f} (reference {ref_after:.4f}); margin {tol:.4f}")
        assert abs(before - ref_before) <= tol
        assert abs(after - ref_after) <= tol
        if c != cm.IN_TUNE:
            assert after <= 0.1 * before
    c = cm.IN_TUNE
    sel = slice(pr.E2E_EDGE, frames - pr.E2E_EDGE)
    voiced = (trk[c, sel, 0] > 0) & (trk[c, sel, 1] >= 0.5)
    assert voiced.all()
    reads = float(np.max(cm.voice_reference(c)[3][sel]))
    cents = 1200.0 * np.abs(np.log2(ratio[c, sel]))
    print(f"in-tune voice: ratios within {cents.max():.5f} cents of 1 (the reference's track reads up to "
          f"{reads:.5f} off the scale)")
    assert reads < 0.01 and cents.max() <= reads + tol
