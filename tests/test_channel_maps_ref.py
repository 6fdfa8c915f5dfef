"""The host side of the maps set per channel, no GPU: the batched correction
planner is one plan per row, the new symbols are exported, and the per-channel reference helpers
(tests/channel_maps_ref.py) are the single-map references when every channel has the same map and
full counts, which is what lets them judge the GPU."""
import ctypes

import numpy as np

import channel_maps_ref as cm
import pitchtrack_ref as pr
import timemap_ref as tm
import varresample_ref as vr
from pvamd import MAJOR, _lib, pitch_correction, rate_map
from signals import synth

A4 = pr.E2E_A4


def tracks():
    """three voices' {f0, strength}: flat, sharp with an unvoiced stretch, in tune"""
    rng = np.random.default_rng(5)
    frames = 40
    trk = np.zeros((3, frames, 2), np.float32)
    for c, cents in enumerate((-35.0, 30.0, 0.0)):
        trk[c, :, 0] = A4 * 2.0 ** ((64 - 69 + (cents + rng.uniform(-3, 3, frames)) / 100.0) / 12.0)
        trk[c, :, 1] = 0.9
    trk[1, 10:17, 1] = 0.2
    return trk


def test_batched_correction_is_the_row_by_row_loop():
    trk = tracks()
    got = pitch_correction(trk, A4, MAJOR, retune=0.5)
    assert got.shape == (3, trk.shape[1]) and got.dtype == np.float64
    for c in range(3):
        assert np.array_equal(got[c], pitch_correction(trk[c], A4, MAJOR, retune=0.5))
        assert np.allclose(got[c], pr.correction(trk[c], A4, MAJOR, 0.5, 0.5), rtol=1e-12, atol=0)
    # one row of positions for all voices, or one per voice
    pos = np.linspace(0.0, trk.shape[1] - 1.0, 55)
    both = np.stack([pos, pos[::-1], pos])
    shared, own = pitch_correction(trk, A4, MAJOR, pos=pos), pitch_correction(trk, A4, MAJOR, pos=both)
    assert shared.shape == own.shape == (3, 55)
    for c in range(3):
        assert np.array_equal(shared[c], pitch_correction(trk[c], A4, MAJOR, pos=pos))
        assert np.array_equal(own[c], pitch_correction(trk[c], A4, MAJOR, pos=both[c]))
    # a 2-D track keeps its result: one voice, one row
    one = pitch_correction(trk[0], A4, MAJOR)
    assert one.shape == (trk.shape[1],) and np.array_equal(one, pitch_correction(trk[:1], A4, MAJOR)[0])


def test_the_new_symbols_are_exported_and_refuse_null():
    L = _lib.lib()
    one = (ctypes.c_double * 1)(0.0)
    assert L.pv_timemap_channels(None) == 0 and L.pv_varresample_map_channels(None) == 0
    assert L.pv_timemap_set_channels(None, one, 1, None, 1, 1) == _lib.PV_ERR_ARG and L.pv_last_error()
    assert L.pv_pitchmap_set_channels(None, one, 1, one, 1, 1, 1, 0) == _lib.PV_ERR_ARG and L.pv_last_error()
    step = (ctypes.c_longlong * 1)(1 << 32)
    assert L.pv_varresampler_set_maps(None, 1, step, step, 1, 1) == _lib.PV_ERR_ARG and L.pv_last_error()


def test_timemap_helper_is_the_single_map_reference():
    N, hop_div, frames = 256, 4, 20
    hop = N // hop_div
    xs = np.stack([synth(frames * hop + 13, 700 + c) for c in range(2)])
    pos = rate_map(frames, 0.73)
    for lock in (False, True):
        got = cm.timemap_channels(xs, N, hop_div, np.stack([pos, pos]), None, lock, frames)
        for c in range(2):
            assert np.array_equal(got[c], tm.timemap_process(xs[c], N, hop_div, pos, lock, frames))
    # a shorter count: that channel's own stretch, then zeros
    rows, counts = cm.padded_rows([pos, pos[:9]])
    assert counts.tolist() == [len(pos), 9] and np.isnan(rows[1, 9:]).all()
    got = cm.timemap_channels(xs, N, hop_div, rows, counts, False, frames)
    short = tm.timemap_process(xs[1], N, hop_div, pos[:9], False, frames)
    assert np.array_equal(got[1, :len(short)], short) and not got[1, len(short):].any()
    assert got.shape[1] == len(pos) * hop + N - hop


def test_resampler_helpers_are_the_single_map_references():
    xs = np.stack([synth(900, 40 + c) for c in range(2)])
    B = 64
    steps = vr.ratio_steps(vr.glide(8, 0.8, 1.4))
    got = cm.varresample_channels(xs, [steps, steps], B, [3, 3], 0, 500)
    assert np.array_equal(got, vr.varresample(xs, steps, B, 3, 0, 500))
    N, hop_div, frames = 256, 4, 20
    hop = N // hop_div
    xs = np.stack([synth(frames * hop + 13, 700 + c) for c in range(2)])
    pos = np.arange(frames, dtype=np.float64)
    plan = vr.plan(N, hop, pos, vr.vibrato(frames))
    got = cm.pitchmap_channels(xs, N, hop_div, [plan, plan], True, frames, 0, frames)
    for c in range(2):
        assert np.array_equal(got[c], vr.pitchmap_process(xs[c], N, hop_div, plan[0], plan[1], True, frames, 0, frames))


def test_the_three_voices_differ_where_they_should():
    xs = cm.voices_input()
    assert xs.shape[0] == 3 and np.array_equal(xs[0], pr.e2e_input())
    before = [cm.voice_reference(c)[0] for c in range(3)]
    after = [cm.voice_reference(c)[1] for c in range(3)]
    print(f"reference medians before {before}, after {after}")
    assert abs(before[0] - pr.e2e_reference()[0]) == 0 and abs(after[0] - pr.e2e_reference()[1]) == 0
    assert before[0] > 30 and before[1] > 25 and before[cm.IN_TUNE] < 0.1
    # the stretches differ in length: under the note raises the pitch (more stretch frames)
    sums = [cm.voice_reference(c)[2].sum() for c in range(3)]
    assert sums[0] > sums[2] > sums[1]
