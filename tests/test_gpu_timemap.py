"""Time-map stretch on the GPU (pv_timemap_process; k_map_sum, k_map_carry and k_synthesis in the
map modes) against the fp64 reference tests/timemap_ref.py: every overlap-add variant of the
synthesis, natural and packed rows, locked and unlocked, maps that stretch, compress, ramp,
freeze and reverse, graph capture and the refusals.  3 channels x 60 analysed frames, output
frames in runs of 8 (rate 0.73: 81 output frames, 11 runs, 3 workgroups, the last run partial) or
16 (PV_RUN_FRAMES).  The phases are the same integers on both sides, so the project's RMS_TOL
holds as for every other synthesis mode with this sincos, FFT and overlap-add."""
import ctypes
import functools

import numpy as np
import pytest

import pvref
import timemap_ref as tm
from gpu_helpers import (MAP_INPUTS, RMS_TOL, channel_errors, make_vocoder, status_of, stretch_inputs, to_dev,
                         write_pcm16)
from pvamd import PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, PhaseVocoder, _lib, rate_map
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 3
FRAMES = MAP_INPUTS["frames"]
MAX_FRAMES = 96

GEOMETRIES = [
    (256, 4),    # LDS ring
    (512, 4),    # hop 128: register overlap-add, one slot per frame
    (1024, 4),   # L = 512, two slots
    (1024, 2),   # four slots
    (2048, 4),   # L = 1024
    (2048, 8),
    (512, 3),    # hop 170: the ring, an unaligned hop
]

IDENTITY = np.arange(FRAMES, dtype=np.float64)
MAPS = {
    "identity": IDENTITY,
    "rate 0.73": rate_map(FRAMES, 0.73),
    "rate 1.37": rate_map(FRAMES, 1.37),
    "ramp 0.5 -> 2": tm.ramp_map(FRAMES, 0.5, 2.0),
    "scrub": tm.scrub_map(),
}


inputs = functools.partial(stretch_inputs, **MAP_INPUTS, channels=C)


def make(monkeypatch, N, hop_div, F=8, **kw):
    pv = make_vocoder(monkeypatch, N, hop_div, TIME_SHIFT, 1.0, F, max_frames=MAX_FRAMES, channels=C, **kw)
    assert pv.outHopSize == pv.hopSize
    return pv


def check_against_reference(out, xs, N, hop_div, pos, lock, what):
    worst = max(channel_errors(out, lambda c: tm.cached(xs[c], N, hop_div, pos, lock, FRAMES), xs.shape[0]))
    print(f"N={N} hop_div={hop_div} lock={lock} {what} ({len(pos)} output frames): rms {worst:.3e}")
    assert worst <= RMS_TOL, f"{what}: rms {worst}"


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div", GEOMETRIES)
def test_map_parity(cuda, monkeypatch, N, hop_div, lock):
    import torch
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    assert pv.time_map_frames == 0
    assert len(MAPS["rate 0.73"]) == 81 and MAPS["scrub"][-1] == FRAMES - 1
    for what, pos in MAPS.items():
        pv.set_time_map(pos)
        assert pv.time_map_frames == len(pos)
        out, spec = pv.time_map_process(xd)
        assert out.shape == (C, pv.output_length(len(pos))) and spec.shape[1] == FRAMES
        check_against_reference(out, xs, N, hop_div, pos, lock, what)
        if what == "identity":
            # ... which is the handle's own scale-1 stretch, up to the 2^-31-turn quantisation
            own, _ = pv.process(xd)
            err = max(rms(out[c].cpu().numpy(), own[c].cpu().numpy()) for c in range(C))
            print(f"  identity against the handle's pv_process: rms {err:.3e}")
            assert own.shape == out.shape and err <= RMS_TOL
        if what == "rate 0.73":
            again, _ = pv.time_map_process(xd)  # a second run is the same bits
            assert torch.equal(out, again)
    pv.set_time_map(None)
    assert pv.time_map_frames == 0


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div", [(256, 4), (1024, 4)])
def test_short_maps(cuda, monkeypatch, N, hop_div, lock):
    """n_out = 1 (one frame), 8 (exactly one run) and 9 (a run and one frame)"""
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    for n_out in (1, 8, 9):
        pos = 3.25 + 1.6 * np.arange(n_out)
        pv.set_time_map(pos)
        out, _ = pv.time_map_process(xd)
        check_against_reference(out, xs, N, hop_div, pos, lock, f"n_out {n_out}")


@pytest.mark.parametrize("lock", [False, True])
def test_packed_rows_and_without_spectrum(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, hop_div, phase_lock=lock, spec_layout=_lib.PV_SPEC_PACKED)
    for what in ("scrub", "rate 0.73"):
        pv.set_time_map(MAPS[what])
        out, spec = pv.time_map_process(xd)
        check_against_reference(out, xs, N, hop_div, MAPS[what], lock, what + " packed")
        out2, none = pv.time_map_process(xd, spectrum=False)
        assert none is None and torch.equal(out, out2)
    # the rows are pv_analysis's
    assert torch.equal(spec, pv.analysis(xd))


@pytest.mark.parametrize("lock", [False, True])
def test_runs_of_16_and_one_channel_alone(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    pos = MAPS["rate 0.73"]
    pv8 = make(monkeypatch, N, hop_div, 8, phase_lock=lock)
    pv8.set_time_map(pos)
    out8, _ = pv8.time_map_process(xd)
    pv16 = make(monkeypatch, N, hop_div, 16, phase_lock=lock)
    pv16.set_time_map(pos)
    out16, _ = pv16.time_map_process(xd)
    check_against_reference(out16, xs, N, hop_div, pos, lock, "runs of 16")
    err = max(rms(out8[c].cpu().numpy(), out16[c].cpu().numpy()) for c in range(C))
    print(f"runs of 8 against runs of 16: rms {err:.3e}")
    assert err <= RMS_TOL
    # a channel run alone is its row of the batch, bit for bit
    one, _ = pv8.time_map_process(xd[1:2].contiguous())
    assert torch.equal(one[0], out8[1])


def test_replacing_the_map_and_leaving_pv_process_alone(cuda, monkeypatch):
    import torch
    N, hop_div = 1024, 4
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    fresh = make(monkeypatch, N, hop_div)
    want, want_spec = fresh.process(xd)
    pv = make(monkeypatch, N, hop_div)
    pv.set_time_map(MAPS["rate 1.37"])
    a, _ = pv.time_map_process(xd)
    pv.set_time_map(MAPS["scrub"])
    b, _ = pv.time_map_process(xd)
    check_against_reference(a, xs, N, hop_div, MAPS["rate 1.37"], False, "first map")
    check_against_reference(b, xs, N, hop_div, MAPS["scrub"], False, "second map")
    # a handle with a map set still runs its own pv_process, the single launch included
    assert bool(pv.single_launch) == bool(fresh.single_launch)
    got, got_spec = pv.process(xd)
    assert torch.equal(got, want) and torch.equal(got_spec, want_spec)
    pv.profile(True)
    pv.time_map_process(xd)
    names = pv.profile_read()
    for k in ("analysis", "map_sum", "map_carry", "synthesis_map", "seam"):
        assert k in names, names


@pytest.mark.parametrize("lock", [False, True])
def test_map_process_captures_into_a_graph(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    pos = MAPS["rate 0.73"]
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    pv.set_time_map(pos)
    ref, _ = pv.time_map_process(xd)
    spec = pv.alloc_spec(C, FRAMES)
    out = pv.alloc_out(C, len(pos))
    L = _lib.lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        st = L.pv_timemap_process(pv._h, xd.data_ptr(), xd.stride(0), xd.shape[1], C, FRAMES, spec.data_ptr(),
                                  spec.stride(0) // 2, out.data_ptr(), out.stride(0), ctypes.c_void_p(s.cuda_stream))
        g.capture_end()
    assert st == _lib.PV_OK
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        out.zero_()


def test_pv_main_rate(cuda, tmp_path):
    """the C++ driver: --rate composes with --phase-lock and refuses a pitch-shift run"""
    import os
    import subprocess

    from conftest import GOLDEN, ROOT
    pv_main = os.path.join(ROOT, "phase-vocoder_amd", "build", "pv_main")
    x = np.load(os.path.join(GOLDEN, "sine440_ch0_32768.npy"))[:16384].astype(np.float32)
    wav_in, dump = str(tmp_path / "in.wav"), str(tmp_path / "o.f32")
    write_pcm16(wav_in, x)
    args = ["--N", "1024", "--hopdiv", "4", "--mode", "std", "--rate", "0.73"]
    r = subprocess.run([pv_main, wav_in, "t", str(tmp_path / "o.wav"), *args, "--phase-lock", "--dump-f32", dump],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dump, np.float32)
    frames = pvref.num_frames(len(x), 256)
    ref = tm.timemap_process(x, 1024, 4, rate_map(frames, 0.73), True)
    assert len(got) == len(ref)
    err = rms(got, ref)
    print(f"pv_main --rate 0.73 --phase-lock ({len(rate_map(frames, 0.73))} output frames): rms {err:.3e}")
    assert err <= RMS_TOL
    r = subprocess.run([pv_main, wav_in, "p", str(tmp_path / "o2.wav"), *args], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "--rate" in r.stderr


def test_timemap_refusals(cuda):
    L = _lib.lib()
    pos = np.arange(8, dtype=np.float64)
    x = to_dev(synth(16 * 256 + 13, 3))
    # REF_COMPAT, PV_PITCH_SHIFT and out_hop != hop handles
    for effect, mode, scale in ((TIME_SHIFT, REF_COMPAT, 1.0), (PITCH_SHIFT, STANDARD, 1.5), (TIME_SHIFT, STANDARD, 1.5)):
        pv = PhaseVocoder(1024, effect, scale, 4, mode=mode, max_frames=16)
        assert status_of(lambda: pv.set_time_map(pos)) == _lib.PV_ERR_UNSUPPORTED
        assert L.pv_last_error()
        assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_UNSUPPORTED
        assert pv.time_map_frames == 0
    pv = PhaseVocoder(1024, TIME_SHIFT, 1.0, 4, mode=STANDARD, max_frames=16)
    frames = pv.num_frames(x.shape[0])
    assert frames == 16
    # process before a successful set
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG
    for bad in ([-1.0], [np.nan], [0.0, np.inf], np.arange(17, dtype=np.float64)):  # (17 > max_frames)
        assert status_of(lambda: pv.set_time_map(bad)) == _lib.PV_ERR_ARG
    one = (ctypes.c_double * 1)(0.0)
    assert L.pv_timemap_set(pv._h, one, 0) == _lib.PV_ERR_ARG
    assert L.pv_timemap_set(pv._h, None, 3) == _lib.PV_ERR_ARG
    assert pv.time_map_frames == 0
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_time_map(pos)
    # a failed set leaves the map as it was
    assert status_of(lambda: pv.set_time_map([-1.0])) == _lib.PV_ERR_ARG and pv.time_map_frames == 8
    pv.time_map_process(x)
    # frames < 1 with channels > 0; channels = 0 does nothing
    assert status_of(lambda: pv.time_map_process(x, frames=0)) == _lib.PV_ERR_ARG
    assert L.pv_timemap_process(pv._h, None, 0, 0, 0, 0, None, 0, None, 0, None) == _lib.PV_OK
    # max i_u > frames - 1
    assert status_of(lambda: pv.time_map_process(x, frames=7)) == _lib.PV_ERR_ARG
    pv.time_map_process(x, frames=8)
    pv.set_time_map([15.0, 15.9])
    pv.time_map_process(x)
    pv.set_time_map([16.0])
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_time_map(pos)
    # the transient reset and the envelope warp under a map
    pv.set_transients("flags")
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_transients("off")
    pv.set_pitch_formant(30)
    assert status_of(lambda: pv.time_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_pitch_formant(0)
    pv.time_map_process(x)
    # capacity
    import torch
    two = torch.zeros((2, x.shape[0]), dtype=torch.float32, device="cuda")
    assert status_of(lambda: pv.time_map_process(two)) == _lib.PV_ERR_ARG  # 2 channels > max_channels
