"""The variable-rate resampler on the GPU (pv_varresample, k_var_resample) against the fp64 reference
tests/varresample_ref.py, and the pitch map built on it (pv_pitchmap_process: the time-map stretch,
locked or not, then the variable-rate resampling) against the reference composition.  C = 3,
n_in = 5003: several tiles of 1024 outputs and a partial one; block lengths below, across and above
the tile; NaN-padded input rows an odd stride apart and sentinel-padded output rows throughout."""
import ctypes
import functools

import numpy as np
import pytest

import pvref
import varresample_ref as vr
from gpu_helpers import (MAP_INPUTS, RMS_TOL, channel_errors, make_vocoder, run_padded, status_of, stretch_inputs,
                         to_dev, to_dev_copy, write_pcm16)
from pvamd import (PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, PhaseVocoder, Resampler, VarResampler, _lib,
                   pitch_map_plan, rate_map)
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 3
N_IN = 5003
PAD = 38  # rows n_in + 38 floats apart: the channels' rows start at different offsets in a 16-byte segment
ONE = 1 << 32

_xs = {}


def signal(n=N_IN):
    if n not in _xs:
        _xs[n] = np.stack([synth(n, 4400 + 13 * c) for c in range(C)])
        _xs[n].setflags(write=False)
    return _xs[n]


def blocks_for(B, mean_ratio, cap=6000):
    """blocks that read about the whole input, at most `cap` outputs"""
    return max(2, int(np.ceil(min(N_IN / mean_ratio, cap) / B)))


def case_map(name, B):
    """(steps as Python integers, start) of a named map"""
    if name.startswith("const "):
        p, q = (int(v) for v in name[6:].split("/"))
        nb = blocks_for(B, p / q)
        return [ONE * p // q] * nb, 0
    if name == "glide":
        nb = blocks_for(B, 1.1)
        return vr.ratio_steps(vr.glide(nb, 0.5, 2.0)), 0
    if name == "vibrato":
        nb = blocks_for(B, 1.0)
        return vr.ratio_steps(vr.vibrato(nb)), 5 * ONE + 0x9e3779b9
    if name == "tail":  # the last blocks read past n_in + W: zeros
        return [ONE * 3 // 2] * (-(-N_IN // B)), 3 * ONE + 12345
    raise KeyError(name)


PARITY_CASES = [
    # map, B, quality
    ("const 3/2", 64, 0), ("const 3/4", 64, 0), ("const 1/4", 64, 0), ("const 4/1", 64, 0),
    ("glide", 64, 0), ("vibrato", 64, 0), ("tail", 64, 0),
    ("glide", 170, 0), ("glide", 1024, 0), ("glide", 4096, 0), ("vibrato", 170, 0),
    ("glide", 64, 1), ("const 4/1", 64, 1), ("vibrato", 1024, 1),
]


@pytest.mark.parametrize("name,B,quality", PARITY_CASES)
def test_varresample_parity(cuda, name, B, quality):
    xs = signal()
    steps, start = case_map(name, B)
    rs = VarResampler(B, quality, max_blocks=len(steps) + 3)
    assert rs.length == 0
    rs.set_map(np.array(steps, np.int64), start)
    assert rs.length == len(steps) * B
    n_out = rs.length - 7  # a multiple of neither the block nor the tile
    assert n_out % B and n_out % 1024
    g = run_padded(rs, xs, PAD, n_out)
    assert np.isfinite(g).all()
    ref = vr.varresample(xs, steps, B, start, quality, n_out)
    assert g.shape == ref.shape
    if name == "tail":
        assert not ref[:, -200:].any() and not g[:, -200:].any()
    for c in range(C):
        err = rms(g[c], ref[c])
        print(f"{name} B={B} quality {quality} channel {c} ({n_out} outputs): rms {err:.3e}, "
              f"max {np.max(np.abs(g[c] - ref[c])):.3e}")
        assert err <= RMS_TOL


@pytest.mark.parametrize("p,q", [(3, 2), (3, 4)])
def test_constant_map_against_the_polyphase_kernel(cuda, p, q):
    xs = signal()
    poly = Resampler(p, q, 0)
    n_out = poly.length(N_IN)
    want = poly(to_dev_copy(xs)).cpu().numpy()
    B = 64
    rs = VarResampler(B, 0, max_blocks=-(-n_out // B))
    rs.set_map(np.full(-(-n_out // B), ONE * p // q, np.int64))
    g = run_padded(rs, xs, PAD, n_out)
    for c in range(C):
        err = rms(g[c], want[c])
        print(f"{p}:{q} channel {c}: rms against k_resample {err:.3e}")
        assert err <= RMS_TOL


def test_ratios_and_steps_set_the_same_map(cuda):
    import torch
    xd = to_dev_copy(signal())
    ratios = vr.vibrato(40)
    a, b = VarResampler(64, 0, max_blocks=40), VarResampler(64, 0, max_blocks=40)
    a.set_map(ratios)
    b.set_map(np.array(vr.ratio_steps(ratios), np.int64))
    assert torch.equal(a(xd), b(xd))


def test_same_bits_again_alone_and_in_a_graph(cuda):
    import torch
    xs = signal()
    xd = to_dev_copy(xs)
    steps, start = case_map("glide", 170)
    rs = VarResampler(170, 0, max_blocks=len(steps))
    rs.set_map(np.array(steps, np.int64), start)
    first = rs(xd)
    assert torch.equal(rs(xd), first)                       # a second run
    assert torch.equal(rs(xd[1].contiguous()), first[1])    # a channel alone is its row of the batch
    out = torch.empty_like(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rs(xd, out=out)
    torch.cuda.synchronize()
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)


def test_all_ones_map_is_the_shifted_copy(cuda):
    xs = signal()
    B = 64
    nb = -(-N_IN // B) + 2
    rs = VarResampler(B, 1, max_blocks=nb)
    rs.set_map(np.full(nb, ONE, np.int64), 7 * ONE)
    g = run_padded(rs, xs, PAD, rs.length - 7)
    assert np.array_equal(g[:, :N_IN - 7], xs[:, 7:]) and not g[:, N_IN - 7:].any()
    rs.set_map(np.ones(nb))  # ratios 1.0, start 0
    assert np.array_equal(run_padded(rs, xs, PAD, N_IN), xs)
    # a later map with a fraction goes through the filter again
    rs.set_map(np.full(nb, ONE, np.int64), 7 * ONE + 1)
    g = run_padded(rs, xs, PAD, N_IN - 7)
    ref = vr.varresample(xs, [ONE] * nb, B, 7 * ONE + 1, 1, N_IN - 7)
    assert not np.array_equal(g, xs[:, 7:]) and max(rms(g[c], ref[c]) for c in range(C)) <= RMS_TOL


def test_varresampler_refusals(cuda):
    import torch
    L = _lib.lib()
    for quality, block, max_blocks in ((2, 64, 8), (0, 15, 8), (0, 4097, 8), (0, 64, 0)):
        assert status_of(lambda: VarResampler(block, quality, max_blocks=max_blocks)) == _lib.PV_ERR_ARG
    rs = VarResampler(64, 0, max_blocks=8)
    x = torch.zeros(4000, device="cuda")
    assert status_of(lambda: rs(x, n_out=0)) == _lib.PV_ERR_ARG              # before a map
    for steps in ([], [ONE] * 9, [ONE, (1 << 30) - 1], [(1 << 34) + 1]):
        assert status_of(lambda: rs.set_map(np.array(steps, np.int64))) == _lib.PV_ERR_ARG
        assert L.pv_last_error()
    assert status_of(lambda: rs.set_map(np.array([ONE], np.int64), -1)) == _lib.PV_ERR_ARG
    assert status_of(lambda: rs.set_map(np.array([ONE], np.int64), (1 << 62) - 10)) == _lib.PV_ERR_ARG
    assert status_of(lambda: rs.set_map([1.0, 4.5])) == _lib.PV_ERR_ARG
    assert L.pv_varresampler_set_map(rs._h, 0, None, 1) == _lib.PV_ERR_ARG
    assert rs.length == 0
    rs.set_map([1.5] * 8)
    # a failed set leaves the map as it was
    assert status_of(lambda: rs.set_map(np.array([1], np.int64))) == _lib.PV_ERR_ARG and rs.length == 512
    y = torch.zeros(600, device="cuda")
    assert L.pv_varresample(rs._h, x.data_ptr(), 4000, 4000, 1, y.data_ptr(), 600, 513, None) == _lib.PV_ERR_ARG
    assert L.pv_varresample(rs._h, x.data_ptr(), 4000, 4000, 1, y.data_ptr(), 600, -1, None) == _lib.PV_ERR_ARG
    assert L.pv_varresample(rs._h, None, 4000, 4000, 1, y.data_ptr(), 600, 512, None) == _lib.PV_ERR_ARG
    assert L.pv_varresample(rs._h, x.data_ptr(), 4000, 4000, 1, None, 600, 512, None) == _lib.PV_ERR_ARG
    # channels or n_out 0: nothing is done
    assert L.pv_varresample(rs._h, None, 0, 0, 0, None, 0, 512, None) == _lib.PV_OK
    assert L.pv_varresample(rs._h, None, 0, 100, 2, None, 0, 0, None) == _lib.PV_OK
    # x and y must not overlap; rows must hold their samples
    assert status_of(lambda: rs(x[:3000], n_out=512, out=x[2900:2900 + 512])) == _lib.PV_ERR_ARG
    two = torch.zeros((2, 1000), device="cuda")
    yy = torch.zeros((2, 512), device="cuda")
    assert L.pv_varresample(rs._h, two.data_ptr(), 999, 1000, 2, yy.data_ptr(), 512, 512, None) == _lib.PV_ERR_ARG
    assert L.pv_varresample(rs._h, two.data_ptr(), 1000, 1000, 2, yy.data_ptr(), 511, 512, None) == _lib.PV_ERR_ARG
    assert L.pv_varresample(rs._h, two.data_ptr(), 1000, 1000, 2, yy.data_ptr(), 512, 512, None) == _lib.PV_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------ pv_pitchmap_process
FRAMES = MAP_INPUTS["frames"]
MAX_FRAMES = 128
GEOMETRIES = [(256, 4), (512, 3), (1024, 4)]

inputs = functools.partial(stretch_inputs, **MAP_INPUTS, channels=C)  # (the stretch's references are shared)


def pitch_maps():
    ident = np.arange(FRAMES, dtype=np.float64)
    slow, fast = rate_map(FRAMES, 0.73), rate_map(FRAMES, 1.37)
    return {"identity + glide 1 -> 1.5": (ident, vr.glide(len(ident), 1.0, 1.5)),
            "rate 0.73 + vibrato": (slow, vr.vibrato(len(slow))),
            "rate 1.37 + glide 1.5 -> 0.75": (fast, vr.glide(len(fast), 1.5, 0.75))}


def make(monkeypatch, N, hop_div, **kw):
    pv = make_vocoder(monkeypatch, N, hop_div, TIME_SHIFT, 1.0, max_frames=MAX_FRAMES, channels=C, **kw)
    assert pv.outHopSize == pv.hopSize
    return pv


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div", GEOMETRIES)
def test_pitch_map_parity(cuda, monkeypatch, N, hop_div, lock):
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    hop = pv.hopSize
    assert pv.pitch_map_output_length == 0
    for what, (pos, ratio) in pitch_maps().items():
        n = len(pos)
        pv.set_pitch_map(pos, ratio)
        # the reference takes the library's plan (tests/test_varresample_ref.py has checked it)
        pos_s, steps = pitch_map_plan(N, hop, pos, ratio)
        assert pv.time_map_frames == len(pos_s) and pv.pitch_map_output_length == pv.output_length(n)
        out, spec = pv.pitch_map_process(xd)
        assert out.shape == (C, n * hop + N - hop) and spec.shape[1] == FRAMES
        worst = max(channel_errors(out, lambda c: vr.cached(xs[c], N, hop_div, pos_s, steps, lock, FRAMES, 0, n), C))
        print(f"N={N} hop_div={hop_div} lock={lock} {what} ({n} frames, stretch {len(pos_s)}): rms {worst:.3e}")
        assert worst <= RMS_TOL, what
    pv.set_pitch_map(None)
    assert pv.pitch_map_output_length == 0 and pv.time_map_frames == 0


@pytest.mark.parametrize("lock", [False, True])
def test_ratio_one_is_the_time_map_stretch(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xd = to_dev(inputs(N, hop_div))
    pos = rate_map(FRAMES, 0.73)
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    pv.set_time_map(pos)
    want, wspec = pv.time_map_process(xd)
    pv.set_pitch_map(pos, np.ones(len(pos)), quality=1)
    got, gspec = pv.pitch_map_process(xd)
    assert torch.equal(got, want) and torch.equal(gspec, wspec)


def test_other_calls_and_clearing(cuda, monkeypatch):
    import torch
    N, hop_div = 1024, 4
    xd = to_dev(inputs(N, hop_div))
    pos, ratio = pitch_maps()["rate 0.73 + vibrato"]
    fresh = make(monkeypatch, N, hop_div)
    want, want_spec = fresh.process(xd)
    pv = make(monkeypatch, N, hop_div)
    pv.set_pitch_map(pos, ratio)
    a, _ = pv.pitch_map_process(xd)
    # a handle with a pitch map set still runs its own pv_process, the single launch included
    assert bool(pv.single_launch) == bool(fresh.single_launch)
    got, got_spec = pv.process(xd)
    assert torch.equal(got, want) and torch.equal(got_spec, want_spec)
    b, _ = pv.pitch_map_process(xd)
    assert torch.equal(a, b)
    pv.profile(True)
    pv.pitch_map_process(xd)
    names = pv.profile_read()
    for k in ("analysis", "map_sum", "map_carry", "synthesis_map", "seam", "var_resample"):
        assert k in names and names[k][1] == 1, names
    pv.profile(False)
    # the caller's own time map turns the pitch map off
    pv.set_time_map(pos)
    assert pv.pitch_map_output_length == 0 and pv.time_map_frames == len(pos)
    assert status_of(lambda: pv.pitch_map_process(xd)) == _lib.PV_ERR_ARG
    pv.set_pitch_map(pos, ratio)
    pv.set_time_map(None)
    assert pv.pitch_map_output_length == 0
    assert status_of(lambda: pv.pitch_map_process(xd)) == _lib.PV_ERR_ARG
    # a new quality replaces the resampler
    pv.set_pitch_map(pos, ratio, quality=1)
    c, _ = pv.pitch_map_process(xd)
    err = max(rms(a[ch].cpu().numpy(), c[ch].cpu().numpy()) for ch in range(C))
    assert 0.0 < err < 1e-2


@pytest.mark.parametrize("lock", [False, True])
def test_without_spectrum_and_in_a_graph(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xd = to_dev(inputs(N, hop_div))
    pos, ratio = pitch_maps()["identity + glide 1 -> 1.5"]
    pv = make(monkeypatch, N, hop_div, phase_lock=lock)
    pv.set_pitch_map(pos, ratio)
    ref, _ = pv.pitch_map_process(xd)
    out2, none = pv.pitch_map_process(xd, spectrum=False)
    assert none is None and torch.equal(out2, ref)
    spec = pv.alloc_spec(C, FRAMES)
    out = torch.zeros_like(ref)
    L = _lib.lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        st = L.pv_pitchmap_process(pv._h, xd.data_ptr(), xd.stride(0), xd.shape[1], C, FRAMES, spec.data_ptr(),
                                   spec.stride(0) // 2, out.data_ptr(), out.stride(0), ctypes.c_void_p(s.cuda_stream))
        g.capture_end()
    assert st == _lib.PV_OK
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        out.zero_()


def test_pitch_map_refusals(cuda):
    L = _lib.lib()
    pos, ratio = np.arange(8, dtype=np.float64), np.full(8, 1.25)
    x = to_dev(synth(16 * 256 + 13, 3))
    for effect, mode, scale in ((TIME_SHIFT, REF_COMPAT, 1.0), (PITCH_SHIFT, STANDARD, 1.5), (TIME_SHIFT, STANDARD, 1.5)):
        pv = PhaseVocoder(1024, effect, scale, 4, mode=mode, max_frames=16)
        assert status_of(lambda: pv.set_pitch_map(pos, ratio)) == _lib.PV_ERR_UNSUPPORTED
        assert L.pv_last_error()
        assert status_of(lambda: pv.pitch_map_process(x)) == _lib.PV_ERR_UNSUPPORTED
        assert pv.pitch_map_output_length == 0
    pv = PhaseVocoder(1024, TIME_SHIFT, 1.0, 4, mode=STANDARD, max_frames=16)
    assert pv.num_frames(x.shape[0]) == 16
    assert status_of(lambda: pv.pitch_map_process(x)) == _lib.PV_ERR_ARG   # process before set
    for bad_pos, bad_ratio, quality in (([-1.0], [1.0], 0), ([0.0], [0.2], 0), ([0.0], [np.nan], 0), ([0.0], [1.0], 2),
                                        (np.arange(17.0), np.ones(17), 0),       # n > max_frames
                                        (np.arange(8.0), np.full(8, 2.5), 0)):   # n_s = 20 > max_frames
        assert status_of(lambda: pv.set_pitch_map(bad_pos, bad_ratio, quality)) == _lib.PV_ERR_ARG
        assert pv.pitch_map_output_length == 0 and pv.time_map_frames == 0
    one = (ctypes.c_double * 1)(1.0)
    assert L.pv_pitchmap_set(pv._h, one, None, 1, 0) == _lib.PV_ERR_ARG
    assert L.pv_pitchmap_set(pv._h, None, one, 1, 0) == _lib.PV_ERR_ARG
    pv.set_pitch_map(pos, ratio)
    assert pv.time_map_frames == 10 and pv.pitch_map_output_length == pv.output_length(8)
    # a failed set leaves the map as it was
    assert status_of(lambda: pv.set_pitch_map([0.0], [9.0])) == _lib.PV_ERR_ARG
    assert pv.pitch_map_output_length == pv.output_length(8)
    pv.pitch_map_process(x)
    assert status_of(lambda: pv.pitch_map_process(x, frames=0)) == _lib.PV_ERR_ARG
    assert status_of(lambda: pv.pitch_map_process(x, frames=7)) == _lib.PV_ERR_ARG   # the map reads row 7
    assert L.pv_pitchmap_process(pv._h, None, 0, 0, 0, 0, None, 0, None, 0, None) == _lib.PV_OK
    pv.set_transients("flags")
    assert status_of(lambda: pv.pitch_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_transients("off")
    pv.set_pitch_formant(30)
    assert status_of(lambda: pv.pitch_map_process(x)) == _lib.PV_ERR_ARG
    pv.set_pitch_formant(0)
    pv.pitch_map_process(x)


def test_pv_main_pitch_glide(cuda, tmp_path):
    """the C++ driver: --pitch-glide composes with --rate and --phase-lock and refuses a pitch-shift run"""
    import os
    import subprocess

    from conftest import GOLDEN, ROOT
    pv_main = os.path.join(ROOT, "phase-vocoder_amd", "build", "pv_main")
    x = np.load(os.path.join(GOLDEN, "sine440_ch0_32768.npy"))[:16384].astype(np.float32)
    wav_in, dump = str(tmp_path / "in.wav"), str(tmp_path / "o.f32")
    write_pcm16(wav_in, x)
    args = ["--N", "1024", "--hopdiv", "4", "--mode", "std", "--rate", "0.73", "--pitch-glide", "1", "1.5"]
    r = subprocess.run([pv_main, wav_in, "t", str(tmp_path / "o.wav"), *args, "--phase-lock", "--dump-f32", dump],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dump, np.float32)
    frames = pvref.num_frames(len(x), 256)
    pos = rate_map(frames, 0.73)
    pos_s, steps = pitch_map_plan(1024, 256, pos, vr.glide(len(pos), 1.0, 1.5))
    ref = vr.pitchmap_process(x, 1024, 4, pos_s, steps, True, None, 0, len(pos))
    assert len(got) == len(ref)
    err = rms(got, ref)
    print(f"pv_main --rate 0.73 --pitch-glide 1 1.5 --phase-lock ({len(pos)} frames): rms {err:.3e}")
    assert err <= RMS_TOL
    r = subprocess.run([pv_main, wav_in, "p", str(tmp_path / "o2.wav"), *args], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "--pitch-glide" in r.stderr
