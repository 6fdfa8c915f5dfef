"""The band-limited resampler on the GPU (pv_resample, k_resample) against the fp64 reference
tests/resample_ref.py, and the pitch shift built on it (pv_pitch_process: the STANDARD time
stretch, locked or not, then the resampling by out_hop / hop) against the reference resampling
of tests/phase_lock_ref.py's stretch.  n_in = 20011 is several workgroup tiles and a partial one
at every ratio; the pitch cases run 76 frames in runs of 8 (PV_RUN_FRAMES), as
test_gpu_phase_lock does, and share its cached references."""
import functools

import numpy as np
import pytest

import pvref
import resample_ref as rr
from gpu_helpers import (LOCK_INPUTS, RMS_TOL, make_vocoder, run_padded, stretch_inputs, to_dev, to_dev_copy,
                         write_pcm16)
from phase_lock_ref import cached, chirp, mean_envelope
from pvamd import PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, PhaseVocoder, Resampler, _lib
from pvamd._lib import PVError
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 3
N_IN = 20011
PAD = 37
FRAMES = LOCK_INPUTS["frames"]

RESAMPLE_CASES = [(3, 2, 0), (3, 4, 0), (2, 1, 0), (1, 4, 0), (4, 1, 0), (701, 512, 0), (127, 170, 0), (3, 2, 1),
                  (127, 170, 1)]

_xs = {}


def signal(n=N_IN):
    if n not in _xs:
        _xs[n] = np.stack([synth(n, 3300 + 11 * c) for c in range(C)])
        _xs[n].setflags(write=False)
    return _xs[n]


def check_parity(p, q, quality, pad):
    xs = signal()
    rs = Resampler(p, q, quality)
    assert rs.length(N_IN) == rr.out_length(p, q, N_IN)
    g = run_padded(rs, xs, pad)
    assert np.isfinite(g).all()
    ref = rr.resample(xs, p, q, quality)
    assert g.shape == ref.shape
    for c in range(C):
        err = rms(g[c], ref[c])
        print(f"{p}:{q} quality {quality} channel {c}: rms {err:.3e}, max {np.max(np.abs(g[c] - ref[c])):.3e}")
        assert err <= RMS_TOL


@pytest.mark.parametrize("p,q,quality", RESAMPLE_CASES)
def test_resample_parity(cuda, p, q, quality):
    check_parity(p, q, quality, PAD)


@pytest.mark.parametrize("p,q,quality", [(3, 2, 0), (127, 170, 1)])
def test_resample_parity_odd_row_stride(cuda, p, q, quality):
    """rows n_in + 38 floats apart: the channels' rows start at different offsets in a 16-byte
    segment (n_in + 37 is a multiple of 4)"""
    check_parity(p, q, quality, PAD + 1)


@pytest.mark.parametrize("p,q,quality", [(3, 2, 0), (1, 4, 0), (4, 1, 0), (127, 170, 1)])
def test_resample_short_inputs(cuda, p, q, quality):
    """inputs shorter than the filter: n_in = 1 and W - 1; n_in = 0 and no channels do nothing"""
    import torch
    rs = Resampler(p, q, quality)
    W = rr.half_width(p, q, quality)
    for n in (1, W - 1):
        xs = signal()[:, 100:100 + n]
        g = run_padded(rs, xs, PAD)
        ref = rr.resample(xs, p, q, quality)
        assert g.shape == ref.shape == (C, rr.out_length(p, q, n))
        assert np.max(np.abs(g - ref)) <= 1e-6
    empty = rs(torch.zeros((C, 0), device="cuda"))
    assert empty.shape == (C, 0)
    none = rs(torch.zeros((0, 100), device="cuda"))
    assert none.shape == (0, rs.length(100))
    assert rs.length(0) == 0


def test_resample_twice_is_the_same_bits(cuda):
    import torch
    xd = to_dev_copy(signal())
    rs = Resampler(701, 512, 0)
    assert torch.equal(rs(xd), rs(xd))


def test_resample_ratio_one_is_a_copy(cuda):
    import torch
    xs = signal()
    for p, q in ((1, 1), (512, 512)):
        g = run_padded(Resampler(p, q, 1), xs, PAD)
        assert np.array_equal(g, xs)
    x1 = to_dev_copy(xs[0])
    assert torch.equal(Resampler(5, 5)(x1), x1)


def test_resampler_refusals(cuda):
    import torch
    for p, q, quality, want in ((4, 1, 0, None), (1, 4, 1, None), (9, 2, 0, _lib.PV_ERR_UNSUPPORTED),
                                (2, 9, 0, _lib.PV_ERR_UNSUPPORTED), (4097, 4096, 0, _lib.PV_ERR_UNSUPPORTED),
                                (8194, 8192, 0, _lib.PV_ERR_UNSUPPORTED), (8192, 8190, 0, None),
                                (3, 2, 2, _lib.PV_ERR_ARG), (3, 2, -1, _lib.PV_ERR_ARG), (0, 1, 0, _lib.PV_ERR_ARG)):
        if want is None:
            Resampler(p, q, quality).close()
            continue
        with pytest.raises(PVError) as e:
            Resampler(p, q, quality)
        assert e.value.status == want, (p, q, quality)
    # x and y must not overlap
    rs = Resampler(3, 2, 0)
    buf = torch.zeros(4000, device="cuda")
    with pytest.raises(PVError) as e:
        rs(buf[:3000], out=buf[1000:1000 + rs.length(3000)])
    assert e.value.status == _lib.PV_ERR_ARG


def test_resample_in_a_graph(cuda):
    """one pv_resample call captured on a side stream and replayed"""
    import torch
    xd = to_dev_copy(signal())
    rs = Resampler(3, 2, 0)
    eager = rs(xd)
    out = torch.empty_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rs(xd, out=out)
    torch.cuda.synchronize()
    out.zero_()
    torch.cuda.synchronize()
    assert not out.any()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------ pv_pitch_process
inputs = functools.partial(stretch_inputs, **LOCK_INPUTS, channels=C)  # (the locked references are shared)


def make(monkeypatch, N, hop_div, scale, **kw):
    return make_vocoder(monkeypatch, N, hop_div, TIME_SHIFT, scale, max_frames=FRAMES + 4, channels=C, **kw)


PITCH_CASES = [
    # N, hop_div, scale, lock, quality, variant
    (256, 4, 1.5, False, 0, "spec"),
    (256, 4, 1.5, True, 0, "spec"),
    (1024, 4, 0.5, False, 0, "spec"),
    (1024, 4, 0.5, True, 0, "nospec"),     # pv_pitch_process(spec = NULL)
    (1024, 4, 1.5, False, 0, "packed"),    # PV_SPEC_PACKED rows
    (1024, 4, 1.5, True, 1, "spec"),       # the best preset
    (2048, 4, 1.37, False, 0, "spec"),     # ratio 701:512
    (2048, 4, 1.37, True, 0, "spec"),
    (512, 3, 0.75, False, 0, "spec"),      # ratio 127:170
    (512, 3, 0.75, True, 0, "spec"),
]


@pytest.mark.parametrize("N,hop_div,scale,lock,quality,variant", PITCH_CASES)
def test_pitch_process_parity(cuda, monkeypatch, N, hop_div, scale, lock, quality, variant):
    xs = inputs(N, hop_div)
    kw = dict(spec_layout=_lib.PV_SPEC_PACKED) if variant == "packed" else {}
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=lock, **kw)
    pv.reserve_pitch(quality)
    hs, hop = pv.outHopSize, pv.hopSize
    assert pv.pitch_output_length(FRAMES) == rr.out_length(hs, hop, pv.output_length(FRAMES))
    out, spec = pv.pitch_process(to_dev(xs), spectrum=(variant != "nospec"))
    g = out.cpu().numpy()
    assert np.isfinite(g).all()
    for c in range(C):
        ref = rr.resample(cached(xs[c], N, hop_div, scale, lock), hs, hop, quality)
        assert g[c].shape == ref.shape
        err = rms(g[c], ref)
        print(f"N={N} hop_div={hop_div} scale={scale} ({hs}:{hop}) lock={lock} channel {c}: rms {err:.3e}, "
              f"max {np.max(np.abs(g[c] - ref)):.3e}")
        assert err <= RMS_TOL
    if variant == "nospec":
        assert spec is None
        return
    s = pv.unpack_spec(spec).cpu().numpy()
    for c in range(C):
        _, ph = pvref.std_analysis(xs[c], N, hop, FRAMES)
        assert np.array_equal(s[c, :FRAMES, :, 1].view(np.uint32), ph.view(np.uint32))


def test_pitch_process_keeps_a_chirps_amplitude(cuda):
    """the reason for the feature: shifted by 1.5 at N = 256, the locked stretch + resampling
    keeps the chirp's amplitude (0.484 in fp64), the unlocked one (0.338) and the bin mapping
    (0.292) lose it"""
    N = 256
    xd = to_dev(chirp())
    pv = PhaseVocoder(N, TIME_SHIFT, 1.5, 4, mode=STANDARD, max_frames=200)
    pv.reserve_pitch(0)
    unlocked = pv.pitch_process(xd)[0].cpu().numpy()[0]
    pv.set_phase_lock(True)
    locked = pv.pitch_process(xd)[0].cpu().numpy()[0]
    mapped = PhaseVocoder(N, PITCH_SHIFT, 1.5, 4, mode=STANDARD, max_frames=200).process(xd)[0].cpu().numpy()[0]
    e = [mean_envelope(y, N) for y in (locked, unlocked, mapped)]
    print(f"mean envelope: locked {e[0]:.4f}, unlocked {e[1]:.4f}, bin mapping {e[2]:.4f}")
    assert len(locked) == 6187
    assert e[0] >= 0.45
    assert e[1] <= 0.37
    assert e[2] <= 0.32


@pytest.mark.parametrize("lock", [False, True])
def test_pitch_process_at_scale_one_is_process(cuda, monkeypatch, lock):
    import torch
    N, hop_div = 1024, 4
    xd = to_dev(inputs(N, hop_div))
    pv = make(monkeypatch, N, hop_div, 1.0, phase_lock=lock)
    pv.reserve_pitch(0)
    assert pv.pitch_output_length(FRAMES) == pv.output_length(FRAMES)
    want, wspec = pv.process(xd)
    got, gspec = pv.pitch_process(xd)
    assert torch.equal(got, want) and torch.equal(gspec, wspec)


def test_pitch_refusals(cuda):
    for effect, mode, scale in ((TIME_SHIFT, REF_COMPAT, 1.0), (PITCH_SHIFT, STANDARD, 1.5)):
        pv = PhaseVocoder(1024, effect, scale, 4, mode=mode, max_frames=16)
        with pytest.raises(PVError) as e:
            pv.reserve_pitch(0)
        assert e.value.status == _lib.PV_ERR_UNSUPPORTED
    xd = to_dev(synth(4096, 1))
    # before reserve_pitch
    pv = PhaseVocoder(1024, TIME_SHIFT, 1.5, 4, mode=STANDARD, max_frames=16)
    with pytest.raises(PVError) as e:
        pv.pitch_process(xd)
    assert e.value.status == _lib.PV_ERR_ARG
    # a bad quality leaves it off
    for quality in (2, -1):
        with pytest.raises(PVError) as e:
            pv.reserve_pitch(quality)
        assert e.value.status == _lib.PV_ERR_ARG
    with pytest.raises(PVError) as e:
        pv.pitch_process(xd)
    assert e.value.status == _lib.PV_ERR_ARG
    # out hop 51 of hop 256: below 1/4
    pv = PhaseVocoder(1024, TIME_SHIFT, 0.2, 4, mode=STANDARD, max_frames=16)
    assert (pv.outHopSize, pv.hopSize) == (51, 256)
    with pytest.raises(PVError) as e:
        pv.reserve_pitch(0)
    assert e.value.status == _lib.PV_ERR_UNSUPPORTED


def test_pitch_process_is_profiled_as_resample(cuda, monkeypatch):
    N, hop_div, scale = 1024, 4, 1.5
    pv = make(monkeypatch, N, hop_div, scale)
    pv.reserve_pitch(0)
    xd = to_dev(inputs(N, hop_div))
    pv.profile(True)
    pv.pitch_process(xd)
    prof = pv.profile_read()
    assert "resample" in prof and prof["resample"][1] == 1 and "synthesis" in prof


def test_pv_main_pitch_resample(cuda, tmp_path):
    """the C++ driver: --pitch-resample composes with --phase-lock and refuses a pitch-shift handle"""
    import os
    import subprocess

    from conftest import GOLDEN, ROOT
    from phase_lock_ref import std_process_lock
    pv_main = os.path.join(ROOT, "phase-vocoder_amd", "build", "pv_main")
    x = np.load(os.path.join(GOLDEN, "sine440_ch0_32768.npy"))
    wav_in, dump = str(tmp_path / "in.wav"), str(tmp_path / "o.f32")
    write_pcm16(wav_in, x)
    args = ["--N", "1024", "--hopdiv", "4", "--scale", "1.5", "--mode", "std", "--pitch-resample", "fast"]
    r = subprocess.run([pv_main, wav_in, "t", str(tmp_path / "o.wav"), *args, "--phase-lock", "--dump-f32", dump],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dump, np.float32)
    ref = rr.resample(std_process_lock(x.astype(np.float32), 1024, 4, 1.5, lock=True), 384, 256, 0)
    assert len(got) == min(len(ref), len(x))
    err = rms(got, ref[:len(got)])
    print(f"pv_main --pitch-resample fast --phase-lock: rms {err:.3e}")
    assert err <= RMS_TOL
    r = subprocess.run([pv_main, wav_in, "p", str(tmp_path / "o2.wav"), *args], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "--pitch-resample" in r.stderr
