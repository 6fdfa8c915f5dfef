"""Formant preservation of the stretch-and-resample pitch shift on the GPU (pv_pitch_set_formant,
k_envelope + k_synthesis in the warp mode) against the fp64 reference tests/pitch_formant_ref.py: output
parity over every size, overlap-add variant and q path, unlocked and locked; natural and packed
rows, resynthesis / process / process without a spectrum; pitch_process end to end; the
identity at scale 1, the toggle, stream segments, graph capture, a non-finite burst, the
formant property and the refusals.

Three channels cut from the voice signal at different offsets (one starts inside the leading
zeros: frames on the 2^-30 floor), about 6000 samples each and never fewer than 37 frames, in runs
of 8 frames (PV_RUN_FRAMES): at least 5 runs, two workgroups, one workgroup seam, the last run
partial."""
import ctypes

import numpy as np
import pytest

import resample_ref as rr
from formant_ref import INPUT_PEAK, formant_peak, voice
from gpu_helpers import RMS_TOL, channel_errors, make_vocoder, run_segments, to_dev
from pitch_formant_ref import cached
from pvamd import PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, PhaseVocoder, _lib
from pvamd._lib import PVError
from signals import rms

pytestmark = pytest.mark.gpu

C = 3
F = 8
OFFSETS = (0, 2500, 5000)  # channel 0 holds the 3000 floor-level lead samples


def frames_for(N, hop_div):
    return max(37, 6000 // (N // hop_div))


def inputs(N, hop_div):
    hop = N // hop_div
    frames = frames_for(N, hop_div)
    n = frames * hop + 13  # not a multiple of the hop
    v = voice(24000)
    assert OFFSETS[-1] + n <= v.shape[0]
    return np.stack([v[o:o + n] for o in OFFSETS]), frames


def make(monkeypatch, N, hop_div, scale, frames, **kw):
    return make_vocoder(monkeypatch, N, hop_div, TIME_SHIFT, scale, F, max_frames=frames + 4, channels=C, **kw)


def check_against_reference(out, xs, N, hop_div, scale, lock, order, what=""):
    worst = max(channel_errors(out, lambda c: cached(xs[c], N, hop_div, scale, lock, order), xs.shape[0]))
    print(f"{what}N={N} hop_div={hop_div} scale={scale} order={order} lock={lock}: worst channel rms {worst:.3e}")
    assert worst <= RMS_TOL
    return worst


# ---------------------------------------------------------------- parity
PARITY = [
    (256, 4, 1.5, 8),      # LDS-ring overlap-add
    (256, 4, 0.75, 64),    # order N/4
    (512, 4, 1.5, 16),
    (512, 3, 1.2, 16),     # hop 170, q = 5: the generic-q ring form
    (1024, 4, 0.5, 32),    # out hop 128: register overlap-add
    (1024, 4, 2.0, 1),     # q = 1, out hop 512, the clamp on half the bins
    (2048, 4, 0.5, 48),    # out hop 256
    (2048, 4, 1.5, 512),   # order N/4
    (2048, 8, 1.37, 48),
]


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,scale,order", PARITY)
def test_warp_parity(cuda, monkeypatch, N, hop_div, scale, order, lock):
    """1e-5 RMS per sample against the fp64 reference, the project's synthesis tolerance
    (k_envelope's 2.5e-6 log-unit error is a relative 2.5e-6 of every magnitude: about 1e-6 of a
    0.5-peak signal).  (Measured values: DESIGN.md §3.10.)"""
    xs, frames = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, scale, frames, phase_lock=lock)
    assert pv.num_frames(xs.shape[1]) == frames and frames % F != 0 and frames > 4 * F
    pv.set_pitch_formant(order)
    assert pv.pitch_formant == order and pv.phase_lock == lock and not pv.single_launch
    out, spec = pv.process(to_dev(xs))
    check_against_reference(out, xs, N, hop_div, scale, lock, order)
    pv.profile(True)
    pv.process(to_dev(xs))
    names = pv.profile_read()
    assert "envelope" in names and "synthesis_warp" in names
    assert "synthesis" not in names and "synthesis_locked" not in names and "synthesis_formant" not in names


# ---------------------------------------------------------------- interfaces
@pytest.mark.parametrize("layout", [_lib.PV_SPEC_NATURAL, _lib.PV_SPEC_PACKED])
def test_rows_and_entry_points(cuda, monkeypatch, layout):
    """natural and packed rows; pv_resynthesis from a caller's spectrum, pv_process with a spectrum
    and pv_process(spec = NULL, the handle's own rows) give the same bits"""
    import torch
    N, hop_div, scale, order = 1024, 4, 1.5, 32
    xs, frames = inputs(N, hop_div)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, hop_div, scale, frames, phase_lock=True, pitch_formant=order, spec_layout=layout)
    out, spec = pv.process(xd)
    check_against_reference(out, xs, N, hop_div, scale, True, order, f"layout {layout}: ")
    again = pv.resynthesis(pv.analysis(xd))
    assert torch.equal(again, out)
    without, none = pv.process(xd, spectrum=False)
    assert none is None and torch.equal(without, out)


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("N,hop_div,scale,order", [(512, 4, 1.5, 16), (1024, 4, 0.75, 32)])
def test_pitch_process_with_the_warp(cuda, monkeypatch, N, hop_div, scale, order, quality):
    xs, frames = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, scale, frames, phase_lock=True, pitch_formant=order)
    pv.reserve_pitch(quality)
    hs, hop = pv.outHopSize, pv.hopSize
    want_len = rr.out_length(hs, hop, pv.output_length(frames))
    assert pv.pitch_output_length(frames) == want_len
    out, _ = pv.pitch_process(to_dev(xs))
    g = out.cpu().numpy()
    assert g.shape == (C, want_len) and np.isfinite(g).all()
    worst = 0.0
    for c in range(C):
        ref = rr.resample(cached(xs[c], N, hop_div, scale, True, order), hs, hop, quality)
        assert g[c].shape == ref.shape
        worst = max(worst, rms(g[c], ref))
    print(f"pitch_process N={N} scale={scale} ({hs}:{hop}) order={order} quality={quality}: worst rms {worst:.3e}")
    assert worst <= RMS_TOL


# ---------------------------------------------------------------- scale 1, toggle
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N", [256, 1024])
def test_scale_one_is_the_plain_stretch(cuda, monkeypatch, N, lock):
    """out hop = hop: i_k = k and r_k = 0, the gain is exp2(0) = 1"""
    import torch
    xs, frames = inputs(N, 4)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, 4, 1.0, frames, phase_lock=lock)
    off, _ = pv.process(xd)
    pv.set_pitch_formant(N // 16)
    on, _ = pv.process(xd)
    d = float((on - off).abs().max())
    print(f"N={N} lock={lock}: max |on - off| at scale 1: {d:.3e}, bit-equal: {torch.equal(on, off)}")
    assert d <= 1e-6


@pytest.mark.parametrize("N,scale,single,differs", [(1024, 2.0, 1, True), (512, 1.0, 1, False), (1024, 0.5, 0, True)])
def test_toggle_restores_the_plain_path(cuda, monkeypatch, N, scale, single, differs):
    import torch
    xs, frames = inputs(N, 4)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, 4, scale, frames)
    info = _lib.new_info()
    read = lambda: (pv._L.pv_get_info(pv._h, ctypes.byref(info)), info.single_launch)
    assert pv.single_launch == single and read() == (_lib.PV_OK, single)
    first, _ = pv.process(xd)
    pv.set_pitch_formant(N // 32)
    assert pv.pitch_formant == N // 32 and pv.single_launch == 0 and read() == (_lib.PV_OK, 0)
    on, _ = pv.process(xd)
    if differs:
        assert not torch.equal(on, first)
        assert rms(on.cpu().numpy(), first.cpu().numpy()) >= 1e-3
    pv.set_pitch_formant(0)
    assert pv.pitch_formant == 0 and pv.single_launch == single and read() == (_lib.PV_OK, single)
    last, _ = pv.process(xd)
    assert torch.equal(last, first)


# ---------------------------------------------------------------- segments, graph
def test_warp_segments_equal_the_whole_stream(cuda):
    N, hop_div, scale, order = 1024, 4, 0.5, 32
    x = voice(24000)
    pv = PhaseVocoder(N, TIME_SHIFT, scale, hop_div, mode=STANDARD, max_frames=200, phase_lock=True,
                      pitch_formant=order)
    whole, _ = pv.process(to_dev(x))
    got = run_segments(pv, x, 3)
    g, w = got.cpu().numpy()[0], whole.cpu().numpy()[0]
    assert g.shape == w.shape
    d = float(np.max(np.abs(g - w)))
    print(f"segments: max |segments - whole| {d:.3e}")
    assert d <= 1e-6


def test_pitch_process_with_the_warp_captures_into_a_graph(cuda, monkeypatch):
    import torch
    N, hop_div, scale, order = 1024, 4, 1.5, 32
    xs, frames = inputs(N, hop_div)
    xd = to_dev(xs)
    pv = make(monkeypatch, N, hop_div, scale, frames, phase_lock=True)
    pv.reserve_pitch(0)
    pv.reserve_spectrum()
    pv.set_pitch_formant(order)
    eager, _ = pv.pitch_process(xd, spectrum=False)
    out = torch.empty_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pv.pitch_process(xd, spectrum=False, out=out)
    torch.cuda.synchronize()
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        assert not out.any()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------------------------------------------------------- non-finite input
def test_nonfinite_burst_stays_in_its_frames(cuda, monkeypatch):
    """The warp keeps no state between frames: only output samples overlapped by frames that
    read the burst may differ from the clean run's, every other sample is the same bits.
    Out hop = 2 hop (q = 1), where the stretch itself carries nothing across frames either: at
    q > 1 its unwrap count is state by design, and the decisions made inside the burst stay
    in it."""
    import torch
    N, hop_div, scale, order = 1024, 4, 2.0, 32
    hop = N // hop_div
    xs, frames = inputs(N, hop_div)
    bad = np.array(xs)
    b0, b1 = 4000, 4210
    bad[:, b0:b0 + 10] = np.nan
    bad[1, b0 + 100] = np.inf
    bad[2, b1 - 1] = -np.inf
    pv = make(monkeypatch, N, hop_div, scale, frames, phase_lock=True, pitch_formant=order)
    hs = pv.outHopSize
    clean, _ = pv.process(to_dev(xs))
    dirty, _ = pv.process(to_dev(bad))
    # frame t reads x[t hop, t hop + N) and writes out[t hs, t hs + N)
    t_first = max(0, (b0 - N) // hop + 1)
    t_last = (b1 - 1) // hop
    assert 0 < t_first <= t_last < frames - 1
    lo, hi = t_first * hs, t_last * hs + N
    assert torch.equal(dirty[:, :lo], clean[:, :lo])
    assert torch.equal(dirty[:, hi:], clean[:, hi:])
    assert torch.isfinite(dirty[:, :lo]).all() and torch.isfinite(dirty[:, hi:]).all()
    assert not torch.isfinite(dirty[:, lo:hi]).all()


# ---------------------------------------------------------------- the property
def test_formant_stays_where_the_input_has_it_on_the_gpu(cuda):
    """(the fp64 reference gives 0.0898 on, 0.1343 off)"""
    N, order, scale = 512, 16, 1.5
    xd = to_dev(voice())
    pv = PhaseVocoder(N, TIME_SHIFT, scale, 4, mode=STANDARD, max_frames=200, phase_lock=True)
    pv.reserve_pitch(0)
    off = formant_peak(pv.pitch_process(xd)[0].cpu().numpy()[0])
    pv.set_pitch_formant(order)
    on = formant_peak(pv.pitch_process(xd)[0].cpu().numpy()[0])
    print(f"peak on {on:.4f}, off {off:.4f}")
    assert abs(on - INPUT_PEAK) <= 0.01
    assert abs(off - scale * INPUT_PEAK) <= 0.01


# ---------------------------------------------------------------- refusals
def test_pitch_formant_refusals(cuda):
    for effect, mode, scale in ((TIME_SHIFT, REF_COMPAT, 1.0), (PITCH_SHIFT, STANDARD, 1.5)):
        pv = PhaseVocoder(1024, effect, scale, 4, mode=mode, max_frames=16)
        with pytest.raises(PVError) as e:
            pv.set_pitch_formant(8)
        assert e.value.status == _lib.PV_ERR_UNSUPPORTED
        assert pv.pitch_formant == 0
        with pytest.raises(PVError) as e:
            PhaseVocoder(1024, effect, scale, 4, mode=mode, max_frames=16, pitch_formant=8)
        assert e.value.status == _lib.PV_ERR_UNSUPPORTED
    pv = PhaseVocoder(1024, TIME_SHIFT, 1.5, 4, mode=STANDARD, max_frames=16)
    for order in (-1, 257, 1 << 20):
        assert pv._L.pv_pitch_set_formant(pv._h, order) == _lib.PV_ERR_ARG
        assert pv.pitch_formant == 0
    # pv_set_formant keeps its refusal on this handle, and leaves the new switch alone
    with pytest.raises(PVError) as e:
        pv.set_formant(8)
    assert e.value.status == _lib.PV_ERR_UNSUPPORTED
    assert pv.formant == 0 and pv.pitch_formant == 0
    pv.set_pitch_formant(256)
    assert pv.pitch_formant == 256 and pv.formant == 0
    pv.set_pitch_formant(1)
    assert pv.pitch_formant == 1
    pv.set_pitch_formant(0)
    assert pv.pitch_formant == 0
    L = _lib.lib()
    assert L.pv_pitch_set_formant(None, 8) == _lib.PV_ERR_ARG and L.pv_pitch_get_formant(None) == 0
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4
