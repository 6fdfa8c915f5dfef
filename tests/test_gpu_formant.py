"""Formant-preserving pitch shift on the GPU (pv_set_formant, k_envelope, k_synthesis in the formant mode)
against the fp64 reference tests/formant_ref.py: the envelope kernel on its own, output parity
over every size, overlap-add variant and ratio class of the split synthesis, spectrum / no
spectrum / packed rows, the harmoniser, stream segments, a non-finite burst, graph capture,
the toggle and the refusals.  Three channels in a buffer wider than the signals; runs of 8 or
16 frames, the last one partial."""
import ctypes

import numpy as np
import pytest

from formant_ref import INPUT_PEAK, cached, formant_peak, log_envelope, voice
from gpu_helpers import RMS_TOL, channel_errors, make_vocoder, run_segments, to_dev, wide
from pvamd import PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, Harmonizer, PhaseVocoder, _lib
from pvamd._lib import PVError
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 3
ENV_TOL = 2e-5  # ten times the 2.0e-6 of an fp32 CPU restatement (natural-log units)


def inputs(n, seed=0):
    """the voice (from inside its leading zeros), plain tones, and a mix of both"""
    v = voice()
    assert 2000 + n <= v.shape[0]
    a = v[2000:2000 + n]
    b = synth(n, 4100 + seed)
    c = (0.5 * v[-n:] + synth(n, 4200 + seed)).astype(np.float32)
    return np.stack([a, b, c])


def length_for(N, hop_div, frames):
    return frames * (N // hop_div) + 13  # not a multiple of the hop


def make(monkeypatch, N, hop_div, scale, F=8, frames=100, **kw):
    return make_vocoder(monkeypatch, N, hop_div, PITCH_SHIFT, scale, F, max_frames=frames + 4, channels=C, **kw)


def check_against_reference(out, xs, N, hop_div, scale, order, what=""):
    errs = channel_errors(out, lambda c: cached(xs[c], N, hop_div, scale, order), xs.shape[0])
    for c, err in enumerate(errs):
        assert err <= RMS_TOL, f"channel {c}: rms {err}"
    print(f"{what}N={N} hop_div={hop_div} scale={scale} order={order}: worst rms {max(errs):.3e}")


# ---------------------------------------------------------------- the envelope kernel
@pytest.mark.parametrize("layout", [_lib.PV_SPEC_NATURAL, _lib.PV_SPEC_PACKED])
@pytest.mark.parametrize("N", [256, 512, 1024, 2048])
def test_envelope_kernel(cuda, monkeypatch, N, layout):
    """le of every frame against numpy on the same fp32 magnitudes; an all-zero channel sits on
    the floor: le = ln 2^-30 everywhere.  (Measured on an MI355X: at most 2.5e-6 over every
    size, layout and order, 9.0e-7 on the all-zero channel)"""
    import torch
    monkeypatch.setenv("PV_RUN_FRAMES", "8")
    hop_div = 4
    n = 8000
    xs = np.stack([voice()[1500:1500 + n], np.zeros(n, np.float32), synth(n, 31)])
    effect, scale = (TIME_SHIFT, 0.5) if N == 512 else (PITCH_SHIFT, 1.5)
    pv = PhaseVocoder(N, effect, scale, hop_div, mode=STANDARD, max_channels=C, max_frames=300, spec_layout=layout)
    spec = pv.analysis(wide(xs))
    frames = spec.shape[1]
    assert frames % 8 != 0
    mag = pv.unpack_spec(spec)[..., 0].cpu().numpy()
    for order in (1, N // 16, N // 4):
        le = pv.spectral_envelope(spec, order)
        assert le.shape == (C, frames, N // 2 + 1)
        g = le.cpu().numpy()
        want = log_envelope(mag, N, order)
        err = float(np.max(np.abs(g - want)))
        zero = float(np.max(np.abs(g[1] - np.log(2.0 ** -30))))
        print(f"N={N} layout={layout} order={order}: max |le - ref| {err:.3e}, zero channel {zero:.3e}")
        assert err <= ENV_TOL
        assert zero <= ENV_TOL
    # the padding of the caller's rows is not written
    B = N // 2 + 1
    env = torch.full((C, frames, B + 7), 3.0, device="cuda")
    st = pv._L.pv_spectral_envelope(pv._h, spec.data_ptr(), spec.stride(0) // 2, C, frames, 4, env.data_ptr(),
                                    env.stride(0), pv._stream())
    assert st == _lib.PV_OK
    assert torch.all(env[..., B:] == 3.0) and torch.all(env[..., :B] != 3.0)


def test_envelope_refusals(cuda):
    pv = PhaseVocoder(1024, TIME_SHIFT, 0.5, 4, mode=STANDARD, max_frames=16)
    spec = pv.alloc_spec(1, 4)
    for order in (0, -1, 257):
        with pytest.raises(PVError) as e:
            pv.spectral_envelope(spec, order)
        assert e.value.status == _lib.PV_ERR_ARG
    assert pv.spectral_envelope(spec, 256).shape == (1, 4, 513)
    rc = PhaseVocoder(1024, TIME_SHIFT, 1.0, 4, mode=REF_COMPAT, max_frames=16)
    with pytest.raises(PVError) as e:
        rc.spectral_envelope(rc.alloc_spec(1, 4), 8)
    assert e.value.status == _lib.PV_ERR_UNSUPPORTED


# ---------------------------------------------------------------- parity
# (ratio 1.5: one source per bin; 0.75: up to two; 2.0 and 1.0: q = 1, single-launch handles at
# N = 512 and 1024; 1.0: the identity; 1.125: q = 8.  hop N/4: register overlap-add from N = 512 on
# (out hop 128, 256, 512), the LDS ring at N = 256.)
PARITY = [(N, 4, s) for N in (256, 512, 1024, 2048) for s in (1.5, 0.75, 2.0, 1.0, 1.125)]
PARITY += [(1024, 8, 1.5), (1024, 8, 0.75), (512, 3, 1.37)]  # hop N/8; hop 170 and a q above 4096: the generic kernels


@pytest.mark.parametrize("N,hop_div,scale", PARITY)
def test_formant_parity(cuda, monkeypatch, N, hop_div, scale):
    """(Measured on an MI355X: worst channel 2.4e-8 .. 1.1e-7 RMS over these cases.)"""
    frames = 27 if N >= 1024 else 45
    F = 16 if N in (512, 2048) else 8
    xs = inputs(length_for(N, hop_div, frames), N)
    order = N // 16
    pv = make(monkeypatch, N, hop_div, scale, F=F, frames=frames)
    assert pv.num_frames(xs.shape[1]) == frames and frames % F != 0
    # (q = 1 at ratios 1 and 2; the single launch exists for out hops of 128 .. 512 up to N = 1024)
    assert bool(pv.single_launch) == (scale in (1.0, 2.0) and hop_div == 4 and N in (512, 1024))
    pv.set_formant(order)
    assert pv.formant == order and not pv.single_launch
    out, spec = pv.process(wide(xs))
    check_against_reference(out, xs, N, hop_div, scale, order)
    pv.profile(True)
    pv.process(wide(xs))
    names = pv.profile_read()
    assert "envelope" in names and "synthesis_formant" in names and "synthesis" not in names


def test_formant_parity_packed_rows_and_resynthesis(cuda, monkeypatch):
    N, hop_div, scale, order, frames = 1024, 4, 1.5, 64, 27
    xs = inputs(length_for(N, hop_div, frames), 1)
    pv = make(monkeypatch, N, hop_div, scale, frames=frames, formant=order, spec_layout=_lib.PV_SPEC_PACKED)
    out, spec = pv.process(wide(xs))
    check_against_reference(out, xs, N, hop_div, scale, order, "packed: ")
    again = pv.resynthesis(spec)
    check_against_reference(again, xs, N, hop_div, scale, order, "packed, resynthesis: ")


@pytest.mark.parametrize("N,order", [(256, 1), (2048, 512)])
def test_formant_parity_extreme_orders(cuda, monkeypatch, N, order):
    frames = 27
    xs = inputs(length_for(N, 4, frames), 2)
    pv = make(monkeypatch, N, 4, 0.75, frames=frames, formant=order)
    out, _ = pv.process(wide(xs))
    check_against_reference(out, xs, N, 4, 0.75, order)


@pytest.mark.parametrize("N,hop_div", [(256, 4), (1024, 4)])
def test_ratio_one_is_the_plain_pitch_shift(cuda, monkeypatch, N, hop_div):
    frames = 27
    xs = inputs(length_for(N, hop_div, frames), 3)
    pv = make(monkeypatch, N, hop_div, 1.0, frames=frames)
    off, _ = pv.process(wide(xs))
    pv.set_formant(N // 16)
    on, _ = pv.process(wide(xs))
    d = float((on - off).abs().max())
    print(f"N={N}: max |on - off| at ratio 1: {d:.3e}")
    assert d <= 1e-6


@pytest.mark.parametrize("N,scale,single", [(2048, 1.5, 0), (512, 2.0, 1)])
def test_without_spectrum_and_toggle(cuda, monkeypatch, N, scale, single):
    """process(spectrum=False) with the feature on analyses every bin (the envelope at the
    target bins reads magnitudes above N/2 / scale): the same bits as with a spectrum buffer.
    pv_get_info says the split path while on, and order 0 restores the plain path's bits."""
    import torch
    frames = 27
    xs = inputs(length_for(N, 4, frames), 4)
    xd = wide(xs)
    never = make(monkeypatch, N, 4, scale, frames=frames)
    want_plain, _ = never.process(xd, spectrum=False)
    pv = make(monkeypatch, N, 4, scale, frames=frames)
    assert pv.single_launch == single
    pv.set_formant(N // 16)
    info = _lib.new_info()
    assert pv._L.pv_get_info(pv._h, ctypes.byref(info)) == _lib.PV_OK and info.single_launch == 0
    with_spec, _ = pv.process(xd)
    without, none = pv.process(xd, spectrum=False)
    assert none is None
    assert torch.equal(with_spec, without)
    check_against_reference(without, xs, N, 4, scale, N // 16, "no spectrum: ")
    assert not torch.equal(without, want_plain)
    pv.set_formant(0)
    assert pv.formant == 0 and pv.single_launch == single
    assert pv._L.pv_get_info(pv._h, ctypes.byref(info)) == _lib.PV_OK and info.single_launch == single
    plain, _ = pv.process(xd, spectrum=False)
    assert torch.equal(plain, want_plain)


def test_harmonizer_with_formants(cuda, monkeypatch):
    import torch
    monkeypatch.setenv("PV_RUN_FRAMES", "8")
    N, ratios, order, frames = 1024, [1.5, 0.75, 2.0], 32, 27
    xs = inputs(length_for(N, 4, frames), 5)
    xd = to_dev(xs)
    hz = Harmonizer(N, ratios, 4, max_channels=C, max_frames=frames + 4, formant=order)
    gains = [0.5, 0.25, 0.125]
    voices, mix, _ = hz.harmonize(xd, gains=gains)
    v = voices.cpu().numpy()
    for k, r in enumerate(ratios):
        pv = PhaseVocoder(N, PITCH_SHIFT, r, 4, mode=STANDARD, max_channels=C, max_frames=frames + 4, formant=order)
        single, _ = pv.process(xd)
        assert torch.equal(voices[k], single), f"voice {k} differs from pv_process"
        check_against_reference(voices[k], xs, N, 4, r, order, f"voice {k}: ")
    want = sum(g * v[k].astype(np.float64) for k, g in enumerate(gains))
    assert np.max(np.abs(mix.cpu().numpy() - want)) <= 1e-6
    # off again: the plain voices
    hz.set_formant(0)
    plain, _, _ = hz.harmonize(xd)
    ref = Harmonizer(N, ratios, 4, max_channels=C, max_frames=frames + 4).harmonize(xd)[0]
    assert torch.equal(plain, ref)
    with pytest.raises(PVError) as e:
        hz.set_formant(N // 4 + 1)
    assert e.value.status == _lib.PV_ERR_ARG


def test_formant_segments_equal_the_whole_stream(cuda):
    N, hop_div, scale, order = 1024, 4, 1.5, 64
    x = np.concatenate([voice(), voice()[3000:11000]])
    pv = PhaseVocoder(N, PITCH_SHIFT, scale, hop_div, mode=STANDARD, max_frames=200, formant=order)
    whole, _ = pv.process(to_dev(x))
    got = run_segments(pv, x, 3)
    g, w = got.cpu().numpy()[0], whole.cpu().numpy()[0]
    assert g.shape == w.shape
    assert np.max(np.abs(g - w)) <= 1e-6
    err = rms(g, cached(x, N, hop_div, scale, order))
    print(f"segments: rms {err:.3e}")
    assert err <= RMS_TOL


def test_formant_nonfinite_burst_stays_in_its_frames(cuda):
    """The feature keeps no state between frames: outside the frames that hold a non-finite
    sample the output is finite and the reference's."""
    N, hop_div, scale, order = 1024, 4, 1.5, 64
    hop = N // hop_div
    x = np.array(voice()[2000:14000])
    x[6000:6010] = np.nan
    x[6100] = np.inf
    x[6200] = -np.inf
    pv = PhaseVocoder(N, PITCH_SHIFT, scale, hop_div, mode=STANDARD, max_frames=100, formant=order)
    out, _ = pv.process(to_dev(x))
    g = out.cpu().numpy()[0]
    with np.errstate(all="ignore"):
        ref = cached(x, N, hop_div, scale, order)
    assert g.shape == ref.shape
    last_bad = (6200 // hop) + 1
    start = (last_bad + 1) * hop + N
    assert np.all(np.isfinite(g[start:])) and np.all(np.isfinite(ref[start:]))
    assert rms(g[start:], ref[start:]) <= RMS_TOL
    first_bad = 6000 // hop - N // hop
    assert first_bad > 0 and np.all(np.isfinite(g[:first_bad * hop]))
    assert rms(g[:first_bad * hop], ref[:first_bad * hop]) <= RMS_TOL
    assert not np.all(np.isfinite(g))


def test_formant_process_captures_into_a_graph(cuda):
    import torch
    N, order = 1024, 64
    x = voice()[2000:12000]
    xd = to_dev(x)
    mk = lambda: PhaseVocoder(N, PITCH_SHIFT, 1.5, 4, mode=STANDARD, max_frames=60, formant=order)
    ref, _ = mk().process(xd, spectrum=False)
    pv = mk()
    pv.reserve_spectrum()
    frames = pv.num_frames(len(x))
    out = pv.alloc_out(1, frames)
    L = _lib.lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        st = L.pv_process(pv._h, xd.data_ptr(), xd.numel(), len(x), 1, frames, None, 0, out.data_ptr(),
                          out.stride(0), ctypes.c_void_p(s.cuda_stream))
        g.capture_end()
    assert st == _lib.PV_OK
    out.zero_()
    torch.cuda.synchronize()
    assert not out.any()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_formant_stays_where_the_input_has_it_on_the_gpu(cuda):
    N, order, scale = 512, 16, 1.5
    xd = to_dev(voice())
    pv = PhaseVocoder(N, PITCH_SHIFT, scale, 4, mode=STANDARD, max_frames=200)
    off = formant_peak(pv.process(xd)[0].cpu().numpy()[0])
    pv.set_formant(order)
    on = formant_peak(pv.process(xd)[0].cpu().numpy()[0])
    print(f"peak on {on:.4f}, off {off:.4f}")
    assert abs(on - INPUT_PEAK) <= 0.01
    assert abs(off - scale * INPUT_PEAK) <= 0.01


def test_formant_refusals(cuda):
    for effect, mode, scale in ((TIME_SHIFT, REF_COMPAT, 1.0), (TIME_SHIFT, STANDARD, 0.5)):
        pv = PhaseVocoder(1024, effect, scale, 4, mode=mode, max_frames=16)
        with pytest.raises(PVError) as e:
            pv.set_formant(8)
        assert e.value.status == _lib.PV_ERR_UNSUPPORTED
        assert pv.formant == 0
    pv = PhaseVocoder(1024, PITCH_SHIFT, 1.5, 4, mode=STANDARD, max_frames=16)
    for order in (-1, 257, 1 << 20):
        assert pv._L.pv_set_formant(pv._h, order) == _lib.PV_ERR_ARG
        assert pv.formant == 0
    pv.set_formant(256)
    assert pv.formant == 256
    pv.set_formant(1)
    assert pv.formant == 1
    pv.set_formant(0)
    assert pv.formant == 0
    assert pv._L.pv_abi_version() == 5 and pv._L.pv_contract_version() == 4
