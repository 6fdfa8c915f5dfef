"""Identity phase locking on the GPU (pv_set_phase_lock, k_synthesis in the locked mode) against the
fp64 reference tests/phase_lock_ref.py: every overlap-add variant and q path of the split
synthesis, spectrum / no spectrum / packed rows / analysis + resynthesis, stream segments,
the toggle and the refusals.  Runs of 8 frames (PV_RUN_FRAMES) and 76 frames per channel: 10
runs, 3 workgroups (two workgroup seams), the last run partial."""
import ctypes
import functools

import numpy as np
import pytest

import pvref
from gpu_helpers import LOCK_INPUTS, RMS_TOL, channel_errors, make_vocoder, run_segments, stretch_inputs, to_dev
from phase_lock_ref import cached, chirp, mean_envelope
from pvamd import PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, PhaseVocoder, _lib
from pvamd._lib import PVError
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 3
FRAMES = LOCK_INPUTS["frames"]

CASES = [
    (256, 4, 1.5),    # small N, LDS-ring overlap-add
    (512, 4, 0.5),    # ring overlap-add
    (1024, 4, 0.5),   # config-3 geometry, out hop 128 (register overlap-add, row prefetch)
    (1024, 4, 1.5),   # out hop 384
    (2048, 4, 1.37),  # odd out hop 701, q = 512
    (512, 3, 0.75),   # hop 170, non-power-of-two q
    (1024, 2, 0.25),  # hop N/2, out hop 128
    (2048, 8, 2.0),   # q = 1 (no unwrap state read), out hop 512
    (256, 4, 2.0),    # q = 1, single-launch handle
]


inputs = functools.partial(stretch_inputs, **LOCK_INPUTS, channels=C)


def make(monkeypatch, N, hop_div, scale, **kw):
    return make_vocoder(monkeypatch, N, hop_div, TIME_SHIFT, scale, max_frames=FRAMES + 4, channels=C, **kw)


def check_against_reference(out, xs, N, hop_div, scale):
    errs = channel_errors(out, lambda c: cached(xs[c], N, hop_div, scale, True), xs.shape[0])
    for c, err in enumerate(errs):
        print(f"N={N} hop_div={hop_div} scale={scale} channel {c}: rms {err:.3e}")
        assert err <= RMS_TOL, f"channel {c}: rms {err}"


def check_phases(pv, spec, xs, N, hop_div):
    s = pv.unpack_spec(spec).cpu().numpy()
    for c in range(xs.shape[0]):
        _, ph = pvref.std_analysis(xs[c], N, N // hop_div, FRAMES)
        assert np.array_equal(s[c, :FRAMES, :, 1].view(np.uint32), ph.view(np.uint32))


@pytest.mark.parametrize("N,hop_div,scale", CASES)
def test_locked_parity(cuda, monkeypatch, N, hop_div, scale):
    xs = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, scale)
    # (the single launch exists up to N = 1024: N = 2048 at q = 1 is a split-path handle
    # whose synthesis reads no unwrap state)
    assert bool(pv.single_launch) == (scale == 2.0 and N <= 1024)
    pv.set_phase_lock(True)
    assert pv.phase_lock and not pv.single_launch
    out, spec = pv.process(to_dev(xs))
    check_against_reference(out, xs, N, hop_div, scale)
    check_phases(pv, spec, xs, N, hop_div)


@pytest.mark.parametrize("N,hop_div,scale", [(1024, 4, 0.5), (1024, 4, 1.5), (2048, 4, 1.37)])
def test_locked_parity_without_spectrum(cuda, monkeypatch, N, hop_div, scale):
    xs = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=True)
    out, none = pv.process(to_dev(xs), spectrum=False)
    assert none is None
    check_against_reference(out, xs, N, hop_div, scale)


def test_locked_parity_packed_rows(cuda, monkeypatch):
    N, hop_div, scale = 1024, 4, 0.5
    xs = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=True, spec_layout=_lib.PV_SPEC_PACKED)
    out, spec = pv.process(to_dev(xs))
    check_against_reference(out, xs, N, hop_div, scale)
    check_phases(pv, spec, xs, N, hop_div)


def test_locked_analysis_then_resynthesis(cuda, monkeypatch):
    N, hop_div, scale = 512, 4, 0.5
    xs = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=True)
    spec = pv.analysis(to_dev(xs))
    out = pv.resynthesis(spec)
    check_against_reference(out, xs, N, hop_div, scale)
    check_phases(pv, spec, xs, N, hop_div)
    pv.profile(True)
    pv.resynthesis(spec)
    assert "synthesis_locked" in pv.profile_read()


def test_locking_changes_the_output(cuda, monkeypatch):
    """(fails without the feature) the locked output is not the unlocked one: the reference's
    locked-minus-unlocked RMS is 0.045 - 0.097 on these inputs."""
    N, hop_div, scale = 1024, 4, 0.5
    xs = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, scale)
    unlocked, _ = pv.process(to_dev(xs))
    pv.set_phase_lock(True)
    locked, _ = pv.process(to_dev(xs))
    for c in range(C):
        d = rms(locked[c].cpu().numpy(), unlocked[c].cpu().numpy())
        print(f"channel {c}: locked - unlocked rms {d:.4f}")
        assert d >= 1e-2


def test_locking_keeps_a_chirps_amplitude_on_the_gpu(cuda):
    N = 256
    xd = to_dev(chirp())
    pv = PhaseVocoder(N, TIME_SHIFT, 1.5, 4, mode=STANDARD, max_frames=200)
    unlocked = mean_envelope(pv.process(xd)[0].cpu().numpy()[0], N)
    pv.set_phase_lock(True)
    locked = mean_envelope(pv.process(xd)[0].cpu().numpy()[0], N)
    print(f"mean envelope: locked {locked:.4f}, unlocked {unlocked:.4f}")
    assert locked >= 0.45
    assert unlocked <= 0.37


@pytest.mark.parametrize("N,hop_div", [(256, 2), (1024, 4)])
def test_locking_is_the_identity_at_scale_one(cuda, monkeypatch, N, hop_div):
    xs = inputs(N, hop_div)
    pv = make(monkeypatch, N, hop_div, 1.0)
    unlocked, _ = pv.process(to_dev(xs))
    pv.set_phase_lock(True)
    locked, _ = pv.process(to_dev(xs))
    for c in range(C):
        assert rms(locked[c].cpu().numpy(), unlocked[c].cpu().numpy()) <= RMS_TOL


def test_locked_edge_cases(cuda, monkeypatch):
    import torch
    N, hop_div, scale = 1024, 4, 0.5
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=True)
    n = FRAMES * (N // hop_div) + 13
    # all-zero input (no peak in any frame): all-zero, finite output
    out, _ = pv.process(torch.zeros((C, n), device="cuda"))
    assert torch.isfinite(out).all() and not out.any()
    # no frames / no channels
    xd = to_dev(inputs(N, hop_div))
    out0, _ = pv.process(xd, frames=0)
    assert out0.shape == (C, 0)
    outc, _ = pv.process(xd[:0])
    assert outc.shape[0] == 0
    # one frame
    x1 = synth(N // hop_div + 100, 5)
    assert pv.num_frames(len(x1)) == 1
    o1, _ = pv.process(to_dev(x1))
    assert rms(o1.cpu().numpy()[0], cached(x1, N, hop_div, scale, True)) <= RMS_TOL
    # a second run is the same bits
    a, _ = pv.process(xd)
    b, _ = pv.process(xd)
    assert torch.equal(a, b)


@pytest.mark.parametrize("N,hop_div,scale,single", [(1024, 4, 0.5, 0), (256, 4, 2.0, 1)])
def test_toggle_restores_the_unlocked_path(cuda, monkeypatch, N, hop_div, scale, single):
    import torch
    xd = to_dev(inputs(N, hop_div))
    never = make(monkeypatch, N, hop_div, scale)
    want, _ = never.process(xd)
    pv = make(monkeypatch, N, hop_div, scale)
    assert pv.single_launch == single
    pv.set_phase_lock(True)
    assert pv.single_launch == 0
    locked, _ = pv.process(xd)
    assert not torch.equal(locked, want)
    pv.set_phase_lock(False)
    assert not pv.phase_lock and pv.single_launch == single
    info = _lib.new_info()
    assert pv._L.pv_get_info(pv._h, ctypes.byref(info)) == _lib.PV_OK and info.single_launch == single
    got, _ = pv.process(xd)
    assert torch.equal(got, want)


def test_locked_segments_equal_the_whole_stream(cuda):
    N, hop_div, scale = 1024, 4, 0.5
    x = synth(80000, 606)
    pv = PhaseVocoder(N, TIME_SHIFT, scale, hop_div, mode=STANDARD, max_frames=1000, phase_lock=True)
    whole, _ = pv.process(to_dev(x))
    got = run_segments(pv, x, 3)
    g, w = got.cpu().numpy()[0], whole.cpu().numpy()[0]
    assert g.shape == w.shape
    assert np.max(np.abs(g - w)) <= 1e-6


def test_phase_lock_refusals(cuda):
    for kw in (dict(effect=TIME_SHIFT, mode=REF_COMPAT), dict(effect=PITCH_SHIFT, mode=STANDARD)):
        pv = PhaseVocoder(1024, kw["effect"], 1.0 if kw["mode"] == REF_COMPAT else 1.5, 4, mode=kw["mode"],
                          max_frames=16)
        with pytest.raises(PVError) as e:
            pv.set_phase_lock(True)
        assert e.value.status == _lib.PV_ERR_UNSUPPORTED
        assert not pv.phase_lock
    pv = PhaseVocoder(1024, TIME_SHIFT, 0.5, 4, mode=STANDARD, max_frames=16)
    assert pv._L.pv_set_phase_lock(pv._h, 2) == _lib.PV_ERR_ARG
    assert pv._L.pv_set_phase_lock(pv._h, -1) == _lib.PV_ERR_ARG
    assert not pv.phase_lock
