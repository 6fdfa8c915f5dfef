"""Transient phase reset on the GPU (pv_set_transient; k_onset, k_pick, k_reset and k_synthesis
in the reset modes) against the fp64 reference tests/transient_ref.py: every overlap-add variant
and q path of the split synthesis with explicit flags, natural and packed rows, locked and
unlocked, the pitch shift built on the stretch, the detector, the toggle, graph capture and the
refusals.  3 channels x 60 frames in runs of 8 (8 runs, 2 workgroups, the last run partial) or
16 frames (PV_RUN_FRAMES).

The flags put every code path on one of the channels (runs of 8):
  channel 0   frame 8 (a run's first frame), 23 (a run's last frame), 33 and 37 (two in one run:
              the later one holds for the runs after it), 58 (the last, partial run)
  channel 1   frame 10 only: run 1, then six runs without a flag — the offset is looked up
              across the workgroup boundary (4 runs)
  channel 2   no flag
"""
import ctypes

import numpy as np
import pytest

import pvref
import transient_ref as T
from gpu_helpers import RMS_TOL, channel_errors, make_vocoder, status_of, stretch_inputs, to_dev
from pvamd import PITCH_SHIFT, REF_COMPAT, STANDARD, TIME_SHIFT, PhaseVocoder, _lib
from resample_ref import resample as resample_ref
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 3
FRAMES = 60
FLAGGED = {0: [8, 23, 33, 37, 58], 1: [10], 2: []}

CASES = [
    (256, 4, 1.5, 8),    # small N, LDS-ring overlap-add
    (1024, 4, 0.5, 8),   # out hop 128: register overlap-add, self-tracked row prefetch
    (1024, 4, 1.5, 16),  # out hop 384: LDS ring at L = 512, runs of 16
    (2048, 4, 1.5, 8),   # L = 1024, LDS ring (out hop 768)
    (1024, 4, 2.0, 8),   # L = 512, out hop 512: register overlap-add with 4 slots per frame, q = 1
    (2048, 4, 0.5, 8),   # L = 1024, register overlap-add (out hop 256), late row loads
    (512, 3, 0.75, 8),   # hop 170: non-power-of-two q (the integer phase path, k_reset's too)
    (256, 4, 2.0, 8),    # q = 1: a single-launch handle on the split path, no carry, no walk
]


def flags_array(frames=FRAMES):
    fl = np.zeros((C, frames), np.uint8)
    for c, ts in FLAGGED.items():
        fl[c, ts] = 1
    return fl


def inputs(N, hop_div):
    return stretch_inputs(N, hop_div, seed0=7300, seed_step=11, frames=FRAMES, channels=C)


def make(monkeypatch, N, hop_div, scale, F=8, **kw):
    return make_vocoder(monkeypatch, N, hop_div, TIME_SHIFT, scale, F, max_frames=FRAMES + 4, channels=C, **kw)


def check_against_reference(out, xs, N, hop_div, scale, lock, fl):
    errs = channel_errors(out, lambda c: T.cached(xs[c], N, hop_div, scale, lock, fl[c]), xs.shape[0])
    for c, err in enumerate(errs):
        print(f"N={N} hop_div={hop_div} scale={scale} lock={lock} channel {c}: rms {err:.3e}")
        assert err <= RMS_TOL, f"channel {c}: rms {err}"


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,scale,F", CASES)
def test_reset_parity_with_explicit_flags(cuda, monkeypatch, N, hop_div, scale, F, lock):
    xs = inputs(N, hop_div)
    fl = flags_array()
    pv = make(monkeypatch, N, hop_div, scale, F, phase_lock=lock)
    assert bool(pv.single_launch) == (scale == 2.0 and not lock)  # (locking alone takes the split path)
    pv.set_transients("flags")
    assert pv.transients == "flags" and not pv.single_launch
    pv.set_transient_flags(to_dev(fl))
    assert np.array_equal(pv.transient_flags(C, FRAMES).cpu().numpy(), fl)
    out, _ = pv.process(to_dev(xs))
    check_against_reference(out, xs, N, hop_div, scale, lock, fl)
    # the reset changed something on the flagged channels, nothing on the unflagged one
    g = out.cpu().numpy()
    plain = T.cached(xs[0], N, hop_div, scale, lock, np.zeros(FRAMES, np.uint8))
    if scale != 1.0:
        assert rms(g[0], plain) >= 1e-3
    # a second run is the same bits
    again, _ = pv.process(to_dev(xs))
    import torch
    assert torch.equal(out, again)


@pytest.mark.parametrize("lock", [False, True])
def test_reset_parity_packed_rows_and_without_spectrum(cuda, monkeypatch, lock):
    N, hop_div, scale = 1024, 4, 0.5
    xs = inputs(N, hop_div)
    fl = flags_array()
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=lock, spec_layout=_lib.PV_SPEC_PACKED, transients="flags")
    pv.set_transient_flags(to_dev(fl))
    out, spec = pv.process(to_dev(xs))
    check_against_reference(out, xs, N, hop_div, scale, lock, fl)
    out2, none = pv.process(to_dev(xs), spectrum=False)
    assert none is None
    import torch
    assert torch.equal(out, out2)


@pytest.mark.parametrize("lock", [False, True])
def test_pitch_process_uses_the_reset_stretch(cuda, monkeypatch, lock):
    """pv_pitch_process at 3:2: the reset stretch into the scratch rows, then the resampling."""
    N, hop_div, scale = 1024, 4, 1.5
    xs = inputs(N, hop_div)
    fl = flags_array()
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=lock, transients="flags")
    assert (pv.outHopSize, pv.hopSize) == (384, 256)
    pv.reserve_pitch(1)
    pv.set_transient_flags(to_dev(fl))
    out, _ = pv.pitch_process(to_dev(xs))
    g = out.cpu().numpy()
    for c in range(C):
        mid = T.cached(xs[c], N, hop_div, scale, lock, fl[c])
        ref = resample_ref(mid, 3, 2, 1)
        assert g[c].shape == ref.shape
        err = rms(g[c], ref)
        print(f"lock={lock} channel {c}: rms {err:.3e}")
        assert err <= RMS_TOL


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,scale", [(1024, 4, 0.5), (256, 4, 1.5), (512, 3, 0.75)])
def test_no_flags_is_the_feature_off_output_bit_for_bit(cuda, monkeypatch, N, hop_div, scale, lock):
    import torch
    xd = to_dev(inputs(N, hop_div))
    off = make(monkeypatch, N, hop_div, scale, phase_lock=lock)
    want, _ = off.process(xd)
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=lock, transients="flags")
    got, _ = pv.process(xd)  # (the handle's flags are zero until set)
    assert torch.equal(got, want)
    pv.set_transient_flags(to_dev(flags_array()))
    changed, _ = pv.process(xd)
    assert not torch.equal(changed, want)
    pv.set_transient_flags(torch.zeros((C, FRAMES), dtype=torch.uint8, device="cuda"))
    assert torch.equal(pv.process(xd)[0], want)
    # the toggle restores the plain path
    pv.set_transient_flags(to_dev(flags_array()))
    pv.set_transients("off")
    assert pv.transients == "off"
    assert torch.equal(pv.process(xd)[0], want)


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,scale", [(1024, 4, 0.5), (2048, 4, 1.5), (512, 3, 0.75)])
def test_run_lengths_8_and_16_agree(cuda, monkeypatch, N, hop_div, scale, lock):
    """The result depends on the run length only through the overlap-add order of the run seams
    (<= 1e-6, as for the plain stretch): the flags fall differently into runs of 8 and of 16."""
    xd = to_dev(inputs(N, hop_div))
    fl = to_dev(flags_array())
    outs = []
    for F in (8, 16):
        pv = make(monkeypatch, N, hop_div, scale, F, phase_lock=lock, transients="flags")
        pv.set_transient_flags(fl)
        outs.append(pv.process(xd)[0].cpu().numpy())
    d = np.abs(outs[0] - outs[1]).max()
    print(f"N={N} scale={scale} lock={lock}: max |F8 - F16| = {d:.3e}")
    assert d <= 1e-6


def detector_input(N, seed, noise=0.0):
    hop = N // 4
    xs = np.stack([T.bursts(FRAMES * hop + 13, seed + c, noise=noise) for c in range(C)])
    assert pvref.num_frames(xs.shape[1], hop) == FRAMES
    return xs


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_onset_strength_and_flags(cuda, monkeypatch, N, packed):
    """pv_onset_strength against the fp64 sums, relative to tot: the fp32 sum of B = N/2 + 1
    non-negative terms in any order is within (B - 1) 2^-24 of the exact sum relative to the sum
    of the terms' magnitudes (<= tot for both rise and tot): 6.1e-5 at N = 2048.  Measured on
    these inputs: see DESIGN.md §3.11; asserted a decade above the measured 2.4e-7 (2.4e-6).
    Flags: on the frames whose three fp64 comparisons are clear by a relative 1e-4 (at most 2 %
    are not) the kernel's flags are the reference's."""
    xs = detector_input(N, 40 + N)
    pv = make(monkeypatch, N, 4, 1.5, spec_layout=_lib.PV_SPEC_PACKED if packed else _lib.PV_SPEC_NATURAL)
    spec = pv.analysis(to_dev(xs))
    got = pv.onset_strength(spec).cpu().numpy().astype(np.float64)
    pv.set_transients("detect")
    pv.process(to_dev(xs), spectrum=False)
    gflags = pv.transient_flags(C, FRAMES).cpu().numpy().astype(bool)
    worst = 0.0
    unclear = 0
    for c in range(C):
        mag, _ = pvref.std_analysis(xs[c], N, N // 4, FRAMES)
        rise, tot = T.strengths(mag)
        e = max(np.max(np.abs(got[c, :, 0] - rise) / tot), np.max(np.abs(got[c, :, 1] - tot) / tot))
        worst = max(worst, e)
        ok = T.clear(rise, tot)
        unclear += int((~ok).sum())
        want = T.pick(rise, tot)
        assert want.sum() >= 2
        assert np.array_equal(gflags[c][ok], want[ok]), (c, np.flatnonzero(gflags[c]), np.flatnonzero(want))
    print(f"N={N} packed={packed}: strength error / tot {worst:.3e}; {unclear} of {C * FRAMES} frames unclear")
    assert worst <= 2.4e-6
    assert unclear <= 0.02 * C * FRAMES


@pytest.mark.parametrize("lock", [False, True])
def test_detect_end_to_end(cuda, monkeypatch, lock):
    """One _DETECT run on a signal whose every frame is clear: the flags are the reference's
    exactly, then the output is the reference's with those flags.
    Locked: the same bursts over a 1e-3 noise floor.  A peak decision compares fp32 magnitudes,
    and the row's magnitudes (hardware square root, <= 1 ulp) are not the oracle's bit for bit:
    on spectra full of near-equal neighbours — a lone click's flat spectrum, a clean tone's
    rounding floor — the locked reference's peaks are not the GPU's, with the feature off as well
    (2.5e-3 .. 4.7e-3 RMS on the clean bursts).  The noise floor keeps neighbours apart, as on the
    inputs of tests/test_gpu_phase_lock.py; that the locked reference holds on this input with
    the feature off is checked first."""
    N, hop_div, scale = 1024, 4, 1.5
    xs = detector_input(N, 200, noise=1e-3) if lock else detector_input(N, 91)
    if lock:
        plain = make(monkeypatch, N, hop_div, scale, phase_lock=True)
        check_against_reference(plain.process(to_dev(xs))[0], xs, N, hop_div, scale, True,
                                np.zeros((C, FRAMES), np.uint8))
    fl = np.zeros((C, FRAMES), np.uint8)
    for c in range(C):
        mag, _ = pvref.std_analysis(xs[c], N, N // hop_div, FRAMES)
        rise, tot = T.strengths(mag)
        assert T.clear(rise, tot).all(), "the end-to-end input must be clear in every frame"
        fl[c] = T.pick(rise, tot)
    pv = make(monkeypatch, N, hop_div, scale, phase_lock=lock, transients="detect")
    out, _ = pv.process(to_dev(xs))
    assert np.array_equal(pv.transient_flags(C, FRAMES).cpu().numpy(), fl)
    check_against_reference(out, xs, N, hop_div, scale, lock, fl)
    pv.profile(True)
    pv.process(to_dev(xs))
    names = pv.profile_read()
    for k in ("onset", "pick", "reset", "synthesis_reset"):
        assert k in names, names


def test_the_reset_keeps_a_clicks_peak_on_the_gpu(cuda):
    """The four figures of tests/test_transient_ref.py, reproduced to 1e-3, and the detector's
    (reported)."""
    N, hop_div, scale = 256, 4, 1.5
    hop = N // hop_div
    x, pos = T.clicks()
    xd = to_dev(x)
    pv = PhaseVocoder(N, TIME_SHIFT, scale, hop_div, mode=STANDARD, max_frames=200)
    frames = pv.num_frames(len(x))
    hs = pv.outHopSize
    fl = T.click_flags(pos, N, hop, frames)
    want = {(False, False): 0.2607, (False, True): 0.5716, (True, False): 0.5163, (True, True): 0.5375}
    for lock in (False, True):
        pv.set_phase_lock(lock)
        for on in (False, True):
            pv.set_transients("flags" if on else "off")
            if on:
                pv.set_transient_flags(to_dev(fl))
            y = pv.process(xd)[0].cpu().numpy()[0]
            got = T.compactness(y, pos, N, hop, hs)
            print(f"lock {lock} reset {on}: {got:.4f}")
            assert abs(got - want[lock, on]) <= 1e-3
        pv.set_transients("detect")
        y = pv.process(xd)[0].cpu().numpy()[0]
        det = np.flatnonzero(pv.transient_flags(1, frames).cpu().numpy()[0])
        print(f"lock {lock} detected frames {det}: {T.compactness(y, pos, N, hop, hs):.4f}")


def test_flags_process_captures_into_a_graph(cuda, monkeypatch):
    """Before pv_transient_reserve a first call under capture is refused (no allocation is
    captured); after it pv_process in the flags mode captures, and the replay gives the
    uncaptured call's bits."""
    import torch
    N, hop_div, scale = 1024, 4, 0.5
    xs = inputs(N, hop_div)
    xd = to_dev(xs)
    fl = to_dev(flags_array())
    ref_pv = make(monkeypatch, N, hop_div, scale, transients="flags")
    ref_pv.set_transient_flags(fl)
    ref, _ = ref_pv.process(xd)
    pv = make(monkeypatch, N, hop_div, scale, transients="flags")
    spec = pv.alloc_spec(C, FRAMES)
    out = pv.alloc_out(C, FRAMES)
    L = _lib.lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call():
        return L.pv_process(pv._h, xd.data_ptr(), xd.stride(0), xd.shape[1], C, FRAMES, spec.data_ptr(),
                            spec.stride(0) // 2, out.data_ptr(), out.stride(0), ctypes.c_void_p(s.cuda_stream))

    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        st = call()
        g.capture_end()
    assert st == _lib.PV_ERR_ARG and b"pv_transient_reserve" in L.pv_last_error()
    pv.reserve_transients()
    pv.reserve_transients()  # idempotent
    pv.set_transient_flags(fl)
    torch.cuda.synchronize()
    out.zero_()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g2.capture_begin()
        st = call()
        g2.capture_end()
    assert st == _lib.PV_OK
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    out.zero_()
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_transient_refusals(cuda):
    L = _lib.lib()
    # REF_COMPAT and PV_PITCH_SHIFT handles
    for kw in (dict(effect=TIME_SHIFT, mode=REF_COMPAT, scale=1.0), dict(effect=PITCH_SHIFT, mode=STANDARD, scale=1.5)):
        pv = PhaseVocoder(1024, kw["effect"], kw["scale"], 4, mode=kw["mode"], max_frames=16)
        assert status_of(lambda: pv.set_transients("flags")) == _lib.PV_ERR_ARG
        assert status_of(lambda: pv.reserve_transients()) == _lib.PV_ERR_ARG
        assert L.pv_last_error()
        assert pv.transients == "off"
    # pv_set_formant (a pitch-shift handle's) and transients exclude each other in either order
    pf = PhaseVocoder(1024, PITCH_SHIFT, 1.5, 4, mode=STANDARD, max_frames=16, formant=30)
    assert status_of(lambda: pf.set_transients("detect")) == _lib.PV_ERR_ARG
    pv = PhaseVocoder(1024, TIME_SHIFT, 1.5, 4, mode=STANDARD, max_frames=16)
    pv.set_transients("detect")
    assert status_of(lambda: pv.set_formant(30)) == _lib.PV_ERR_ARG and pv.formant == 0
    assert status_of(lambda: pv.set_pitch_formant(30)) == _lib.PV_ERR_ARG and pv.pitch_formant == 0
    pv.set_transients("off")
    pv.set_pitch_formant(30)
    assert status_of(lambda: pv.set_transients("flags")) == _lib.PV_ERR_ARG and pv.transients == "off"
    pv.set_pitch_formant(0)
    # bad mode / threshold
    assert L.pv_set_transient(pv._h, 3, 0.0) == _lib.PV_ERR_ARG
    assert L.pv_set_transient(pv._h, -1, 0.0) == _lib.PV_ERR_ARG
    for thr in (1.0, -0.1, 1.5, float("nan")):
        assert L.pv_set_transient(pv._h, 2, thr) == _lib.PV_ERR_ARG
    assert pv.transients == "off"
    # the stream segments and pv_resynthesis while the mode is not OFF
    x = to_dev(synth(16 * 256 + 13, 3))
    spec = pv.analysis(x)
    pv.set_transients("flags")
    assert status_of(lambda: pv.resynthesis(spec)) == _lib.PV_ERR_ARG
    assert status_of(lambda: pv.segment_summary(spec)) == _lib.PV_ERR_ARG
    assert status_of(lambda: pv.segment_resynthesis(spec, 0)) == _lib.PV_ERR_ARG
    pv.set_transients("off")
    pv.resynthesis(spec)
    pv.segment_summary(spec)
    # capacity
    import torch
    big = torch.zeros((2, 8), dtype=torch.uint8, device="cuda")
    assert status_of(lambda: pv.set_transient_flags(big)) == _lib.PV_ERR_ARG  # 2 channels > max_channels
