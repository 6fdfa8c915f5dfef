"""The real-time pitch map on the GPU (pv_rt_pitchmap_reserve / pv_rt_pitchmap_push; DESIGN.md
§3.16): the emitted stream against tests/rt_pitchmap_ref.py's fp64 stream and against the GPU's
own batched pitch_map_process, its independence of how the stream is cut into pushes, of the other
channels and of the captured callback, the clamp, a silent lead-in, the reset, the refusals, and a
live pitch correction.  5 channels: one more than the 4 waves of a real-time workgroup.  Every
test ratio is an fp32 value."""
import numpy as np
import pytest

import pitchtrack_ref as pr
import pvref
import rt_pitchmap_ref as rm
from gpu_helpers import RMS_TOL, status_of, to_dev
from pvamd import MAJOR, PITCH_SHIFT, STANDARD, TIME_SHIFT, PhaseVocoder, RealTimeVocoder, _lib, pitch_correction
from signals import rms, synth

pytestmark = pytest.mark.gpu

C = 5
WIDE = (0.25, 4.0)
MID = (0.5, 2.0)


def signal(n, seed, channels=C):
    return np.stack([synth(n, seed + 13 * c) for c in range(channels)])


def sequence(kind, T, channels=C):
    """[channels, T] float32 ratios"""
    if kind == "vibrato":  # +-6 %, a different phase per channel
        return np.stack([rm.vibrato(T, 0.06, 23.0, 1.3 * c) for c in range(channels)])
    one = {"one": lambda: rm.constant(T, 1.0), "1.5": lambda: rm.constant(T, 1.5), "0.75": lambda: rm.constant(T, 0.75),
           "glide": lambda: rm.glide(T, 0.5, 2.0), "alternating": lambda: rm.alternating(T, 0.25, 4.0)}[kind]()
    return np.tile(one, (channels, 1))


def cuts_of(T, per_push):
    """T frames in pushes of per_push frames (an int, or a pattern that repeats), the rest last"""
    pat = [per_push] if isinstance(per_push, int) else list(per_push)
    out, i = [], 0
    while sum(out) < T:
        out.append(min(pat[i % len(pat)], T - sum(out)))
        i += 1
    return out


def make(N, hop_div, lock, quality=0, rng=MID, max_frames=4, channels=C):
    rt = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div, channels=channels, phase_lock=lock)
    rt.reserve_pitch_map(quality, max_frames, ratio_min=rng[0], ratio_max=rng[1])
    return rt


def run(rt, xs, ratios, per_push, spec=None, phases=None):
    """xs [C, T hop], ratios [C, T] (None: no ratio argument) -> the emitted stream [C, T hop]"""
    hop = rt.hopSize
    xd = to_dev(xs)
    rd = None if ratios is None else to_dev(np.asarray(ratios, np.float32))
    outs, t = [], 0
    for nf in cuts_of(xs.shape[1] // hop, per_push):
        r = None if rd is None else rd[:, t:t + nf].contiguous()
        s = None if spec is None else spec[:, :nf]
        outs.append(rt.pitch_map_push(xd[:, t * hop:(t + nf) * hop].contiguous(), r, spec=s).cpu().numpy())
        if phases is not None:
            phases.append(spec.cpu().numpy()[:, :nf, :rt.spec_bins, 1].copy())
        t += nf
    return np.concatenate(outs, axis=1)


# ------------------------------------------------------------------ parity against the reference
GEOMETRIES = [(256, 4, 40, 0), (512, 3, 40, 0), (1024, 4, 24, 1), (2048, 4, 16, 0)]  # N, hop_div, frames, quality
KINDS = ["one", "1.5", "0.75", "glide", "vibrato", "alternating"]


@pytest.mark.parametrize("per_push", [1, 3, 4])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,hop_div,T,quality", GEOMETRIES)
def test_stream_matches_reference(cuda, N, hop_div, T, quality, kind, lock, per_push):
    """RMS_TOL against the fp64 stream (computed once per case and shared by the push sizes); the
    analysis phases of the returned rows are the oracle's bit for bit.  Constant 1, 1.5, 0.75, a glide
    0.5 -> 2 and a +-6 % vibrato under [1/2, 2]; 1/4 and 4 alternating under [1/4, 4]: spans of 0
    and of 4 stretched frames."""
    import torch
    hop = N // hop_div
    rng = WIDE if kind == "alternating" else MID
    rt = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div, channels=C, phase_lock=lock)
    st = status_of(lambda: rt.reserve_pitch_map(quality, 4, ratio_min=rng[0], ratio_max=rng[1]))
    if N == 2048 and st == _lib.PV_ERR_UNSUPPORTED:
        return  # documented: no k_rt_map for n_samps = 2048
    assert st == _lib.PV_OK
    G = rm.plan(hop, quality, *rng)["G"]
    assert rt.pitch_map_latency == (G + 1) * hop and T - 1 - G >= 8
    xs = signal(T * hop, 6100 + N)
    ratios = sequence(kind, T)
    spec = torch.zeros((C, 4, rt.spec_stride, 2), dtype=torch.float32, device="cuda")
    phases = []
    g = run(rt, xs, ratios, per_push, spec, phases)
    assert g.shape == (C, T * hop) and np.isfinite(g).all()
    assert not g[:, :(G + 1) * hop].any() and g[:, (G + 1) * hop:].any()
    gph = np.concatenate(phases, axis=1)
    for c in range(C):
        ref = rm.cached(xs[c], N, hop_div, ratios[c], lock, quality, *rng)
        err = rms(g[c], ref)
        print(f"N={N} hop {hop} {kind} lock {lock} quality {quality} per push {per_push} channel {c}: rms {err:.3e}")
        assert err <= RMS_TOL, f"channel {c}: rms {err}"
        xp = np.concatenate([np.zeros(N - hop, np.float32), xs[c]])
        _, ph = pvref.std_analysis(xp, N, hop, T)
        assert np.array_equal(gph[c].view(np.uint32), ph.view(np.uint32)), f"channel {c}: phases differ"


# ------------------------------------------------------------------ against the batched GPU path
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,T,kind", [(256, 4, 40, "glide"), (512, 3, 30, "vibrato"), (1024, 4, 24, "glide")])
def test_stream_matches_batched_pitch_map(cuda, N, hop_div, T, kind, lock):
    """The GPU's batched pitch_map_process of the zero-prefixed stream (positions = arange, the
    ratios per channel) over a longer input: its first blocks, clear of the batch's tail, against
    the stream behind its latency.  1e-6 absolute, the real-time-against-batched bound."""
    hop = N // hop_div
    T2 = T + 12
    xs = signal(T2 * hop, 6500 + N)
    ratios = sequence(kind, T2)
    rt = make(N, hop_div, lock)
    G = rm.plan(hop, 0, *MID)["G"]
    g = run(rt, xs[:, :T * hop], ratios[:, :T], 3)
    n = T2 - 1
    xp = np.concatenate([np.zeros((C, N - hop), np.float32), xs], axis=1)
    pv = PhaseVocoder(N, TIME_SHIFT, 1.0, hop_div, mode=STANDARD, max_channels=C, max_frames=4 * T2, phase_lock=lock)
    pv.set_pitch_map(np.tile(np.arange(n, dtype=np.float64), (C, 1)), ratios[:, 1:].astype(np.float64))
    out, _ = pv.pitch_map_process(to_dev(xp))
    b = out.cpu().numpy()
    nb = T - 1 - G
    d = float(np.max(np.abs(g[:, (G + 1) * hop:] - b[:, :nb * hop])))
    print(f"N={N} {kind} lock {lock}: stream - batched pitch map over {nb} blocks: max abs {d:.3e}")
    assert np.abs(b[:, :nb * hop]).max() > 0.05
    assert d <= 1e-6


@pytest.mark.parametrize("ratio", [2.0, 0.5])
def test_taps_are_the_batched_kernel_s_bit_for_bit(cuda, monkeypatch, ratio):
    """At a constant ratio of 2 or 1/2 the stretched frames' fractions (0 and 1/2, or 0) are exact in
    both plans, and with the batched stretch in one run of 256 frames (no seam: its overlap-add is
    then the stream's, frame after frame) the stretched samples are the same bit for bit.  So must
    the outputs be: k_rt_varresample's tap loop (pv_varresample.hpp vartap::output) and the one in
    k_var_resample's body are the same operations in the same order."""
    monkeypatch.setenv("PV_RUN_FRAMES", "256")
    N, hop_div, T, T2 = 256, 4, 40, 52
    hop = N // hop_div
    xs = signal(T2 * hop, 7300)
    ratios = np.full((C, T2), ratio, np.float32)
    rt = make(N, hop_div, True)
    G = rm.plan(hop, 0, *MID)["G"]
    g = run(rt, xs[:, :T * hop], ratios[:, :T], 3)
    xp = np.concatenate([np.zeros((C, N - hop), np.float32), xs], axis=1)
    pv = PhaseVocoder(N, TIME_SHIFT, 1.0, hop_div, mode=STANDARD, max_channels=C, max_frames=4 * T2, phase_lock=True)
    assert pv.frames_per_run == 256
    pv.set_pitch_map(np.tile(np.arange(T2 - 1, dtype=np.float64), (C, 1)), ratios[:, 1:].astype(np.float64))
    out, _ = pv.pitch_map_process(to_dev(xp))
    nb = T - 1 - G
    a, b = g[:, (G + 1) * hop:], out.cpu().numpy()[:, :nb * hop]
    print(f"ratio {ratio}: stream - batched pitch map: max abs {float(np.max(np.abs(a - b))):.3e}")
    assert np.abs(b).max() > 0.05
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ bit-identical
@pytest.mark.parametrize("N,T,kind,rng,quality", [(256, 48, "vibrato", MID, 0), (256, 48, "alternating", WIDE, 0),
                                                  (256, 48, "glide", MID, 1), (2048, 24, "alternating", WIDE, 0)])
def test_stream_does_not_depend_on_the_chunking(cuda, N, T, kind, rng, quality):
    """1 frame per push, 4 per push, and 3, 1, 2 in turn: the same bits (at the largest size under
    [1/4, 4] too: spans of 0 and 4 stretched frames in pushes of 4 fill the row the most)"""
    hop_div = 4
    xs = signal(T * (N // hop_div), 880)
    ratios = sequence(kind, T)
    got = [run(make(N, hop_div, True, quality, rng), xs, ratios, pp) for pp in (1, 4, (3, 1, 2))]
    assert got[0].any()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_a_channel_alone_equals_its_row_of_the_batch(cuda):
    N, hop_div, T = 512, 4, 30
    xs = signal(T * (N // hop_div), 77)
    ratios = sequence("vibrato", T)
    whole = run(make(N, hop_div, True), xs, ratios, 2)
    for c in (0, 4):
        alone = run(make(N, hop_div, True, channels=1), xs[c:c + 1], ratios[c:c + 1], 2)
        assert alone.any() and np.array_equal(alone[0], whole[c])


@pytest.mark.parametrize("launch", ["direct", "graph"])
def test_callback_with_pinned_ratios_equals_push(cuda, monkeypatch, launch):
    """the captured callback reads its ratios from the pinned buffer at replay time"""
    monkeypatch.setenv("PV_RT_LAUNCH", launch)
    N, hop_div, T, nf = 256, 4, 30, 2
    hop = N // hop_div
    xs = signal(T * hop, 310)
    ratios = sequence("vibrato", T)
    a, b = make(N, hop_div, True, max_frames=nf), make(N, hop_div, True, max_frames=nf)
    b.capture(nf)
    assert b.host_in.shape == (C, nf * hop) and b.host_out.shape == (C, nf * hop)
    assert b.host_ratios.shape == (C, nf) and (b.host_ratios == 1.0).all()
    ga = run(a, xs, ratios, nf)
    n = nf * hop
    gb = []
    for j in range(T // nf):
        if j % 2:  # through the argument, or written in place
            gb.append(b.callback(xs[:, j * n:(j + 1) * n], ratios[:, j * nf:(j + 1) * nf]).copy())
        else:
            b.host_ratios[...] = ratios[:, j * nf:(j + 1) * nf]
            gb.append(b.callback(xs[:, j * n:(j + 1) * n]).copy())
    gb = np.concatenate(gb, axis=1)
    assert ga.any() and np.array_equal(ga, gb)
    # without ratios the callback keeps the last ones; ratios of 1 are the NULL argument's
    import torch
    torch.cuda.synchronize()
    b.reset()
    a.reset()
    torch.cuda.synchronize()
    b.host_ratios[...] = 1.0
    again = np.concatenate([b.callback(xs[:, j * n:(j + 1) * n]).copy() for j in range(6)], axis=1)
    assert np.array_equal(again, run(a, xs[:, :6 * n], None, nf))


def test_out_of_range_and_nan_ratios_are_clamped(cuda):
    N, hop_div, T = 256, 4, 30
    xs = signal(T * (N // hop_div), 4242)
    wild = sequence("vibrato", T)
    wild[:, 3::5] = 7.5
    wild[:, 4::7] = 0.01
    wild[:, 6::9] = np.nan
    wild[1, 10] = np.inf
    wild[2, 11] = -np.inf
    wild[3, 12] = -1.0
    tame = np.where(np.isnan(wild), MID[0], np.clip(wild, MID[0], MID[1])).astype(np.float32)
    a = run(make(N, hop_div, True), xs, wild, 3)
    b = run(make(N, hop_div, True), xs, tame, 3)
    assert np.isfinite(a).all() and a.any() and np.array_equal(a, b)


def test_a_silent_lead_in_delays_the_stream(cuda):
    """Three silent frames at ratio 1 in front of a stream (whose own first ratio is 1): the stream's
    output, 3 hop later, bit for bit — Phi, the positions and every tap's fraction are the same.
    Where the stream alone emits its G + 1 blocks of zeros by definition, the delayed one emits the
    blocks below the stream's block 0: their taps reach the first stretched samples, an input of
    N - hop zeros resynthesised, which are zero up to the fp32 rounding of one frame (below 1e-6)."""
    N, hop_div, T = 256, 4, 30
    hop = N // hop_div
    xs = signal(T * hop, 515)
    ratios = sequence("glide", T)
    ratios[:, 0] = 1.0
    G = rm.plan(hop, 0, *MID)["G"]
    own = run(make(N, hop_div, True), xs, ratios, 2)
    led = run(make(N, hop_div, True), np.concatenate([np.zeros((C, 3 * hop), np.float32), xs], axis=1),
              np.concatenate([np.ones((C, 3), np.float32), ratios], axis=1), 2)
    lat = (G + 1) * hop
    assert own[:, lat:].any()
    assert not led[:, :lat].any()
    assert np.array_equal(led[:, 3 * hop + lat:], own[:, lat:])
    pre = float(np.max(np.abs(led[:, lat:3 * hop + lat])))
    print(f"the blocks below the stream's block 0: max abs {pre:.3e}")
    assert pre <= 1e-6


# ------------------------------------------------------------------ after a reset
def test_after_a_reset_the_other_pushes_are_a_fresh_handle_s(cuda):
    import torch
    N, hop_div, T = 256, 4, 12
    hop = N // hop_div
    xs = signal(T * hop, 99)
    xd = to_dev(xs)
    for lock in (False, True):
        used = make(N, hop_div, lock)
        run(used, xs, sequence("glide", T), 4)
        fresh = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div, channels=C, phase_lock=lock)
        torch.cuda.synchronize()
        used.reset()
        want = np.concatenate([fresh.push(xd[:, j * hop:(j + 1) * hop].contiguous()).cpu().numpy() for j in range(T)], 1)
        got = np.concatenate([used.push(xd[:, j * hop:(j + 1) * hop].contiguous()).cpu().numpy() for j in range(T)], 1)
        assert want.any() and np.array_equal(got, want)
        # pv_rt_pitch_push on the same handle (out hop = hop: the push itself), and the map again
        run(used, xs, sequence("vibrato", T), 3)
        used.reserve_pitch(0, max_frames=4)
        used.reset()
        fresh.reset()
        torch.cuda.synchronize()
        want = np.concatenate([fresh.push(xd[:, j * hop:(j + 1) * hop].contiguous()).cpu().numpy() for j in range(T)], 1)
        got = np.concatenate([used.pitch_push(xd[:, j * hop:(j + 1) * hop].contiguous()).cpu().numpy() for j in range(T)], 1)
        assert np.array_equal(got, want)
        used.reset()
        again = run(used, xs, sequence("glide", T), 4)
        assert np.array_equal(again, run(make(N, hop_div, lock), xs, sequence("glide", T), 4))


# ------------------------------------------------------------------ refusals
def test_refusals(cuda):
    import torch
    N, hop_div = 256, 4
    hop = N // hop_div
    x = torch.zeros((1, 2 * hop), dtype=torch.float32, device="cuda")
    r = torch.ones((1, 2), dtype=torch.float32, device="cuda")
    # a PV_PITCH_SHIFT handle, out_hop != hop, hop < 16
    assert status_of(lambda: RealTimeVocoder(N, PITCH_SHIFT, 1.5, hop_div).reserve_pitch_map()) == _lib.PV_ERR_UNSUPPORTED
    assert status_of(lambda: RealTimeVocoder(N, TIME_SHIFT, 1.5, hop_div).reserve_pitch_map()) == _lib.PV_ERR_UNSUPPORTED
    assert status_of(lambda: RealTimeVocoder(N, TIME_SHIFT, 1.0, 32).reserve_pitch_map()) == _lib.PV_ERR_UNSUPPORTED
    rt = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div)
    assert rt.pitch_map_latency == 0
    # push before a successful reserve
    assert status_of(lambda: rt.pitch_map_push(x, r)) == _lib.PV_ERR_ARG
    # bad quality, max_nframes <= 0, bad ranges
    for quality, mx, lo, hi in ((2, 1, 0.5, 2.0), (-1, 1, 0.5, 2.0), (0, 0, 0.5, 2.0), (0, -3, 0.5, 2.0),
                                (0, 1, 0.2, 2.0), (0, 1, 0.5, 4.5), (0, 1, 2.0, 0.5), (0, 1, float("nan"), 2.0),
                                (0, 1, 0.5, float("nan"))):
        assert status_of(lambda: rt.reserve_pitch_map(quality, mx, ratio_min=lo, ratio_max=hi)) == _lib.PV_ERR_ARG
    assert rt.pitch_map_latency == 0
    # G > 64: hop 16, best preset, [1/4, 4] needs 68 callbacks
    small = RealTimeVocoder(N, TIME_SHIFT, 1.0, 16)
    assert rm.plan(16, 1, *WIDE)["G"] == 68
    assert status_of(lambda: small.reserve_pitch_map(1, 1, ratio_min=0.25, ratio_max=4.0)) == _lib.PV_ERR_ARG
    small.reserve_pitch_map(0, 1, ratio_min=0.25, ratio_max=4.0)
    assert small.pitch_map_latency == (rm.plan(16, 0, *WIDE)["G"] + 1) * 16
    # more frames than reserved, in a push and in a capture
    rt.reserve_pitch_map(0, 1, ratio_min=0.84, ratio_max=1.19)
    assert rt.pitch_map_latency == 2 * hop
    assert status_of(lambda: rt.pitch_map_push(x, r)) == _lib.PV_ERR_ARG
    assert status_of(lambda: rt.capture(2)) == _lib.PV_ERR_ARG
    assert rt.pitch_map_push(x[:, :hop], r[:, :1]).shape == (1, hop)
    assert rt.pitch_map_push(x[:, :hop]).shape == (1, hop)
    # the pinned ratios exist only behind a captured pitch map callback
    import ctypes
    fr = ctypes.POINTER(ctypes.c_float)()
    assert rt._L.pv_rt_pitchmap_host_ratios(rt._h, ctypes.byref(fr)) == _lib.PV_ERR_ARG
    # the later successful reserve decides what is captured
    rt.reserve_pitch(0, max_frames=1)
    rt.capture(1)
    assert rt.host_ratios is None
    assert rt._L.pv_rt_pitchmap_host_ratios(rt._h, ctypes.byref(fr)) == _lib.PV_ERR_ARG
    assert len(rt._L.pv_last_error()) > 0
    rt2 = RealTimeVocoder(N, TIME_SHIFT, 1.0, hop_div)
    rt2.reserve_pitch(0, max_frames=1)
    rt2.reserve_pitch_map(0, 1)
    rt2.capture(1)
    assert rt2.host_ratios is not None
    # the setup call comes before pv_rt_capture
    assert status_of(lambda: rt2.reserve_pitch_map(0, 1)) == _lib.PV_ERR_ARG
    assert rt2.callback(np.zeros((1, hop), np.float32), np.ones((1, 1), np.float32)).shape == (1, hop)


def test_reserve_out_of_memory_leaves_the_feature_off(cuda):
    """scratch rows of 256 channels x 4e6 frames x 64 samples x ratio 2 (0.5 TB) cannot be allocated;
    the rows are the first allocation, so nothing else is taken before it fails"""
    import torch
    rt = RealTimeVocoder(256, TIME_SHIFT, 1.0, 4, channels=256)
    assert status_of(lambda: rt.reserve_pitch_map(0, max_frames=4_000_000)) == _lib.PV_ERR_NOMEM
    assert rt.pitch_map_latency == 0
    x = torch.zeros((256, 64), dtype=torch.float32, device="cuda")
    assert status_of(lambda: rt.pitch_map_push(x)) == _lib.PV_ERR_ARG
    assert rt.push(x).shape == (256, 64)


# ------------------------------------------------------------------ live correction
def test_live_correction(cuda):
    """DESIGN.md §3.14's voice corrected live: per callback pitch_map_push(spec = rows), the GPU's
    pitch_track of the row on a batch handle of the same geometry, the host's causal correction of
    the track so far, and its last ratio pushed with the next frame.  The median distance to the
    scale of the rows' track (before) and of the emitted stream's (after) must reproduce the
    reference's figures (tests/test_rt_pitchmap_ref.py: 34.99 -> 1.90 cents) within
    1200 log2(1 + 2 F0_TOL) cents, §3.14's margin."""
    import torch
    N, hop_div = pr.E2E_N, pr.E2E_HOP_DIV
    hop = N // hop_div
    x = pr.e2e_input()
    T = len(x) // hop
    ref_before, ref_after = rm.live_reference()
    tol = 1200.0 * np.log2(1.0 + 2.0 * pr.F0_TOL)
    fmin, fmax = pr.E2E_RANGE
    rt = make(N, hop_div, True, 0, rm.LIVE_RANGE, max_frames=1, channels=1)
    pv = PhaseVocoder(N, TIME_SHIFT, 1.0, hop_div, mode=STANDARD, max_channels=1, max_frames=T + 8)
    xd = to_dev(x[None, :T * hop])
    rows = torch.zeros((1, 1, rt.spec_stride, 2), dtype=torch.float32, device="cuda")
    ratio = torch.ones((1, 1), dtype=torch.float32, device="cuda")
    track, outs = [], []
    for t in range(T):
        outs.append(rt.pitch_map_push(xd[:, t * hop:(t + 1) * hop].contiguous(), ratio, spec=rows).cpu().numpy())
        track.append(pv.pitch_track(rows, fmin, fmax)[0, 0].cpu().numpy())
        c = pitch_correction(np.stack(track), pr.E2E_A4, MAJOR, strength_min=0.5, retune=1.0)
        ratio = to_dev(np.full((1, 1), c[-1], np.float32))
    trk = np.stack(track)
    before = pr.median_cents(trk[:, 0], trk[:, 1])
    y = np.concatenate(outs, axis=1)[:, rt.pitch_map_latency:]
    frames = pvref.num_frames(y.shape[1], hop)
    trk2 = pv.pitch_track(pv.analysis(to_dev(y), frames=frames), fmin, fmax)[0].cpu().numpy()
    after = pr.median_cents(trk2[:, 0], trk2[:, 1])
    print(f"median cents off the scale, live: before {before:.4f} (reference {ref_before:.4f}), "
          f"after {after:.4f} (reference {ref_after:.4f}); margin {tol:.4f}")
    assert abs(before - ref_before) <= tol
    assert abs(after - ref_after) <= tol
    assert after <= 0.1 * before
