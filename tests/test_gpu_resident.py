"""The channel-resident time stretch (pv_resident.hip; PV_RESIDENT): one workgroup per channel,
the spectrum rows in LDS.  Its output is the split path's bit for bit — every frame count around
the pipeline's fill and drain and around the run and four-run boundaries, ragged inputs, the
signal zoo (and with it the oracle's per-hop bound), repeated calls on one handle, a side stream,
a captured graph without any reserve — and every call it does not serve takes the split path."""
import ctypes

import numpy as np
import pytest

from gpu_helpers import ZOO_SAMPLES, to_dev, zoo_input, zoo_reference
from pvamd import STANDARD, TIME_SHIFT, PhaseVocoder, _lib
from signals import ZOO_NAMES, assert_hop_parity, synth

pytestmark = pytest.mark.gpu

N, HOP_DIV, SCALE, HOP = 1024, 4, 0.5, 256
SPLIT_KERNELS = ("analysis", "carry", "synthesis")


def _vocoder(monkeypatch, resident, C, frames, run_frames=8, scale=SCALE, **kw):
    """resident: "0", "1" or None (the knob unset)"""
    monkeypatch.setenv("PV_RUN_FRAMES", str(run_frames))
    if resident is None:
        monkeypatch.delenv("PV_RESIDENT", raising=False)
    else:
        monkeypatch.setenv("PV_RESIDENT", resident)
    pv = PhaseVocoder(N, TIME_SHIFT, scale, HOP_DIV, mode=STANDARD, max_channels=C, max_frames=frames, **kw)
    assert pv.frames_per_run == run_frames and not pv.single_launch
    return pv


def _run(pv, xd, **kw):
    """(out, spec, names of the kernels the call launched)"""
    pv.profile(True)
    pv.profile_reset()
    out, spec = pv.process(xd, **kw)
    prof = pv.profile_read()
    pv.profile(False)
    return out, spec, set(prof)


def _assert_resident(kernels):
    assert kernels == {"resident"}, kernels


def _assert_split(kernels):
    assert "resident" not in kernels and all(k in kernels for k in SPLIT_KERNELS), kernels


def _same(a, b, what):
    import torch
    assert a.shape == b.shape, what
    if not torch.equal(a, b):
        g, r = a.cpu().numpy(), b.cpu().numpy()
        bad = g.view(np.uint32) != r.view(np.uint32)
        c, i = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} samples differ, first at channel {c} sample {i} "
                             f"(frame {i // 128}): resident {g[c, i]!r} split {r[c, i]!r}")


def _samples_for(frames):
    return HOP * (frames + 1)  # num_frames(n) = ceil((n - hop) / hop)


F = 8
# pipeline fill and drain; around a run, around the four-run group; many runs and a partial one
FRAME_COUNTS = [1, 2, 3, 7, 8, 9, F - 1, F, F + 1, 4 * F, 4 * F + 1, 9 * F + 5]


@pytest.mark.parametrize("C", [1, 3, 5])
def test_bit_identical_to_the_split_path(cuda, monkeypatch, C):
    tmax = max(FRAME_COUNTS)
    xs = np.stack([synth(_samples_for(tmax), 900 + c) for c in range(C)])
    ps = _vocoder(monkeypatch, "0", C, tmax)
    pr = _vocoder(monkeypatch, "1", C, tmax)
    assert ps.resident_min_channels == 0 and pr.resident_min_channels == 1
    for T in sorted(set(FRAME_COUNTS)):
        xd = to_dev(xs[:, :_samples_for(T)])
        assert pr.num_frames(xd.shape[1]) == T
        want, _, ks = _run(ps, xd, spectrum=False)
        got, none, kr = _run(pr, xd, spectrum=False)
        _assert_split(ks)
        _assert_resident(kr)
        assert none is None
        _same(got, want, f"C={C} frames={T}")


@pytest.mark.parametrize("n", [HOP * 10 + 77, HOP * 21 + 1, 900, 769, 1023, 1024, 1025])
def test_ragged_inputs(cuda, monkeypatch, n):
    """a length that is no multiple of the hop, and inputs between N - hop and N samples: the
    last frames read past the end (zeros).  The rows are n samples of a buffer with an even
    row stride (an odd stride takes the split path: test_fallbacks_take_the_split_path); what
    lies behind sample n must not be read as signal."""
    C = 3
    xs = np.stack([synth(n + (n & 1) + 2, 40 + c) for c in range(C)])
    xd = to_dev(xs)
    assert xd.stride(0) % 2 == 0
    ps = _vocoder(monkeypatch, "0", C, 64)
    pr = _vocoder(monkeypatch, "1", C, 64)
    want, _, ks = _run(ps, xd, n_samples=n, spectrum=False)
    got, _, kr = _run(pr, xd, n_samples=n, spectrum=False)
    _assert_split(ks)
    _assert_resident(kr)
    _same(got, want, f"n={n}")


def test_longer_runs(cuda, monkeypatch):
    """F = 16, 9 F + 5 frames"""
    C, T = 3, 9 * 16 + 5
    xd = to_dev(np.stack([synth(_samples_for(T), 7 + c) for c in range(C)]))
    want, _, _ = _run(_vocoder(monkeypatch, "0", C, T, run_frames=16), xd, spectrum=False)
    got, _, kr = _run(_vocoder(monkeypatch, "1", C, T, run_frames=16), xd, spectrum=False)
    _assert_resident(kr)
    _same(got, want, "F=16")


def test_signal_zoo(cuda, monkeypatch):
    """the ten adversarial signals as channels: the split path's bits, and on the same run the
    oracle's per-hop bound (as tests/test_gpu_signals.py)"""
    xs = zoo_input(ZOO_SAMPLES, N)
    frames = -(-(ZOO_SAMPLES - HOP) // HOP)
    # (12001 samples in rows of an even stride)
    xd = to_dev(np.concatenate([xs, np.zeros((len(xs), 1), np.float32)], axis=1))
    want, _, ks = _run(_vocoder(monkeypatch, "0", len(xs), frames), xd, n_samples=ZOO_SAMPLES, spectrum=False)
    pr = _vocoder(monkeypatch, "1", len(xs), frames)
    got, _, kr = _run(pr, xd, n_samples=ZOO_SAMPLES, spectrum=False)
    _assert_split(ks)
    _assert_resident(kr)
    _same(got, want, "zoo")
    g = got.cpu().numpy()
    refs, port, hs = zoo_reference(N, HOP_DIV, TIME_SHIFT, SCALE)
    assert hs == pr.outHopSize and np.isfinite(g).all()
    for c, name in enumerate(ZOO_NAMES):
        assert g[c].shape == refs[c].shape
        assert_hop_parity(g[c], refs[c], port[c], hs, what=f"resident {name}")


def test_handle_state_and_side_stream(cuda, monkeypatch):
    """two calls of different channel and frame counts on one handle, then the first again:
    its result comes back; the same call on a non-default stream"""
    import torch
    a = to_dev(np.stack([synth(_samples_for(37), 1 + c) for c in range(5)]))
    b = to_dev(np.stack([synth(_samples_for(11), 9 + c) for c in range(2)]))
    ps = _vocoder(monkeypatch, "0", 5, 40)
    pr = _vocoder(monkeypatch, "1", 5, 40)
    first, _, kr = _run(pr, a, spectrum=False)
    _assert_resident(kr)
    _same(first, ps.process(a, spectrum=False)[0], "first call")
    second, _, kr = _run(pr, b, spectrum=False)
    _assert_resident(kr)
    _same(second, ps.process(b, spectrum=False)[0], "second call")
    _same(pr.process(a, spectrum=False)[0], first, "first call repeated")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out, _ = pr.process(a, spectrum=False)
    side.synchronize()
    _same(out, first, "side stream")


def test_graph_capture_needs_no_reserve(cuda, monkeypatch):
    """the resident call allocates nothing: it is captured on a fresh handle, and two replays
    into a zeroed buffer give the uncaptured call's bits"""
    import torch
    C, T = 3, 29
    xd = to_dev(np.stack([synth(_samples_for(T), 60 + c) for c in range(C)]))
    want, _ = _vocoder(monkeypatch, "0", C, T).process(xd, spectrum=False)
    pr = _vocoder(monkeypatch, "1", C, T)
    out = torch.zeros_like(want)
    L = _lib.lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        st = L.pv_process(pr._h, xd.data_ptr(), xd.stride(0), xd.shape[1], C, T, None, 0, out.data_ptr(),
                          out.stride(0), ctypes.c_void_p(s.cuda_stream))
        g.capture_end()
    assert st == _lib.PV_OK, L.pv_last_error()
    for k in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(out, want, f"replay {k}")


def test_fallbacks_take_the_split_path(cuda, monkeypatch):
    """a caller spectrum, phase locking, an out hop the kernel does not serve, an unaligned input
    row stride, and the knob unset below the automatic threshold: the split path's launches, and
    the bits of a PV_RESIDENT=0 handle"""
    import torch
    C, T = 3, 21
    n = _samples_for(T)
    xs = np.stack([synth(n, 80 + c) for c in range(C)])
    xd = to_dev(xs)
    ps = _vocoder(monkeypatch, "0", C, T)
    pr = _vocoder(monkeypatch, "1", C, T)
    # a caller spectrum
    want, wspec, _ = _run(ps, xd)
    got, gspec, k = _run(pr, xd)
    _assert_split(k)
    _same(got, want, "caller spectrum: out")
    _same(gspec, wspec, "caller spectrum: rows")
    # phase lock on
    pl0 = _vocoder(monkeypatch, "0", C, T, phase_lock=True)
    pl1 = _vocoder(monkeypatch, "1", C, T, phase_lock=True)
    got, _, k = _run(pl1, xd, spectrum=False)
    assert "resident" not in k and "synthesis_locked" in k, k
    _same(got, pl0.process(xd, spectrum=False)[0], "phase lock")
    # stretch 0.75: out hop 192
    p0 = _vocoder(monkeypatch, "0", C, T, scale=0.75)
    p1 = _vocoder(monkeypatch, "1", C, T, scale=0.75)
    assert p1.outHopSize == 192 and p1.resident_min_channels == 0
    got, _, k = _run(p1, xd, spectrum=False)
    _assert_split(k)
    _same(got, p0.process(xd, spectrum=False)[0], "out hop 192")
    # an odd input row stride
    wide = torch.zeros((C, n + 1), dtype=torch.float32, device="cuda")
    wide[:, :n] = xd
    xo = wide[:, :n]
    assert xo.stride(0) % 2 == 1
    got, _, k = _run(pr, xo, spectrum=False)
    _assert_split(k)
    _same(got, ps.process(xd, spectrum=False)[0], "odd ldx")
    # the knob unset: C = 3 channels are below any automatic threshold (0: the path is off)
    pa = _vocoder(monkeypatch, None, C, T)
    assert pa.resident_min_channels == 0 or pa.resident_min_channels > C
    got, _, k = _run(pa, xd, spectrum=False)
    _assert_split(k)
    _same(got, ps.process(xd, spectrum=False)[0], "knob unset")
