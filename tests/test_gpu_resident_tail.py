"""The analysis waves of the channel-resident stretch (pv_resident.hip) walk a channel in a
steady-state loop of vector loads, two frames per trip with the input registers rotated, and
hand the channel's last frames to a bounds-checked loop; the handoff can fall on either rotation
phase of either wave.  Every handoff, a long channel in which both phases recur across the run
boundaries, and two calls of different lengths on one handle: the split path's bits
(PV_RESIDENT=1 against PV_RESIDENT=0, torch.equal), from exactly the kernel `resident`."""
import functools

import numpy as np
import pytest

from gpu_helpers import to_dev
from pvamd import STANDARD, TIME_SHIFT, PhaseVocoder

pytestmark = pytest.mark.gpu

N, HOP_DIV, SCALE, HOP = 1024, 4, 0.5, 256
F = 8            # PV_RUN_FRAMES
C = 3
MAX_FRAMES = 64
# n = N + hop m + d: lastfull = (n - N) / hop = m, so m = 0 .. 7 puts the last fast frame on both
# waves (m even / odd) and both rotation phases (m / 2 even / odd); m = 0: wave 1 has no fast
# frame and wave 0 exactly one, m = 1: wave 1 exactly one.  d = 0: the frame after the last fast
# one starts its zeros exactly at a pair; d = 1, 255: inside one.  258, 511, 1022: no fast frame.
HANDOFFS = [N + HOP * m + d for m in range(8) for d in (0, 1, 255)] + [258, 511, 1022]
LONG_FRAMES = 4 * F + 3


@functools.lru_cache(maxsize=None)
def _noise(n, seed0):
    """C rows of full-scale uniform noise, n samples each, different seeds: no bin is small, and
    a swapped or shifted mirrored bin cannot cancel"""
    xs = np.stack([np.random.default_rng(seed0 + c).uniform(-1.0, 1.0, n).astype(np.float32) for c in range(C)])
    xs.setflags(write=False)
    return xs


def _vocoder(monkeypatch, resident, frames=MAX_FRAMES):
    monkeypatch.setenv("PV_RUN_FRAMES", str(F))
    monkeypatch.setenv("PV_RESIDENT", resident)
    pv = PhaseVocoder(N, TIME_SHIFT, SCALE, HOP_DIV, mode=STANDARD, max_channels=C, max_frames=frames)
    assert pv.frames_per_run == F and not pv.single_launch
    return pv


def _run(pv, xd, n):
    """(out, names of the kernels the call launched)"""
    pv.profile(True)
    pv.profile_reset()
    out, spec = pv.process(xd, n_samples=n, spectrum=False)
    prof = pv.profile_read()
    pv.profile(False)
    assert spec is None
    return out, set(prof)


def _same(a, b, what):
    import torch
    assert a.shape == b.shape, what
    if not torch.equal(a, b):
        g, r = a.cpu().numpy(), b.cpu().numpy()
        bad = g.view(np.uint32) != r.view(np.uint32)
        c, i = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} samples differ, first at channel {c} sample {i} "
                             f"(frame {i // 128}): resident {g[c, i]!r} split {r[c, i]!r}")


def _rows(n, seed0):
    """n samples of noise per row in a buffer of an even row stride; behind sample n lies more
    full-scale noise, which must not be read as signal"""
    xd = to_dev(np.array(_noise(n + (n & 1) + 2, seed0)))
    assert xd.stride(0) % 2 == 0 and xd.shape[1] > n
    return xd


def _check(ps, pr, xd, n, what):
    want, ks = _run(ps, xd, n)
    got, kr = _run(pr, xd, n)
    assert "resident" not in ks and ks, ks
    assert kr == {"resident"}, kr
    _same(got, want, what)
    return got


@pytest.mark.parametrize("n", HANDOFFS)
def test_handoff_at_every_phase(cuda, monkeypatch, n):
    ps, pr = _vocoder(monkeypatch, "0"), _vocoder(monkeypatch, "1")
    lastfull = (n - N) // HOP if n >= N else -1
    frames = pr.num_frames(n)
    assert lastfull < frames and frames - 1 - lastfull <= N // HOP, (n, lastfull, frames)
    _check(ps, pr, _rows(n, 300), n, f"n={n} (lastfull {lastfull}, {frames} frames)")


def test_long_channel(cuda, monkeypatch):
    """4 F + 3 frames: both rotation phases recur across the run boundaries"""
    n = HOP * (LONG_FRAMES + 1)
    ps, pr = _vocoder(monkeypatch, "0"), _vocoder(monkeypatch, "1")
    assert pr.num_frames(n) == LONG_FRAMES
    _check(ps, pr, _rows(n, 300), n, f"{LONG_FRAMES} frames")


def test_call_to_call_state(cuda, monkeypatch):
    """two calls with different inputs of different lengths on one handle (the first leaves the
    fast loop at the other rotation phase than the second): the second call's output is a fresh
    handle's, and both are the split path's"""
    na, nb = N + HOP * 9 + 77, N + HOP * 4 + 1
    xa, xb = _rows(na, 500), _rows(nb, 700)
    ps, pr = _vocoder(monkeypatch, "0"), _vocoder(monkeypatch, "1")
    _check(ps, pr, xa, na, "first call")
    second = _check(ps, pr, xb, nb, "second call")
    fresh, kf = _run(_vocoder(monkeypatch, "1"), xb, nb)
    assert kf == {"resident"}, kf
    _same(second, fresh, "second call against a fresh handle")
