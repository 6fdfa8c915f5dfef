"""What the GPU test modules share (a helper: no tests in here).  torch is imported inside the
functions, so importing this module, as collecting the tests does, needs neither torch nor a
GPU.  pytest does not rewrite the asserts of a helper module, so each carries its own message.
"""
import functools
import socket
import struct

import numpy as np

import pvref
from pvamd import STANDARD, PhaseVocoder, _lib
from pvamd._lib import PVError
from pvamd.dist import assemble_segments, frame_segments
from signals import rms, synth, zoo_rows

RMS_TOL = 1e-5  # BASELINE.json north_star: <= 1e-5 RMS per sample vs the CPU reference
SENTINEL = -77.25  # fills the padding of the resamplers' output rows
ZOO_SAMPLES = 12001  # the zoo's length in test_gpu_signals and test_gpu_resident: the last frame is ragged

# stretch_inputs' (seed0, seed_step, frames) of the modules that share cached references: the
# references are keyed on the input, so two modules share them by drawing the same input
LOCK_INPUTS = dict(seed0=9100, seed_step=7, frames=76)   # test_gpu_phase_lock, test_gpu_resample
MAP_INPUTS = dict(seed0=8100, seed_step=11, frames=60)   # test_gpu_timemap, test_gpu_varresample


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_dev_copy(a):
    """a device copy of a read-only host array (the shared inputs are read-only)"""
    return to_dev(np.array(a))


def wide(xs):
    """device rows with a stride larger than the signals"""
    import torch
    buf = torch.full((xs.shape[0], xs.shape[1] + 40), 7.0, device="cuda")
    buf[:, :xs.shape[1]] = to_dev(np.array(xs, np.float32))
    return buf[:, :xs.shape[1]]


def padded_input(xs, pad):
    """rows of xs in a [C, n + pad] tensor whose padding is NaN"""
    import torch
    buf = torch.full((xs.shape[0], xs.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :xs.shape[1]] = to_dev_copy(xs)
    return buf


def run_padded(rs, xs, pad, n_out=None):
    """resample the rows of xs from NaN-padded rows into sentinel-padded rows; returns the output
    rows after checking that the sentinel survived.  n_out=None: a Resampler, whose output length
    follows from the input's; otherwise a VarResampler, which is told n_out"""
    import torch
    n = xs.shape[1]
    buf = padded_input(xs, pad)
    kw = {} if n_out is None else {"n_out": n_out}
    if n_out is None:
        n_out = rs.length(n)
    ybuf = torch.full((xs.shape[0], n_out + 5), SENTINEL, dtype=torch.float32, device="cuda")
    rs(buf[:, :n], out=ybuf[:, :n_out], **kw)
    tail = ybuf[:, n_out:]
    assert (tail == SENTINEL).all(), f"written past the {n_out} outputs of a row: {tail.cpu().numpy()!r}"
    return ybuf[:, :n_out].cpu().numpy()


def status_of(fn):
    """the status fn() is refused with (the error carries a message), PV_OK if it is not"""
    try:
        fn()
    except PVError as e:
        assert len(str(e)) > 0, f"a PVError of status {e.status} without a message"
        return e.status
    return _lib.PV_OK


def pv_frames(n, hop=256):
    return max(1, -(-(n - hop) // hop))


def free_port():
    """a TCP port for a process group's rendezvous on this host"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def write_pcm16(path, x):
    """x = int16/32768 values (exact): write them back bit-exactly as mono 16-bit PCM."""
    ints = np.round(np.asarray(x, np.float64) * 32768.0).astype("<i2")
    body = ints.tobytes()
    hdr = b"RIFF" + struct.pack("<i", 36 + len(body)) + b"WAVE"
    hdr += b"fmt " + struct.pack("<ihhiihh", 16, 1, 1, 44100, 88200, 2, 16)
    hdr += b"data" + struct.pack("<i", len(body))
    open(path, "wb").write(hdr + body)


def oracle_stream(x, N, hop_div, effect, scale, K):
    """(the stream's first K hops prefixed with N - hop zeros, the oracle's K frames of it): what
    a real-time handle computes"""
    hop = N // hop_div
    xp = np.concatenate([np.zeros(N - hop, np.float32), x[:K * hop]])
    return xp, pvref.std_process(xp, N, hop_div, ord(effect), scale, frames=K)


def run_segments(pv, x, nseg):
    """the stream x as nseg consecutive frame segments (pv_segment_*), assembled"""
    import torch
    xd = to_dev(x) if not isinstance(x, torch.Tensor) else x
    xd = xd.unsqueeze(0) if xd.dim() == 1 else xd
    n = xd.shape[1]
    total = pv.num_frames(n)
    hop = pv.hopSize
    sums, blocks, firsts = [], [], []
    for f0, nf in frame_segments(total, nseg):
        if nf == 0:
            continue
        spec = pv.analysis(xd[:, f0 * hop:], frames=nf, n_samples=n - f0 * hop)
        before = torch.stack(sums).contiguous() if sums else None
        blocks.append(pv.segment_resynthesis(spec, f0, before, frames=nf))
        sums.append(pv.segment_summary(spec, nf))
        firsts.append(f0)
    return assemble_segments(blocks, firsts, pv.outHopSize, pv.output_length(total))


@functools.lru_cache(maxsize=None)
def zoo_input(n, N):
    """signals.zoo_rows(n, N), shared read-only"""
    xs = zoo_rows(n, N)
    xs.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def zoo_reference(N, hop_div, effect, scale):
    """(oracle fp64 outputs per channel, port outputs [C, len], out hop) of zoo_input(ZOO_SAMPLES,
    N): computed once per geometry and shared, read-only"""
    xs = zoo_input(ZOO_SAMPLES, N)
    refs = [pvref.std_process(x, N, hop_div, ord(effect), scale) for x in xs]
    port, _ = pvref.port_std_process_batch(xs, N, hop_div, ord(effect), scale)
    for a in refs + [port]:
        a.setflags(write=False)
    return refs, port, pvref.out_hop(N, hop_div, ord(effect), scale)


def stretch_inputs(N, hop_div, seed0, seed_step, frames, channels=3):
    """[channels, frames * hop + 13] tones: `frames` frames, not a multiple of the hop"""
    hop = N // hop_div
    n = frames * hop + 13
    got = pvref.num_frames(n, hop)
    assert got == frames, f"{n} samples at hop {hop} are {got} frames, not {frames}"
    return np.stack([synth(n, seed0 + seed_step * c + N) for c in range(channels)])


def make_vocoder(monkeypatch, N, hop_div, effect, scale, F=8, *, max_frames, channels=3, **kw):
    """a STANDARD handle whose runs are F frames long (PV_RUN_FRAMES)"""
    monkeypatch.setenv("PV_RUN_FRAMES", str(F))
    pv = PhaseVocoder(N, effect, scale, hop_div, mode=STANDARD, max_channels=channels, max_frames=max_frames, **kw)
    assert pv.frames_per_run == F, f"runs of {pv.frames_per_run} frames with PV_RUN_FRAMES={F}"
    return pv


def channel_errors(out, reference, channels):
    """rms of every channel of the device tensor `out` (finite) against reference(c) (of the
    same shape): the loop the modules' check_against_reference share"""
    g = out.cpu().numpy()
    assert np.isfinite(g).all(), f"{np.sum(~np.isfinite(g))} non-finite output samples"
    errs = []
    for c in range(channels):
        ref = reference(c)
        assert g[c].shape == ref.shape, f"channel {c}: output {g[c].shape}, reference {ref.shape}"
        errs.append(rms(g[c], ref))
    return errs
