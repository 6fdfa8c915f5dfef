#!/usr/bin/env python3
"""Cost of the pitch tracker on the config-3 batch (developer tool).

1024 channels x 10 s, N = 1024, hop 256, packed rows, on one GPU: the spectrum is analysed once,
then each kernel runs alone on the same rows under pv_profile events, 3 warm-up + 10 timed steps
per entry, the entries alternating three times in one process —
  pitch      pv_pitch_track, lags 8 .. N/4 (k_pitch)
  pitch_all  pv_pitch_track, lags 2 .. N/2 - 1
  onset      pv_onset_strength (k_onset: reads the same rows, no transform)
  envelope   pv_spectral_envelope at order N/16 (k_envelope: two transforms per frame, writes a row)

  python3 scripts/pitchtrack_cost.py profiles/pitchtrack_c3.json [--channels 1024]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "phase-vocoder_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pvamd import STANDARD, TIME_SHIFT, PhaseVocoder, _lib

    N, hop_div, C = 1024, 4, a.channels
    L = N // 2
    n = int(a.seconds * 44100)
    rng = np.random.default_rng(3)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / 44100.0
    x = torch.zeros((C, n), device="cuda")
    for _ in range(3):
        f = torch.from_numpy(rng.uniform(55, 4000, C).astype(np.float32)).cuda()[:, None]
        p = torch.from_numpy(rng.uniform(0, 6.28, C).astype(np.float32)).cuda()[:, None]
        x += 0.1 * torch.sin(6.2831853 * f * t[None, :] + p)
    frames = _lib.frame_count(n, N // hop_div)
    pv = PhaseVocoder(N, TIME_SHIFT, 0.5, hop_div, mode=STANDARD, max_channels=C, max_frames=frames,
                      spec_layout=_lib.PV_SPEC_PACKED)
    spec = pv.analysis(x)
    del x
    dst = torch.zeros((C, frames, 2), dtype=torch.float32, device="cuda")
    env = torch.zeros((C, frames, L + 8), dtype=torch.float32, device="cuda")
    s, ld = pv._stream(), spec.stride(0) // 2

    def check(st):
        _lib.check(st, "pitchtrack_cost")

    steps = {
        "pitch": lambda: check(pv._L.pv_pitch_track(pv._h, spec.data_ptr(), ld, C, frames, 8, N // 4, 0.0,
                                                    dst.data_ptr(), dst.stride(0) // 2, s)),
        "pitch_all": lambda: check(pv._L.pv_pitch_track(pv._h, spec.data_ptr(), ld, C, frames, 2, N // 2 - 1, 0.0,
                                                        dst.data_ptr(), dst.stride(0) // 2, s)),
        "onset": lambda: check(pv._L.pv_onset_strength(pv._h, spec.data_ptr(), ld, C, frames, dst.data_ptr(),
                                                       dst.stride(0) // 2, s)),
        "envelope": lambda: check(pv._L.pv_spectral_envelope(pv._h, spec.data_ptr(), ld, C, frames, N // 16,
                                                             env.data_ptr(), env.stride(0), s)),
    }
    kernel = {"pitch": "pitch", "pitch_all": "pitch", "onset": "onset", "envelope": "envelope"}

    def entry(name):
        step = steps[name]
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        pv.profile(True)
        pv.profile_reset()
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        cap = 32
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_double * cap)()
        cnt = (ctypes.c_int * cap)()
        m = pv._L.pv_profile_read(pv._h, names, ms, cnt, cap)
        pv.profile(False)
        got = {names[i].decode(): (ms[i], cnt[i]) for i in range(m)}
        assert got[kernel[name]][1] == 10, got
        return round(got[kernel[name]][0] / 10, 4)

    res = {name: [] for name in steps}
    for _ in range(3):
        for name in steps:
            res[name].append(entry(name))
            print(name, res[name][-1], flush=True)
    voiced = float((dst[..., 0] > 0).float().mean())
    # what k_pitch moves: the row's N/2 + 1 {mag, phase} pairs (packed: N/2 slots) and one float2
    pitch_bytes = C * frames * (8 * (L + 1) + 8)
    doc = {"what": "config-3 batch (%d channels x %g s, N = 1024, hop 256, packed rows) on one GPU: ms per launch of "
                   "pv_pitch_track, pv_onset_strength and pv_spectral_envelope on the same analysed rows, pv_profile "
                   "events" % (C, a.seconds),
           "method": "one process; per entry 3 warm-up + 10 timed launches; the entries alternate three times",
           "device": torch.cuda.get_device_name(0), "frames_per_channel": frames, "frames_per_run": pv.frames_per_run,
           "sources_sha": _lib.sources_sha(), "pitch_bytes_per_launch": pitch_bytes,
           "pitch_frac_of_8TBps": [round(pitch_bytes / (v * 1e-3) / 8e12, 4) for v in res["pitch"]],
           "frames_with_a_pick": round(voiced, 4), "ms": res}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
