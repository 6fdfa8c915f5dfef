#!/usr/bin/env python3
"""Cost of the transient phase reset on the config-3 batch (developer tool).

1024 channels x 10 s, N = 1024, hop 256, time stretch 0.5, packed rows, pv_process without a
spectrum output, on one GPU: per-kernel pv_profile event times, 3 warm-up + 10 timed steps per
entry, the entries alternating three times in one process —
  off            the feature off (k_synthesis; the parent commit's code, scripts/asm_diff.py)
  locked         phase locking alone (synthesis_locked)
  flags_0/1/8    the caller's flags with 0, 1 and 8 flagged runs per channel
  locked_flags_8 the same with phase locking
  detect         the detector at the default threshold on the benchmark's tones (few onsets)

  python3 scripts/transient_cost.py profiles/transient_c3.json [--channels 1024]
"""
import argparse
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

    N, hop_div, scale, C = 1024, 4, 0.5, a.channels
    n = int(a.seconds * 44100)
    rng = np.random.default_rng(3)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / 44100.0
    x = torch.zeros((C, n), device="cuda")
    for _ in range(3):
        f = torch.from_numpy(rng.uniform(55, 4000, C).astype(np.float32)).cuda()[:, None]
        p = torch.from_numpy(rng.uniform(0, 6.28, C).astype(np.float32)).cuda()[:, None]
        x += 0.1 * torch.sin(6.2831853 * f * t[None, :] + p)
    frames = _lib.frame_count(n, N // hop_div)
    pv = PhaseVocoder(N, TIME_SHIFT, scale, hop_div, mode=STANDARD, max_channels=C, max_frames=frames,
                      spec_layout=_lib.PV_SPEC_PACKED)
    F = pv.frames_per_run
    nruns = (frames + F - 1) // F
    out = pv.alloc_out(C, frames)
    pv.reserve_transients()

    def flags(k):
        fl = torch.zeros((C, frames), dtype=torch.uint8, device="cuda")
        for r in np.linspace(1, nruns - 2, k).astype(int) if k else []:
            fl[:, r * F + F // 2] = 1
        return fl

    def entry(lock, mode, k):
        pv.set_transients("off")
        pv.set_phase_lock(lock)
        pv.set_transients(mode)
        if mode == "flags":
            pv.set_transient_flags(flags(k))
        for _ in range(3):
            pv.process(x, out=out, spectrum=False)
        torch.cuda.synchronize()
        pv.profile(True)
        pv.profile_reset()
        for _ in range(10):
            pv.process(x, out=out, spectrum=False)
        torch.cuda.synchronize()
        cap = 16
        import ctypes
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_double * cap)()
        cnt = (ctypes.c_int * cap)()
        m = pv._L.pv_profile_read(pv._h, names, ms, cnt, cap)
        pv.profile(False)
        return {names[i].decode(): round(ms[i] / cnt[i], 4) for i in range(m)}

    plan = [("off", False, "off", 0), ("locked", True, "off", 0), ("flags_0", False, "flags", 0),
            ("flags_1", False, "flags", 1), ("flags_8", False, "flags", 8), ("locked_flags_8", True, "flags", 8),
            ("detect", False, "detect", 0)]
    res = {name: [] for name, *_ in plan}
    for _ in range(3):
        for name, lock, mode, k in plan:
            res[name].append(entry(lock, mode, k))
            print(name, res[name][-1], flush=True)
    onset_bytes = C * frames * 8 * (N // 2)  # packed rows: N/2 float2 per frame
    doc = {"what": "config-3 batch (%d channels x %g s, N = 1024, hop 256, time stretch 0.5, packed rows, pv_process "
                   "without a spectrum output) on one GPU: average ms per launch of every kernel, pv_profile events" % (C, a.seconds),
           "method": "one process; per entry 3 warm-up + 10 timed pv_process steps; the entries alternate three times",
           "device": torch.cuda.get_device_name(0), "frames_per_channel": frames, "frames_per_run": F,
           "runs_per_channel": nruns, "sources_sha": _lib.sources_sha(), "onset_bytes_per_step": onset_bytes,
           "onset_frac_of_8TBps": [round(onset_bytes / (e["onset"] * 1e-3) / 8e12, 4) for e in res["detect"]],
           "avg_ms": res}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
