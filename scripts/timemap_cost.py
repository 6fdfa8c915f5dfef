#!/usr/bin/env python3
"""Cost of the time-map stretch on the config-3 geometry (developer tool).

1024 channels x 10 s, N = 1024, hop 256, scale 1, packed rows, no spectrum output, on one GPU:
per-kernel pv_profile event times, 3 warm-up + 10 timed steps per entry, the entries alternating
three times in one process.  One handle, created with PV_FUSED=0 so that its pv_process runs the
split path —
  split / split_locked     pv_process: the parent commit's kernels (scripts/asm_diff.py), the
                           baseline the second row per frame and map_sum are read against
  map_R / map_R_locked     pv_timemap_process with pvamd.rate_map(frames, R), R = 1.0, 0.73, 1.37
                           (R = 0.73 synthesises 1 / 0.73 times the frames of the baseline)

  python3 scripts/timemap_cost.py profiles/timemap_c3.json [--channels 1024]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "phase-vocoder_amd"))

RATES = (1.0, 0.73, 1.37)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    a = ap.parse_args()
    os.environ["PV_FUSED"] = "0"
    import numpy as np
    import torch
    from pvamd import STANDARD, TIME_SHIFT, PhaseVocoder, _lib, rate_map

    N, hop_div, C = 1024, 4, a.channels
    n = int(a.seconds * 44100)
    rng = np.random.default_rng(3)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / 44100.0
    x = torch.zeros((C, n), device="cuda")
    for _ in range(3):
        f = torch.from_numpy(rng.uniform(55, 4000, C).astype(np.float32)).cuda()[:, None]
        p = torch.from_numpy(rng.uniform(0, 6.28, C).astype(np.float32)).cuda()[:, None]
        x += 0.1 * torch.sin(6.2831853 * f * t[None, :] + p)
    frames = _lib.frame_count(n, N // hop_div)
    maps = {r: rate_map(frames, r) for r in RATES}
    max_frames = max(frames, max(len(m) for m in maps.values()))
    pv = PhaseVocoder(N, TIME_SHIFT, 1.0, hop_div, mode=STANDARD, max_channels=C, max_frames=max_frames,
                      spec_layout=_lib.PV_SPEC_PACKED)
    assert not pv.single_launch
    F = pv.frames_per_run
    out = pv.alloc_out(C, max_frames)
    pv.reserve_spectrum()

    def entry(lock, rate):
        pv.set_phase_lock(lock)
        if rate is None:
            step = lambda: pv.process(x, out=out, spectrum=False)  # noqa: E731
        else:
            pv.set_time_map(maps[rate])
            step = lambda: pv.time_map_process(x, out=out, spectrum=False)  # noqa: E731
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
        return {names[i].decode(): round(ms[i] / cnt[i], 4) for i in range(m)}

    plan = [("split", False, None), ("split_locked", True, None)]
    for r in RATES:
        plan += [(f"map_{r}", False, r), (f"map_{r}_locked", True, r)]
    res = {name: [] for name, *_ in plan}
    for _ in range(3):
        for name, lock, rate in plan:
            res[name].append(entry(lock, rate))
            print(name, res[name][-1], flush=True)
    doc = {"what": "config-3 geometry (%d channels x %g s, N = 1024, hop 256, scale 1, packed rows, no spectrum output) "
                   "on one GPU: average ms per launch of every kernel, pv_profile events" % (C, a.seconds),
           "method": "one process, one handle (PV_FUSED=0); per entry 3 warm-up + 10 timed steps; the entries "
                     "alternate three times",
           "device": torch.cuda.get_device_name(0), "frames_per_channel": frames, "frames_per_run": F,
           "output_frames": {str(r): int(len(m)) for r, m in maps.items()}, "sources_sha": _lib.sources_sha(),
           "avg_ms": res}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
