#!/usr/bin/env python3
"""Cost of the pitch map on the config-3 geometry (developer tool).

1024 channels x 10 s, N = 1024, hop 256, packed rows, no spectrum output, on one GPU: per-kernel
pv_profile event times, 3 warm-up + 10 timed steps per entry, the entries alternating three times
in one process —
  pitchmap / pitchmap_locked   pv_pitchmap_process: identity tempo, the ratio gliding 1 -> 1.5
                               geometrically, quality 0 (analysis, map_sum, map_carry,
                               synthesis_map, seam, var_resample)
  pitch_3_2                    pv_pitch_process on a second handle at scale 1.5, quality 0: its
                               `resample` launch (k_resample at 3:2, a kernel this change does not
                               touch: scripts/asm_diff.py) writes the same number of output samples

  python3 scripts/pitchmap_cost.py profiles/pitchmap_c3.json [--channels 1024]
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
    os.environ["PV_FUSED"] = "0"
    import numpy as np
    import torch
    from pvamd import STANDARD, TIME_SHIFT, PhaseVocoder, _lib, pitch_map_plan

    N, hop_div, C = 1024, 4, a.channels
    hop = N // hop_div
    n = int(a.seconds * 44100)
    rng = np.random.default_rng(3)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / 44100.0
    x = torch.zeros((C, n), device="cuda")
    for _ in range(3):
        f = torch.from_numpy(rng.uniform(55, 4000, C).astype(np.float32)).cuda()[:, None]
        p = torch.from_numpy(rng.uniform(0, 6.28, C).astype(np.float32)).cuda()[:, None]
        x += 0.1 * torch.sin(6.2831853 * f * t[None, :] + p)
    frames = _lib.frame_count(n, hop)
    pos = np.arange(frames, dtype=np.float64)
    ratio = 1.5 ** (np.arange(frames) / (frames - 1.0))
    pos_s, steps = pitch_map_plan(N, hop, pos, ratio)
    pm = PhaseVocoder(N, TIME_SHIFT, 1.0, hop_div, mode=STANDARD, max_channels=C, max_frames=len(pos_s) + 1,
                      spec_layout=_lib.PV_SPEC_PACKED)
    pm.set_pitch_map(pos, ratio, 0)
    pm.reserve_spectrum()
    pm_out = torch.empty((C, pm.pitch_map_output_length), dtype=torch.float32, device="cuda")
    pr = PhaseVocoder(N, TIME_SHIFT, 1.5, hop_div, mode=STANDARD, max_channels=C, max_frames=frames,
                      spec_layout=_lib.PV_SPEC_PACKED)
    pr.reserve_pitch(0)
    pr.reserve_spectrum()
    pr_out = torch.empty((C, pr.pitch_output_length(frames)), dtype=torch.float32, device="cuda")

    def entry(pv, step):
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

    def pitchmap(lock):
        pm.set_phase_lock(lock)
        return entry(pm, lambda: pm.pitch_map_process(x, out=pm_out, spectrum=False))

    plan = [("pitchmap", lambda: pitchmap(False)), ("pitchmap_locked", lambda: pitchmap(True)),
            ("pitch_3_2", lambda: entry(pr, lambda: pr.pitch_process(x, out=pr_out, spectrum=False)))]
    res = {name: [] for name, _ in plan}
    for _ in range(3):
        for name, run in plan:
            res[name].append(run())
            print(name, res[name][-1], flush=True)
    doc = {"what": "config-3 geometry (%d channels x %g s, N = 1024, hop 256, packed rows, no spectrum output) on one "
                   "GPU: average ms per launch of every kernel, pv_profile events" % (C, a.seconds),
           "method": "one process (PV_FUSED=0); per entry 3 warm-up + 10 timed steps; the entries alternate three times",
           "device": torch.cuda.get_device_name(0), "frames_per_channel": frames, "stretch_frames": int(len(pos_s)),
           "output_samples_per_channel": {"pitchmap": int(pm_out.shape[1]), "pitch_3_2": int(pr_out.shape[1])},
           "sources_sha": _lib.sources_sha(), "avg_ms": res}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
