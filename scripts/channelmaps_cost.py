#!/usr/bin/env python3
"""Cost of the maps set per channel on the config-3 batch (developer tool).

1024 channels x 10 s, N = 1024, hop 256, scale 1, packed rows, no spectrum output, on one GPU:
pv_pitchmap_process, per-kernel pv_profile event times, 3 warm-up + 10 timed steps per entry, the
entries alternating three times in one process —
  parent_shared     the library given with --parent-lib (the parent commit's build) with one glide
                    map, ratio 1 -> 1.5 geometrically over the identity tempo (left out without it)
  shared            this tree's library with the same shared map: what the stride costs the shared path
  per_channel_same  this tree's library with that map installed per channel for every channel
  per_channel       this tree's library with a different map in every channel: a vibrato of +-6 %
                    with a phase per channel, every fourth channel at ratio 1 throughout (a copy)
Both libraries are driven through the same few ctypes calls, not through pvamd, whose wrapper
loads one library per process.

  python3 scripts/channelmaps_cost.py profiles/channelmaps_c3.json [--parent-lib path/to/libpv.so]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "phase-vocoder_amd"))

vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int


class Lib:
    """the calls the measurement needs, of any build of libpv at ABI 5"""

    def __init__(self, path, _lib):
        self.L = L = ctypes.CDLL(os.path.abspath(path))
        self._lib = _lib
        L.pv_last_error.restype = ctypes.c_char_p
        L.pv_sources_sha.restype = ctypes.c_char_p
        L.pv_create.argtypes = [ctypes.POINTER(_lib.pv_config), ctypes.POINTER(vp)]
        L.pv_destroy.argtypes = [vp]
        L.pv_reserve_spectrum.argtypes = [vp]
        L.pv_pitchmap_set.argtypes = [vp, vp, vp, ci, ci]
        if hasattr(L, "pv_pitchmap_set_channels"):
            L.pv_pitchmap_set_channels.argtypes = [vp, vp, ll, vp, ll, ci, ci, ci]
        L.pv_pitchmap_output_length.argtypes = [vp]
        L.pv_pitchmap_output_length.restype = ll
        L.pv_timemap_frames.argtypes = [vp]
        L.pv_pitchmap_process.argtypes = [vp, vp, ll, ll, ci, ci, vp, ll, vp, ll, vp]
        L.pv_profile_enable.argtypes = [vp, ci]
        L.pv_profile_reset.argtypes = [vp]
        L.pv_profile_reset.restype = None
        L.pv_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ci), ci]
        self.sha = L.pv_sources_sha().decode()

    def ok(self, st, what):
        if st != 0:
            raise RuntimeError(f"{what}: status {st}: {self.L.pv_last_error().decode()}")

    def handle(self, N, hop_div, C, max_frames):
        _lib = self._lib
        cfg = _lib.config(N, hop_div, ord("t"), 1.0, _lib.PV_MODE_STANDARD, C, max_frames,
                          spec_layout=_lib.PV_SPEC_PACKED)
        h = vp()
        self.ok(self.L.pv_create(ctypes.byref(cfg), ctypes.byref(h)), "pv_create")
        self.ok(self.L.pv_reserve_spectrum(h), "pv_reserve_spectrum")
        return h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--parent-lib", default=None, help="libpv.so built from the parent commit")
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    a = ap.parse_args()
    os.environ["PV_FUSED"] = "0"
    import numpy as np
    import torch
    from pvamd import _lib, pitch_map_plan

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
    glide = 1.5 ** (np.arange(frames) / (frames - 1.0))
    # a vibrato of +-6 % with a period of 23 frames and a phase per channel; every fourth channel in tune
    phase = rng.uniform(0, 2 * np.pi, C)
    vib = 1.0 + 0.06 * np.sin(2 * np.pi * np.arange(frames)[None, :] / 23.0 + phase[:, None])
    vib[::4] = 1.0
    pos_all = np.ascontiguousarray(np.broadcast_to(pos, (C, frames)))
    glide_all = np.ascontiguousarray(np.broadcast_to(glide, (C, frames)))
    n_s_glide = len(pitch_map_plan(N, hop, pos, glide)[0])
    n_s_vib = [len(pitch_map_plan(N, hop, pos, vib[c])[0]) for c in range(C)]
    max_frames = max(n_s_glide, max(n_s_vib)) + 1
    out = torch.empty((C, frames * hop + N - hop), dtype=torch.float32, device="cuda")

    def dp(arr):
        return arr.ctypes.data_as(vp)

    def entry(lib, h):
        L = lib.L
        assert L.pv_pitchmap_output_length(h) == out.shape[1]
        s = vp(torch.cuda.current_stream().cuda_stream)

        def step():
            lib.ok(L.pv_pitchmap_process(h, x.data_ptr(), x.stride(0), n, C, frames, None, 0, out.data_ptr(),
                                         out.stride(0), s), "pv_pitchmap_process")
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        lib.ok(L.pv_profile_enable(h, 1), "pv_profile_enable")
        L.pv_profile_reset(h)
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        cap = 32
        names, ms, cnt = (ctypes.c_char_p * cap)(), (ctypes.c_double * cap)(), (ci * cap)()
        m = L.pv_profile_read(h, names, ms, cnt, cap)
        lib.ok(L.pv_profile_enable(h, 0), "pv_profile_enable")
        res = {names[i].decode(): round(ms[i] / cnt[i], 4) for i in range(m)}
        res["total"] = round(sum(res.values()), 4)
        return res

    tree = Lib(_lib.LIB_PATH, _lib)
    th = tree.handle(N, hop_div, C, max_frames)

    def shared(lib, h):
        lib.ok(lib.L.pv_pitchmap_set(h, dp(pos), dp(glide), frames, 0), "pv_pitchmap_set")
        return entry(lib, h)

    def per_channel(ratio):
        tree.ok(tree.L.pv_pitchmap_set_channels(th, dp(pos_all), frames, dp(ratio), frames, C, frames, 0),
                "pv_pitchmap_set_channels")
        return entry(tree, th)

    plan = [("shared", lambda: shared(tree, th)), ("per_channel_same", lambda: per_channel(glide_all)),
            ("per_channel", lambda: per_channel(vib))]
    parent = None
    if a.parent_lib:
        parent = Lib(a.parent_lib, _lib)
        ph = parent.handle(N, hop_div, C, max_frames)
        plan.insert(0, ("parent_shared", lambda: shared(parent, ph)))
    res = {name: [] for name, _ in plan}
    for _ in range(3):
        for name, run in plan:
            res[name].append(run())
            print(name, res[name][-1], flush=True)
    doc = {"what": "config-3 batch at scale 1 (%d channels x %g s, N = 1024, hop 256, packed rows, no spectrum output) "
                   "on one GPU, pv_pitchmap_process: average ms per launch of every kernel and their sum, pv_profile "
                   "events" % (C, a.seconds),
           "method": "one process (PV_FUSED=0); per entry 3 warm-up + 10 timed steps; the entries alternate three times",
           "entries": {"parent_shared": "the parent commit's library, one glide map 1 -> 1.5 for all channels",
                       "shared": "this tree, the same shared map",
                       "per_channel_same": "this tree, that map installed per channel",
                       "per_channel": "this tree, a vibrato of +-6 % with a phase per channel, every fourth channel "
                                      "at ratio 1 throughout"},
           "device": torch.cuda.get_device_name(0), "frames_per_channel": frames,
           "stretch_frames": {"glide": n_s_glide, "per_channel_min": int(min(n_s_vib)), "per_channel_max": int(max(n_s_vib))},
           "output_samples_per_channel": int(out.shape[1]),
           "sources_sha": {"tree": tree.sha, "parent": parent.sha if parent else None}, "avg_ms": res}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
