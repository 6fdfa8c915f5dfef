#!/usr/bin/env python3
"""Cost of the envelope warp (pv_pitch_set_formant) on the stretch that feeds
the stretch-and-resample pitch shift, at config 3's geometry: N = 1024, hop 256, 1024 channels x
10 s, no spectrum output, time stretch 0.5 and 1.5, phase locking on, order 64.

Variants, each with its own handle, in one process:

  parent   the locked stretch of another build of the library (--parent-lib, e.g.
           scripts/variant_from_rev.sh HEAD~ parent), when given
  off      the locked stretch of this build, the feature off
  on       pv_pitch_set_formant(order): k_envelope + k_synthesis in the warp mode in place of
           k_synthesis in the locked mode

A round is `--warmup` untimed and `--steps` timed pv_process calls of one variant with the
per-launch profile on (pv_profile_enable: device events around every launch); the variants take
turns, `--rounds` rounds each.  Reported per kernel and round: mean ms per launch; then the range
over the rounds, the bytes a frame moves (spectrum row, envelope row, output samples), the
fraction of 8 TB/s that is, the ratio (envelope + warp) / locked and warp / locked, and whether
the feature-off times sit inside the parent's spread.  Prints one JSON document; --out writes it
to a file too.

usage: python scripts/pitch_formant_cost.py [--parent-lib PATH] [--channels 1024] [--seconds 10]
                                            [--steps 10] [--warmup 3] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "phase-vocoder_amd"))
from pvamd import _lib  # noqa: E402

N, HOP_DIV, ORDER, SR = 1024, 4, 64, 44100
HBM_BYTES_PER_S = 8e12


def bind(path):
    """the entry points used here, of this build's library or of one that lacks the newer ones"""
    L = ctypes.CDLL(os.path.abspath(path))
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.pv_sources_sha.restype = ctypes.c_char_p
    L.pv_last_error.restype = ctypes.c_char_p
    L.pv_create.argtypes = [ctypes.POINTER(_lib.pv_config), ctypes.POINTER(vp)]
    L.pv_destroy.argtypes = [vp]
    L.pv_destroy.restype = None
    L.pv_output_length.argtypes = [vp, i]
    L.pv_output_length.restype = ll
    L.pv_set_phase_lock.argtypes = [vp, i]
    L.pv_reserve_spectrum.argtypes = [vp]
    L.pv_process.argtypes = [vp, vp, ll, ll, i, i, vp, ll, vp, ll, vp]
    L.pv_profile_enable.argtypes = [vp, i]
    L.pv_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_int), i]
    L.pv_profile_reset.argtypes = [vp]
    L.pv_profile_reset.restype = None
    if hasattr(L, "pv_pitch_set_formant"):
        L.pv_pitch_set_formant.argtypes = [vp, i]
    return L


def ok(L, status, what):
    if status != 0:
        raise RuntimeError(f"{what}: status {status}: {L.pv_last_error().decode()}")


class Variant:
    def __init__(self, name, L, scale, C, frames, order):
        self.name, self.L = name, L
        cfg = _lib.config(N, HOP_DIV, _lib.PV_TIME_SHIFT, scale, _lib.PV_MODE_STANDARD, C, frames, 0)
        self.h = ctypes.c_void_p()
        ok(L, L.pv_create(ctypes.byref(cfg), ctypes.byref(self.h)), "pv_create")
        ok(L, L.pv_set_phase_lock(self.h, 1), "pv_set_phase_lock")
        if order:
            ok(L, L.pv_pitch_set_formant(self.h, order), "pv_pitch_set_formant")
        ok(L, L.pv_reserve_spectrum(self.h), "pv_reserve_spectrum")
        self.olen = int(L.pv_output_length(self.h, frames))
        self.rounds = []

    def step(self, x, n, C, frames, out, stream):
        ok(self.L, self.L.pv_process(self.h, x.data_ptr(), x.stride(0), n, C, frames, None, 0, out.data_ptr(),
                                     out.stride(0), stream), "pv_process")

    def read(self):
        cap = 16
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_double * cap)()
        cnt = (ctypes.c_int * cap)()
        k = self.L.pv_profile_read(self.h, names, ms, cnt, cap)
        return {names[j].decode(): ms[j] / max(cnt[j], 1) for j in range(k)}

    def close(self):
        self.L.pv_destroy(self.h)


def measure(torch, libs, scale, C, n, args):
    hop = N // HOP_DIV
    frames = _lib.frame_count(n, hop)
    gen = torch.Generator(device="cuda").manual_seed(11)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / SR
    x = torch.zeros((C, n), device="cuda")
    for _ in range(3):  # the bench's generator: 3 sines f ~ U[55, 4000] Hz, a = 0.1, noise 1e-3
        f = torch.empty((C, 1), device="cuda").uniform_(55.0, 4000.0, generator=gen)
        p = torch.empty((C, 1), device="cuda").uniform_(0.0, 6.2831853, generator=gen)
        x += 0.1 * torch.sin(6.2831853 * f * t + p)
    x += torch.empty((C, n), device="cuda").uniform_(-1e-3, 1e-3, generator=gen)
    variants = []
    if "parent" in libs:
        variants.append(Variant("parent", libs["parent"], scale, C, frames, 0))
    variants += [Variant("off", libs["this"], scale, C, frames, 0), Variant("on", libs["this"], scale, C, frames, ORDER)]
    out = torch.empty((C, variants[0].olen), device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(args.rounds):
        for v in variants:
            for _ in range(args.warmup):
                v.step(x, n, C, frames, out, stream)
            torch.cuda.synchronize()
            ok(v.L, v.L.pv_profile_enable(v.h, 1), "pv_profile_enable")
            v.L.pv_profile_reset(v.h)
            for _ in range(args.steps):
                v.step(x, n, C, frames, out, stream)
            torch.cuda.synchronize()
            v.rounds.append(v.read())
            ok(v.L, v.L.pv_profile_enable(v.h, 0), "pv_profile_enable")
            assert bool(torch.isfinite(out[:, ::257]).all())
    hs = (variants[0].olen - N) // (frames - 1)  # out hop: olen = (frames - 1) hs + N
    spec_row, env_row, out_row = 8 * (N // 2 + 8), 4 * (N // 2 + 16), 4 * hs
    bytes_per_frame = {"envelope": spec_row + env_row, "synthesis_warp": spec_row + env_row + out_row,
                       "synthesis_locked": spec_row + out_row}
    res = {"frames_per_channel": frames, "out_hop": hs, "bytes_per_frame": bytes_per_frame, "variants": {}}
    for v in variants:
        kern = {}
        for k in sorted(set().union(*[r.keys() for r in v.rounds])):
            ms = [round(r[k], 4) for r in v.rounds if k in r]
            e = {"ms_per_launch": ms, "min_ms": min(ms), "max_ms": max(ms)}
            if k in bytes_per_frame:
                total = bytes_per_frame[k] * frames * C
                e["fraction_of_8TBps"] = [round(total / (m * 1e-3) / HBM_BYTES_PER_S, 3) for m in (max(ms), min(ms))]
            kern[k] = e
        res["variants"][v.name] = kern
        v.close()
    on, off = res["variants"]["on"], res["variants"]["off"]
    lk = off["synthesis_locked"]
    res["warp_over_locked"] = [round(on["synthesis_warp"]["min_ms"] / lk["max_ms"], 3),
                               round(on["synthesis_warp"]["max_ms"] / lk["min_ms"], 3)]
    res["envelope_plus_warp_over_locked"] = [
        round((on["synthesis_warp"]["min_ms"] + on["envelope"]["min_ms"]) / lk["max_ms"], 3),
        round((on["synthesis_warp"]["max_ms"] + on["envelope"]["max_ms"]) / lk["min_ms"], 3)]
    if "parent" in res["variants"]:
        pl = res["variants"]["parent"]["synthesis_locked"]
        res["off_inside_parent_spread"] = bool(lk["min_ms"] <= pl["max_ms"] and pl["min_ms"] <= lk["max_ms"])
    del x, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    _lib.lib()  # refuses a stale build
    libs = {"this": bind(_lib.LIB_PATH)}
    if args.parent_lib:
        libs["parent"] = bind(args.parent_lib)
    n = int(round(args.seconds * SR))
    doc = {"what": f"locked time stretch with and without the envelope warp (order {ORDER}): N = {N}, hop "
                   f"{N // HOP_DIV}, {args.channels} channels x {args.seconds} s, pv_process(spec = NULL), natural rows",
           "method": f"one process, per-launch device events (pv_profile_enable); {args.rounds} rounds per variant, "
                     f"the variants taking turns; a round is {args.warmup} warm-up and {args.steps} timed steps; "
                     "ms per launch is the round's mean; ranges are over the rounds",
           "device": torch.cuda.get_device_name(0),
           "sources_sha": {k: L.pv_sources_sha().decode() for k, L in libs.items()}}
    for scale in (0.5, 1.5):
        doc[f"scale_{scale}"] = measure(torch, libs, scale, args.channels, n, args)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
