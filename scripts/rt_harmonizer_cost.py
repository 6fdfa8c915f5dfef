#!/usr/bin/env python3
"""Cost of one real-time harmoniser callback (pv_rt_harmonizer_push) at BASELINE
config 5's geometry — 256 channels, N = 256, hop 64, one frame per callback, locked, ratios within
+-3 semitones ([0.84, 1.19], G = 1) — by scripts/rt_pitch_latency.py's method, for V = 1, 2, 4, 8:

  map            the single pitch-map callback (pv_rt_pitchmap_push; §3.16's figure)
  harm_V         one harmoniser handle with V voices: one callback
  handles_V      V pitch-map handles called back in sequence, each pushed the same input: what V
                 voices cost without the harmoniser (timed around the V callbacks together)

Voice v plays the interval SEMITONES[v]; the V handles play the same intervals.  One process; every
variant has its own pv_rt(s) and captured callback(s); after a warm-up the variants are timed in
turn, in an order that rotates from round to round (host wall clock around the synchronous
pv_rt_callback, pinned buffers filled in place outside the timed region).  Reports p50 / p99 per
repeat, their median over the repeats and the spread, for PV_RT_LAUNCH = graph and direct, and
per V whether the harmoniser is cheaper than the V handles by more than the handles' spread.
Prints one JSON document; --out writes it to a file too.

usage: python scripts/rt_harmonizer_cost.py [--callbacks 2000] [--repeats 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rt_pitchmap_latency as base  # noqa: E402
from rt_pitch_latency import C, DEADLINE_MS, HOP_DIV, N, _lib, ok  # noqa: E402

HOP = N // HOP_DIV
RANGE = (0.84, 1.19)  # +-3 semitones
SEMITONES = (0, 3, -3, 2, -2, 1, -1, 0)
VOICES = (1, 2, 4, 8)


def ratio_of(v):
    return np.float32(2.0 ** (SEMITONES[v] / 12.0))


def bind(path):
    L = base.bind(path)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fpp = ctypes.POINTER(ctypes.POINTER(ctypes.c_float))
    L.pv_rt_harmonizer_reserve.argtypes = [vp, i, i, i, f, f]
    L.pv_rt_harmonizer_latency.argtypes = [vp]
    L.pv_rt_harmonizer_host_controls.argtypes = [vp, fpp, fpp]
    return L


class MapHandle:
    """a scale-1 locked pv_rt with the pitch map at one constant ratio, captured"""

    def __init__(self, L, ratio):
        self.L = L
        cfg = _lib.config(N, HOP_DIV, _lib.PV_TIME_SHIFT, 1.0, _lib.PV_MODE_STANDARD, C, 1, 0)
        self.h = ctypes.c_void_p()
        ok(L, L.pv_rt_create(ctypes.byref(cfg), C, ctypes.byref(self.h)), "pv_rt_create")
        ok(L, L.pv_rt_set_phase_lock(self.h, 1), "pv_rt_set_phase_lock")
        ok(L, L.pv_rt_pitchmap_reserve(self.h, 0, 1, *RANGE), "pv_rt_pitchmap_reserve")
        ok(L, L.pv_rt_capture(self.h, 1), "pv_rt_capture")
        fi, fo, fr = (ctypes.POINTER(ctypes.c_float)() for _ in range(3))
        ok(L, L.pv_rt_host_buffers(self.h, ctypes.byref(fi), ctypes.byref(fo)), "pv_rt_host_buffers")
        ok(L, L.pv_rt_pitchmap_host_ratios(self.h, ctypes.byref(fr)), "pv_rt_pitchmap_host_ratios")
        self.host_in = np.ctypeslib.as_array(fi, shape=(C, HOP))
        self.host_out = np.ctypeslib.as_array(fo, shape=(C, HOP))
        np.ctypeslib.as_array(fr, shape=(C, 1))[:] = ratio

    def close(self):
        self.L.pv_rt_destroy(self.h)


class Handles:
    """V pitch-map handles called back in sequence"""

    def __init__(self, name, L, voices):
        self.name, self.L = name, L
        self.handles = [MapHandle(L, ratio_of(v)) for v in range(voices)]

    def fill(self, block):
        for m in self.handles:  # (the same input V times: V input copies)
            m.host_in[:] = block

    def callback(self):
        t0 = time.perf_counter_ns()
        for m in self.handles:
            st = self.L.pv_rt_callback(m.h, None, None)
            if st != 0:
                ok(self.L, st, "pv_rt_callback")
        t1 = time.perf_counter_ns()
        return (t1 - t0) * 1e-3  # us

    def outputs(self):
        return [m.host_out for m in self.handles]

    def close(self):
        for m in self.handles:
            m.close()


class Harmonizer:
    """one handle with V voices, captured"""

    def __init__(self, name, L, voices):
        self.name, self.L = name, L
        cfg = _lib.config(N, HOP_DIV, _lib.PV_TIME_SHIFT, 1.0, _lib.PV_MODE_STANDARD, C, 1, 0)
        self.h = ctypes.c_void_p()
        ok(L, L.pv_rt_create(ctypes.byref(cfg), C, ctypes.byref(self.h)), "pv_rt_create")
        ok(L, L.pv_rt_set_phase_lock(self.h, 1), "pv_rt_set_phase_lock")
        ok(L, L.pv_rt_harmonizer_reserve(self.h, voices, 0, 1, *RANGE), "pv_rt_harmonizer_reserve")
        self.latency = L.pv_rt_harmonizer_latency(self.h)
        ok(L, L.pv_rt_capture(self.h, 1), "pv_rt_capture")
        fi, fo, fr, fg = (ctypes.POINTER(ctypes.c_float)() for _ in range(4))
        ok(L, L.pv_rt_host_buffers(self.h, ctypes.byref(fi), ctypes.byref(fo)), "pv_rt_host_buffers")
        ok(L, L.pv_rt_harmonizer_host_controls(self.h, ctypes.byref(fr), ctypes.byref(fg)), "pv_rt_harmonizer_host_controls")
        self.host_in = np.ctypeslib.as_array(fi, shape=(C, HOP))
        self.host_out = np.ctypeslib.as_array(fo, shape=(C, HOP))
        np.ctypeslib.as_array(fr, shape=(C, voices, 1))[:] = np.array([ratio_of(v) for v in range(voices)])[None, :, None]

    def fill(self, block):
        self.host_in[:] = block

    def callback(self):
        t0 = time.perf_counter_ns()
        st = self.L.pv_rt_callback(self.h, None, None)
        t1 = time.perf_counter_ns()
        ok(self.L, st, "pv_rt_callback")
        return (t1 - t0) * 1e-3  # us

    def outputs(self):
        return [self.host_out]

    def close(self):
        self.L.pv_rt_destroy(self.h)


def measure(launch, L, callbacks, repeats, warmup):
    os.environ["PV_RT_LAUNCH"] = launch  # read by pv_rt_capture
    variants = [Handles("map", L, 1)]
    for V in VOICES:
        variants += [Harmonizer(f"harm_{V}", L, V), Handles(f"handles_{V}", L, V)]
    rng = np.random.default_rng(5)
    block = rng.uniform(-0.5, 0.5, (64, C, HOP)).astype(np.float32)
    for k in range(warmup):
        for v in variants:
            v.fill(block[k % 64])
            v.callback()
    res = {v.name: {"p50_us": [], "p99_us": []} for v in variants}
    for _ in range(repeats):
        t = {v.name: np.empty(callbacks) for v in variants}
        for k in range(callbacks):
            for j in range(len(variants)):  # the order rotates: no variant always follows the same one
                v = variants[(j + k) % len(variants)]
                v.fill(block[k % 64])
                t[v.name][k] = v.callback()
        for name, a in t.items():
            res[name]["p50_us"].append(round(float(np.percentile(a, 50)), 2))
            res[name]["p99_us"].append(round(float(np.percentile(a, 99)), 2))
    for v in variants:
        for o in v.outputs():
            assert np.isfinite(o).all() and o.any(), v.name
        v.close()
    for r in res.values():
        for k in ("p50_us", "p99_us"):
            r[k.replace("_us", "_median_us")] = round(float(np.median(r[k])), 2)
            r[k.replace("_us", "_spread_us")] = round(float(np.max(r[k]) - np.min(r[k])), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--callbacks", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--out")
    args = ap.parse_args()
    _lib.lib()  # refuses a stale build
    L = bind(_lib.LIB_PATH)
    doc = {"what": f"pv_rt_callback cost of V live voices, {C} channels, N = {N}, hop {HOP}, one frame per callback, "
                   f"locked, fast preset, ratios 2^(s/12) for s in {list(SEMITONES)} within {list(RANGE)}: harm_V one "
                   "harmoniser callback, handles_V V pitch-map callbacks in sequence, map the single pitch-map "
                   "callback; host wall clock around the synchronous call(s)",
           "method": f"one process, {args.warmup} warm-up rounds, then {args.repeats} repeats of {args.callbacks} "
                     "rounds; a round times every variant once, in an order that rotates from round to round",
           "sources_sha": L.pv_sources_sha().decode(),
           "deadline_us": round(DEADLINE_MS * 1e3, 1)}
    checks = {}
    for launch in ("graph", "direct"):
        r = doc[launch] = measure(launch, L, args.callbacks, args.repeats, args.warmup)
        for V in VOICES:
            h, s = r[f"harm_{V}"], r[f"handles_{V}"]
            checks[f"{launch}_harm_{V}_cheaper_than_{V}_handles_by_more_than_their_spread"] = bool(
                h["p50_median_us"] < s["p50_median_us"] - s["p50_spread_us"])
            checks[f"{launch}_harm_{V}_saves_us"] = round(s["p50_median_us"] - h["p50_median_us"], 2)
        checks[f"{launch}_harm_1_minus_map_us"] = round(r["harm_1"]["p50_median_us"] - r["map"]["p50_median_us"], 2)
        checks[f"{launch}_handles_1_minus_map_us"] = round(r["handles_1"]["p50_median_us"] - r["map"]["p50_median_us"], 2)
    doc["checks"] = checks
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
