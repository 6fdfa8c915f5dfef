#!/usr/bin/env python3
"""Latency of one real-time callback with the pitch map (pv_rt_pitchmap_push; DESIGN.md §3.16,
§4.4) at BASELINE config 5's geometry — 256 channels, N = 256, hop 64, one frame per callback —
by scripts/rt_pitch_latency.py's method, for the variants

  parent_plain   the plain stretch callback (time stretch 1.5) of another build of the library
                 (--parent-lib, e.g. scripts/variant_from_rev.sh HEAD~ parent), when given
  plain          the plain stretch callback of this build
  plain_again    a second pv_rt of the same kind: what two instances of one code differ by
  locked_pitch   locked + pv_rt_pitch_reserve: the fixed 3:2 shifter (two launches)
  map_const      locked + pv_rt_pitchmap_reserve([1/2, 2], fast preset), every ratio 1.5
  map_vibrato    the same with a +-6 % vibrato, a new ratio per channel every callback, written
                 into the pinned ratio buffer

One process; every variant has its own pv_rt and captured callback; after a warm-up the variants
are timed in turn, one callback each, in an order that rotates from round to round (host wall
clock around the synchronous pv_rt_callback, pinned buffers filled in place).  Reports p50 / p99
per repeat, their median over the repeats and the spread, for PV_RT_LAUNCH = graph and direct.
Prints one JSON document; --out writes it to a file too.

usage: python scripts/rt_pitchmap_latency.py [--parent-lib PATH] [--callbacks 2000] [--repeats 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rt_pitch_latency as base  # noqa: E402
from rt_pitch_latency import C, HOP_DIV, N, Variant, _lib, ok  # noqa: E402

HOP = N // HOP_DIV
RANGE = (0.5, 2.0)


def bind(path):
    L = base.bind(path)
    if hasattr(L, "pv_rt_pitchmap_reserve"):
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.pv_rt_pitchmap_reserve.argtypes = [vp, i, i, f, f]
        L.pv_rt_pitchmap_latency.argtypes = [vp]
        L.pv_rt_pitchmap_host_ratios.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    return L


class MapVariant:
    """a scale-1 pv_rt with locking and the pitch map; ratios(k): the [C, 1] ratios of callback k"""

    def __init__(self, name, L, ratios):
        self.name, self.L, self.ratios = name, L, ratios
        cfg = _lib.config(N, HOP_DIV, _lib.PV_TIME_SHIFT, 1.0, _lib.PV_MODE_STANDARD, C, 1, 0)
        self.h = ctypes.c_void_p()
        ok(L, L.pv_rt_create(ctypes.byref(cfg), C, ctypes.byref(self.h)), "pv_rt_create")
        ok(L, L.pv_rt_set_phase_lock(self.h, 1), "pv_rt_set_phase_lock")
        ok(L, L.pv_rt_pitchmap_reserve(self.h, 0, 1, *RANGE), "pv_rt_pitchmap_reserve")
        self.latency = L.pv_rt_pitchmap_latency(self.h)
        ok(L, L.pv_rt_capture(self.h, 1), "pv_rt_capture")
        fi, fo, fr = (ctypes.POINTER(ctypes.c_float)() for _ in range(3))
        ok(L, L.pv_rt_host_buffers(self.h, ctypes.byref(fi), ctypes.byref(fo)), "pv_rt_host_buffers")
        ok(L, L.pv_rt_pitchmap_host_ratios(self.h, ctypes.byref(fr)), "pv_rt_pitchmap_host_ratios")
        self.host_in = np.ctypeslib.as_array(fi, shape=(C, HOP))
        self.host_out = np.ctypeslib.as_array(fo, shape=(C, HOP))
        self.host_ratios = np.ctypeslib.as_array(fr, shape=(C, 1))
        self.k = 0

    def callback(self):
        self.host_ratios[:] = self.ratios(self.k)  # (outside the timed region, like the input's fill)
        self.k += 1
        return Variant.callback(self)

    def close(self):
        self.L.pv_rt_destroy(self.h)


def measure(launch, libs, callbacks, repeats, warmup):
    os.environ["PV_RT_LAUNCH"] = launch  # read by pv_rt_capture
    phase = (1.3 * np.arange(C, dtype=np.float64))[:, None]
    vib = [(1.0 + 0.06 * np.sin(2.0 * np.pi * k / 23.0 + phase)).astype(np.float32) for k in range(23)]
    const = np.full((C, 1), 1.5, np.float32)
    variants = []
    if "parent" in libs:
        variants.append(Variant("parent_plain", libs["parent"]))
    variants += [Variant("plain", libs["this"]), Variant("locked_pitch", libs["this"], lock=True, pitch=True),
                 MapVariant("map_const", libs["this"], lambda k: const),
                 MapVariant("map_vibrato", libs["this"], lambda k: vib[k % 23]), Variant("plain_again", libs["this"])]
    rng = np.random.default_rng(5)
    block = rng.uniform(-0.5, 0.5, (64, C, HOP)).astype(np.float32)
    for k in range(warmup):
        for v in variants:
            v.host_in[:] = block[k % 64]
            v.callback()
    res = {v.name: {"p50_us": [], "p99_us": []} for v in variants}
    for _ in range(repeats):
        t = {v.name: np.empty(callbacks) for v in variants}
        for k in range(callbacks):
            for j in range(len(variants)):  # the order rotates: no variant always follows the same one
                v = variants[(j + k) % len(variants)]
                v.host_in[:] = block[k % 64]
                t[v.name][k] = v.callback()
        for name, a in t.items():
            res[name]["p50_us"].append(round(float(np.percentile(a, 50)), 2))
            res[name]["p99_us"].append(round(float(np.percentile(a, 99)), 2))
    for v in variants:
        assert np.isfinite(v.host_out).all() and v.host_out.any(), v.name
        if isinstance(v, MapVariant):
            res[v.name]["latency_samples"] = v.latency
        v.close()
    for r in res.values():
        for k in ("p50_us", "p99_us"):
            r[k.replace("_us", "_median_us")] = round(float(np.median(r[k])), 2)
            r[k.replace("_us", "_spread_us")] = round(float(np.max(r[k]) - np.min(r[k])), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--callbacks", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--out")
    args = ap.parse_args()
    _lib.lib()  # refuses a stale build
    libs = {"this": bind(_lib.LIB_PATH)}
    if args.parent_lib:
        libs["parent"] = bind(args.parent_lib)
    doc = {"what": f"pv_rt_callback latency, {C} channels, N = {N}, hop {HOP}, one frame per callback; plain and "
                   f"locked_pitch at time stretch {base.SCALE}, the pitch map at scale 1 with ratios in {list(RANGE)}: "
                   "host wall clock around the synchronous call",
           "method": f"one process, {args.warmup} warm-up rounds, then {args.repeats} repeats of {args.callbacks} "
                     "rounds; a round times one callback of every variant in turn, in an order that rotates from round to round",
           "sources_sha": {k: L.pv_sources_sha().decode() for k, L in libs.items()},
           "deadline_us": round(base.DEADLINE_MS * 1e3, 1)}
    for launch in ("graph", "direct"):
        doc[launch] = measure(launch, libs, args.callbacks, args.repeats, args.warmup)
    checks = {"map_p99_under_deadline": all(doc[m][v]["p99_median_us"] < doc["deadline_us"]
                                            for m in ("graph", "direct") for v in ("map_const", "map_vibrato"))}
    if "parent_plain" in doc["graph"]:
        # the spread of repeated runs of one code: over the repeats, and between two instances
        checks["plain_equals_parent_within_spread"] = all(
            abs(doc[m]["plain"]["p50_median_us"] - doc[m]["parent_plain"]["p50_median_us"])
            <= max(doc[m]["plain"]["p50_spread_us"], doc[m]["parent_plain"]["p50_spread_us"],
                   abs(doc[m]["plain"]["p50_median_us"] - doc[m]["plain_again"]["p50_median_us"]))
            for m in ("graph", "direct"))
    doc["checks"] = checks
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
