#!/usr/bin/env python3
"""Latency of one real-time callback (pv_rt_callback) at BASELINE config 5's geometry — 256
channels, N = 256, hop 64, one frame per callback, time stretch 1.5 — for the variants of
DESIGN.md §4.4:

  parent_plain   the plain stretch callback of another build of the library (--parent-lib, e.g.
                 scripts/variant_from_rev.sh HEAD~ parent), when given
  plain          the plain stretch callback of this build
  plain_again    a second pv_rt of the same kind: what two instances of one code differ by
  locked         pv_rt_set_phase_lock(1)
  locked_pitch   locked + pv_rt_pitch_reserve (fast preset): two launches per callback

One process; every variant has its own pv_rt and captured callback; after a warm-up the variants
are timed in turn, one callback each, in an order that rotates from round to round,
`--callbacks` rounds per repeat (host wall clock around the
synchronous pv_rt_callback, pinned buffers filled in place).  Reports p50 / p99 per repeat, their
median over the repeats and the spread (max - min over the repeats), for PV_RT_LAUNCH = graph
and direct.  Prints one JSON document; --out writes it to a file too.

usage: python scripts/rt_pitch_latency.py [--parent-lib PATH] [--callbacks 2000] [--repeats 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "phase-vocoder_amd"))
from pvamd import _lib  # noqa: E402

C, N, HOP_DIV, SCALE = 256, 256, 4, 1.5
DEADLINE_MS = 64 / 44100 * 1e3  # config 5: one 64-sample callback at 44.1 kHz


def bind(path):
    """the pv_rt_* entry points of a library (this build's, or one that lacks the newer ones)"""
    L = ctypes.CDLL(os.path.abspath(path))
    vp, i = ctypes.c_void_p, ctypes.c_int
    fpp = ctypes.POINTER(ctypes.POINTER(ctypes.c_float))
    L.pv_sources_sha.restype = ctypes.c_char_p
    L.pv_last_error.restype = ctypes.c_char_p
    L.pv_rt_create.argtypes = [ctypes.POINTER(_lib.pv_config), i, ctypes.POINTER(vp)]
    L.pv_rt_destroy.argtypes = [vp]
    L.pv_rt_destroy.restype = None
    L.pv_rt_capture.argtypes = [vp, i]
    L.pv_rt_host_buffers.argtypes = [vp, fpp, fpp]
    L.pv_rt_callback.argtypes = [vp, vp, vp]
    if hasattr(L, "pv_rt_pitch_reserve"):
        L.pv_rt_set_phase_lock.argtypes = [vp, i]
        L.pv_rt_pitch_reserve.argtypes = [vp, i, i]
        L.pv_rt_pitch_latency.argtypes = [vp]
    return L


def ok(L, status, what):
    if status != 0:
        raise RuntimeError(f"{what}: status {status}: {L.pv_last_error().decode()}")


class Variant:
    def __init__(self, name, L, lock=False, pitch=False):
        self.name, self.L = name, L
        cfg = _lib.config(N, HOP_DIV, _lib.PV_TIME_SHIFT, SCALE, _lib.PV_MODE_STANDARD, C, 1, 0)
        self.h = ctypes.c_void_p()
        ok(L, L.pv_rt_create(ctypes.byref(cfg), C, ctypes.byref(self.h)), "pv_rt_create")
        if lock:
            ok(L, L.pv_rt_set_phase_lock(self.h, 1), "pv_rt_set_phase_lock")
        if pitch:
            ok(L, L.pv_rt_pitch_reserve(self.h, 0, 1), "pv_rt_pitch_reserve")
        ok(L, L.pv_rt_capture(self.h, 1), "pv_rt_capture")
        fi, fo = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_float)()
        ok(L, L.pv_rt_host_buffers(self.h, ctypes.byref(fi), ctypes.byref(fo)), "pv_rt_host_buffers")
        hop = N // HOP_DIV
        self.host_in = np.ctypeslib.as_array(fi, shape=(C, hop))
        self.host_out = np.ctypeslib.as_array(fo, shape=(C, hop if pitch else int(SCALE * hop)))

    def callback(self):
        t0 = time.perf_counter_ns()
        st = self.L.pv_rt_callback(self.h, None, None)
        t1 = time.perf_counter_ns()
        ok(self.L, st, "pv_rt_callback")
        return (t1 - t0) * 1e-3  # us

    def close(self):
        self.L.pv_rt_destroy(self.h)


def measure(launch, libs, callbacks, repeats, warmup):
    os.environ["PV_RT_LAUNCH"] = launch  # read by pv_rt_capture
    variants = []
    if "parent" in libs:
        variants.append(Variant("parent_plain", libs["parent"]))
    variants += [Variant("plain", libs["this"]), Variant("locked", libs["this"], lock=True),
                 Variant("locked_pitch", libs["this"], lock=True, pitch=True), Variant("plain_again", libs["this"])]
    rng = np.random.default_rng(5)
    block = rng.uniform(-0.5, 0.5, (64, C, N // HOP_DIV)).astype(np.float32)
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
    doc = {"what": f"pv_rt_callback latency, {C} channels, N = {N}, hop {N // HOP_DIV}, one frame per callback, "
                   f"time stretch {SCALE}: host wall clock around the synchronous call",
           "method": f"one process, {args.warmup} warm-up rounds, then {args.repeats} repeats of {args.callbacks} "
                     "rounds; a round times one callback of every variant in turn, in an order that rotates from round to round",
           "sources_sha": {k: L.pv_sources_sha().decode() for k, L in libs.items()},
           "deadline_us": round(DEADLINE_MS * 1e3, 1)}
    for launch in ("graph", "direct"):
        doc[launch] = measure(launch, libs, args.callbacks, args.repeats, args.warmup)
    g = doc["graph"]
    checks = {"locked_pitch_p99_under_deadline": all(doc[m]["locked_pitch"]["p99_median_us"] < doc["deadline_us"]
                                                      for m in ("graph", "direct"))}
    if "parent_plain" in g:
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
