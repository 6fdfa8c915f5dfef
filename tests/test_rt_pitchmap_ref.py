"""The real-time pitch map, CPU side (include/pv.h pv_rt_pitchmap_*): the numpy
restatement (tests/rt_pitchmap_ref.py) pinned to the offline pitch-map reference, the integer
facts behind the latency G, the library's host-side plan against the restatement, the quality of
the stream (a glide lands on pitch; a live correction pulls a flat voice onto the scale), the new
kernels' resource usage, and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pitchtrack_ref as pr
import pvref
import rt_pitchmap_ref as rm
import varresample_ref as vr
from pvamd import _lib
from signals import rms, synth
from test_varresample_ref import frame_peak

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "phase-vocoder_amd", "csrc")
TABLES_DUMP = os.path.join(ROOT, "phase-vocoder_amd", "build", "tables_dump")

RANGES = ((0.25, 4.0), (0.5, 2.0), (0.84, 1.19))


# ------------------------------------------------------------------ pinned to the offline reference
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,T,seq", [
    (256, 4, 40, "glide"),
    (256, 4, 40, "vibrato"),
    (512, 3, 30, "alternating"),
])
def test_stream_is_the_offline_pitch_map_delayed(N, hop_div, T, seq, lock):
    """The emitted stream against varresample_ref.pitchmap_process(plan(pos = arange, ratio)) of
    the zero-prefixed stream, delayed by (G + 1) hop, over the blocks that stay clear of the offline
    tail (its last span repeats the last row).  The two differ in the last bit of a: 1e-7 RMS, the
    bound of the pins of timemap_ref and varresample_ref."""
    hop = N // hop_div
    rmin, rmax = (0.25, 4.0) if seq == "alternating" else (0.5, 2.0)
    ratios = {"glide": rm.glide(T, 0.5, 2.0), "vibrato": rm.vibrato(T),
              "alternating": rm.alternating(T, 0.25, 4.0)}[seq]
    x = synth(T * hop, 4100 + N)
    got = rm.stream(x, N, hop_div, ratios, lock, 0, rmin, rmax)
    G = rm.plan(hop, 0, rmin, rmax)["G"]
    # offline: n = T - 1 final frames, frame b sounds at row b with the ratio of span b
    n = T - 1
    xp = np.concatenate([np.zeros(N - hop, np.float32), x])
    assert pvref.num_frames(len(xp), hop) >= T
    pos_s, steps = vr.plan(N, hop, np.arange(n, dtype=np.float64), ratios[1:].astype(np.float64))
    assert steps[:n] == rm.steps_of(ratios, rmin, rmax)
    off = vr.pitchmap_process(xp, N, hop_div, pos_s, steps, lock, T, 0, n)
    # block b is clear of the tail when everything it reads lies below the first stretched frame
    # of the last span (position n - 1, which the offline map holds)
    first_tail = next(v for v, p in enumerate(pos_s) if p >= n - 2) * hop
    nb = max(b for b in range(T - 1 - G) if rm.block_reach(steps[:n], hop, 0, b) < first_tail) + 1
    assert nb >= (T - 1 - G) // 2
    a, b = got[(G + 1) * hop:(G + 1 + nb) * hop], off[:nb * hop]
    err = rms(a, b)
    print(f"N={N} hop {hop} {seq} lock {lock}: G {G}, {nb} blocks, rms {err:.3e}, signal rms {rms(b, 0 * b):.3f}")
    assert rms(b, 0 * b) > 1e-2
    assert err <= 1e-7
    assert not got[:(G + 1) * hop].any()


# ------------------------------------------------------------------ integer properties
def test_latency_formula_and_worked_values():
    assert rm.plan(64, 0, 0.84, 1.19) == dict(d_min=rm.step_of(0.84, 0.84, 1.19), d_max=rm.step_of(1.19, 0.84, 1.19),
                                              W_max=23, G=1, latency=128, K=24, row_len=248, ring_cap=2)
    for hop in (64, 128, 256, 512):
        assert rm.plan(hop, 0, 0.84, 1.19)["G"] == 1
    assert [rm.plan(h, 0, 0.25, 4.0)["G"] for h in (64, 128, 256)] == [5, 3, 2]
    assert rm.plan(128, 1, 0.25, 4.0)["G"] == 9
    for hop in (16, 64, 100, 512):
        for q in (0, 1):
            for lo, hi in RANGES:
                p = rm.plan(hop, q, lo, hi, 3)
                assert p["G"] == -(-(p["W_max"] << 32) // (hop * p["d_min"])) and p["latency"] == (p["G"] + 1) * hop
                assert p["W_max"] == vr.block_filter(p["d_max"], q)[1] and p["K"] >= p["W_max"] and p["K"] % 4 == 0
    # the steps are exact: a NaN reads as ratio_min, a ratio outside the range as its end
    assert rm.step_of(np.nan, 0.5, 2.0) == 1 << 31 and rm.step_of(9.0, 0.5, 2.0) == 1 << 33
    assert rm.step_of(0.1, 0.5, 2.0) == 1 << 31 and rm.step_of(np.float32(1.1), 0.5, 2.0) == int(np.float32(1.1) * 2.0 ** 32)
    assert rm.steps_of([7.0, 1.0, 1.5], 0.5, 2.0) == [1 << 32, 3 << 31]  # frame 0's ratio is ignored


def sequences(lo, hi, T, seed, G):
    rng = np.random.default_rng(seed)
    yield "spikes", rm.spikes(T, lo, hi, G + 3)
    yield "random", rng.uniform(lo, hi, T).astype(np.float32)
    yield "min/max", rm.alternating(T, lo, hi)
    yield "max/min", rm.alternating(T, hi, lo)
    yield "min", rm.constant(T, lo)
    yield "max", rm.constant(T, hi)


def test_no_block_reads_a_sample_that_is_not_final():
    """With G every block reads only stretched samples below ceil(Sigma_t / 2^32), which its callback
    or an earlier one has made final.  200 frames; random, alternating, constant-extreme sequences
    and the widest filter followed by the shortest spans; hops 16 .. 512; both presets; the three
    ranges.  G is a bound, not always the least delay (the ceilings leave slack at some
    geometries), but at the worked geometries of DESIGN.md §3.16 and most others G - 1 is too
    little: some sequence then reads beyond what is final."""
    T = 200
    worst, tight, loose = None, set(), set()
    for hop in (16, 64, 100, 128, 256, 512):
        for quality in (0, 1):
            for lo, hi in RANGES:
                p = rm.plan(hop, quality, lo, hi)
                if p["G"] > 64:
                    continue
                short = []
                for name, ratios in sequences(lo, hi, T, 17 * hop + quality, p["G"]):
                    steps = rm.steps_of(ratios, lo, hi)
                    s = rm.least_slack(steps, hop, quality, p["G"])
                    assert s >= 0, (hop, quality, lo, hi, name, s)
                    worst = s if worst is None else min(worst, s)
                    short.append(rm.least_slack(steps, hop, quality, p["G"] - 1) if p["G"] >= 1 else -1)
                    # the row holds what a push can leave (k_rt_map appends without a check): when
                    # the stretch of a push of nf frames ending with frame t is done, the final
                    # samples above row[K], which is where the block after the last emitted one
                    # starts — block max(0, t - nf - G) — and the steps waiting in the ring
                    S = rm.knots(steps, hop)
                    for nf in (1, 4):
                        pn = rm.plan(hop, quality, lo, hi, nf)
                        for t in range(nf - 1, T, nf):
                            first = max(0, t - nf - pn["G"])  # the next block to emit before this push
                            assert pn["K"] + rm.final_below(steps, hop, t) - (S[first] >> 32) <= pn["row_len"]
                            assert t - first <= pn["ring_cap"]
                    for t in range(1, T):
                        assert rm.final_below(steps, hop, t) >= rm.guaranteed_below(steps, hop, t)
                (tight if min(short) < 0 else loose).add((hop, quality, lo, hi))
    print(f"least slack over all sequences: {worst} samples; G - 1 is too little at {len(tight)} geometries, "
          f"would do at {sorted(loose)}")
    assert {(64, 0, 0.84, 1.19), (64, 0, 0.25, 4.0), (128, 0, 0.25, 4.0), (256, 0, 0.25, 4.0),
            (128, 1, 0.25, 4.0)} <= tight
    assert len(tight) >= 3 * len(loose)


def test_a_prefix_of_the_stream_is_the_stream_of_the_prefix():
    N, hop_div, T, T0 = 256, 4, 30, 17
    hop = N // hop_div
    x = synth(T * hop, 91)
    ratios = rm.vibrato(T, 0.3, 7.0)
    for lock in (False, True):
        whole = rm.stream(x, N, hop_div, ratios, lock)
        part = rm.stream(x[:T0 * hop], N, hop_div, ratios[:T0], lock)
        assert part.any() and np.array_equal(whole[:T0 * hop], part)


# ------------------------------------------------------------------ the library's plan
def test_library_plan_is_the_restatement():
    """pvtab::rt_pitchmap_plan through tables_dump (no device): the steps of the range's ends,
    W_max, G, the latency, and the sizes of the scratch row and of the step ring"""
    if not os.path.exists(TABLES_DUMP):
        pytest.skip("tables_dump not built")
    for hop in (16, 64, 100, 512):
        for quality in (0, 1):
            for lo, hi in RANGES + ((1.0, 1.0), (0.3, 0.31)):
                for nf in (1, 4):
                    lo32, hi32 = np.float32(lo), np.float32(hi)
                    r = subprocess.run([TABLES_DUMP, "rtpitchmap", str(hop), str(quality), float(lo32).hex(),
                                        float(hi32).hex(), str(nf)], capture_output=True, text=True, check=True)
                    keys = ("d_min", "d_max", "W_max", "G", "latency", "K", "row_len", "ring_cap")
                    got = dict(zip(keys, (int(v) for v in r.stdout.split())))
                    assert got == rm.plan(hop, quality, lo32, hi32, nf), (hop, quality, lo, hi, nf)
    for args in (("64", "0", "0.2", "2", "1"), ("64", "0", "0.5", "4.5", "1"), ("64", "0", "2", "0.5", "1"),
                 ("64", "0", "nan", "2", "1"), ("64", "0", "0.5", "nan", "1"), ("64", "2", "0.5", "2", "1"),
                 ("64", "0", "0.5", "2", "0"), ("0", "0", "0.5", "2", "1")):
        r = subprocess.run([TABLES_DUMP, "rtpitchmap", *args], capture_output=True, text=True, check=True)
        assert r.stdout.strip() == "refused", args


# ------------------------------------------------------------------ quality
@pytest.mark.parametrize("lock", [False, True])
def test_a_live_glide_lands_on_pitch_at_full_amplitude(lock):
    """DESIGN.md §3.13's tone, glided 1 -> 1.5 through the streaming definition: every frame of the
    stream lands on the curve within 0.1 analysis bin.  Locked, at an amplitude of at least 0.45
    (measured 0.4999).  Unlocked the amplitude is 0.4129 from the first frames on: a stream starts
    with an onset (its N - hop zeros, then the tone), the onset row's phases go into Phi(0), and
    without locking nothing restores the coherence between the bins of the tone's lobe.  That is
    the offline definition's own figure on the same prefixed input, not the streaming form's: the
    unlocked stream must match the offline pitch map's amplitude frame for frame."""
    N, hop_div = 256, 4
    hop = N // hop_div
    T = 200
    x = (0.5 * np.sin(2.0 * np.pi * 0.05 * np.arange(T * hop))).astype(np.float32)
    ratios = rm.glide(T, 1.0, 1.5)
    G = rm.plan(hop, 0, 0.5, 2.0)["G"]
    y = rm.stream(x, N, hop_div, ratios, lock)[(G + 1) * hop:]
    xp = np.concatenate([np.zeros(N - hop, np.float32), x])
    pos_s, steps = vr.plan(N, hop, np.arange(T - 1, dtype=np.float64), ratios[1:].astype(np.float64))
    off = vr.pitchmap_process(xp, N, hop_div, pos_s, steps, lock, T, 0, T - 1)
    n = len(y) // hop - hop_div
    worst_f, least_a, worst_d = 0.0, 1.0, 0.0
    for u in range(8, n - 8):
        f, a = frame_peak(y[u * hop:u * hop + N], N)
        # the frame's centre in blocks; block b carries the ratio pushed with frame b + 1
        centre = u + N / (2.0 * hop)
        want = 0.05 * N * 1.5 ** ((centre + 1.0) / (T - 1.0))
        worst_f, least_a = max(worst_f, abs(f - want)), min(least_a, a)
        worst_d = max(worst_d, abs(a - frame_peak(off[u * hop:u * hop + N], N)[1]))
    print(f"lock {lock}: worst peak offset {worst_f:.4f} bin, least amplitude {least_a:.4f}, "
          f"largest amplitude difference to the offline pitch map {worst_d:.2e}")
    assert worst_f <= 0.1
    assert worst_d <= 1e-6
    # (a deviation from the 0.45 of §3.13 for the unlocked stream, DESIGN.md §3.16: its measured
    # 0.4129 is held with the 25 % margin of tests/test_pitchtrack_ref.py)
    assert least_a >= (0.45 if lock else 0.4129 / 1.25)


def test_live_correction_in_the_reference():
    """The voice held 35 cents under E4 with +-15 cents of vibrato (N = 1024, hop 256, locked, C
    major, retune 1), corrected live: the ratio pushed with frame b + 1 comes from the track of row
    b.  The alignment is the offline one's (34.99 -> 2.61 cents, tests/test_pitchtrack_ref.py), so
    the figures sit next to it; the measured ones are rt_pitchmap_ref.LIVE_BEFORE / LIVE_AFTER, held
    with that test's 25 % margin."""
    before, after = rm.live_reference()
    print(f"median cents off the scale, live: before {before:.3f}, after {after:.3f}")
    assert 34.0 <= before <= 36.0
    assert abs(before - rm.LIVE_BEFORE) <= 0.05
    assert after <= 1.25 * rm.LIVE_AFTER and after <= 0.1 * before


# ------------------------------------------------------------------ the kernels' resources
def usage_rows(text):
    rows_, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            rows_[cur] = {}
        elif cur and ":" in body:
            k, v = body.split(":", 1)
            rows_[cur][k.strip()] = v.strip()
    return rows_


@pytest.mark.slow
def test_rt_pitchmap_kernels_have_no_spills(tmp_path, device_asm):
    """pv_rt_pitchmap.hip for gfx950 with the Makefile's device flags: k_rt_map at L = 128 .. 1024,
    unlocked and locked, and k_rt_varresample.  None spills a vector register, none uses scratch or
    AGPRs.  The scalar registers the compiler parks in vector-register lanes (no memory: scratch is
    0) are lock_offsets' ballot words and the frame loop's addresses, as in k_rt: every k_rt_map
    stays at or below the k_rt of the same size and locking."""
    out = str(tmp_path / "pv_rt_pitchmap.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(CSRC, "pv_rt_pitchmap.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows_ = usage_rows(r.stdout + r.stderr)
    rt = usage_rows(device_asm["pv_rt"][1])
    want = [f"_ZN2pv8k_rt_mapILi{L}ELb{b}EEEvNS_11RtMapParamsE" for L in (128, 256, 512, 1024) for b in (0, 1)]
    assert sorted(rows_) == sorted(want + ["_ZN2pv16k_rt_varresampleENS_11RtVarParamsE"])
    for name, info in sorted(rows_.items()):
        print(f"{name}: VGPRs {info['VGPRs']} spill {info['VGPRs Spill']} SGPRs parked {info['SGPRs Spill']} "
              f"occupancy {info['Occupancy [waves/SIMD]']}")
        assert info["VGPRs Spill"] == "0" and info["ScratchSize [bytes/lane]"] == "0" and info["AGPRs"] == "0"
        m = re.match(r"_ZN2pv8k_rt_mapILi(\d+)ELb(\d)E", name)
        if m:
            mode = 6 if m.group(2) == "1" else 0
            peers = [int(i["SGPRs Spill"]) for n, i in rt.items() if n.startswith(f"_ZN2pv4k_rtILi{m.group(1)}ELi{mode}E")]
            assert len(peers) == 2 and int(info["SGPRs Spill"]) <= min(peers), (name, info["SGPRs Spill"], peers)
        else:
            assert info["SGPRs Spill"] == "0"


# ------------------------------------------------------------------ refusals without a device
def test_symbols_and_refusals_without_a_gpu():
    L = _lib.lib()
    for s in ("pv_rt_pitchmap_reserve", "pv_rt_pitchmap_latency", "pv_rt_pitchmap_push", "pv_rt_pitchmap_host_ratios"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_abi_version() == 5
    assert L.pv_rt_pitchmap_latency(None) == 0
    assert L.pv_rt_pitchmap_reserve(None, 0, 1, 0.5, 2.0) == _lib.PV_ERR_ARG and len(L.pv_last_error()) > 0
    assert L.pv_rt_pitchmap_push(None, None, 0, 1, None, 0, None, 0, None, 0, None) == _lib.PV_ERR_ARG
    assert len(L.pv_last_error()) > 0
    fr = ctypes.POINTER(ctypes.c_float)()
    assert L.pv_rt_pitchmap_host_ratios(None, ctypes.byref(fr)) == _lib.PV_ERR_ARG and len(L.pv_last_error()) > 0
