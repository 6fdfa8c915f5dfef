"""The real-time harmoniser, CPU side (include/pv.h pv_rt_harmonizer_*): the numpy
restatement (tests/rt_harmonizer_ref.py) against the real-time pitch map's, the gain ramp, the
quality of a live chord, the new kernels' resource usage, and what the library answers without a
device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rt_harmonizer_ref as rh
import rt_pitchmap_ref as rm
from pvamd import _lib, interval_ratios
from signals import synth
from test_rt_pitchmap_ref import usage_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "phase-vocoder_amd", "csrc")

NEW_SYMBOLS = ("pv_rt_harmonizer_max_voices", "pv_rt_harmonizer_reserve", "pv_rt_harmonizer_voices",
               "pv_rt_harmonizer_latency", "pv_rt_harmonizer_push", "pv_rt_harmonizer_host_controls")


# ------------------------------------------------------------------ the restatement
def test_one_voice_at_gain_one_is_the_pitch_map_stream():
    N, hop_div, T = 256, 4, 30
    hop = N // hop_div
    x = synth(T * hop, 4242)
    ratios = rm.vibrato(T, 0.2, 11.0)
    for lock in (False, True):
        mix, ys = rh.stream(x, N, hop_div, ratios[None], np.ones((1, T), np.float32), lock)
        want = rm.stream(x, N, hop_div, ratios, lock)
        assert want.any() and np.array_equal(ys[0], want)
        assert float(np.max(np.abs(mix - want))) == 0.0


def test_the_ramp_is_exact_at_a_constant_gain_and_linear_over_one_block():
    hop, T = 170, 9  # 1 / hop is inexact
    for g in (0.3, 1.0, 1.0 / 3.0, 7.25):
        const = np.full(T, g, np.float32)
        assert np.array_equal(rh.ramp32(const, hop), np.full((T - 1, hop), np.float32(g)))
        assert np.array_equal(rh.ramp64(const, hop), np.full((T - 1, hop), np.float64(np.float32(g))))
    # frame 0's gain is ignored: block 0 ramps from its own gain
    odd = np.full(T, 0.5, np.float32)
    odd[0] = 9.0
    assert np.array_equal(rh.ramp32(odd, hop), np.full((T - 1, hop), np.float32(0.5)))
    # a step 0 -> 1 pushed with frame 4: block 3 is the ramp (j + 1) / hop, ending on 1 exactly,
    # the blocks before are 0 and the blocks after are 1
    step = np.zeros(T, np.float32)
    step[4:] = 1.0
    for ramp in (rh.ramp32, rh.ramp64):
        r = ramp(step, hop)
        assert not r[:3].any() and (r[4:] == 1.0).all()
        assert np.allclose(r[3], np.arange(1, hop + 1) / hop, rtol=2e-7, atol=0) and r[3, -1] <= 1.0
        assert abs(float(r[3, -1]) - 1.0) <= 2.0 ** -23 and (np.diff(r[3]) > 0).all()
    # and back down: a NaN reads as 0
    off = np.ones(T, np.float32)
    off[5] = np.nan
    r = rh.ramp64(off, hop)
    assert (r[:4] == 1.0).all() and np.allclose(r[4], 1.0 - np.arange(1, hop + 1) / hop, atol=1e-7) and r[4, -1] == 0.0
    assert np.allclose(r[5], np.arange(1, hop + 1) / hop, atol=1e-7)
    # through the latency: the gain of block b multiplies emitted block b + G + 1
    G = 2
    s = rh.gain_stream(step, hop, G)
    assert not s[:(G + 1 + 3) * hop].any() and s[(G + 1 + 3) * hop] == pytest.approx(1.0 / hop)
    assert (s[(G + 1 + 4) * hop:] == 1.0).all() and len(s) == T * hop


def test_the_mix_is_the_gain_weighted_sum_of_the_voices():
    N, hop_div, T = 256, 4, 24
    hop = N // hop_div
    x = synth(T * hop, 77)
    ratios = np.stack([rm.constant(T, 1.0), rm.glide(T, 0.5, 2.0), rm.vibrato(T)])
    rng = np.random.default_rng(5)
    gains = rng.uniform(0.0, 1.0, (3, T)).astype(np.float32)
    gains[1, 5] = np.nan
    mix, ys = rh.stream(x, N, hop_div, ratios, gains, True)
    G = rm.plan(hop, 0, 0.5, 2.0)["G"]
    want = np.zeros(T * hop)
    for b in range(T - 1 - G):
        for v in range(3):
            g1 = 0.0 if np.isnan(gains[v, b + 1]) else float(gains[v, b + 1])
            g0 = g1 if b == 0 else (0.0 if np.isnan(gains[v, b]) else float(gains[v, b]))
            j = np.arange(hop)
            o = (G + 1 + b) * hop
            want[o:o + hop] += (g0 + (j + 1) / hop * (g1 - g0)) * ys[v, o:o + hop]
    assert mix.any() and float(np.max(np.abs(mix - want))) <= 1e-15
    assert not mix[:(G + 1) * hop].any()


def test_interval_ratios():
    r = interval_ratios([0, 4, 7, 12, -12])
    assert r.dtype == np.float32 and r[0] == 1.0 and r[3] == 2.0 and r[4] == 0.5
    assert r[1] == np.float32(2.0 ** (4.0 / 12.0)) and r[2] == np.float32(2.0 ** (7.0 / 12.0))
    assert interval_ratios(7).shape == () and interval_ratios(7) == r[2]


# ------------------------------------------------------------------ quality
def test_a_live_chord_lands_on_pitch_at_full_amplitude():
    """N = 1024, hop 256, 64 frames, [1/2, 2] (G = 1, latency 512), a 0.05 cycles / sample sine of
    amplitude 0.5, three voices at 2^(0/12), 2^(4/12), 2^(7/12) with the gains 0.5, 0.3, 0.2; a
    Hann-windowed segment of 8192 samples from 2 N after the latency.  Locked, the mix's three
    peaks lie within 0.02 analysis bin (§3.13's bound for a tone) of 0.05 ratio at no less than 0.98
    of gain 0.5.  Measured on this reference: offsets up to 0.0004 bin at 1.0000 of the amplitude
    (0.2500, 0.1500, 0.1000).  Unlocked the two shifted voices keep 0.826 and 0.780 of theirs (the
    onset's incoherence, §3.16); those figures are printed, not held."""
    x = rh.chord_input()
    ratios, gains = rh.chord_controls()
    hop = rh.CHORD_N // rh.CHORD_HOP_DIV
    lat = rm.plan(hop, 0, 0.5, 2.0)["latency"]
    assert lat == 512
    for lock in (True, False):
        mix, _ = rh.stream(x, rh.CHORD_N, rh.CHORD_HOP_DIV, ratios, gains, lock)
        peaks = rh.chord_peaks(mix, lat)
        print(f"lock {lock}: " + ", ".join(f"voice {v}: {df:+.4f} bin, {a:.4f} of its amplitude"
                                           for v, (df, a) in enumerate(peaks)))
        if lock:
            for df, a in peaks:
                assert abs(df) <= rh.CHORD_BIN_TOL
                assert a >= rh.CHORD_AMP_FLOOR


# ------------------------------------------------------------------ the kernels' resources
@pytest.mark.slow
def test_rt_harmonizer_kernels_have_no_spills(tmp_path):
    """pv_rt_harmon.hip for gfx950 with the Makefile's device flags: k_rt_hmap at L = 128 .. 1024,
    unlocked and locked, and k_rt_hresample.  None spills a vector register, none uses scratch or
    AGPRs (the scalar registers the compiler parks in vector-register lanes are no memory: scratch
    is 0).  k_rt_hresample's static LDS is the window table and the per-voice block state."""
    out = str(tmp_path / "pv_rt_harmon.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(CSRC, "pv_rt_harmon.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows_ = usage_rows(r.stdout + r.stderr)
    want = [f"_ZN2pv9k_rt_hmapILi{L}ELb{b}EEEvNS_12RtHMapParamsE" for L in (128, 256, 512, 1024) for b in (0, 1)]
    assert sorted(rows_) == sorted(want + ["_ZN2pv14k_rt_hresampleENS_12RtHVarParamsE"])
    for name, info in sorted(rows_.items()):
        print(f"{name}: VGPRs {info['VGPRs']} spill {info['VGPRs Spill']} SGPRs parked {info['SGPRs Spill']} "
              f"occupancy {info['Occupancy [waves/SIMD]']} static LDS {info['LDS Size [bytes/block]']}")
        assert info["VGPRs Spill"] == "0" and info["ScratchSize [bytes/lane]"] == "0" and info["AGPRs"] == "0"
        # 8 waves of 64 at L <= 512 and 4 at L = 1024 are one workgroup: two waves, or one, per SIMD
        m = name.startswith("_ZN2pv9k_rt_hmap")
        if m:
            L = int(name.split("ILi")[1].split("E")[0])
            assert int(info["Occupancy [waves/SIMD]"]) >= (2 if L <= 512 else 1)
            assert info["LDS Size [bytes/block]"] == "0"  # (dynamic: sized by the voices at the launch)


def test_workgroup_lds_of_the_largest_geometries():
    """DESIGN.md §3.17's LDS figures, from the carve-up's arithmetic (RtHGeo in pv_rt_harmon.hip;
    Geo<L>::TILE is 570 float2 at L = 512 and 1089 at L = 1024): 95.7 KiB at L = 512 with 8 voices,
    122.1 KiB at L = 1024 with 4, both inside the 160 KiB of a workgroup."""
    def lds(L, tile, V):
        N = 2 * L
        shared = 2 * L + 2 * (L + 2) + 3 * N + 4 * (L + 2)
        return 4 * (shared + V * (2 * tile + N))
    assert lds(512, 570, 8) == 97968 and lds(1024, 1089, 4) == 125008
    assert max(lds(512, 570, 8), lds(1024, 1089, 4)) <= 160 * 1024


# ------------------------------------------------------------------ without a device
def test_symbols_and_answers_without_a_gpu():
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4
    assert [L.pv_rt_harmonizer_max_voices(n) for n in (128, 256, 512, 1024, 2048, 4096)] == [0, 8, 8, 8, 4, 0]
    assert L.pv_rt_harmonizer_latency(None) == 0 and L.pv_rt_harmonizer_voices(None) == 0
    assert L.pv_rt_harmonizer_reserve(None, 3, 0, 1, 0.5, 2.0) == _lib.PV_ERR_ARG and len(L.pv_last_error()) > 0
    assert L.pv_rt_harmonizer_push(None, None, 0, 1, None, None, 0, None, 0, None, 0, None, 0, None) == _lib.PV_ERR_ARG
    assert len(L.pv_last_error()) > 0
    fr, fg = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_float)()
    assert L.pv_rt_harmonizer_host_controls(None, ctypes.byref(fr), ctypes.byref(fg)) == _lib.PV_ERR_ARG
    assert len(L.pv_last_error()) > 0
