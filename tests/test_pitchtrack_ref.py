"""The pitch tracker's fp64 reference (tests/pitchtrack_ref.py) on its own, without a GPU: what it
finds on voices, a sinusoid, noise and empty frames (the figures of DESIGN.md §3.14), the
conditions the GPU parity test rests on (clear frames, the fp32 restatement that sizes its
tolerance, the end-to-end correction), the correction planner of libpv against its definition,
its host code under AddressSanitizer and UBSan in a program of its own, the ABI, and the
kernel's registers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pitchtrack_ref as pr
import pvref
from pvamd import CHROMATIC, MAJOR, PVError, _lib, pitch_correction

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "phase-vocoder_amd", "csrc")
FRAMES = 45

F0_TOL, STRENGTH_TOL = pr.F0_TOL, pr.STRENGTH_TOL


def rows(x, N, frames=FRAMES):
    mag, _ = pvref.std_analysis(x, N, N // 4, frames)
    return mag


def rel_err(r, f, N, frames=FRAMES):
    return np.abs(r["f0"] / pr.frame_f0(f, N, N // 4, frames) - 1.0)


# ---------------------------------------------------------------- what the reference finds
# bounds: the measured worst over N = 256 .. 2048 (printed below) times 1.25
@pytest.mark.parametrize("N", pr.PARITY_SIZES)
def test_reference_finds_f0(N):
    """12-harmonic voices, hop N/4, 45 frames, lags [8, N/4].  Measured over the four sizes:
    steady (period 0.17 N) median 3.7e-5 .. 5.1e-5, worst 5.9e-5, strength >= 0.995; a glide over
    1.5 octaves worst 2.0e-3; noise 0.05 worst 3.9e-3, strength >= 0.944; a lone sinusoid
    2.1e-4, strength 1.000; a period of 11.3 samples 1.06e-2 (the parabola's bias at short lags);
    a period of 0.4 N with lags up to N/2 - 1 worst 8.3e-3, strength >= 0.598."""
    hop = N // 4
    n = FRAMES * hop + N
    f0 = 1.0 / (0.17 * N)
    x, f = pr.voice(n, f0, 1)
    r = pr.track(rows(x, N), N, 8, N // 4)
    e = rel_err(r, f, N)
    print(f"N={N} steady: median {np.median(e):.3g} worst {e.max():.3g} strength >= {r['strength'].min():.4f}")
    assert np.median(e) <= 6.4e-5 and e.max() <= 7.4e-5 and r["strength"].min() >= 0.99

    x, f = pr.voice(n, 1.0 / (0.24 * N), 2, glide_octaves=1.5)
    r = pr.track(rows(x, N), N, 8, N // 4)
    e = rel_err(r, f, N)
    print(f"N={N} glide: median {np.median(e):.3g} worst {e.max():.3g} strength >= {r['strength'].min():.4f}")
    assert e.max() <= 2.5e-3 and r["strength"].min() >= 0.96

    x, f = pr.voice(n, f0, 3, noise=0.05)
    r = pr.track(rows(x, N), N, 8, N // 4)
    e = rel_err(r, f, N)
    print(f"N={N} noisy: median {np.median(e):.3g} worst {e.max():.3g} strength >= {r['strength'].min():.4f}")
    assert e.max() <= 4.8e-3 and r["strength"].min() >= 0.93

    x = (0.5 * np.sin(pr.TWO_PI * f0 * np.arange(n) + 0.3)).astype(np.float32)
    r = pr.track(rows(x, N), N, 8, N // 4)
    e = np.abs(r["f0"] / f0 - 1.0)
    print(f"N={N} sinusoid: worst {e.max():.3g} strength >= {r['strength'].min():.4f}")
    assert e.max() <= 2.6e-4 and r["strength"].min() >= 0.999

    x, f = pr.voice(n, 1.0 / 11.3, 5)
    r = pr.track(rows(x, N), N, 8, N // 4)
    e = np.abs(r["f0"] * 11.3 - 1.0)
    print(f"N={N} period 11.3: worst {e.max():.3g}")
    assert e.max() <= 1.33e-2

    x, f = pr.voice(n, 1.0 / (0.4 * N), 4)
    r = pr.track(rows(x, N), N, 8, N // 2 - 1)
    e = rel_err(r, f, N)
    print(f"N={N} period 0.4 N: median {np.median(e):.3g} worst {e.max():.3g} strength >= {r['strength'].min():.4f}")
    assert e.max() <= 1.04e-2 and r["strength"].min() >= 0.55


@pytest.mark.parametrize("N", pr.PARITY_SIZES)
def test_white_noise_stays_below_the_default_threshold(N):
    """(Measured: strength at most 0.33 at N = 256, 0.22, 0.18, 0.14 at N = 2048.)"""
    x = pr.white(FRAMES * (N // 4) + N, 6)
    for rg in pr.parity_ranges(N):
        r = pr.track(rows(x, N), N, *rg)
        print(f"N={N} lags {rg}: strength <= {r['strength'].max():.3f}")
        assert r["strength"].max() < 0.5 * 0.8


def test_empty_and_non_finite_frames_give_nothing():
    N = 256
    mag = np.abs(rows(pr.white(5 * 64 + N, 1), N, 5))
    mag[1] = 0.0
    mag[2, 7] = np.nan          # counts as 0: the frame still has a pitch result
    mag[3, 9] = np.inf          # the maximum is not finite
    mag[4] = np.nan
    r = pr.track(mag, N, 8, 64)
    assert r["tau"][0] > 0 and r["tau"][2] > 0
    for t in (1, 3, 4):
        assert r["f0"][t] == 0 and r["strength"][t] == 0 and r["tau"][t] == 0
    assert np.array_equal(pr.lag_of(r["f0"]), r["tau"])


def test_scaling_by_a_power_of_two_is_exact_in_the_reference():
    N = 512
    mag = rows(pr.parity_inputs(N)[1], N)
    a = pr.track(mag, N, 8, 128, dtype=np.float32)
    for k in (-20, 20):
        b = pr.track(mag * np.float32(2.0 ** k), N, 8, 128, dtype=np.float32)
        assert np.array_equal(a["f0"].view(np.uint32), b["f0"].view(np.uint32))
        assert np.array_equal(a["strength"].view(np.uint32), b["strength"].view(np.uint32))


# ---------------------------------------------------------------- what the GPU test rests on
@pytest.mark.parametrize("N", pr.PARITY_SIZES)
def test_parity_inputs_are_clear_and_size_the_tolerance(N):
    """The reference alone meets the GPU parity test's condition (at most 5 % of a case's frames
    unclear; measured: none on the clean voice, at most 2 of 45 elsewhere), and the fp32
    restatement of the same steps picks the same lag on every clear frame and stays within a tenth
    of F0_TOL / STRENGTH_TOL on the frames with equal lags."""
    xs = pr.parity_inputs(N)
    for rg in pr.parity_ranges(N):
        for c in range(xs.shape[0]):
            mag = rows(xs[c], N, pr.PARITY_FRAMES)
            r64 = pr.track(mag, N, *rg)
            r32 = pr.track(mag, N, *rg, dtype=np.float32)
            unclear = int((~r64["clear"]).sum())
            same = r64["tau"] == r32["tau"]
            ef = float(np.abs(r32["f0"][same].astype(np.float64) / r64["f0"][same] - 1.0).max())
            es = float(np.abs(r32["strength"][same].astype(np.float64) - r64["strength"][same]).max())
            print(f"N={N} lags {rg} channel {c}: unclear {unclear}, fp32 f0 {ef:.3g} strength {es:.3g}")
            assert unclear <= 0.05 * pr.PARITY_FRAMES
            assert np.all(same | ~r64["clear"])
            assert np.all(r64["tau"] > 0)
            assert ef <= F0_TOL / 10 and es <= STRENGTH_TOL / 10


def test_end_to_end_correction_in_the_reference():
    """A voice held 35 cents under E4 with +-15 cents of vibrato, N = 1024, hop 256, phase lock on:
    the median distance to the C-major scale over the voiced frames away from the ends drops from
    (measured) 34.99 cents to 2.61: what is left is the vibrato that the frame-wise curve trails."""
    before, after = pr.e2e_reference()
    print(f"median cents off the scale: before {before:.3f}, after {after:.3f}")
    assert 34.0 <= before <= 36.0
    assert after <= 3.3 and after <= 0.1 * before


# ---------------------------------------------------------------- the planner
A4 = 440.0 / 44100.0


def flat_track(cents, note=64, frames=20, strength=0.9):
    f0 = np.float32(A4 * 2.0 ** ((note - 69 + cents / 100.0) / 12.0))
    return np.tile(np.array([f0, strength], np.float32), (frames, 1))


def test_planner_snaps_a_flat_voice():
    trk = flat_track(-30.0)
    ratio = pitch_correction(trk, A4, MAJOR)
    assert ratio.dtype == np.float64 and ratio.shape == (20,)
    want = 2.0 ** (0.3 / 12.0)
    assert np.allclose(ratio, want, rtol=1e-7)  # (f0 is an fp32 value)
    assert np.allclose(ratio, pr.correction(trk, A4, pr.MAJOR), rtol=1e-12, atol=0)
    # the same through an iterable of pitch classes
    assert np.array_equal(ratio, pitch_correction(trk, A4, [0, 2, 4, 5, 7, 9, 11]))
    assert MAJOR == pr.MAJOR == 0xAB5 and CHROMATIC == pr.CHROMATIC == 0xFFF


def test_planner_tie_goes_to_the_lower_note():
    # f0 = 2 a4 exactly: note 81 (A5), between the allowed G#5 and A#5
    a4 = float(np.float32(A4))
    trk = np.array([[np.float32(2.0) * np.float32(A4), 1.0]], np.float32)
    ratio = pitch_correction(trk, a4, [8, 10])
    assert abs(ratio[0] - 2.0 ** (-1.0 / 12.0)) < 1e-15
    assert np.array_equal(ratio, pr.correction(trk, a4, (1 << 8) | (1 << 10)))


def test_planner_holds_over_unvoiced_frames_and_glides():
    trk = flat_track(-30.0)
    trk[0] = (0.0, 0.0)                       # unvoiced from the start: s[-1] = 0
    trk[5:9, 1] = 0.2                         # below the threshold
    trk[10] = (np.nan, 0.9)
    trk[11] = (-0.01, 0.9)
    trk[12] = (trk[1, 0], np.nan)
    trk[14] = flat_track(+20.0)[0]            # another correction, then held
    trk[15:, 0] = 0.0
    for retune in (1.0, 0.35):
        ratio = pitch_correction(trk, A4, MAJOR, strength_min=0.5, retune=retune)
        assert np.allclose(ratio, pr.correction(trk, A4, pr.MAJOR, 0.5, retune), rtol=1e-12, atol=0)
    ratio = pitch_correction(trk, A4, MAJOR)
    up, down = 2.0 ** (0.3 / 12.0), 2.0 ** (-0.2 / 12.0)
    assert ratio[0] == 1.0
    assert np.allclose(ratio[1:14], up, rtol=1e-7) and np.allclose(ratio[14:], down, rtol=1e-7)
    # retune < 1: the one-pole curve towards the correction
    g = pitch_correction(flat_track(-30.0), A4, MAJOR, retune=0.25)
    s = np.log2(g)
    c = np.log2(up)
    # (f0 is an fp32 value: its rounding moves the 0.3 semitones by up to 1e-6 semitones)
    assert np.allclose(s, c * (1.0 - 0.75 ** np.arange(1, 21)), rtol=5e-6)


def test_planner_sparse_mask_and_positions():
    # only C allowed: E4 - 30 cents goes up to C5 or down to C4 (the nearer: C4, 3.7 semitones down)
    trk = flat_track(-30.0)
    ratio = pitch_correction(trk, A4, [0])
    assert np.allclose(ratio, 2.0 ** (-3.7 / 12.0), rtol=1e-7)
    # positions: rounded to the nearest frame, clamped to the track
    trk = np.concatenate([flat_track(-30.0, frames=4), flat_track(+20.0, frames=4)])
    pos = np.array([-3.0, 0.0, 3.49, 3.5, 7.0, 99.0, 2.0])
    ratio = pitch_correction(trk, A4, MAJOR, pos=pos)
    assert ratio.shape == (7,)
    assert np.allclose(ratio, pr.correction(trk, A4, pr.MAJOR, pos=pos), rtol=1e-12, atol=0)
    up, down = 2.0 ** (0.3 / 12.0), 2.0 ** (-0.2 / 12.0)
    assert np.allclose(ratio, [up, up, up, down, down, down, up], rtol=1e-7)


def test_planner_refusals():
    trk = flat_track(-30.0)
    bad = [dict(a4=0.0), dict(a4=-1.0), dict(a4=float("nan")), dict(a4=float("inf")), dict(scale=0), dict(scale=4096),
           dict(strength_min=float("nan")), dict(retune=0.0), dict(retune=1.01), dict(retune=float("nan")),
           dict(pos=np.array([0.0, np.nan])), dict(pos=np.array([np.inf])), dict(pos=np.array([]))]
    for kw in bad:
        args = dict(a4=A4, scale=MAJOR)
        args.update(kw)
        with pytest.raises(PVError) as e:
            pitch_correction(trk, **args)
        assert e.value.status == _lib.PV_ERR_ARG, kw
    with pytest.raises(PVError):
        pitch_correction(np.zeros((0, 2), np.float32), A4, MAJOR)
    L = _lib.lib()
    cfg = _lib.pv_pitch_correct(_lib.ABI_VERSION, A4, MAJOR, 0.5, 1.0)
    out = np.zeros(20)
    vp = ctypes.c_void_p
    ok = (trk.ctypes.data_as(vp), 20, None, 20, ctypes.byref(cfg), out.ctypes.data_as(vp))
    assert L.pv_pitch_correct_plan(*ok) == _lib.PV_OK
    for i in (0, 4, 5):  # a NULL track, cfg, ratio
        a = list(ok)
        a[i] = None
        assert L.pv_pitch_correct_plan(*a) == _lib.PV_ERR_ARG
        assert L.pv_last_error().decode()
    stale = _lib.pv_pitch_correct(_lib.ABI_VERSION - 1, A4, MAJOR, 0.5, 1.0)
    assert L.pv_pitch_correct_plan(ok[0], 20, None, 20, ctypes.byref(stale), ok[5]) == _lib.PV_ERR_ARG
    assert "abi_version" in L.pv_last_error().decode()


# ---------------------------------------------------------------- ABI, host code, registers
def test_pitch_track_symbols_and_null_handle():
    L = _lib.lib()
    for s in ("pv_pitch_track", "pv_pitch_correct_plan"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert "PV_PITCH_TRACK_DEFAULT_KAPPA 0.9f" in open(_lib.HEADER).read()
    assert _lib.PV_PITCH_TRACK_DEFAULT_KAPPA == pr.KAPPA
    assert L.pv_pitch_track(None, None, 0, 1, 1, 8, 64, 0.0, None, 0, None) == _lib.PV_ERR_ARG
    assert L.pv_last_error().decode() == "null handle"
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4


def test_planner_host_code_under_sanitizers():
    """pv_tables.cpp's planner in a program of its own (host/pitch_correct_check.cpp), built with
    -fsanitize=address,undefined by the host compiler and run: no report, every check passes, and
    its first case's ratios are this reference's."""
    subprocess.run(["make", "-s", "-C", CSRC, "pitch-correct-san"], check=True)
    exe = os.path.join(ROOT, "phase-vocoder_amd", "build", "pitch_correct_check_san")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split()
    assert lines[-1] == "ok" and len(lines) == 13
    trk = np.tile(np.array([np.float32(A4 * 2.0 ** (-0.3 / 12.0)), 0.9], np.float32), (9, 1))
    trk[2] = (0.0, 0.0)
    trk[3] = (np.nan, 0.9)
    trk[4] = (np.inf, 0.9)
    trk[5] = (-0.01, 0.9)
    trk[6] = (0.01, np.nan)
    trk[7] = (1e-45, 0.9)
    want = pr.correction(trk, A4, pr.MAJOR, 0.5, 0.5, pos=np.arange(12.0))
    assert np.allclose([float(v) for v in lines[:12]], want, rtol=1e-12, atol=0)


@pytest.mark.slow
def test_pitch_kernel_has_no_spills(tmp_path):
    """pv_pitchtrack.hip for gfx950 with the Makefile's device flags: four instantiations, none
    spills, none uses scratch.  (VGPRs 50, 56, 80, 136 at L = 128 .. 1024: DESIGN.md §3.14.)"""
    out = str(tmp_path / "pv_pitchtrack.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(CSRC, "pv_pitchtrack.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows_, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
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
    assert sorted(rows_) == sorted(f"_ZN2pv7k_pitchILi{L}EEEvNS_11PitchParamsE" for L in (128, 256, 512, 1024))
    for name, info in sorted(rows_.items()):
        print(f"{name}: VGPRs {info['VGPRs']} spill {info['VGPRs Spill']} occupancy {info['Occupancy [waves/SIMD]']}")
        assert info["VGPRs Spill"] == "0" and info["SGPRs Spill"] == "0" and info["ScratchSize [bytes/lane]"] == "0"
