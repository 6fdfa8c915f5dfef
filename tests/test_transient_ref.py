"""Transient phase reset, CPU side: the numpy reference (tests/transient_ref.py) against the
phase-locking reference it extends, the properties the reset exists for (a flagged frame is the
input's frame; a click keeps its peak), the detector's test input, the new ABI symbols, and the
reset kernels' register budget."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pvref
from phase_lock_ref import std_process_lock
from pvamd import _lib
from signals import rms, synth
from transient_ref import (DEFAULT_THRESHOLD, bursts, clear, click_flags, click_frames, clicks, compactness, pick,
                           std_process_reset, strengths)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N,hop_div,scale", [(256, 4, 1.5), (512, 3, 0.75), (1024, 4, 0.5)])
def test_without_flags_the_reference_is_the_phase_lock_reference(N, hop_div, scale, lock):
    x = synth(12 * N + 37, 11)
    ref = std_process_lock(x, N, hop_div, scale, lock)
    frames = pvref.num_frames(len(x), N // hop_div)
    for flags in (None, np.zeros(frames, np.uint8)):
        got = std_process_reset(x, N, hop_div, scale, lock, flags)
        assert got.shape == ref.shape
        assert rms(got, ref) <= 1e-15


@pytest.mark.parametrize("lock", [False, True])
def test_a_flagged_frames_spectrum_is_the_analysis_spectrum(lock):
    N, hop_div, scale = 256, 4, 1.5
    x = synth(30 * 64 + 5, 3)
    frames = pvref.num_frames(len(x), N // hop_div)
    flags = np.zeros(frames, np.uint8)
    flags[[0, 7, 19]] = 1  # (frame 0's flag is ignored)
    sp = []
    std_process_reset(x, N, hop_div, scale, lock, flags, spectra=sp)
    for t in (7, 19):
        Y, X = sp[t]
        assert np.max(np.abs(Y - X)) <= 1e-12 * max(1.0, np.max(np.abs(X)))
    # and an unflagged frame's is not (the stretch moves the phases)
    Y, X = sp[12]
    assert np.max(np.abs(Y - X)) >= 1e-3 * np.max(np.abs(X))
    Y, X = sp[0]
    # (frame 0: closed(0) = rho-scaled analysis phase, not the analysis phase itself)
    assert np.max(np.abs(Y - X)) >= 1e-3 * np.max(np.abs(X))


def test_a_flag_changes_nothing_before_its_frame_and_has_no_run_boundaries():
    """The reference has no runs: its output depends on the flags alone, and a flag at frame t0
    changes no sample before t0's first output position.  (Stated here so that the GPU test,
    whose kernels do have runs, mirrors it: tests/test_gpu_transient.py.)"""
    N, hop_div, scale = 256, 4, 1.5
    x = synth(40 * 64 + 5, 4)
    hs = pvref.out_hop(N, hop_div, ord("t"), scale)
    frames = pvref.num_frames(len(x), N // hop_div)
    plain = std_process_reset(x, N, hop_div, scale, False, None)
    flags = np.zeros(frames, np.uint8)
    flags[17] = 1
    got = std_process_reset(x, N, hop_div, scale, False, flags)
    assert np.array_equal(got[:17 * hs], plain[:17 * hs])
    assert rms(got[17 * hs:], plain[17 * hs:]) >= 1e-3


def test_the_reset_keeps_a_clicks_peak():
    """The figure the feature exists for: 0.8-amplitude clicks every 1536
    samples over a 0.05-amplitude tone, N = 256, hop 64, stretch 1.5, the frame nearest each
    click flagged.  Energy within +-N/8 of a click's output position over the energy within +-N,
    mean over the clicks, fp64 reference:
        unlocked off 0.2607, on 0.5716; locked off 0.5163, on 0.5375.
    With the detector's own flags at the default threshold (frames 8, 32, 56, 80, 104: one frame
    before the nearest-centre frames 9, 33, 57, 81, 105 — the first frame the click enters with
    weight): unlocked 0.6404, locked 0.5875 (reported, not asserted)."""
    N, hop_div, scale = 256, 4, 1.5
    hop = N // hop_div
    x, pos = clicks()
    frames = pvref.num_frames(len(x), hop)
    hs = pvref.out_hop(N, hop_div, ord("t"), scale)
    fl = click_flags(pos, N, hop, frames)
    want = {(False, False): 0.2607, (False, True): 0.5716, (True, False): 0.5163, (True, True): 0.5375}
    got = {}
    for lock in (False, True):
        for on in (False, True):
            y = std_process_reset(x, N, hop_div, scale, lock, fl if on else None)
            got[lock, on] = compactness(y, pos, N, hop, hs)
            print(f"lock {lock} reset {on}: {got[lock, on]:.4f}")
            assert abs(got[lock, on] - want[lock, on]) <= 5e-4
        assert got[lock, True] > got[lock, False]
    mag, _ = pvref.std_analysis(x, N, hop, frames)
    det = pick(*strengths(mag), DEFAULT_THRESHOLD)
    print("detected frames", np.flatnonzero(det), "nearest-centre frames", click_frames(pos, N, hop))
    for lock in (False, True):
        y = std_process_reset(x, N, hop_div, scale, lock, det)
        print(f"lock {lock} detected flags: {compactness(y, pos, N, hop, hs):.4f}")


def test_detector_rule_and_test_input():
    rise = np.array([5.0, 0.1, 3.0, 3.0, 0.2, 4.0], np.float64)
    tot = np.full(6, 5.0)
    #                 t=0 never; 2: > before, >= after (tie: the first of equals); 3: not > before
    assert list(np.flatnonzero(pick(rise, tot, 0.3))) == [2, 5]
    assert list(np.flatnonzero(pick(rise, tot, 0.7))) == [5]
    # a NaN magnitude adds nothing
    m = np.array([[1, np.nan, 2], [2, 1, np.nan]], np.float32)
    r, t = strengths(m)
    assert list(r) == [3.0, 1.0] and list(t) == [3.0, 3.0]
    # the GPU detector test's input: fewer than 2 % of its frames are too close to call
    for N, seed in ((256, 5), (1024, 6)):
        hop = N // 4
        x = bursts(70 * hop + 13, seed)
        frames = pvref.num_frames(len(x), hop)
        mag, _ = pvref.std_analysis(x, N, hop, frames)
        rise, tot = strengths(mag)
        ok = clear(rise, tot)
        fl = pick(rise, tot)
        print(f"N={N}: {frames} frames, {int(fl.sum())} flagged, {int((~ok).sum())} unclear")
        assert (~ok).mean() < 0.02 and 2 <= fl.sum() <= frames // 4


def test_transient_symbols_and_null_handle():
    L = _lib.lib()
    for s in ("pv_transient_reserve", "pv_set_transient", "pv_get_transient", "pv_transient_set_flags",
              "pv_transient_get_flags", "pv_onset_strength"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_set_transient(None, 1, 0.0) == _lib.PV_ERR_ARG
    assert L.pv_transient_reserve(None) == _lib.PV_ERR_ARG
    assert L.pv_get_transient(None) == 0
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4
    assert _lib.PV_TRANSIENT_DEFAULT_THRESHOLD == DEFAULT_THRESHOLD
    hdr = open(_lib.HEADER).read()
    assert f"#define PV_TRANSIENT_DEFAULT_THRESHOLD {DEFAULT_THRESHOLD}f" in hdr


@pytest.mark.slow
def test_reset_kernels_with_prefetch_have_no_spills(tmp_path):
    """pv_transient.hip for gfx950 with the Makefile's device flags: no instantiation spills a
    VGPR; the k_synthesis instantiations that take syn_run's self-tracked row prefetch (register
    overlap-add at L = 512: DT 1, 2, 4, both reset modes) use no AGPRs either, and
    scripts/prefetch_hazards.py passes on the assembly."""
    csrc = os.path.join(ROOT, "phase-vocoder_amd", "csrc")
    out = str(tmp_path / "pv_transient.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(csrc, "pv_transient.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur and ":" in body:
            k, v = body.split(":", 1)
            rows[cur][k.strip()] = v.strip()
    checked = syn = 0
    for name, info in sorted(rows.items()):
        print(f"{name}: VGPRs {info['VGPRs']} AGPRs {info['AGPRs']} spill {info['VGPRs Spill']} "
              f"occupancy {info['Occupancy [waves/SIMD]']}")
        assert info["VGPRs Spill"] == "0", (name, info)
        # k_synthesis<L, MODE = kModeReset (10) / kModeLockedReset (11), DT, QPOW2, LANEK = false, NR = L / 64>
        m = re.match(r"_ZN2pv11k_synthesisILi(\d+)ELi1[01]ELi(\d)ELb([01])ELb0ELi(\d+)EE", name)
        if m:
            syn += 1
            assert int(m.group(4)) * 64 == int(m.group(1)), name
            if int(m.group(1)) == 512 and int(m.group(2)) > 0:
                checked += 1
                assert info["AGPRs"] == "0" and int(info["Occupancy [waves/SIMD]"]) >= 2, (name, info)
    assert syn == 40 and checked == 6 and len(rows) == 40 + 4 + 8 + 1
    h = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "prefetch_hazards.py"), out],
                       capture_output=True, text=True, timeout=600)
    assert h.returncode == 0 and h.stdout.strip().endswith("0 hazard(s)"), h.stdout[-3000:]
