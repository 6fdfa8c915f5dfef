"""Time-map stretch, CPU side: the numpy reference (tests/timemap_ref.py) pinned to the oracle by
the identity map, the integer properties the design rests on (the identity telescopes; runs and
carries give the sequential sum), the quality the locked map exists for, and the host split and
the new ABI symbols through ctypes, without a GPU."""
import ctypes

import numpy as np
import pytest

import pvref
from phase_lock_ref import chirp, mean_envelope
from pvamd import _lib
import pvamd
import timemap_ref as tm
from signals import rms, synth


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("N", [256, 512, 1024])
def test_identity_map_is_the_oracles_scale_1_stretch(N, lock):
    hop_div = 4
    x = synth(14 * N + 37, 21)
    frames = pvref.num_frames(len(x), N // hop_div)
    ref = pvref.std_process(x, N, hop_div, ord("t"), 1.0)
    got = tm.timemap_process(x, N, hop_div, np.arange(frames, dtype=np.float64), lock)
    assert got.shape == ref.shape
    err = rms(got, ref)
    print(f"N={N} lock={lock}: rms {err:.3g}")
    assert err <= 1e-7


@pytest.mark.parametrize("lock", [False, True])
def test_identity_map_telescopes_to_the_analysis_phase(lock):
    N, hop = 256, 64
    x = synth(40 * hop + 11, 4)
    frames = pvref.num_frames(len(x), hop)
    mag, ph = pvref.std_analysis(x, N, hop, frames)
    P = tm.phase_turns(ph)
    assert P.min() >= 0 and P.max() < 2 ** 32 and np.all(P % 2 == 0)
    m, Psi = tm.output_phases(mag, P, np.arange(frames, dtype=np.float64), lock)
    assert np.array_equal(Psi, P)
    assert np.array_equal(m.view(np.uint32), mag.view(np.uint32))  # a = 0: fma(0, d, m) = m


def test_runs_with_carries_give_the_sequential_sum():
    N, hop = 256, 64
    x = synth(60 * hop + 200, 9)
    frames = pvref.num_frames(len(x), hop)
    _, ph = pvref.std_analysis(x, N, hop, frames)
    P = tm.phase_turns(ph)
    rng = np.random.default_rng(3)
    maps = [tm.rate_map(frames, 0.73), tm.rate_map(frames, 1.37), tm.ramp_map(frames, 0.5, 2.0), tm.scrub_map(),
            rng.uniform(0, frames - 1e-6, 37), np.full(9, frames - 1.0), np.array([3.25])]
    for pos in maps:
        idx, _ = tm.split(pos)
        seq = tm.scan(P, idx)
        for run in (8, 16, 5):
            assert np.array_equal(tm.scan(P, idx, run), seq), (len(pos), run)
    # the last row's step is 0: a map that stays there stays at P(frames - 1)
    idx, _ = tm.split(np.full(9, frames - 1.0))
    assert np.array_equal(tm.scan(P, idx), np.tile(P[frames - 1], (9, 1)))


def test_locked_map_keeps_a_chirps_envelope():
    N, hop_div = 256, 4
    x = chirp()
    frames = pvref.num_frames(len(x), N // hop_div)
    for name, pos in (("rate 0.73", tm.rate_map(frames, 0.73)), ("rate 1.37", tm.rate_map(frames, 1.37)),
                      ("ramp 0.5 -> 2", tm.ramp_map(frames, 0.5, 2.0))):
        env = [mean_envelope(tm.timemap_process(x, N, hop_div, pos, lock), N) for lock in (False, True)]
        print(f"{name} ({len(pos)} output frames): unlocked {env[0]:.3f} locked {env[1]:.3f}")
        assert env[1] >= 0.45 and env[0] < env[1]


def test_rate_map_is_the_packages():
    for frames, rate in ((60, 0.73), (60, 1.37), (95, 1.0), (2, 0.5)):
        assert np.array_equal(pvamd.rate_map(frames, rate), tm.rate_map(frames, rate))
    assert len(pvamd.rate_map(60, 0.73)) == 81 and pvamd.rate_map(60, 1.0)[-1] == 59.0


def test_timemap_split_on_the_host():
    pos = np.array([0.0, 7.0, 3.5, 59.0, 12.25, 0.1, 1e9 + 0.75, 1.0 - 2.0 ** -40], np.float64)
    idx, frac = pvamd.timemap_split(pos)
    assert idx.dtype == np.int32 and frac.dtype == np.float32
    assert list(idx) == [0, 7, 3, 59, 12, 0, 1000000000, 0]
    assert list(frac[:5]) == [0.0, 0.0, 0.5, 0.0, 0.25]
    assert frac[5] == np.float32(0.1) and frac[6] == 0.75 and frac[7] == 1.0  # (the fp32 rounding may reach 1)
    ri, rf = tm.split(pos)
    assert np.array_equal(ri, idx) and np.array_equal(rf.view(np.uint32), frac.view(np.uint32))
    for bad in ([-0.5], [np.nan], [np.inf], [1.0, -np.inf], [2.0 ** 30], [0.0, 2.0 ** 31]):
        with pytest.raises(pvamd.PVError) as e:
            pvamd.timemap_split(bad)
        assert e.value.status == _lib.PV_ERR_ARG
    L = _lib.lib()
    one = (ctypes.c_double * 1)(1.5)
    i1, f1 = (ctypes.c_int * 1)(), (ctypes.c_float * 1)()
    assert L.pv_timemap_split(one, 1, i1, f1) == _lib.PV_OK and i1[0] == 1 and f1[0] == 0.5
    assert L.pv_timemap_split(one, 0, i1, f1) == _lib.PV_ERR_ARG
    assert L.pv_timemap_split(one, -1, i1, f1) == _lib.PV_ERR_ARG
    assert L.pv_timemap_split(None, 1, i1, f1) == _lib.PV_ERR_ARG
    assert L.pv_timemap_split(one, 1, None, f1) == _lib.PV_ERR_ARG
    assert L.pv_timemap_split(one, 1, i1, None) == _lib.PV_ERR_ARG
    assert b"pv_timemap_split" in L.pv_last_error()


def test_timemap_symbols_and_null_handle():
    L = _lib.lib()
    for s in ("pv_timemap_split", "pv_timemap_set", "pv_timemap_frames", "pv_timemap_process"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    one = (ctypes.c_double * 1)(0.0)
    assert L.pv_timemap_set(None, one, 1) == _lib.PV_ERR_ARG
    assert L.pv_timemap_set(None, None, 0) == _lib.PV_ERR_ARG
    assert L.pv_timemap_frames(None) == 0
    assert L.pv_timemap_process(None, None, 0, 0, 1, 1, None, 0, None, 0, None) == _lib.PV_ERR_ARG
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4


@pytest.mark.slow
def test_map_kernels_have_no_spills(tmp_path):
    """pv_timemap.hip for gfx950 with the Makefile's device flags: no instantiation spills a VGPR
    or uses an AGPR, and the k_synthesis instantiations of both map modes (L = 128 .. 1024, the
    four overlap-add forms) keep at least 2 waves/SIMD."""
    import os
    import re
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(root, "include"), "-o",
                        str(tmp_path / "pv_timemap.s"),
                        os.path.join(root, "phase-vocoder_amd", "csrc", "pv_timemap.hip")],
                       capture_output=True, text=True, timeout=900)
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
    syn = 0
    for name, info in sorted(rows.items()):
        print(f"{name}: VGPRs {info['VGPRs']} AGPRs {info['AGPRs']} spill {info['VGPRs Spill']} "
              f"occupancy {info['Occupancy [waves/SIMD]']}")
        assert info["VGPRs Spill"] == "0" and info["AGPRs"] == "0" and info["ScratchSize [bytes/lane]"] == "0", (name, info)
        # k_synthesis<L, MODE = kModeMap (12) / kModeLockedMap (13), DT, QPOW2 = true, LANEK = false, NR = L / 64>
        m = re.match(r"_ZN2pv11k_synthesisILi(\d+)ELi1[23]ELi(\d)ELb1ELb0ELi(\d+)EE", name)
        if m:
            syn += 1
            assert int(m.group(3)) * 64 == int(m.group(1)), name
            assert int(info["Occupancy [waves/SIMD]"]) >= 2, (name, info)
    assert syn == 32 and len(rows) == 32 + 4 + 1
