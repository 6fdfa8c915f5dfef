"""Identity phase locking, CPU side: the numpy reference (tests/phase_lock_ref.py) against
the oracle, the property locking exists for (a chirp keeps its amplitude), the new ABI
symbols, and the locked kernels' register budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pvref
from phase_lock_ref import chirp, mean_envelope, owners, peaks, std_process_lock
from pvamd import _lib
from signals import rms, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("N,hop_div,scale", [(256, 4, 1.5), (512, 3, 0.75), (1024, 8, 1.37), (2048, 2, 0.5)])
def test_unlocked_reference_is_the_oracle(N, hop_div, scale):
    x = synth(12 * N + 37, 11)
    ref = pvref.std_process(x, N, hop_div, ord("t"), scale)
    got = std_process_lock(x, N, hop_div, scale, lock=False)
    assert got.shape == ref.shape
    err = rms(got, ref)
    print(f"N={N} hop_div={hop_div} scale={scale}: rms {err:.3e}")
    assert err <= 1e-12


def test_peak_and_owner_rule():
    m = np.array([0, 1, 3, 1, 0, 0, 2, 2, 0, 5], np.float32)
    #             .  .  P  .  .  .  =  =  .  P   (equal neighbours: neither is a peak)
    pk = peaks(m)
    assert list(np.flatnonzero(pk)) == [2, 9]
    # ties go to the lower peak: bins 5 (3 from 2, 4 from 9) .. ; midpoint of 2 and 9 is 5.5
    assert list(owners(pk)) == [2, 2, 2, 2, 2, 2, 9, 9, 9, 9]
    pk2 = np.zeros(7, bool)
    pk2[[1, 5]] = True
    assert list(owners(pk2)) == [1, 1, 1, 1, 5, 5, 5]  # bin 3 is 2 from both: the lower one
    # no peak (all-zero and NaN frames): every bin owns itself
    assert not peaks(np.zeros(9, np.float32)).any()
    assert not peaks(np.full(9, np.nan, np.float32)).any()
    assert list(owners(np.zeros(5, bool))) == [0, 1, 2, 3, 4]
    # the ends: only the neighbours inside the row count
    assert list(np.flatnonzero(peaks(np.array([4, 1, 0, 1, 3], np.float32)))) == [0, 4]
    # a NaN is no peak and keeps its neighbours at distance 1 and 2 from being one
    assert list(np.flatnonzero(peaks(np.array([0, 5, 0, np.nan, 0, 0, 7, 0], np.float32)))) == [6]


def test_locking_keeps_a_chirps_amplitude():
    """0.5-amplitude chirp stretched by 1.5 at N = 256, hop N/4: the unlocked vocoder loses
    a third of the amplitude (the main lobe's bins drift apart), the locked one keeps it."""
    N = 256
    x = chirp()
    locked = mean_envelope(std_process_lock(x, N, 4, 1.5, lock=True), N)
    unlocked = mean_envelope(std_process_lock(x, N, 4, 1.5, lock=False), N)
    print(f"mean envelope: locked {locked:.4f}, unlocked {unlocked:.4f}")
    assert locked >= 0.45
    assert unlocked <= 0.37


@pytest.mark.parametrize("N,hop_div", [(256, 2), (1024, 4)])
def test_locking_is_the_identity_at_scale_one(N, hop_div):
    x = synth(10 * N + 5, 12)
    a = std_process_lock(x, N, hop_div, 1.0, lock=True)
    b = std_process_lock(x, N, hop_div, 1.0, lock=False)
    assert rms(a, b) <= 1e-12


def test_phase_lock_symbols_and_null_handle():
    L = _lib.lib()
    for s in ("pv_set_phase_lock", "pv_get_phase_lock"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_set_phase_lock(None, 1) == _lib.PV_ERR_ARG
    assert L.pv_get_phase_lock(None) == 0
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4


@pytest.mark.slow
def test_locked_kernels_with_prefetch_have_no_spills(tmp_path):
    """pv_locked.hip for gfx950 with the Makefile's device flags (k_synthesis in the locked
    mode, and nothing else): the instantiations that take syn_run's self-tracked row prefetch (register overlap-add at L = 512: DT 1, 2, 4)
    must have no spilled VGPRs and no AGPRs (the prefetched registers may not be moved
    while the loads are in flight), and scripts/prefetch_hazards.py must pass on the assembly."""
    csrc = os.path.join(ROOT, "phase-vocoder_amd", "csrc")
    out = str(tmp_path / "pv_locked.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(csrc, "pv_locked.hip")], capture_output=True, text=True, timeout=900)
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
    checked = 0
    for name, info in sorted(rows.items()):
        # k_synthesis<L, MODE = kModeLocked (6), DT, QPOW2, LANEK = false, NR = L / 64>
        m = re.match(r"_ZN2pv11k_synthesisILi(\d+)ELi6ELi(\d)ELb([01])ELb0ELi(\d+)EE", name)
        assert m and int(m.group(4)) * 64 == int(m.group(1)), name
        print(f"L={m.group(1)} DT={m.group(2)} QPOW2={m.group(3)}: VGPRs {info['VGPRs']} AGPRs {info['AGPRs']} "
              f"spill {info['VGPRs Spill']} occupancy {info['Occupancy [waves/SIMD]']}")
        if int(m.group(1)) == 512 and int(m.group(2)) > 0:
            checked += 1
            assert info["VGPRs Spill"] == "0" and info["AGPRs"] == "0", (name, info)
    assert len(rows) == 22 and checked == 3
    import sys
    h = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "prefetch_hazards.py"), out],
                       capture_output=True, text=True, timeout=600)
    assert h.returncode == 0 and h.stdout.strip().endswith("0 hazard(s)"), h.stdout[-3000:]
