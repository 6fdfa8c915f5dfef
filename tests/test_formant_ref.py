"""Formant-preserving pitch shift, CPU side: the numpy reference (tests/formant_ref.py) against
the oracle, the property the feature exists for (the formant stays where the input has it), the
new ABI symbols, and the new kernels' registers."""
import os
import re
import subprocess

import numpy as np
import pytest

import pvref
from formant_ref import (FLOOR, INPUT_PEAK, formant_peak, log_envelope, pitch_map, std_process_formant, voice)
from pvamd import _lib
from signals import rms, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("N,hop_div,scale", [(256, 4, 1.5), (512, 4, 0.75), (1024, 8, 1.37), (2048, 2, 2.0)])
def test_reference_without_envelope_is_the_oracle(N, hop_div, scale):
    x = synth(12 * N + 37, 21)
    ref = pvref.std_process(x, N, hop_div, ord("p"), scale)
    got = std_process_formant(x, N, hop_div, scale, 0)
    assert got.shape == ref.shape
    err = rms(got, ref)
    print(f"N={N} hop_div={hop_div} scale={scale}: rms {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("N,hop_div,order", [(256, 4, 1), (512, 2, 32), (1024, 4, 256)])
def test_ratio_one_is_the_plain_pitch_shift(N, hop_div, order):
    x = synth(10 * N + 5, 22)
    a = std_process_formant(x, N, hop_div, 1.0, order)
    b = std_process_formant(x, N, hop_div, 1.0, 0)
    assert np.max(np.abs(a - b)) <= 1e-9


def test_envelope_definition():
    N = 256
    B = N // 2 + 1
    # a constant row is its own envelope; zeros and NaNs sit on the floor
    assert np.allclose(log_envelope(np.full(B, 3.0, np.float32), N, 1), np.log(3.0), atol=1e-12)
    row = np.zeros(B, np.float32)
    row[7] = np.nan
    assert np.allclose(log_envelope(row, N, 5), np.log(FLOOR), atol=1e-12)
    # order N/4 keeps quefrencies 0 .. N/4: a cosine of quefrency q <= order passes, above it is removed
    k = np.arange(B)
    for q, keep in ((3, True), (64, True), (65, False)):
        lg = 0.5 * np.cos(2 * np.pi * q * k / N)
        le = log_envelope(np.exp(lg).astype(np.float32), N, 64)
        assert np.allclose(le, lg if keep else 0.0, atol=1e-6), q
    # the map of the oracle: ratio 0.75 gives some bins two sources, 1.5 at most one
    first, cnt = pitch_map(N, 0.75)
    assert cnt.max() == 2 and first[0] == 0 and cnt.sum() == B
    first, cnt = pitch_map(N, 1.5)
    assert cnt.max() == 1 and first[3] == 2 and cnt[1] == 0


@pytest.mark.parametrize("N,order,scale", [(512, 16, 1.5), (1024, 32, 0.75), (2048, 48, 1.25)])
def test_formant_stays_where_the_input_has_it(N, order, scale):
    """harmonics of 0.004 cycles/sample under a resonance at 0.09: the plain pitch shift moves
    the resonance with the partials, the formant-preserving one keeps it.  (Reference values:
    on 0.0898 / 0.0903 / 0.0898, off 0.1323 / 0.0684 / 0.1104.)"""
    x = voice()
    assert abs(formant_peak(x) - INPUT_PEAK) <= 0.01
    on = formant_peak(std_process_formant(x, N, 4, scale, order))
    off = formant_peak(std_process_formant(x, N, 4, scale, 0))
    print(f"N={N} order={order} scale={scale}: peak on {on:.4f}, off {off:.4f}")
    assert abs(on - INPUT_PEAK) <= 0.01
    assert abs(off - scale * INPUT_PEAK) <= 0.01


def test_formant_symbols_and_null_handle():
    L = _lib.lib()
    for s in ("pv_set_formant", "pv_get_formant", "pv_spectral_envelope", "pv_harmonizer_set_formant"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_set_formant(None, 8) == _lib.PV_ERR_ARG
    assert L.pv_get_formant(None) == 0
    assert L.pv_spectral_envelope(None, None, 0, 1, 1, 8, None, 0, None) == _lib.PV_ERR_ARG
    assert L.pv_harmonizer_set_formant(None, 8) == _lib.PV_ERR_ARG
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4


@pytest.mark.slow
def test_formant_kernels_have_no_spills(tmp_path):
    """pv_formant.hip for gfx950 with the Makefile's device flags: k_envelope at the four sizes
    and the 20 instantiations of k_synthesis in the formant mode spill no VGPR and use no scratch; the
    envelope kernel stays within the registers of its occupancy."""
    csrc = os.path.join(ROOT, "phase-vocoder_amd", "csrc")
    out = str(tmp_path / "pv_formant.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(csrc, "pv_formant.hip")], capture_output=True, text=True, timeout=900)
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
    env, syn = {}, 0
    for name, info in sorted(rows.items()):
        print(f"{name}: VGPRs {info['VGPRs']} spill {info['VGPRs Spill']} scratch {info['ScratchSize [bytes/lane]']}")
        assert info["VGPRs Spill"] == "0" and info["ScratchSize [bytes/lane]"] == "0", (name, info)
        m = re.match(r"_ZN2pv10k_envelopeILi(\d+)E", name)
        if m:
            env[int(m.group(1))] = int(info["VGPRs"])
            continue
        # k_synthesis<L, MODE = kModeFormant (7), DT, QPOW2, LANEK = false, NR = L / 64>
        m = re.match(r"_ZN2pv11k_synthesisILi(\d+)ELi7ELi(\d)ELb([01])ELb0ELi(\d+)EE", name)
        assert m and int(m.group(4)) * 64 == int(m.group(1)), name
        syn += 1
    assert len(rows) == 24 and sorted(env) == [128, 256, 512, 1024] and syn == 20
    # 8 waves/SIMD up to L = 256 (<= 64 VGPRs), 6 at L = 512 (<= 80; 26 KB of LDS per workgroup:
    # 6 workgroups per CU), 3 at L = 1024 (<= 168; 51 KB: 3 workgroups per CU)
    assert env[128] <= 64 and env[256] <= 64 and env[512] <= 80 and env[1024] <= 168
