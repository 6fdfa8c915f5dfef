"""Band-limited resampler, CPU side: what the fp64 reference (tests/resample_ref.py) does to
tones in the pass band and above the output Nyquist, the pitch shift it gives a locked time
stretch (the chirp figures of DESIGN.md §3.8), the length formula, the new ABI symbols, and the
kernel's register budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pvref
import resample_ref as rr
from phase_lock_ref import chirp, mean_envelope, std_process_lock
from pvamd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_IN = 20000


def tone(f, n=N_IN):
    return np.sin(2.0 * np.pi * f * np.arange(n, dtype=np.float64))


def core(y, p, q, quality):
    """the output without its first and last 2W samples"""
    w2 = 2 * rr.half_width(p, q, quality)
    return y[w2:len(y) - w2], w2


def amplitude(y, f_out, p, q, quality):
    """least-squares amplitude of the tone f_out (cycles per output sample) in the core of y"""
    c, w2 = core(y, p, q, quality)
    t = np.arange(w2, w2 + len(c), dtype=np.float64)
    A = np.stack([np.sin(2 * np.pi * f_out * t), np.cos(2 * np.pi * f_out * t)], axis=1)
    coef, *_ = np.linalg.lstsq(A, c, rcond=None)
    return float(np.hypot(coef[0], coef[1]))


def core_rms(y, p, q, quality):
    c, _ = core(y, p, q, quality)
    return float(np.sqrt(np.mean(c * c)))


def in_out(p, q, f):
    """a tone at f cycles per sample of the lower of the two rates (the rate whose Nyquist the
    filter protects: s = rolloff min(1, Q/P) puts the cutoff at rolloff / 2 of it) -> its input
    and output frequencies.  Above 1 the lower rate is the output's; below 1 it is the input's, and
    the output frequency f P / Q is lower still."""
    return (f * q / p, f) if p > q else (f, f * p / q)


PASS_RATIOS = [(3, 2), (3, 4), (701, 512), (127, 170)]
ALIAS_CASES = [(3, 2, 0.4), (3, 2, 0.45), (2, 1, 0.3), (2, 1, 0.4), (2, 1, 0.45), (701, 512, 0.4), (701, 512, 0.45)]


@pytest.mark.parametrize("p,q", PASS_RATIOS)
def test_fast_preset_keeps_the_pass_band(p, q):
    """tones up to 0.30 cycles per sample (of the lower rate, so the output frequency is at most
    0.30: 0.71 of the cutoff 0.425) keep their amplitude within 1e-4"""
    for f in (0.01, 0.1, 0.2, 0.30):
        f_in, f_out = in_out(p, q, f)
        assert f_in < 0.5 and f_out <= 0.30
        a = amplitude(rr.resample(tone(f_in), p, q, 0), f_out, p, q, 0)
        print(f"fast {p}:{q} output tone {f_out:.4f}: amplitude {a:.7f}")
        assert abs(a - 1.0) <= 1e-4


@pytest.mark.parametrize("p,q,f_in", ALIAS_CASES)
def test_fast_preset_rejects_what_would_alias(p, q, f_in):
    """an input tone that would land above the output Nyquist: 1.6e-5 RMS or less measured"""
    assert f_in * p / q > 0.5
    r = core_rms(rr.resample(tone(f_in), p, q, 0), p, q, 0)
    print(f"fast {p}:{q} input tone {f_in}: rms {r:.3e}")
    assert r <= 1e-4


@pytest.mark.parametrize("p,q", [(3, 2), (127, 170)])
def test_best_preset_keeps_the_pass_band(p, q):
    """below 0.9 of the output Nyquist the amplitude stays within 1e-4; at 0.9 (0.45 cycles per
    output sample) it measures 0.99744"""
    for f in (0.01, 0.2, 0.4, 0.44):
        f_in, f_out = in_out(p, q, f)
        a = amplitude(rr.resample(tone(f_in), p, q, 1), f_out, p, q, 1)
        print(f"best {p}:{q} output tone {f_out:.4f}: amplitude {a:.7f}")
        assert abs(a - 1.0) <= 1e-4
    f_in, f_out = in_out(p, q, 0.45)
    a = amplitude(rr.resample(tone(f_in), p, q, 1), f_out, p, q, 1)
    print(f"best {p}:{q} output tone {f_out:.4f}: amplitude {a:.7f}")
    assert abs(a - 0.99744) <= 1e-4


@pytest.mark.parametrize("p,q,f_in", ALIAS_CASES)
def test_best_preset_rejects_what_would_alias(p, q, f_in):
    """2.3e-8 RMS or less measured"""
    r = core_rms(rr.resample(tone(f_in), p, q, 1), p, q, 1)
    print(f"best {p}:{q} input tone {f_in}: rms {r:.3e}")
    assert r <= 1e-6


def test_locked_stretch_then_resample_keeps_a_chirps_amplitude():
    """0.5-amplitude chirp shifted by 1.5 at N = 256, hop N/4: mean envelope 0.292 by the bin
    mapping, 0.338 by the unlocked stretch resampled 3:2, 0.484 by the locked one."""
    N = 256
    x = chirp()
    locked = rr.resample(std_process_lock(x, N, 4, 1.5, lock=True), 3, 2, 0)
    unlocked = rr.resample(std_process_lock(x, N, 4, 1.5, lock=False), 3, 2, 0)
    mapped = pvref.std_process(x, N, 4, ord("p"), 1.5)
    e = [mean_envelope(y, N) for y in (locked, unlocked, mapped)]
    print(f"mean envelope: locked {e[0]:.4f}, unlocked {e[1]:.4f}, bin mapping {e[2]:.4f}; "
          f"{len(locked)} samples out for {len(x)} in")
    assert len(locked) == 6187
    assert e[0] >= 0.45
    assert e[1] <= 0.37
    assert e[2] <= 0.32


def test_ratio_one_returns_the_input():
    x = np.random.default_rng(3).standard_normal(1000)
    for p, q in ((1, 1), (7, 7), (4096, 4096)):
        assert np.array_equal(rr.resample(x, p, q, 0), x)
        assert rr.out_length(p, q, 1000) == 1000


@pytest.mark.parametrize("p,q,quality", [(3, 2, 0), (3, 4, 0), (1, 4, 0), (4, 1, 0), (701, 512, 0), (127, 170, 1)])
def test_output_length(p, q, quality):
    """n_out = ceil(n_in Q / P): every m with m P / Q < n_in, also for inputs shorter than the filter"""
    W = rr.half_width(p, q, quality)
    for n_in in (0, 1, W - 1, 1000):
        n_out = rr.out_length(p, q, n_in)
        assert n_out == -((-n_in * q) // p)
        assert (n_out - 1) * p < n_in * q <= n_out * p or n_in == 0
        y = rr.resample(np.ones(n_in), p, q, quality)
        assert y.shape == (n_out,) and np.isfinite(y).all()


def test_resample_symbols_and_null_handles():
    L = _lib.lib()
    for s in ("pv_resampler_create", "pv_resampler_destroy", "pv_resample_length", "pv_resample",
              "pv_pitch_reserve", "pv_pitch_output_length", "pv_pitch_process"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_pitch_reserve(None, 0) == _lib.PV_ERR_ARG
    assert L.pv_pitch_output_length(None, 10) == 0
    assert L.pv_pitch_process(None, None, 0, 0, 1, 1, None, 0, None, 0, None) == _lib.PV_ERR_ARG
    assert L.pv_resample(None, None, 0, 0, 1, None, 0, None) == _lib.PV_ERR_ARG
    assert L.pv_resample_length(None, 100) == 0
    L.pv_resampler_destroy(None)
    # refused before any device is touched
    h = ctypes.c_void_p()
    for p, q, quality, want in ((9, 2, 0, _lib.PV_ERR_UNSUPPORTED), (2, 9, 0, _lib.PV_ERR_UNSUPPORTED),
                                (4097, 4096, 0, _lib.PV_ERR_UNSUPPORTED), (3, 2, 2, _lib.PV_ERR_ARG),
                                (3, 2, -1, _lib.PV_ERR_ARG), (0, 2, 0, _lib.PV_ERR_ARG), (3, -2, 0, _lib.PV_ERR_ARG)):
        assert L.pv_resampler_create(p, q, quality, 0, ctypes.byref(h)) == want, (p, q, quality)
        assert not h.value
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4


@pytest.mark.slow
def test_resample_kernels_have_no_spills(tmp_path):
    """pv_resample.hip for gfx950 with the Makefile's device flags: no instantiation spills"""
    csrc = os.path.join(ROOT, "phase-vocoder_amd", "csrc")
    out = str(tmp_path / "pv_resample.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(csrc, "pv_resample.hip")], capture_output=True, text=True, timeout=900)
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
    kernels = [n for n in rows if "k_resample" in n]
    assert len(kernels) == 4 and len(rows) == 5, sorted(rows)  # R = 8, 4, 2, 1 and k_copy_rows
    for name, info in sorted(rows.items()):
        print(f"{name}: VGPRs {info['VGPRs']} AGPRs {info['AGPRs']} spill {info['VGPRs Spill']} "
              f"occupancy {info['Occupancy [waves/SIMD]']}")
        assert info["VGPRs Spill"] == "0" and info["SGPRs Spill"] == "0", (name, info)
