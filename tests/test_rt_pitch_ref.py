"""CPU side of the real-time pitch shift (pv_rt_pitch_push): the latency
formula D = floor(W Q / P) of tests/rt_pitch_ref.py is enough (a callback's outputs never read
a stretched sample a later callback produces), the reference stream is what its definition
says, the chirp figures of the delayed, prefixed stream, and the new ABI symbols."""
import numpy as np
import pytest

import resample_ref as rr
import rt_pitch_ref as rp
from phase_lock_ref import mean_envelope
from pvamd import _lib

# (out_hop, hop): 3:2, 1:2, 1:4, 4:1, 116:85 (N = 512 / 3 at 1.37), 170:341, 127:170
RATIOS = [(96, 64), (32, 64), (16, 64), (256, 64), (232, 170), (170, 341), (127, 170)]


def test_latency_examples():
    assert rp.latency(96, 64, 0) == 19
    assert rp.latency(96, 64, 1) == 68
    assert rp.latency(16, 64, 0) == 76
    assert rp.latency(64, 64, 0) == 0 and rp.latency(64, 64, 1) == 0
    for hs, hop in RATIOS:
        for quality in (0, 1):
            P, Q = rr.reduce_ratio(hs, hop)
            W = rr.half_width(P, Q, quality)
            D = rp.latency(hs, hop, quality)
            assert D == (W * Q) // P
            assert W * Q - D * P >= 0  # the kernel's offset that keeps its dividend non-negative


@pytest.mark.parametrize("hs,hop", RATIOS)
@pytest.mark.parametrize("quality", [0, 1])
def test_a_callback_reads_no_later_sample(hs, hop, quality):
    """the first T hop samples of z computed from S[:T out_hop] are those computed from a
    longer S, bit for bit: D is late enough"""
    rng = np.random.default_rng(hs * 1000 + hop + quality)
    S = rng.standard_normal(9 * hs)
    full = rp.stream_reference(S, hs, hop, quality)
    for T in (1, 2, 3, 7):
        cut = rp.stream_reference(S[:T * hs], hs, hop, quality)
        assert len(cut) >= T * hop
        assert np.array_equal(cut[:T * hop], full[:T * hop]), (T, hs, hop, quality)


@pytest.mark.parametrize("hs,hop", [(96, 64), (16, 64), (127, 170)])
def test_one_sample_less_latency_is_too_little(hs, hop):
    """with D - 1 some callback's last output would read a sample of the next callback: D is
    the smallest latency of this form (the last output of callback T reads up to
    S[floor((T hop - 1 - D) P / Q) + W])"""
    P, Q = rr.reduce_ratio(hs, hop)
    W = rr.half_width(P, Q, 0)
    D = rp.latency(hs, hop, 0)
    worst = lambda d: max(((T * hop - 1 - d) * P) // Q + W - T * hs for T in range(1, 2 * Q + 2))
    assert worst(D) <= -1
    assert worst(D - 1) >= 0


@pytest.mark.parametrize("hs,hop,quality", [(96, 64, 0), (16, 64, 0), (232, 170, 1)])
def test_stream_reference_is_its_definition(hs, hop, quality):
    """z[m'] = y[m' - D] with y from the sum over S as written, negative m included"""
    rng = np.random.default_rng(5)
    n = 4 * hs
    S = rng.standard_normal(n)
    P, Q = rr.reduce_ratio(hs, hop)
    W = rr.half_width(P, Q, quality)
    D = rp.latency(hs, hop, quality)
    z = rp.stream_reference(S, hs, hop, quality)
    Sat = lambda i: S[i] if 0 <= i < n else 0.0
    for mp in list(range(0, 12)) + [D - 1, D, D + 1, 2 * hop - 1, 2 * hop, 4 * hop - 1]:
        m = mp - D
        i_m, r_m = (m * P) // Q, (m * P) % Q  # python: floor toward -inf, r in [0, Q)
        j = np.arange(-W + 1, W + 1)
        y = float(np.sum(np.array([Sat(i_m + jj) for jj in j]) * rr.kernel(j - r_m / Q, P, Q, quality)))
        assert abs(z[mp] - y) <= 1e-12, mp


def test_ratio_one_has_no_latency_and_no_filter():
    S = np.random.default_rng(1).standard_normal(640)
    assert np.array_equal(rp.stream_reference(S, 64, 64, 0), S)


def test_rt_chirp_figures():
    """the reason for the feature, in fp64: the locked real-time stream keeps the chirp's
    amplitude, the unlocked one loses it (offline: 0.484 and 0.338)"""
    e = [mean_envelope(rp.rt_chirp_reference(lock), 256) for lock in (True, False)]
    print(f"mean envelope of the real-time stream: locked {e[0]:.5f}, unlocked {e[1]:.5f}")
    assert abs(e[0] - rp.RT_CHIRP_LOCKED) <= 1e-5
    assert abs(e[1] - rp.RT_CHIRP_UNLOCKED) <= 1e-5


def test_rt_pitch_symbols_and_null_handles():
    L = _lib.lib()
    for s in ("pv_rt_set_phase_lock", "pv_rt_get_phase_lock", "pv_rt_pitch_reserve", "pv_rt_pitch_latency",
              "pv_rt_pitch_push"):
        assert s in _lib.declared_symbols() and hasattr(L, s)
    assert L.pv_rt_set_phase_lock(None, 1) == _lib.PV_ERR_ARG
    assert L.pv_rt_get_phase_lock(None) == 0
    assert L.pv_rt_pitch_reserve(None, 0, 1) == _lib.PV_ERR_ARG
    assert L.pv_rt_pitch_latency(None) == 0
    assert L.pv_rt_pitch_push(None, None, 0, 1, None, 0, None, 0, None) == _lib.PV_ERR_ARG
    assert L.pv_abi_version() == 5 and L.pv_contract_version() == 4
