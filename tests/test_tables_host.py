"""The host-side arithmetic of libpv (csrc/pv_tables.cpp), checked without a GPU: the
stand-alone tables_dump program (host/tables_dump.cpp, built by the plain host compiler) writes
the tables of a configuration, and they must equal, bit for bit, the oracle's (pvref), the
Python copies (pvamd.tables) and integer recomputations here.  The run-length choices must
reproduce the committed, measured ones (the comments in pv_tables.cpp)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pvref
import resample_ref as rr
from conftest import ROOT
from pvamd import tables

CSRC = os.path.join(ROOT, "phase-vocoder_amd", "csrc")
EXE = os.path.join(ROOT, "phase-vocoder_amd", "build", "tables_dump")
REF_COMPAT, STANDARD = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.run(["make", "-s", "-C", CSRC, "../build/tables_dump"], check=True)


def run(*args, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("PV_")}
    e.update(env)
    return subprocess.run([EXE, *map(str, args)], capture_output=True, check=True, env=e).stdout


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def dump(N, hop_div, mode, effect, scale, window=0):
    """the arrays tables_dump writes, by name (the order is documented in tables_dump.cpp)"""
    raw = run(N, hop_div, mode, effect, scale, window)
    head = np.frombuffer(raw, np.int64, 16)
    names = "N hop hs L_ana L_syn bins p q p_mod q_pow2 src_hi repeat64 rho_bits inv_q_bits".split()
    d = dict(zip(names, (int(v) for v in head)))
    B, off = d["bins"], [128]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, off[0])
        off[0] += a.nbytes
        return a

    d["win"], d["gain"] = take(np.float32, N), take(np.float32, N)
    d["tw_ana"] = take(np.float32, 2 * d["L_ana"])
    d["tws_ana"] = take(np.float32, 2 * (d["L_ana"] + 1))
    d["tw_syn"] = take(np.float32, (len(raw) - off[0] - 4 * (2 * (N // 2 + 1)) - B * (4 + 8 + 4 + 4 + 4)) // 4)
    d["tws_syn"] = take(np.float32, 2 * (N // 2 + 1))
    d["ek"], d["jk"], d["jk_mod"] = take(np.float32, B), take(np.int64, B), take(np.uint32, B)
    d["first"], d["cnt"] = take(np.int32, B), take(np.int32, B)
    assert off[0] == len(raw)
    return d


@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_windows_equal_the_oracle_and_the_python_copies(N):
    hann = dump(N, 4, STANDARD, "t", 1.0)["win"]
    assert np.array_equal(bits(hann), bits(pvref.hann_periodic(N)))
    assert np.array_equal(bits(hann), bits(tables.hann_periodic(N)))
    hamming = dump(N, 4, REF_COMPAT, "t", 1.0, tables.PV_WINDOW_HAMMING_REF)["win"]
    assert np.array_equal(bits(hamming), bits(pvref.hamming_ref(N)))
    assert np.array_equal(bits(hamming), bits(tables.hamming_ref(N)))
    assert np.array_equal(bits(dump(N, 4, REF_COMPAT, "t", 1.0, tables.PV_WINDOW_DEFAULT)["win"]), bits(hamming))
    hann_ref = dump(N, 4, REF_COMPAT, "t", 1.0, tables.PV_WINDOW_HANN_REF)["win"]
    assert np.array_equal(bits(hann_ref), bits(pvref.hann_ref(N)))
    assert np.array_equal(bits(hann_ref), bits(tables.hann_ref(N)))


@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_split_twiddles_equal_the_oracle(N):
    d = dump(N, 4, STANDARD, "t", 1.0)
    assert np.array_equal(bits(d["tws_syn"]), bits(pvref.split_twiddles(N)))
    assert np.array_equal(bits(d["tws_ana"]), bits(pvref.split_twiddles(N)))  # STANDARD: 2 L_ana = N
    c = dump(N, 4, REF_COMPAT, "t", 1.0)
    assert np.array_equal(bits(c["tws_ana"]), bits(pvref.split_twiddles(2 * N)))


@pytest.mark.parametrize("N,hop_div", [(256, 2), (1024, 4), (2048, 8)])
def test_expected_advance_equals_the_oracle(N, hop_div):
    d = dump(N, hop_div, STANDARD, "t", 1.0)
    e, j = pvref.expected_advance(N, N // hop_div)
    assert np.array_equal(bits(d["ek"]), bits(e))
    assert np.array_equal(d["jk"], j.astype(np.int64))


@pytest.mark.parametrize("L", [128, 256, 512, 1024])
def test_analysis_fft_table_equals_the_oracle(L):
    d = dump(2 * L, 4, STANDARD, "t", 1.0)
    tw = d["tw_ana"].reshape(L, 2)
    if L <= 512:  # the contract-v3 pass table, zero-padded to L entries
        ref = pvref.analysis_fft_table(L).reshape(-1, 2)
        assert pvref.fft_v3_applies(L) and len(ref) <= L
    else:  # the radix-2 master table e^{-2 pi i m/L} in the stage-major layout: stage Ns at [Ns-1, 2Ns-1)
        master = pvref.fft_twiddles(L).reshape(L // 2, 2)
        ref = np.concatenate([master[np.arange(Ns) * (L // (2 * Ns))] for Ns in 2 ** np.arange(int(np.log2(L)))])
        assert len(ref) == L - 1
    assert np.array_equal(bits(tw[:len(ref)]), bits(ref))
    assert not tw[len(ref):].any()
    # the synthesis block: the same L-point table first, then the second table of tw_syn_len
    assert len(d["tw_syn"]) == 2 * {128: L, 256: L + L // 2, 512: L + L // 2, 1024: 2 * L}[L]
    assert np.array_equal(bits(d["tw_syn"][:2 * L]), bits(d["tw_ana"]))


def f32_bits(v):
    return int(np.float32(v).view(np.uint32))


@pytest.mark.parametrize("scale,hs,p,q", [(0.5, 128, 1, 2), (1.5, 384, 3, 2), (0.75, 192, 3, 4)])
def test_time_stretch_ratio_is_reduced(scale, hs, p, q):
    d = dump(1024, 4, STANDARD, "t", scale)
    assert (d["hop"], d["hs"], d["p"], d["q"], d["p_mod"], d["q_pow2"]) == (256, hs, p, q, p % q, 1)
    assert d["rho_bits"] == f32_bits(hs / 256) and d["inv_q_bits"] == f32_bits(1.0 / q)


@pytest.mark.parametrize("scale,p,q", [(1.5, 3, 2), (2.0, 2, 1)])
def test_pitch_ratio_and_map(scale, p, q):
    """pitch 2.0 reduces to q = 1, which gates the single-launch path"""
    d = dump(1024, 4, STANDARD, "p", scale)
    assert (d["hs"], d["p"], d["q"], d["p_mod"], d["q_pow2"]) == (256, p, q, p % q, 1)
    assert d["rho_bits"] == f32_bits(scale) and d["inv_q_bits"] == f32_bits(1.0 / q)
    B = d["bins"]
    kp = np.floor(scale * np.arange(B, dtype=np.float64) + 0.5).astype(np.int64)
    first, cnt = np.full(B, -1, np.int32), np.zeros(B, np.int32)
    for k in range(B):
        if 0 <= kp[k] < B:
            if first[kp[k]] < 0:
                first[kp[k]] = k
            cnt[kp[k]] += 1
    assert np.array_equal(d["first"], first) and np.array_equal(d["cnt"], cnt)
    assert d["src_hi"] == max(int(f + c - 1) for f, c in zip(first, cnt) if c > 0)
    assert dump(1024, 4, STANDARD, "t", 1.5)["src_hi"] == B - 1  # no map: every bin is read


@pytest.mark.parametrize("effect,scale", [("t", 0.5), ("t", 1.5), ("t", 0.75), ("p", 1.5), ("p", 2.0), ("p", 1.25)])
def test_jk_mod_is_the_integer_recipe(effect, scale):
    d = dump(1024, 4, STANDARD, effect, scale)
    _, j = pvref.expected_advance(1024, 256)
    q = d["q"]
    ref = [(d["p_mod"] * (int(jk) % q)) % q for jk in j]
    assert d["jk_mod"].tolist() == ref
    # the bins repeat mod 64 (what lets the synthesis keep e_k and jk_mod per lane)
    ek, jm = d["ek"], d["jk_mod"]
    rep = ek[-1] == ek[0] and all(ek[k] == ek[k & 63] and jm[k] == jm[k & 63] for k in range(64, d["bins"] - 1))
    assert d["repeat64"] == int(rep) == 1


def ulp_distance(a, b):
    def ordered(x):
        i = bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return np.abs(ordered(a) - ordered(b))


@pytest.mark.parametrize("p,q,quality", [(3, 2, 0), (1, 2, 1), (2, 3, 0)])
def test_resampler_rows(p, q, quality):
    """<= 1 ulp, not bit equality: resample_ref evaluates the same h(tau) in another form
    (np.sinc(s tau) = sin(pi (s tau)) / (pi (s tau)) against sin(a) / a with a = (pi s) tau, and
    numpy's Chebyshev i0 against the library's power series), so the two fp64 values can differ in
    their last bits and, rarely, round to neighbouring floats."""
    raw = run("resample", p, q, quality)
    P, Q, ql, W = (int(v) for v in np.frombuffer(raw, np.int64, 4))
    assert (P, Q) == rr.reduce_ratio(p, q) and ql == quality and W == rr.half_width(p, q, quality)
    rows = np.frombuffer(raw, np.float32, offset=32).reshape(Q, 2 * W)
    t = np.arange(2 * W, dtype=np.float64)
    ref = np.stack([rr.kernel(t - W + 1 - r / Q, P, Q, quality) for r in range(Q)]).astype(np.float32)
    assert int(ulp_distance(rows, ref).max()) <= 1


def choose(*args, **env):
    return tuple(int(v) for v in run("choose", *args, **env).split())


def test_run_length_choices_are_the_measured_ones():
    # config 3: 1024 channels x 1722 frames, N 1024, hop 256, stretch 0.5; 4 waves per workgroup
    # and 5 workgroups per CU (4 with the 4-wave/SIMD analysis): F = 88
    c3 = (1024, 1722, 1024, 4, STANDARD, "t", 0.5)
    assert choose(*c3, 5, 4)[0] == 88
    assert choose(*c3, 4, 4)[0] == 88
    assert choose(*c3, 0, 4)[0] == 48  # the runtime cannot say: no round fit
    # PV_RUN_FRAMES: even values in [8, 256] only
    assert choose(*c3, 5, 4, PV_RUN_FRAMES="33")[0] == 88
    assert choose(*c3, 5, 4, PV_RUN_FRAMES="64")[0] == 64
    # L_syn >= 1024 caps F at 32 (the config-4 slice: 1024 channels x 861 frames, N 2048)
    assert choose(1024, 861, 2048, 4, STANDARD, "p", 1.5, 5, 4)[0] == 32
    # a run's output span covers the overlap tail: F hs >= N - hs
    assert choose(1, 1, 1024, 4, STANDARD, "t", 0.0625, 0, 4)[0] == 64
    # config 2: one stream of 10335 frames, pitch 2.0: F = 8, single-launch runs of 3 frames
    c2 = (1, 10335, 1024, 4, STANDARD, "p", 2.0, 0, 4)
    assert choose(*c2) == (8, 3)
    assert choose(*c2, PV_FUSED="0") == (8, 0)
    assert choose(*c2, PV_FUSED_FRAMES="2") == (8, 3) and choose(*c2, PV_FUSED_FRAMES="6") == (8, 6)


def test_balanced_rounds_of_the_single_launch():
    """config 2: 3445 runs of 3 frames = 862 workgroups = 3 x 256 + 94 -> 768 workgroups,
    1119 runs of 4 frames (pv_tables.cpp fused_rounds)"""
    assert run("balance", 10335, 3).split() == [b"768", b"1119"]
    assert run("balance", 10335, 3, PV_FUSED_BALANCE="0").split() == [b"862", b"0"]
    assert run("balance", 3 * 4 * 256, 3).split() == [b"256", b"0"]  # whole rounds already
    assert run("balance", 300, 3).split() == [b"25", b"0"]  # less than one round
