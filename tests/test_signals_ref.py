"""CPU checks of the signal zoo's yardstick (tests/signals.py): the fp32 port that bounds the
GPU's per-hop error must itself be close to the oracle on every zoo signal (so it cannot
hide a failure), the oracle must be exactly invariant under a power-of-two input scale (the
property tests/test_gpu_signals.py asks of the GPU), and assert_hop_parity must catch the
defects the 1e-5 RMS bound lets through."""
import re

import numpy as np
import pytest

import pvref
from signals import PORT_CAP, ZOO_NAMES, assert_hop_parity, hop_errors, rms, synth, zoo, zoo_rows

# (N, hop_div, effect, scale): the geometries of tests/test_gpu_signals.py
GEOMETRIES = [
    (1024, 4, "t", 0.5), (1024, 4, "p", 1.5), (2048, 4, "p", 0.75), (2048, 4, "p", 2.0), (256, 2, "t", 1.0),
    (256, 4, "t", 1.5), (1024, 3, "t", 0.5), (512, 3, "t", 1.37), (1024, 4, "t", 2.0), (2048, 8, "p", 1.25),
    (512, 4, "p", 2.0), (1024, 4, "p", 2.0),
]
assert PORT_CAP == 2e-6  # a cap on the yardstick, not a measurement (worst measured: 5.95e-7, `square`)


def test_zoo_shapes_and_denormal_tail():
    z = zoo(12000, 1024)
    assert tuple(z) == ZOO_NAMES
    for k, v in z.items():
        assert v.dtype == np.float32 and v.shape == (12000,) and np.isfinite(v).all(), k
    d = z["decay"]
    tiny = np.finfo(np.float32).tiny
    assert np.all(d != 0)
    assert np.sum(np.abs(d) < tiny) >= 300 and np.abs(d[-200:]).max() < tiny  # a denormal tail
    # the exactly-real signals are what they say: one bin of the fp64 DFT, the rest at
    # the level of the fp32 rounding of the samples
    for name, b in (("dc", 0), ("nyquist", 512), ("bin_cos", 32)):
        X = np.abs(np.fft.rfft(z[name][:1024].astype(np.float64)))
        assert np.argmax(X) == b and np.sum(X > 1e-6 * X[b]) == 1, name
    # the oracle's analysis of the denormal tail is finite and its last frames have phases
    mag, ph = pvref.std_analysis(d, 1024, 256)
    assert np.isfinite(mag).all() and np.isfinite(ph).all()
    assert all(np.any(ph[t] != 0) for t in range(-4, 0))


@pytest.mark.parametrize("N,hop_div,effect,scale", GEOMETRIES)
def test_port_within_cap_on_the_zoo(N, hop_div, effect, scale):
    xs = zoo_rows(12000, N)
    hs = pvref.out_hop(N, hop_div, ord(effect), scale)
    port, _ = pvref.port_std_process_batch(xs, N, hop_div, ord(effect), scale, None, 2)
    assert np.isfinite(port).all()
    for c, name in enumerate(ZOO_NAMES):
        ref = pvref.std_process(xs[c], N, hop_div, ord(effect), scale)
        assert np.isfinite(ref).all(), name
        E_port = hop_errors(port[c], ref, hs).max()
        assert E_port <= PORT_CAP, f"{name}: E_port {E_port:.3e} (output peak {np.abs(ref).max():.3g})"


@pytest.mark.parametrize("N,hop_div", [(1024, 4), (256, 2)])
def test_compat_port_within_cap(N, hop_div):
    x = zoo(12000, N)["noise_fs"]
    port, _ = pvref.port_compat_process_batch(x[None], N, hop_div, None, 1)
    ref = pvref.compat_process(x, N, hop_div)
    assert np.isfinite(port).all() and np.isfinite(ref).all()
    E_port = hop_errors(port[0], ref, N // hop_div).max()
    assert E_port <= PORT_CAP, f"E_port {E_port:.3e} (output peak {np.abs(ref).max():.3g})"


def test_compat_port_all_zero_bin_has_phase_zero():
    """`square` at N = 1024: in fp32 a bin of frame 23 cancels to exactly 0 + 0i (the fp64
    oracle keeps a residue there); its phase is 0 as in pvr_compat_analysis_frame, not
    atanf(0/0), so the frame stays finite and within the cap"""
    x = zoo(12001, 1024)["square"]
    port, _ = pvref.port_compat_process_batch(x[None], 1024, 4, None, 1)
    ref = pvref.compat_process(x, 1024, 4)
    assert np.isfinite(port).all()
    assert hop_errors(port[0], ref, 256).max() <= PORT_CAP


@pytest.mark.parametrize("N,hop_div,scale,hs", [(1024, 4, 0.5, 128), (256, 2, 1.5, 192)])
def test_compat_port_out_hop(N, hop_div, scale, hs):
    """the compat port at the out hop of a time scale (the yardstick of the REF_COMPAT draws of
    tests/test_gpu_random_configs.py) against the oracle at that hop"""
    x = zoo(12000, N)["synth"]
    port, _ = pvref.port_compat_process_batch(x[None], N, hop_div, None, 1, out_hop=hs)
    ref = pvref.compat_process(x, N, hop_div, out_hop=hs)
    assert port[0].shape == ref.shape
    assert hop_errors(port[0], ref, hs).max() <= PORT_CAP


@pytest.mark.parametrize("k", [20, -20])
@pytest.mark.parametrize("N,hop_div,effect,scale", [(1024, 4, "t", 0.5), (512, 4, "p", 1.5)])
def test_oracle_power_of_two_scale_is_exact(N, hop_div, effect, scale, k):
    """x * 2^k: the same phases bit for bit, magnitudes and the fp64 output scaled exactly
    (every signal but `decay`, whose denormals do not scale)."""
    z = zoo(12000, N)
    s = 2.0 ** k
    for name in ZOO_NAMES:
        if name == "decay":
            continue
        x = z[name]
        xs = (x.astype(np.float64) * s).astype(np.float32)
        assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) * s)  # the scaling is exact
        m0, p0 = pvref.std_analysis(x, N, N // hop_div)
        m1, p1 = pvref.std_analysis(xs, N, N // hop_div)
        assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32)), name
        assert np.array_equal(m1.astype(np.float64), m0.astype(np.float64) * s), name
        o0 = pvref.std_process(x, N, hop_div, ord(effect), scale)
        o1 = pvref.std_process(xs, N, hop_div, ord(effect), scale)
        assert np.array_equal(o1, o0 * s), name


# ---------------------------------------------------------------- the helper has teeth
@pytest.fixture(scope="module")
def case():
    """synth(40000, 31) at N = 1024, hop_div 4, stretch 0.5 (out hop 128): oracle and port"""
    x = synth(40000, 31)
    ref = pvref.std_process(x, 1024, 4, ord("t"), 0.5)
    port, _ = pvref.port_std_process_batch(x[None], 1024, 4, ord("t"), 0.5, None, 1)
    ref.setflags(write=False)
    port.setflags(write=False)
    return ref, port[0], 128


def _defects(port, hs):
    n = len(port)
    t = np.arange(n)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    seam = port.astype(np.float64)
    seam[::128 * hs] += 1e-3
    first = port.astype(np.float64)
    first[::hs] *= 1.001
    frame = port.astype(np.float64)
    frame[60 * hs:60 * hs + 1024] += 1e-4 * hann
    return [
        ("seam sample +1e-3, one per 128 hops", seam, True),
        ("first sample of every hop 0.1 % off", first, True),
        ("gain off by 2e-5", port.astype(np.float64) * (1 + 2e-5), True),
        ("spurious tone at 1e-6", port + 1e-6 * np.sin(2 * np.pi * 0.0371 * t), True),
        ("one whole frame off by 1e-4", frame, False),
    ]


def test_port_itself_passes(case):
    ref, port, hs = case
    assert assert_hop_parity(port, ref, port, hs, what="port") == 1.0
    assert hop_errors(port, ref, hs).max() <= 1e-7 and rms(port, ref) <= 2e-8


def test_a_wrong_yardstick_fails_too(case):
    """a port that is itself off by more than PORT_CAP cannot widen the bound: the check fails
    whatever the result under test is"""
    ref, port, hs = case
    bad_port = (port * np.float32(1 + 2e-5)).astype(np.float32)
    assert hop_errors(bad_port, ref, hs).max() > PORT_CAP
    with pytest.raises(AssertionError, match="yardstick"):
        assert_hop_parity(port, ref, bad_port, hs, what="bad port")


@pytest.mark.parametrize("i", range(5))
def test_defects_fail_hop_parity(case, i):
    """the defects a wrong seam tail, gain entry, twiddle, gather or overlap-add slot would
    cause: each fails the per-hop check; the first four pass the old 1e-5 RMS bound"""
    ref, port, hs = case
    name, g, passes_old = _defects(port, hs)[i]
    g = g.astype(np.float32)
    old = rms(g, ref)
    assert (old <= 1e-5) == passes_old, f"{name}: rms {old:.3e}"
    with pytest.raises(AssertionError) as ei:
        assert_hop_parity(g, ref, port, hs, what=name)
    print(f"{name}: rms {old:.2e} ({'passes' if passes_old else 'fails'} 1e-5); {ei.value}")


@pytest.mark.parametrize("F,off", [(16, 0), (88, 127)])
def test_run_seam_defect_is_named(case, F, off):
    """one sample per run of F frames off by 1e-4 (a wrong seam): the message names the hop
    and the offset inside it"""
    ref, port, hs = case
    g = port.copy()
    g[F * hs + off::F * hs] += np.float32(1e-4)
    assert np.any(g != port)
    assert rms(g, ref) <= 1e-5
    with pytest.raises(AssertionError) as ei:
        assert_hop_parity(g, ref, port, hs, what="seam")
    m = re.search(r"hop (\d+) of \d+ .* offset (\d+) inside", str(ei.value))
    assert m, str(ei.value)
    assert int(m.group(1)) % F == 0 and int(m.group(1)) >= F and int(m.group(2)) == off
    assert re.search(r"= \d+\.\d x E_port", str(ei.value))
