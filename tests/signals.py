"""The test signals, `rms` and the per-hop parity check (a helper: no tests in here).

`synth` is the three-tone generator of every parity test; `zoo` is the set of inputs the synthesis and analysis parity tests run besides `synth`;
`assert_hop_parity` bounds every output hop of a result by the error the fp32 CPU port
(oracle/pvport.c) has on the very same input, so that the bound follows the input's scale and
conditioning instead of being one global RMS figure.
"""
import os

import numpy as np

ZOO_NAMES = ("synth", "noise_fs", "impulses", "dc", "nyquist", "bin_cos", "square", "gaps", "step", "decay")

EPS32 = 2.0 ** -23  # one unit in the last place of an fp32 number in [1, 2)
# Cap on the yardstick itself, wherever it is used: a port defect must fail the check, not
# loosen it.  Not a measurement (the worst E_port seen is 8.3e-7, REF_COMPAT on full-scale
# noise at an output peak of 7.5; STANDARD on the zoo 6e-7, on `synth` 1e-7).
PORT_CAP = 2e-6


def synth(n, seed, sr=44100, tones=3):
    """configs 2-4 generator: 3 sines f~U[55,4000] Hz, a=0.1, + U(+-1e-3) noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = np.zeros(n)
    for _ in range(tones):
        f = rng.uniform(55, 4000)
        ph = rng.uniform(0, 2 * np.pi)
        x += 0.1 * np.sin(2 * np.pi * f * t + ph)
    x += rng.uniform(-1e-3, 1e-3, n)
    return x.astype(np.float32)


def zoo(n, N):
    """dict of float32 signals of length n (t = 0 .. n-1) for an analysis of N points, in the
    order of ZOO_NAMES:

    synth     synth(n, 31): three 0.1-amplitude sines + U(+-1e-3) noise
    noise_fs  default_rng(1).uniform(-0.99, 0.99, n): full-scale broadband
    impulses  0.9 where t % 397 == 5, else 0 (397 is prime: every hop phase is hit)
    dc        0.75
    nyquist   0.75 * (1 - 2 * (t & 1))
    bin_cos   0.5 * cos(2 pi (N/32) t / N): exactly centred on bin N/32
    square    +0.9 for (t // 50) even, -0.9 for odd (half-period 50 samples)
    gaps      synth(n, 5), zeroed where (t // 1500) is odd: digital silence
              inside the stream, repeatedly
    step      0 for t < 5000, then 0.8
    decay     synth(n, 9) * 2^(-t/95), the product in fp64, then cast to
              fp32: at n = 12000 the last ~400 samples are fp32 denormals, none is zero
    """
    t = np.arange(n)
    z = {}
    z["synth"] = synth(n, 31)
    z["noise_fs"] = np.random.default_rng(1).uniform(-0.99, 0.99, n)
    z["impulses"] = np.where(t % 397 == 5, 0.9, 0.0)
    z["dc"] = np.full(n, 0.75)
    z["nyquist"] = 0.75 * (1 - 2 * (t & 1))
    z["bin_cos"] = 0.5 * np.cos(2 * np.pi * (N // 32) * t / N)
    z["square"] = np.where((t // 50) % 2 == 0, 0.9, -0.9)
    z["gaps"] = np.where((t // 1500) % 2 == 0, synth(n, 5), np.float32(0))
    z["step"] = np.where(t < 5000, 0.0, 0.8)
    z["decay"] = synth(n, 9).astype(np.float64) * 2.0 ** (-t / 95.0)
    assert tuple(z) == ZOO_NAMES
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in z.items()}


def zoo_rows(n, N, names=ZOO_NAMES):
    """the zoo as the rows of one [len(names), n] float32 array (one channel per signal)"""
    z = zoo(n, N)
    return np.stack([z[k] for k in names])


def rms(a, b=None):
    d = np.asarray(a, np.float64) - (0.0 if b is None else np.asarray(b, np.float64))
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def _abs_err(g, ref64):
    g, ref64 = np.asarray(g), np.asarray(ref64)
    assert g.shape == ref64.shape and g.ndim == 1, (g.shape, ref64.shape)
    return np.abs(g.astype(np.float64) - ref64.astype(np.float64))


def hop_errors(g, ref64, hs):
    """max-abs error of g against ref64 over each whole output hop of hs samples; a trailing
    partial hop is an entry of its own."""
    e = _abs_err(g, ref64)
    whole = len(e) // hs
    out = list(e[:whole * hs].reshape(whole, hs).max(axis=1)) if whole else []
    if len(e) > whole * hs:
        out.append(e[whole * hs:].max())
    return np.asarray(out, np.float64)


# (PV_HOP_PARITY_REPORT=1 prints the measured ratio of every call: the table of DESIGN.md §3.4)
def assert_hop_parity(g, ref64, port, hs, K=4, what=""):
    """g (the result under test) against ref64 (the oracle), with the fp32 CPU port's output
    for the same input as the yardstick:

      E_port = hop_errors(port, ref64, hs).max(), itself at most PORT_CAP
      every hop of g within K * max(E_port, 2^-23 * max|ref64|)
      rms(g, ref64)  within K * max(rms(port, ref64), 2^-23 * rms(ref64))

    The floors are one fp32 unit in the last place of the output's peak (its RMS): no fp32
    result can be asked for more.  A failure names the hop, the offset of the worst sample
    inside it and the ratio to E_port, so a seam or first-sample defect shows as such.
    Returns the worst hop's error over E_port (over the floor where the port is exact)."""
    g = np.asarray(g)
    assert np.isfinite(g).all(), f"{what}: {np.sum(~np.isfinite(g))} non-finite samples"
    ref64 = np.asarray(ref64, np.float64)
    e_port = hop_errors(port, ref64, hs)
    assert np.isfinite(e_port).all(), f"{what}: the port's output is not finite"
    E_port = float(e_port.max())
    assert E_port <= PORT_CAP, f"{what}: the yardstick is off: E_port {E_port:.3e} > {PORT_CAP:.0e}"
    peak = float(np.abs(ref64).max())
    unit = max(E_port, EPS32 * peak)
    e = _abs_err(g, ref64)
    eh = hop_errors(g, ref64, hs)
    h = int(np.argmax(eh))
    if eh[h] > K * unit:
        off = int(np.argmax(e[h * hs:(h + 1) * hs]))
        bad = int(np.sum(eh > K * unit))
        ratio = eh[h] / E_port if E_port > 0 else float("inf")
        raise AssertionError(
            f"{what}: hop {h} of {len(eh)} (out hop {hs}), worst sample at offset {off} inside it "
            f"(sample {h * hs + off}): |err| {eh[h]:.3e} = {ratio:.1f} x E_port ({E_port:.3e}), "
            f"limit {K} x {unit:.3e}; {bad} hops over the limit, output peak {peak:.3g}")
    r_g, r_port = rms(g, ref64), rms(port, ref64)
    r_lim = K * max(r_port, EPS32 * rms(ref64))
    assert r_g <= r_lim, f"{what}: rms {r_g:.3e} > {K} x max(port rms {r_port:.3e}, 2^-23 rms(ref)) = {r_lim:.3e}"
    ratio = float(eh[h] / (E_port if E_port > 0 else unit)) if unit > 0 else 0.0
    if os.environ.get("PV_HOP_PARITY_REPORT"):
        print(f"hop parity: {what}: worst hop {eh[h]:.3e} = {ratio:.2f} x E_port {E_port:.3e}, "
              f"rms {r_g:.3e} (port {r_port:.3e})")
    return ratio
