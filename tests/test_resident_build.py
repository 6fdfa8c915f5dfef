"""The resources k_resident compiles to in the library's own build: the Makefile's resource check
of pv_resident.hip (`make resource-usage-pv_resident`: the flags its object is built with, a
per-object flag included), against the bounds that keep four workgroups of three waves on a CU.
tests/test_resident_host.py checks the compile without per-object flags."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "phase-vocoder_amd", "csrc")


def _resource_rows(remarks):
    rows, cur = {}, None
    for line in remarks.splitlines():
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
    return rows


def test_library_build_of_k_resident():
    r = subprocess.run(["make", "-C", CSRC, "resource-usage-pv_resident"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    # the command make echoes is the library's: the common flags and pv_resident's own
    line = next(ln for ln in r.stdout.splitlines() if "pv_resident.hip" in ln and "hipcc" in ln)
    for flag in ("-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"):
        assert flag in line.split(), line
    rows = {n: i for n, i in _resource_rows(r.stdout + r.stderr).items() if re.match(r"_ZN2pv10k_residentILi512ELi1E", n)}
    assert len(rows) == 1, rows
    (name, info), = rows.items()
    print(name, info)
    assert int(info["VGPRs"]) <= 168, info
    assert info["VGPRs Spill"] == "0" and info["SGPRs Spill"] == "0", info
    assert info["AGPRs"] == "0", info
    assert info["ScratchSize [bytes/lane]"] == "0", info
    assert int(info["Occupancy [waves/SIMD]"]) >= 3, info
