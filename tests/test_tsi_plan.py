"""The host plan of the TSI context (4c_amd/csrc/fcg_tsi_plan.cpp), on the CPU:
tests/cxx/tsi_plan_check.cpp compiled with g++ alone from the plan and the box-mesh builder (no
libfourc_gpu, no ROCm: the plan is host-only) and run -- once plain and once under AddressSanitizer
and UBSan (a stand-alone host program)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4c_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cxx", "tsi_plan_check.cpp"),
           os.path.join(CSRC, "fcg_tsi_plan.cpp"), os.path.join(CSRC, "fcg_boxmesh.cpp")]


def _build(out, extra):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-O2", "-Wall", "-pthread", *extra, "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-o", out, *SOURCES]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout + p.stderr
    return out


# the sanitizer runtimes linked statically: the run then does not depend on the order in which the
# loader brings in shared libraries
@pytest.mark.parametrize("name,extra", [("plain", []),
                                        ("sanitized", ["-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=undefined",
                                                       "-static-libasan", "-static-libubsan"])])
def test_tsi_host_plan(tmp_path, name, extra):
    """hex8 2x2x2 (an interior node with 8 incidences), hex8 3x2x2 on both of 2 ranks, hex27 2x1x1
    and hex27 2x2x1 on rank 1 of 2 (each ranked mesh with ghosts and incidences without a row),
    thermo numbering and block graphs derived from the structural graph as fcg.TsiGraph does:
    every owned (e, a) has its incidence inside its node's range with inc_ele = e and inc_loc = a,
    every incidence is hit once, elements ascend inside a node, unowned pairs have -1; the three
    position tables name node b's columns in the k_ST, k_TS and k_TT rows; rn_srow ascends with
    the same node's thermo row beside it; per Gauss point N sums to 1 and dN to 0 (1e-14), the
    weights to 8 within the relative 1.5e-13 of the 13-digit hex27 constants (plus the sum's own
    roundings); all four meshes are node-consistent, hex8 2x2x2 with two thermo LIDs swapped is
    accepted and is not; max_row_tt = 27 on hex8 2x2x2.  Every refusal of fcg_tsi_create that a
    small descriptor can reach is provoked by one tampered copy and compared by status and exact
    text, alone and together with each later one (the earlier one is reported).  The refusal of
    more than 2^31 incidences cannot be reached at test size and is left out."""
    exe = _build(str(tmp_path / f"tsi_plan_check_{name}"), extra)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout, p.stdout + p.stderr
    print(p.stdout)
