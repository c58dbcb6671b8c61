"""The host plan of the scalar AMG of K_TT (4c_amd/csrc/fcg_samg_plan.cpp), on the CPU:
tests/cxx/samg_plan_check.cpp compiled with g++ alone from the plan, the graph routines of
fcg_amg_setup.cpp and the box-mesh builder (no libfourc_gpu, no ROCm: the plan is host-only) and
run -- once plain and once under AddressSanitizer and UBSan (a stand-alone host program)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4c_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cxx", "samg_plan_check.cpp"),
           os.path.join(CSRC, "fcg_samg_plan.cpp"), os.path.join(CSRC, "fcg_amg_setup.cpp"),
           os.path.join(CSRC, "fcg_boxmesh.cpp")]


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
def test_scalar_amg_host_plan(tmp_path, name, extra):
    """hex8 (6, 5, 4) node graph, the x = 0 face skipped, coarsened to at least three levels: every
    node that is not skipped lies in exactly one aggregate and skipped nodes in none (their
    prolongator rows empty); each tentative column has unit 2-norm; the A P and A_c patterns hold
    every structural product with ascending columns; every product-plan pair lands on its entry
    of C and each product is listed once; the level sizes decrease; P^T's permutation is one."""
    exe = _build(str(tmp_path / f"samg_plan_check_{name}"), extra)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout, p.stdout + p.stderr
    print(p.stdout)
