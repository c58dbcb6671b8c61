"""The regular-tile classifier of the structured plan, on the CPU:
tests/cxx/sweep_regular_plan_check.cpp compiled with g++ alone from the plan unit and the box-mesh
builder (no libfourc_gpu, no ROCm) and run.  It checks the regular (tile, layer) count of the
38 x 37 x 11 box against the count derived from the tile geometry (one z-segment and several),
that every plane flagged regular reproduces its full record's row0, len, base and npos from the
compact record and the position pattern, and the 6 x 5 x 4 box (no regular tile), the box with a
hole and both ranks of a two-rank split."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4c_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cxx", "sweep_regular_plan_check.cpp"),
           os.path.join(CSRC, "fcg_create_plan.cpp"), os.path.join(CSRC, "fcg_boxmesh.cpp")]


def test_regular_tiles_are_classified_as_the_geometry_says(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "sweep_regular_plan_check")
    cmd = [cxx, "-std=c++17", "-O2", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-o", exe, *SOURCES]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout + p.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout, p.stdout + p.stderr
