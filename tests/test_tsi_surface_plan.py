"""The host plan of a thermal surface (4c_amd/csrc/fcg_tsi_surface_plan.cpp), on the CPU:
tests/cxx/tsi_surface_plan_check.cpp compiled with g++ alone from the plan and the box-mesh builder
(no libfourc_gpu, no ROCm: the plan is host-only) and run -- once plain and once under AddressSanitizer
and UBSan (a stand-alone host program)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4c_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cxx", "tsi_surface_plan_check.cpp"),
           os.path.join(CSRC, "fcg_tsi_surface_plan.cpp"), os.path.join(CSRC, "fcg_boxmesh.cpp")]


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
def test_tsi_surface_host_plan(tmp_path, name, extra):
    """hex8 3x3x3 and hex27 2x2x2 with all faces of the box's sides, and both ranks of hex8 3x3x4 and
    hex27 2x2x4 split in two (ghost columns, faces with unowned nodes, and one added face without an owned node),
    thermo numbering and the k_TT graph derived from the structural graph as fcg.TsiGraph does: every
    owned face node has exactly one surface row and the rows ascend; the incidences of a row are exactly
    the (face, local node) pairs of its node, faces ascending; the compact columns are the union of the
    faces' columns, ascending and unique; s_pos lies in the row of the k_TT graph and names the column;
    every slot leads back to its node's column; max_row is the longest compact row.  Row lengths by the
    node's place: hex8 3x3x3 side-interior and box-edge nodes 4 faces and 9 columns, a corner 3 faces and
    7; hex27 2x2x2 a face-centre node 9, mid-edge nodes 15, a side's centre and a box edge's middle node
    25, a corner 19.  (The lengths 15 and 19 belong to hex27: a hex8 box has no node with them.)  The
    shape tables sum to 1 / 0 / 0 per Gauss point and the weights to 4.  A node id outside the range, a
    repeated node, n_faces < 0 and a face whose coupling the k_TT graph lacks return FCG_ERR_ARG with the
    face in the message; an empty face list is a surface without rows."""
    exe = _build(str(tmp_path / f"tsi_surface_plan_check_{name}"), extra)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout, p.stdout + p.stderr
    print(p.stdout)
