"""CPU: csrc/eigen3.hpp's product formulation of the normals' finish (one copy
of each FastEigen3x3 arm chosen by selects, quotients of a shared divisor
through one reciprocal) against its *_ref text, on the host.

tests/eigen_exact_main.cpp is built with the host compiler as a stand-alone
program and compares the two bit for bit (memcmp: signed zeros and NaN
payloads count) over
  * > 5M quotients: moment sums over small integer counts, random pairs (a
    quarter with near-all-ones mantissas), the whole exponent range (quotients
    and residuals that overflow or underflow), the guard's edges, and every
    pair of special values (+-0, subnormals, infinities, NaNs, ...);
  * > 2M covariances through the solver: random SPD, rank 1 and 2, all zero,
    diagonal, two and three equal eigenvalues (half_det = +-1), half_det = 0,
    imax ties and |e0[0]| == |e0[1]|, indefinite matrices, entries scaled by
    2^+-40 and beyond;
  * moment sets of k in {3, 4, 30, 31, 64} float32 points: unit cube, 5e5
    offset, identical, collinear, coplanar on an axis plane.
No case may differ and none is excluded."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open3d-py-extension_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "eigen_exact_main.cpp")

QUOTIENT_FAMILIES = ("quot_small_int", "quot_random", "quot_full_range", "quot_guard_edges", "quot_special")
SOLVER_FAMILIES = ("solver_spd", "solver_rank12", "solver_zero_diag", "solver_equal_eigs", "solver_half_det_zero",
                   "solver_ties", "solver_indefinite")
MOMENT_FAMILIES = ("mom_unit_cube", "mom_offset_5e5", "mom_identical", "mom_collinear", "mom_axis_plane")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("eigen_exact") / "eigen_exact")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, MAIN, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    fam = {m.group(1): (int(m.group(2)), int(m.group(3)))
           for m in re.finditer(r"^(\w+) cases=(\d+) diff=(\d+)$", p.stdout, re.M)}
    fast = re.search(r"^quot_fast_path=(\d+)$", p.stdout, re.M)
    return {"rc": p.returncode, "out": p.stdout, "fam": fam, "fast": int(fast.group(1)) if fast else 0}


def test_every_family_ran_and_none_differs(report):
    print(report["out"])
    fam = report["fam"]
    for name in QUOTIENT_FAMILIES + SOLVER_FAMILIES + MOMENT_FAMILIES:
        assert name in fam and fam[name][0] > 0, name
    differing = {k: v for k, v in fam.items() if v[1]}
    assert not differing, differing
    assert report["rc"] == 0


def test_case_counts(report):
    fam = report["fam"]
    nq = sum(fam[k][0] for k in QUOTIENT_FAMILIES)
    ns = sum(fam[k][0] for k in SOLVER_FAMILIES + MOMENT_FAMILIES)
    assert nq >= 5_000_000, nq
    assert ns >= 2_000_000, ns
    for k in MOMENT_FAMILIES:
        assert fam[k][0] >= 100_000, k
    # the three-instruction form is what most quotients went through (the
    # comparison is not ordinary division against itself), and the guarded
    # remainder is there too
    assert 0.5 * nq < report["fast"] < nq, (report["fast"], nq)
