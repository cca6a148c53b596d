"""
plan_columns (phiflow_amd/csrc/column_march.hpp) against the launch-plan formulas it replaced: tools/column_plan_sweep.cpp holds them as they stood and compares over
lattices of 1..300 x 1..40 x 1..200 samples, both targets, forced chunks, one chunk, the tile shapes of the vector divergence. The forced chunk in particular changes
no output of any kernel -- it only distributes the planes -- so no parity test can see whether it is honoured; this one does. Host code, no GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_matches_the_formulas_it_replaced(tmp_path):
    exe = str(tmp_path / "column_plan_sweep")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "tests", "hipemu", "include"), "-x", "c++",
                    os.path.join(ROOT, "tools", "column_plan_sweep.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith(", 0 differences"), r.stdout[-2000:]
