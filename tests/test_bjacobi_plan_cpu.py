"""The host planner of the block-Jacobi layout (csrc/bjacobi_plan.hpp) against the layout's naive definition:
tests/bjacobi_plan_check.cpp, a stand-alone program on the header's host part, built here with the address and undefined-behaviour
sanitizers and run.  Its cases: n = 1; block sizes 1, 3, 5, 17 and 32, with and without a ragged last block; sizes cycling 1 .. 32; a
slice filled to exactly 64; a block that would straddle a slice and must start the next; no blocks at all; and the refusals of a
malformed block_ptr.  Per case: the slices' first rows, row counts and bases, the slot count, every position's code, every entry's
slot (the formula, inside its slice, no slot twice)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_matches_the_naive_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bjacobi_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "sprsolve_amd", "csrc"),
                            os.path.join(ROOT, "tests", "bjacobi_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr                  # (the undefined-behaviour sanitizer reports and goes on)
