"""The plan of the on-chip batch solvers (csrc/batch_plan.hpp) against the numbers the header states: tests/batch_plan_check.cpp,
a stand-alone program on the header alone, built here with the address and undefined-behaviour sanitizers and run.  Its cases: B(n)
at 0, 1, 64, 65, 128, 129, 256, 257 and 1024 and its shape up to 5000; the vectors, LDS bytes and row caps of both solvers for all
four scalar types, each cap's vectors within 64 KiB and the next multiple of 64 rows beyond it; the codes it does not know."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_matches_the_statement_under_sanitizers(tmp_path):
    exe = str(tmp_path / "batch_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "sprsolve_amd", "csrc"),
                            os.path.join(ROOT, "tests", "batch_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr                  # (the undefined-behaviour sanitizer reports and goes on)
