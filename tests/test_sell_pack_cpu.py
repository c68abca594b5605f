"""The host packer of the sliced-row layout (csrc/sell.hpp, shared by ILU(0) and AMG) against the layout's naive definition:
tests/sell_pack_check.cpp, a stand-alone program on the header's host part, built here with the address and undefined-behaviour
sanitizers and run.  Its cases: the natural order with 0, 1, 63, 64, 65 and 129 rows (row lengths 0 .. 9; one slice of empty rows
only) and level-major positions with levels of 1, 64 and 65 rows (part-filled slices, empty lanes); per case the row lengths, the
slice bases, the slot count, every entry's slot, and column 0 / all-zero bits in every padded slot."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packer_matches_the_naive_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sell_pack_check")
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "sprsolve_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sell_pack_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr                  # (the undefined-behaviour sanitizer reports and goes on)
