"""CPU: the operand tables and the int8 arithmetic of the matrix-core level blur (csrc/blur_tab.h) at the level-0
sizes of tests/test_gpu_blur_level0.py's frames and at 640 x 480, emulated by tests/blur_tab_check.cpp and compared
pixel by pixel with a direct integer 7x7 REFLECT_101 blur.  Built and run as tests/test_blur_tab.py does it (own
main, the header only, host sanitizers)."""
import os
import subprocess

from conftest import ROOT
from test_gpu_blur_level0 import SHAPES, level_sizes


def test_level0_blur_tables_and_arithmetic(tmp_path, oracle):
    levels = [level_sizes(oracle, *s)[0] for s in SHAPES]
    assert levels == [s[:2] for s in SHAPES] and (640, 480) in levels, levels
    exe = os.path.join(str(tmp_path), "blur_tab_check")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "rgbd-slam_amd", "csrc"), os.path.join(ROOT, "tests", "blur_tab_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    args = [str(v) for wh in levels for v in wh]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last == f"OK sizes {8 + 64 + len(levels)} fails 0", last
