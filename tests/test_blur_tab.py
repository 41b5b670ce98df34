"""CPU: the operand tables of the level blur on the matrix cores (csrc/blur_tab.h) and the arithmetic of its two
int8 products, emulated by tests/blur_tab_check.cpp (own main, the header only) and compared pixel by pixel with a
direct integer 7x7 REFLECT_101 blur.  Built with the host sanitizers; the level sizes of
tests/test_gpu_blur_tiles.py's shapes are passed on top of the program's own (the 640 x 480 pyramid, every
residue of w and h mod 32)."""
import os
import subprocess

from conftest import ROOT
from test_gpu_blur_tiles import SHAPES, TALL, level_sizes, tiled


def test_blur_tables_and_arithmetic(tmp_path, oracle):
    levels = [wh for W, H, n, sc in SHAPES + [TALL] for wh in tiled(level_sizes(oracle, W, H, n, sc))]
    assert len(levels) >= 8, levels
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
