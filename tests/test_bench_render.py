"""CPU: bench.py renders its frames with one process per core; the bytes are those of the serial renderer, so the
benchmark's inputs are the same on every host and from run to run.  Run in a fresh child process: the renderer
forks, which the bench does before anything touches the GPU."""
import os
import subprocess
import sys

from conftest import ROOT

_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tools")
import bench
import synth
for n, seed, preset in ((4, 1000, "fr1"), (1, 1017, "lowtex")):
    a = bench.render_sequence(n, seed, preset)
    b = synth.sequence(n, seed=seed, preset=preset)
    assert a[0].dtype == np.uint8 and a[1].dtype == np.uint16 and a[0].shape == (n, 480, 640, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3], (n, seed, preset)
print("render ok")
"""


def test_parallel_render_equals_serial():
    env = dict(os.environ, OMP_NUM_THREADS="3")   # three renderer processes: 4 frames split 1 + 1 + 2; one frame: serial
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=110, env=env)
    assert out.returncode == 0 and "render ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
