"""Seeded inputs of the plain FAST extractor's tests (test infrastructure): the 640 x 480 frames whose corner-count
regimes are pinned by tests/test_fast_model.py, so that tests/test_gpu_fast.py cannot pass on an easy one,
and the model's frames over them, computed once per session and left unchanged."""
import functools

import numpy as np

from conftest import synth_seq
import fast_model as F
import oracle_lib as O

# name -> (strict maxima at t = 1, corners at t = 10, kept by retainBest(1000))
COUNTS = {"fr1": (17147, 13715, 1016), "fr2": (17234, 13747, 1007), "fr3": (15901, 11504, 1027),
          "lowtex": (11937, 656, 656), "noise": (31945, 31337, 1001), "binary": (3956, 3956, 3956)}
_PRESETS = {"fr1": 3, "fr2": 3, "fr3": 11, "lowtex": 7}


@functools.lru_cache(maxsize=None)
def _noise():
    rs = np.random.RandomState(5)
    uniform = rs.randint(0, 256, (480, 640)).astype(np.uint8)
    binary = (rs.randint(0, 2, (480, 640)) * 255).astype(np.uint8)   # every corner scores 254
    return uniform, binary


@functools.lru_cache(maxsize=None)
def frame(name, f=0):
    """(bgr [480, 640, 3], depth [480, 640] u16, cam) of frame f of a rendered preset, or of a pattern over fr1's depth."""
    if name in _PRESETS:
        bgr, depth, _, cam = synth_seq(5, seed=_PRESETS[name], preset=name)
        return bgr[f], depth[f], cam
    _, depth, _, cam = synth_seq(5, seed=3, preset="fr1")
    g = {"noise": _noise()[0], "binary": _noise()[1], "flat": np.full((480, 640), 128, np.uint8)}[name]
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)), depth[0], cam


@functools.lru_cache(maxsize=None)
def gray(name, f=0):
    return O.gray(frame(name, f)[0])


@functools.lru_cache(maxsize=None)
def model_frame(name, descriptor="brief", f=0, nfeatures=1000, threshold=10):
    bgr, depth, cam = frame(name, f)
    return F.Extractor(F.params(nfeatures, threshold, descriptor)).frame(bgr, depth, cam)
