"""The oracle pinned against the reference's own code where it compiles without its external libraries.

Only System/Random.cpp builds that way (OpenCV, Eigen, PCL, g2o are absent): `make -C oracle ref`
compiles it into oracle/_ref where the reference is available.  The reference seeds with time(NULL) once
(Random::initSeed, :8-14); after that first call, srand(seed) on the same libc fixes the stream, so randomInt
(:16-21) is compared draw for draw with the oracle's restatement (orc_random_int on the restated glibc TYPE_3
rand) that every RansacSE3 sample is drawn from (Solver/SolverSE3.cpp:136-149).

The reference's draws are recorded in tests/golden/random_ref.npz (tests/make_golden.py random_ref), so the
comparison runs everywhere; where oracle/_ref is built, the live library is compared with the record too."""
import ctypes as C
import os

import numpy as np
import pytest

from make_golden import RANDOM_REF_DRAWS, RANDOM_REF_RANGES, RANDOM_REF_SEEDS, random_ref_draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "librandom_ref.so")


@pytest.fixture(scope="module")
def recorded():
    g = np.load(os.path.join(ROOT, "tests", "golden", "random_ref.npz"))
    assert g["seeds"].tolist() == RANDOM_REF_SEEDS and [tuple(r) for r in g["ranges"].tolist()] == RANDOM_REF_RANGES
    assert g["draws"].shape == (len(RANDOM_REF_SEEDS), len(RANDOM_REF_RANGES), RANDOM_REF_DRAWS)
    return g["draws"]


@pytest.mark.parametrize("seed", RANDOM_REF_SEEDS)
@pytest.mark.parametrize("lo,hi", RANDOM_REF_RANGES)
def test_random_int_matches_reference(oracle, recorded, seed, lo, hi):
    want = recorded[RANDOM_REF_SEEDS.index(seed), RANDOM_REF_RANGES.index((lo, hi))].tolist()
    if os.path.exists(REF_SO):   # the reference's own code, live, where it was compiled
        assert random_ref_draws(REF_SO, seed, lo, hi) == want
    r = oracle.rng(seed)
    f = oracle.lib().orc_random_int
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int]
    got = [f(C.addressof(r), lo, hi) for _ in range(RANDOM_REF_DRAWS)]
    assert got == want
    assert all(lo <= v <= hi for v in got)
