"""Regenerate tests/golden/*.npz from the oracle (run on CPU: python tests/make_golden.py).

Inputs are not stored: they are regenerated from (seed, preset) by tools/synth.py (integer
hashing + float64, deterministic); bgr_sum guards against generator drift.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import oracle_lib as O  # noqa: E402
import synth  # noqa: E402


def main():
    out = os.path.join(HERE, "golden")
    os.makedirs(out, exist_ok=True)
    bgr, depth, _, cam = synth.sequence(2, seed=3, preset="fr1")
    p, oc = O.orb_params(1000), O.camera(cam)
    f0 = O.frame(bgr[0], depth[0], p, oc)
    f1 = O.frame(bgr[1], depth[1], p, oc)
    np.savez_compressed(os.path.join(out, "frame_fr1_seed3.npz"), bgr_sum=np.int64(bgr[0].astype(np.int64).sum()),
                        kps=f0["kps"], desc=f0["desc"], xyz=f0["xyz"])
    m = O.match(f0["desc"], f1["desc"], np.zeros(len(f0["kps"]), np.uint8), f0["xyz"][:, 2], f1["xyz"][:, 2], 0.9)
    ok, T, inl, rm = O.ransac_se3(f0["xyz"], f1["xyz"], m, O.ransac_params(), O.rng(42), O.Sticky())
    np.savez_compressed(os.path.join(out, "pair_fr1_seed3.npz"), matches=m, T21=T, inliers=inl,
                        rmse=np.float32(rm))
    print("golden written:", len(f0["kps"]), "kps,", len(m), "matches,", len(inl), "inliers")
    # Extractor(SVO, BRIEF, NORMAL) on the same frame, default BRIEF table (orc_svo.cpp)
    s0 = O.svo_frame(bgr[0], depth[0], O.svo_params(), oc)
    np.savez_compressed(os.path.join(out, "svo_frame_fr1_seed3.npz"), bgr_sum=np.int64(bgr[0].astype(np.int64).sum()),
                        kps=s0["kps"], desc=s0["desc"], xyz=s0["xyz"], pattern=O.brief_default_pattern())
    print("svo golden written:", len(s0["kps"]), "kps")
    random_ref(out)


RANDOM_REF_SEEDS = [1, 7, 42, 12345, 2 ** 31 + 5]
RANDOM_REF_RANGES = [(0, 999), (0, 3), (5, 5), (-10, 10), (0, 2 ** 20)]
RANDOM_REF_DRAWS = 3000


def random_ref_draws(ref_so, seed, lo, hi, n=RANDOM_REF_DRAWS):
    """n draws of the reference's Random::randomInt(lo, hi) after srand(seed) (oracle/_ref/librandom_ref.so, the
    reference's System/Random.cpp compiled by `make -C oracle ref`)."""
    import ctypes as C
    ref = C.CDLL(ref_so)
    libc = C.CDLL("libc.so.6")
    rint = ref._ZN6Random9randomIntEii
    rint.restype = C.c_int
    rint.argtypes = [C.c_int, C.c_int]
    ref._ZN6Random8initSeedEv()   # the reference's one-time srand(time(NULL)); later calls do not reseed
    libc.srand(C.c_uint(seed))
    return [rint(lo, hi) for _ in range(n)]


def random_ref(out=os.path.join(HERE, "golden")):
    """random_ref.npz: what the reference's randomInt returned, recorded where the reference is available, so
    tests/test_oracle_ref.py needs no reference at test time."""
    ref_so = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "librandom_ref.so")
    if not os.path.exists(ref_so):
        print("random_ref.npz kept as it is: oracle/_ref not built (make -C oracle ref)")
        return
    draws = np.array([[random_ref_draws(ref_so, s, lo, hi) for lo, hi in RANDOM_REF_RANGES] for s in RANDOM_REF_SEEDS],
                     np.int32)
    np.savez_compressed(os.path.join(out, "random_ref.npz"), seeds=np.array(RANDOM_REF_SEEDS, np.int64),
                        ranges=np.array(RANDOM_REF_RANGES, np.int64), draws=draws)
    print("random_ref golden written:", draws.shape)


if __name__ == "__main__":
    main()
