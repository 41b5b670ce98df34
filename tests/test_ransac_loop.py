"""CPU: the RANSAC loop rules that the host control and the kernels share (csrc/pnp_dev.h: cv::RNG, getSubset, the
accept step, RANSACUpdateNumIters; csrc/ransac_dev.h: sampleMatches, RansacSE3's accept rule), compiled as host code
into tests/ransac_loop_check.cpp and held to the oracle's own copies (orc_update_num_iters, orc_cvrng_uniform_stream,
the restated glibc rand()).

RansacSE3::sampleMatches: neither tests/chain_model.py nor tests/lane_sort_model.py holds a sampler model and
orc_solver exports none, so the check is against the restatement of tests/ransac_se3_cases.py with a set over the
oracle's orc_random_int, together with the properties (ascending, distinct, n == SS, two draws per attempt)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ransac_se3_cases import sample_model

COUNTS = [5, 6, 61, 400, 4096]
MAX_ITERS = [1, 2, 24, 500, 3000]
SEED = (1 << 64) - 1


def build_check(out_dir, extra=()):
    """tests/ransac_loop_check.cpp (its own main, the two headers only) as host code, the product's fp flags."""
    exe = os.path.join(str(out_dir), "ransac_loop_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-fno-fast-math", *extra, "-I",
           os.path.join(ROOT, "rgbd-slam_amd", "csrc"), os.path.join(ROOT, "tests", "ransac_loop_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("ransac_loop"))


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def test_update_num_iters_matches_oracle(oracle, check_exe):
    """Every (count, g, maxIters) of count 5..600, g 5..count (about 900k calls) by one checksum per count; a count
    whose checksum differs is dumped and its first differing call named.  Then the clamps of p and ep."""
    f = oracle._pnp_sigs().orc_update_num_iters
    lines = run(check_exe, "uni")
    sums = {int(l.split()[1]): int(l.split()[2]) for l in lines if l.startswith("uni ")}
    assert sorted(sums) == list(range(5, 601))
    for count in range(5, 601):
        want = np.array([f(0.85, (count - g) / count, 5, mi) for g in range(5, count + 1) for mi in MAX_ITERS], np.uint64)
        cs = int((want * np.arange(1, len(want) + 1, dtype=np.uint64)).sum(dtype=np.uint64))
        if cs != sums[count]:
            got = [int(x) for x in run(check_exe, "unidump", str(count))]
            k = next(i for i, (a, b) in enumerate(zip(got, want.tolist())) if a != b)
            pytest.fail("count %d g %d maxIters %d: %d, oracle %d" % (count, 5 + k // 5, MAX_ITERS[k % 5], got[k], want[k]))
    clamps = [l.split() for l in lines if l.startswith("clamp ")]
    assert len(clamps) == 5 * 5 * 5
    for _, p, ep, mi, got in clamps:
        assert int(got) == f(float(p), float(ep), 5, int(mi)), (p, ep, mi)
    assert {(p, ep) for _, p, ep, _, _ in clamps} >= {("-1", "0"), ("0", "1"), ("1", "0"), ("2", "1.5")}


def oracle_stream(oracle, count, n):
    out = np.zeros(n, np.int32)
    oracle._pnp_sigs().orc_cvrng_uniform_stream(SEED, count, n, out)
    return out.tolist()


def test_cvrng_matches_oracle(oracle, check_exe):
    """20000 uniform(0, count) values from seed ~0: past the flag chain's 8192-entry table."""
    lines = run(check_exe, "rng")
    assert [int(l.split()[1].rstrip(":")) for l in lines] == COUNTS
    for l, count in zip(lines, COUNTS):
        got = [int(x) for x in l.split()[2:]]
        assert len(got) == 20000 and got == oracle_stream(oracle, count, 20000), count


def test_get_subset_matches_restatement(oracle, check_exe):
    """2000 subsets per count against getSubset restated over the oracle's stream: 5 indices, an index equal to
    an earlier one of the subset drawn again (count = 5 and 6: most draws are redraws)."""
    lines = run(check_exe, "subset")
    for l, count in zip(lines, COUNTS):
        got = [int(x) for x in l.split()[2:]]
        stream = iter(oracle_stream(oracle, count, 60000))
        want = []
        for _ in range(2000):
            idx = []
            while len(idx) < 5:
                v = next(stream)
                if v not in idx:
                    idx.append(v)
            want += idx
        assert got == want, count


def good_sequences():
    """Inlier counts per iteration for count = 400 (-1: no model): rising maxima, ties with maxGood, values <= 4,
    a late accept that ends the loop at once, never accepting, no model at all."""
    r = np.random.RandomState(7)
    n = 600
    seqs = [r.randint(-1, 151, n), r.choice([-1, 3, 4, 5, 100, 100, 120, 120, 121], n), r.randint(-1, 5, n),
            np.full(n, -1), np.where(np.arange(n) == 300, 200, r.randint(-1, 5, n)),
            np.where(np.arange(n) == 77, 5, r.randint(-1, 5, n)),   # the smallest count that is accepted, alone
            np.minimum(np.arange(n) // 3, 135) * (r.randint(0, 4, n) > 0) - 1]
    for it in (120, 250, 480):   # an accept in the last iteration of a span (evaluated = 8, 24, 56, 120, 248, 504)
        s = r.randint(-1, 5, n)
        s[it - 1] = 5
        s[it] = 90
        seqs.append(s)
    return [s.astype(int).tolist() for s in seqs]


def replay_model(oracle, good, count, iterations):
    """RANSACPointSetRegistrator::run's bookkeeping, restated; niters from the oracle's RANSACUpdateNumIters."""
    f = oracle._pnp_sigs().orc_update_num_iters
    it, niters, max_good, best = 0, iterations, 0, -1
    while it < niters and it < len(good):
        g = good[it]
        if g >= 0 and g > max(max_good, 4):
            max_good, best = g, it
            niters = f(0.85, (count - g) / count, 5, niters)
        it += 1
    return [it, niters, max_good, best]


SAMPLE_CASES = [(4, 4, 200), (10, 4, 200), (100, 4, 200), (2304, 4, 200), (8, 8, 100), (3, 4, 5)]


def se3_sequences():
    """(M, minTh, iters, [(n, err)]): falling errors with rising and tied inlier counts, invalid hypotheses
    (n = 0), counts under minTh, the two n += 10 steps and the > 0.8 break."""
    r = np.random.RandomState(11)
    out = []
    for M, top in [(100, 45), (100, 70), (100, 78), (100, 95), (37, 30), (100, 9)]:
        H = 200
        n = np.minimum(r.randint(0, top + 1, H), np.arange(H) // 2 + 5)
        n[r.randint(0, 5, H) == 0] = 0
        n[1::7] = n[0:-1:7]   # ties of the inlier count
        err = np.abs(r.normal(0, 1, H)) * np.linspace(3, 0.2, H)
        err[1::7] = np.minimum(err[1::7], err[0:-1:7])
        out.append((M, 10, 200, list(zip(n.tolist(), err.tolist()))))
    return out


def se3_model(M, min_th, iters, hyps):
    """SolverSE3.cpp:88-102 restated: float rmse, the reference's size() * 0.5 / 0.75 / 0.8 tests"""
    rmse, best_h, best_n, valid, h, n = np.float32(1e6), -1, 0, 0, 0, 0
    while n < iters:
        cnt, err = hyps[h]
        h += 1
        if cnt > 0:
            valid += 1
            if err <= float(rmse) and cnt >= best_n and cnt >= min_th:
                rmse, best_h, best_n = np.float32(err), h - 1, cnt
                if cnt > M * 0.5:
                    n += 10
                if cnt > M * 0.75:
                    n += 10
                if cnt > M * 0.8:
                    break
        n += 1
    return [h, best_h, valid, best_n, float(rmse)]


def test_loops_match_restatements(oracle, check_exe, tmp_path):
    """The PnP replay fed in one span and in spans of 8, 16, 32, ... gives the same (iter, niters, maxGood, best) as
    the restatement over orc_update_num_iters; sampleMatches the restatement's ids and rand() counts; RansacSE3's
    accept rule the restated loop's outcome."""
    goods, se3s, seed = good_sequences(), se3_sequences(), 12345
    rng = oracle.rng(seed)
    raw = [oracle.lib().orc_rng_rand(C.byref(rng)) for _ in range(30000)]
    with open(tmp_path / "cases.txt", "w") as f:
        for g in goods:
            f.write("good 400 500 " + " ".join(map(str, g)) + "\n")
        f.write("rand " + " ".join(map(str, raw)) + "\n")
        for M, SS, nh in SAMPLE_CASES:
            f.write("sample %d %d %d\n" % (M, SS, nh))
        for M, th, iters, hyps in se3s:
            f.write("se3 %d %d %d %d\n" % (M, th, iters, len(hyps)))
            f.writelines("%d %r\n" % (n, e) for n, e in hyps)
    lines = run(check_exe, "file", str(tmp_path / "cases.txt"))
    heads = [i for i, l in enumerate(lines) if l.startswith("case ")]
    blocks = [(lines[i].split()[1], lines[i + 1:j]) for i, j in zip(heads, heads[1:] + [len(lines)])]
    assert [k for k, _ in blocks] == ["good"] * len(goods) + ["sample"] * len(SAMPLE_CASES) + ["se3"] * len(se3s)
    accepted = 0
    for g, (_, body) in zip(goods, blocks):
        want = replay_model(oracle, g, 400, 500)
        one, spans = ([int(x) for x in l.split(":")[1].split()] for l in body)
        assert body[0].startswith("replay span 0:") and body[1].startswith("replay span 8:")
        assert one == spans == want, (one, spans, want)
        accepted += want[3] >= 0
    assert accepted >= 5 and any(replay_model(oracle, g, 400, 500)[3] < 0 for g in goods)
    for (M, SS, nh), (_, body) in zip(SAMPLE_CASES, blocks[len(goods):]):
        want = sample_model(oracle, seed, M, SS, nh)
        assert len(body) == nh
        for l, (ids, calls) in zip(body, want):
            head, _, tail = l.partition(":")
            got = [int(x) for x in tail.split()]
            assert [int(x) for x in head.split()] == [len(ids), calls] and got == ids, (M, SS, l, ids, calls)
            assert got == sorted(set(got)) and len(got) == (SS if M >= SS else 0)
    for (M, th, iters, hyps), (_, body) in zip(se3s, blocks[len(goods) + len(SAMPLE_CASES):]):
        h, best_h, valid, best_n, rmse = body[0].split()
        got = [int(h), int(best_h), int(valid), int(best_n), float.fromhex(rmse)]
        assert got == se3_model(M, th, iters, hyps), (M, got)
