"""The owning buffer types of rgbd-slam_amd/csrc/devmem.h on their failure paths (tests/devmem_check.cpp,
mode "fail"): a request of 2^60 bytes fails on every machine, and without a device every allocation does."""
import os
import subprocess

import pytest

from conftest import ROOT


def build_check(out_dir):
    """tests/devmem_check.cpp (its own main, includes devmem.h only) compiled as host code with hipcc."""
    exe = os.path.join(str(out_dir), "devmem_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "rgbd-slam_amd", "csrc"),
           os.path.join(ROOT, "tests", "devmem_check.cpp"), "-o", exe, "-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("devmem"))


def test_failed_allocations_leave_buffers_empty(check_exe):
    """After a failed reserve / alloc: get() == nullptr and capacity() == 0, a second reserve asks the allocator
    again, moves from empty and failed buffers leave both sides empty; an Event that could not be created
    (no device) reports the error and its destructor destroys nothing."""
    r = subprocess.run([check_exe, "fail"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devmem_check fail: all checks passed" in r.stdout, r.stdout
