"""The host utilities of csrc/gb_common.h -- gb::parallel, gb::thread_count, gb::thread_ws and
gb::round_up -- through the stand-alone tests/cpp/hostutil_check.cpp, which makes no HIP call."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc") or os.path.exists("/dev/kfd"),
                    reason="needs make and hipcc, and runs on machines without a GPU only")
def test_hostutil_sanitize():
    """`make hostutil-sanitize`: the program under the address and undefined-behaviour sanitizers on the CPU."""
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run(["make", "-s", "hostutil-sanitize"], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
