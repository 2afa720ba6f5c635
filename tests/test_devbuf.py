"""gb::DevBuf / gb::PinnedBuf (csrc/gb_common.h), the owning grow-only buffers behind every leg's
device and pinned memory, through the stand-alone tests/cpp/devbuf_check.cpp: the allocation-failure
path where no device exists (a failed reserve leaves the buffer empty, sets the error, and can be
repeated and destroyed), the success path on a device."""
import os
import subprocess

import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "tests", "_build", "devbuf_check")


def _run(*args):
    if not os.path.exists(BIN):
        # the program is a build product that lies under tests/: where that folder was replaced after
        # the build it is gone, so make it again from the library that the build left (a few seconds)
        target = os.path.relpath(BIN, ROOT)
        m = subprocess.run(["make", "-s", target], cwd=ROOT, capture_output=True, text=True, timeout=900)
        if m.returncode != 0 or not os.path.exists(BIN):
            pytest.fail(f"{BIN} not built and `make {target}` failed:\n" + m.stdout[-2000:] + m.stderr[-2000:])
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def test_reserve_failure_leaves_buffer_empty():
    r = _run()
    if r.returncode == 77:
        pytest.skip("a device is present: allocations succeed here")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DevBuf: failure path ok" in r.stdout and "PinnedBuf: failure path ok" in r.stdout


@pytest.mark.gpu
def test_reserve_grow_and_move_on_device():
    r = _run("--device")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DevBuf: success path ok" in r.stdout and "PinnedBuf: success path ok" in r.stdout
