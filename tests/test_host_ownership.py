"""Ownership by type (csrc/sns_devbuf.h) on the host: DevBuf over a CPU allocator, under AddressSanitizer with leak detection."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_ownership_under_sanitizers(tmp_path):
    """tests/devbuf_main.cpp: a stand-alone program that defines the allocator functions behind DevBuf over malloc / free with a
    byte counter.  alloc twice frees the first allocation; move construction empties the source; move assignment frees the
    target; self-move is harmless; a growing std::vector<DevBuf<double>> and a std::deque of a struct of DevBufs that grows under
    a live reference keep the counter right; a failing allocator leaves the buffer null and returns SNS_E_HIP; the counter is 0
    at exit.  Leak detection is ON: a leak is what this guards against."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "devbuf_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc"),
                            os.path.join(ROOT, "tests", "devbuf_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert "devbuf: ok, live bytes at exit 0" in run.stdout and "ERROR" not in run.stderr
