"""CPU: the rectangular entry of the EMD solver (csrc/emd_simplex.hpp with Tr != Tc, the code the
masked pair kernel of stag.hip runs) under AddressSanitizer + UndefinedBehaviorSanitizer.  A
stand-alone host program (tests/native/emd_rect_sanitize_main.cpp with tests/native/
emd_rect_host.cpp) is built with -fsanitize=address,undefined exactly as tests/test_sanitize_cpu.py
builds its program and driven over random rectangular problems with 1..40 rows and columns; any
sanitizer report or a wrong / non-terminating solve fails the test.  Host only: nothing is
loaded into Python, and the GPU code itself cannot be sanitized on this pool."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emd_rect_solver_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "emd_rect_sanitize"
    src = [os.path.join(ROOT, "tests", "native", "emd_rect_host.cpp"),
           os.path.join(ROOT, "tests", "native", "emd_rect_sanitize_main.cpp")]
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=all", "-o", str(exe)] + src
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "160 problems, 0 bad" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
