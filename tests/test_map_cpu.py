"""No device: the allocator and the owner of the maps the library hands out (csrc/lsfm_map.cpp, lsfm_map.hpp) and host_system_of
(lsfm_system.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer with leak detection, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_alloc_under_asan_ubsan():
    """tests/sanitize/sanitize_map.cpp: map_alloc at (m, n, nU, nW) = (1, 0, 0, 0), (2, 1, 1, 1), (3, 2, 4, 3), with and without pose_origin
    and a map to copy the scalars from; MapOut with and without give(); lsfm_map_release twice; host_system_of without features."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sanitize_map")
    csrc = os.path.join(ROOT, "linearsfm_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "sanitize", "sanitize_map.cpp"), os.path.join(csrc, "lsfm_map.cpp"), os.path.join(csrc, "lsfm_system.cpp")]
    deps = srcs + [os.path.join(csrc, "lsfm_map.hpp"), os.path.join(csrc, "lsfm_system.hpp"), os.path.join(ROOT, "include", "lsfm.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                               "-o", exe] + srcs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "sanitize_map: ok (12 maps)" in p.stdout, (p.stdout[-2000:], p.stderr[-6000:])
