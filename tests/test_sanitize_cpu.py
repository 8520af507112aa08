"""AddressSanitizer + UndefinedBehaviorSanitizer over the code that runs on the host: the library's reader / writers
(linearsfm_amd/csrc/lsfm_io.cpp), its ordering + symbolic factorisation (lsfm_symbolic.cpp), its checks of a system from host arrays
(lsfm_system.cpp), the release of its maps (lsfm_map.cpp) and the oracle (oracle/lsfm_oracle.c,
lsfm_chol.c), built with -fsanitize=address,undefined -fno-sanitize-recover=all into tests/sanitize/_build/sanitize_host and run over
small join trees (tests/sanitize/sanitize_host.cpp says what it exercises).  GPU sanitizers are not available on the pool; the device
code is covered by the parity tests instead."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from linearsfm_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "sanitize_host.cpp")
OUT = os.path.join(ROOT, "tests", "sanitize", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def san_exe():
    if shutil.which("g++") is None or shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "sanitize_host")
    srcs = [SRC, os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_io.cpp"), os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_symbolic.cpp"),
            os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_system.cpp"), os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_map.cpp"),
            os.path.join(ROOT, "oracle", "lsfm_oracle.c"), os.path.join(ROOT, "oracle", "lsfm_chol.c")]
    deps = srcs + [os.path.join(ROOT, "oracle", f) for f in ("lsfm_oracle.h", "lsfm_solve_num.inc", "lsfm_chol_num.inc")] + \
        [os.path.join(ROOT, "include", "lsfm.h"), os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_symbolic.hpp"),
         os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_system.hpp"), os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_map.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        objs = []
        for s in srcs:
            o = os.path.join(OUT, os.path.basename(s) + ".o")
            cc = ["gcc", "-std=gnu99"] if s.endswith(".c") else ["g++", "-std=c++17"]
            subprocess.check_call(cc + SAN + ["-fopenmp", "-pthread", "-c", s, "-o", o])
            objs.append(o)
        subprocess.check_call(["g++"] + SAN + ["-fopenmp", "-pthread", "-o", exe] + objs + ["-lm"])
    return exe


@pytest.mark.parametrize("typ,N,npf,vis,seed", [("Stereo", 9, 6, 4, 3), ("Monocular", 7, 7, 4, 5), ("Stereo", 1, 5, 4, 1)])
def test_host_code_under_asan_ubsan(oracle, san_exe, tmp_path, typ, N, npf, vis, seed):
    mono = typ == "Monocular"
    maps = (synth.make_mono_set if mono else synth.make_stereo_set)(N, new_per_frame=npf, vis=vis, seed=seed)
    import ctypes as C
    for k, m in enumerate(maps):
        g = oracle.dict_to_map(oracle.localmap_to_dict(m))
        assert oracle.lib().orc_write_map(str(tmp_path / f"localmap_{k + 1}.txt").encode(), int(mono), C.byref(g)) == 0
        oracle.lib().orc_map_free(C.byref(g))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="3")
    p = subprocess.run([san_exe, str(tmp_path), str(N), typ], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert "sanitize_host: ok" in p.stdout
