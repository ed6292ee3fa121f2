"""The tile schedule of the persistent conv kernels (csrc/conv_schedule.h) by itself, on the host: tests/tile_schedule_walk.cpp
includes only that header, walks every workgroup of 972 launches (N in {1, 2, 3} x nine tile grids x nine grid sizes --
multiples of 8 and not -- x interior pass allowed or not x the 4x8x8 and the 8x8x8 tile) and checks that every tile of the
launch is produced exactly once and in the right pass, that a workgroup's counts add up, that int_next equals
int_init(k + WPX) and that `tile` is the raster index.  Built with AddressSanitizer + UndefinedBehaviorSanitizer where
the host compiler links them (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "tile_schedule_walk.cpp")
INC = os.path.join(ROOT, "h-denseformer_amd", "csrc")


def _host_compiler():
    for cxx in (shutil.which("g++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and os.path.exists(cxx):
            return cxx
    return None


def test_tile_schedule_walk(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    exe = str(tmp_path / "tile_schedule_walk")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:   # a compiler without the sanitizer runtimes; a real error fails this build too
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    w = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    out = w.stdout + w.stderr
    assert w.returncode == 0, out[-3000:]
    assert out.strip().splitlines()[-1] == "PASS 972", out[-3000:]
