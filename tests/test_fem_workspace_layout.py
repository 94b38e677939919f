"""The two FEM workspace layouts (csrc/fem_layout.h: `StepLayout` of tacex_fem_step, `BallLayout` of tacex_fem_ball_step) checked on the
CPU by a stand-alone C++ program, tests/fem_layout_check.cpp: every offset and total against the expressions the host layer used
before the layouts had a header of their own, region order, overlap, the end of the last region and alignment, for
V in {4, 495, 2232} x T in {1, 1920} x B in {1, 2, 3, 512} (the odd B: the int32 env order rounded up to doubles) and, for the ball
scene, (nv, nt) in {(4, 4), (42, 80)}.  The header is plain C++17: a host compiler builds it without HIP."""
import re
import shutil
import subprocess

import pytest
from conftest import REPO


def _compiler():
    for cand in ("c++", "g++", "clang++"):
        if shutil.which(cand):
            return [shutil.which(cand)]
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and shutil.which(cand):
            return [cand, "-x", "c++"]
    pytest.fail("no C++ compiler found (c++, g++, clang++ or hipcc)")


def test_workspace_layouts_are_what_the_host_layer_used(tmp_path):
    exe = tmp_path / "fem_layout_check"
    cmd = _compiler() + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{REPO / 'tacex_amd' / 'csrc'}",
                         str(REPO / "tests" / "fem_layout_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    # 3 V x 2 T x 4 B step layouts + as many ball layouts for each of the two bodies
    assert "72 layouts checked, 0 failures" in r.stdout, r.stdout


def test_no_workspace_arithmetic_outside_the_layout_header():
    """The host layer (everything from `struct tacex_fem_ctx` on) takes sizes and offsets from the layout structs: it never calls the
    per-env block sizes itself.  (The kernels above it keep their per-env uses.)"""
    src = (REPO / "tacex_amd" / "csrc" / "fem_kernels.hip").read_text()
    host = src[src.index("struct tacex_fem_ctx"):]
    assert "newton_ws_doubles(" not in host and "ball_ws_doubles(" not in host
    assert "dev_nwt" not in src
    # the kernel headers the translation unit includes (fem_ball.h is older than the split and indexes its env block in its kernel): one
    # of them also holds host code - the LDS sizes of the CU-resident kernel - and that one stays clear of the block sizes as well
    csrc = REPO / "tacex_amd" / "csrc"
    headers = [h for h in re.findall(r'^#include "(fem_\w+\.h)"', src, flags=re.M) if h not in ("fem_layout.h", "fem_ball.h")]
    assert len(headers) >= 6, headers
    with_host_code = [h for h in headers if re.search(r"^(static|inline)\s|__host__", (csrc / h).read_text(), flags=re.M)]
    assert "fem_newton_lds.h" in with_host_code, with_host_code
    for h in with_host_code:
        code = re.sub(r"//[^\n]*", "", (csrc / h).read_text())  # (comments may name the functions)
        assert "newton_ws_doubles(" not in code and "ball_ws_doubles(" not in code, h
