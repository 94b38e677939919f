"""The Taxim workspace layouts (csrc/taxim_layout.h: `PassLayout` of the render workspace, `ShadowLayout` of the shadow branch's regions
behind it, `obs_resize_floats` of the observation scratch) checked on the CPU by a stand-alone C++ program, tests/taxim_layout_check.cpp:
every offset and total against the expressions the host layer used before the layouts had a header of their own, region order, overlap,
256-byte alignment, the end of the last region, and that a chunk's regions lie in front of the whole batch's contact rows, for
(H, W) in {(16,16), (17,20), (240,320), (480,640)} (17x20: B*H*W*4 misses the alignment) x B in {1, 2, 63, 64, 65, 512, 2048} (64 / 65 cross
the alignment of the B-sized vectors; 2048 frames of 480x640 pass 2^31 bytes).  The header is plain C++17: a host compiler builds it."""
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
    exe = tmp_path / "taxim_layout_check"
    cmd = _compiler() + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{REPO / 'tacex_amd' / 'csrc'}",
                         str(REPO / "tests" / "taxim_layout_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    # 4 sizes x 7 B x (pass layout + shadow layout + 3 observation sizes)
    assert "140 layouts checked, 0 failures" in r.stdout, r.stdout


def test_no_workspace_arithmetic_outside_the_layout_header():
    """The C API takes every workspace size and address from the layout structs, and the observation scratch bound from
    `obs_resize_floats`: no alignment helper, no rows-region helper and no spelling of max(H * ow, oh * W) of its own."""
    src = (REPO / "tacex_amd" / "csrc" / "tacex_capi.hip").read_text()
    assert "align_up(" not in src and "workspace_rows" not in src
    assert "H * obs_w" not in src
    # either product of the max, whatever the observation size is called
    assert not re.search(r"\bH\s*\*\s*(p\.|p->)?(obs_w|ow)\b", src)
    assert not re.search(r"\b(obs_hh|obs_h|oh)\s*\*\s*(c->|p\.)?W\b", src)
    for name in ("PassLayout(", "ShadowLayout(", "obs_resize_floats("):
        assert name in src
