"""CPU: the operand plane, LDS image, fragment plane, MFMA C/D and attention-ready slab layouts of regennet_amd/csrc/rgn_layout.h, checked exhaustively on the host.

tests/layout_check.cpp includes only that header - the text the kernels and the packer compile - and checks over small domains that the image chunk
map is a bijection, that a DMA lane fetching the chunk the source rule names fills the image as the readers expect, that an element written through the
accumulator-run offset is read back through the fragment offset, that the plane and fragment-plane offsets are bijections equal to the packer's
former literals, the granule / lane rule of the fragment plane, that the C/D row map covers a tile, and that the attention-ready slab offset is a bijection in which a
token row of a head is dh contiguous elements and a head's slab starts at its base."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_layout_header_passes_its_host_check(tmp_path):
    exe = str(tmp_path / "layout_check")
    cc = subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "regennet_amd", "csrc"),
                         os.path.join(ROOT, "tests", "layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "layout ok" in r.stdout
