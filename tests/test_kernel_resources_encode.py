"""cvd_encode.hip compiled for gfx950 with the library's flags: no kernel has scratch; the VGPRs,
the LDS and the occupancy of each are printed (pytest -s).  Nothing else is inspected."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "detecting-convolutional-codes-via-markovian-statistics_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not shutil.which(HIPCC), reason="ROCm hipcc not present")
def test_encode_kernels_no_scratch(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = (re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
             + re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split())
    out = subprocess.run([HIPCC, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "cvd_encode.hip",
                          "-o", str(tmp_path / "cvd_encode.o")], cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        field = lambda f: int(re.search(re.escape(f) + r": (\d+)", b).group(1))
        vgprs, scratch = field(" VGPRs"), field("ScratchSize [bytes/lane]")
        occ, lds = field("Occupancy [waves/SIMD]"), field("LDS Size [bytes/block]")
        print(f"{name}: VGPRs {vgprs}, scratch {scratch}, LDS {lds} bytes, occupancy {occ} waves/SIMD")
        assert scratch == 0, (name, b)
        seen += 1
    assert seen, "no kernel was reported"
