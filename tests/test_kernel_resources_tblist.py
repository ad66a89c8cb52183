"""cvd_decode_tblist.hip compiled for gfx950 with the library's flags: one kernel for every code
shape ((m = 1..8) x (n = 2, 3)) at every list width (2, 4, 8) and nothing else, none of them with
scratch; the VGPRs, the LDS and the occupancy of each are printed (pytest -s).  The static LDS is
the exchange buffer above 64 states (the tile of decisions is dynamic)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "detecting-convolutional-codes-via-markovian-statistics_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not shutil.which(HIPCC), reason="ROCm hipcc not present")
def test_tblist_kernels_no_scratch(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "cvd_decode_tblist.o" in re.search(r"^OBJS := (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^cvd_decode_tblist\.o:", mk, re.M)
    flags = (re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
             + re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split())
    out = subprocess.run([HIPCC, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "cvd_decode_tblist.hip",
                          "-o", str(tmp_path / "cvd_decode_tblist.o")], cwd=CSRC, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        field = lambda f: int(re.search(re.escape(f) + r": (\d+)", b).group(1))
        vgprs, scratch = field(" VGPRs"), field("ScratchSize [bytes/lane]")
        occ, lds = field("Occupancy [waves/SIMD]"), field("LDS Size [bytes/block]")
        inst = re.search(r"viterbi_frames_tblist_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", name)
        assert inst, name
        m, n, LL = (int(g) for g in inst.groups())
        print(f"m={m} n={n} L={LL}: VGPRs {vgprs}, scratch {scratch}, static LDS {lds} bytes, occupancy {occ} waves/SIMD")
        assert scratch == 0, (name, b)
        assert occ >= 1
        assert (m, n, LL) not in seen
        seen[(m, n, LL)] = vgprs
    assert sorted(seen) == [(m, n, LL) for m in range(1, 9) for n in (2, 3) for LL in (2, 4, 8)]
