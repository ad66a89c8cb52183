"""Register budgets that let a generator wave sit beside the m = 6 detector's four waves on a
SIMD (512 VGPRs per SIMD lane, allocated in granules of 8): the detector
k1s as the JIT builds it for a model that does not walk (walk mode compiled out,
-DCVD_K1S_WALK=0) at <= 112 VGPRs, so that 4 x 112 leave 64; and the small form of the k = 1,
n = 2 generator at <= 64.  No scratch in either, and the generator block's LDS fits beside the
detector block's.  Compiled here as the JIT (csrc/spec_resource.py) and the library Makefile
(`make resource`) do; no GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "detecting-convolutional-codes-via-markovian-statistics_amd", "csrc")
SPEC = os.path.join(CSRC, "spec_resource.py")
HAVE_CLANG = bool(shutil.which("/opt/rocm/lib/llvm/bin/clang++"))

# upload_model's variant defines (rtc_variant_defs + kNoWalkDef)
K1S = {
    "k1s_pf": ["-DCVD_K1B_BITSLICE=1", "-DCVD_K1S_PF=1", "-DCVD_K1B_BLOCK=1024", "-DCVD_FILTER_PAT_BITS=10",
               "-DCVD_K1S_WALK=0"],
    "k1s_ldsf": ["-DCVD_K1B_BITSLICE=1", "-DCVD_K1B_LDSF=1", "-DCVD_K1B_BLOCK=1024", "-DCVD_FILTER_PAT_BITS=10",
                 "-DCVD_K1S_WALK=0"],
    "k1s_global": ["-DCVD_K1B_BITSLICE=1", "-DCVD_K1S_WALK=0"],
}
DET_VGPRS, GEN_VGPRS = 112, 64
CU_LDS = 160 * 1024
DET_DYN_LDS = 128 * 1024   # the pre-filter or the LDS filter of a 1,024-thread block


def _fields(text, name):
    return [int(x) for x in re.findall(name + r": (\d+)", text)]


@pytest.fixture(scope="module")
def det_lds():
    """static LDS of the detector block, filled in by the k1s cases (pf and ldsf agree)"""
    return {}


@pytest.mark.skipif(not HAVE_CLANG, reason="ROCm clang not present")
@pytest.mark.parametrize("variant", sorted(K1S))
def test_k1s_without_walk_leaves_room_for_a_generator_wave(variant, det_lds):
    out = subprocess.run([sys.executable, SPEC, "m6", *K1S[variant]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    vgpr, agpr = _fields(out.stdout, r" VGPRs"), _fields(out.stdout, r"AGPRs")
    scratch, occ = _fields(out.stdout, r"ScratchSize \[bytes/lane\]"), _fields(out.stdout, r"Occupancy \[waves/SIMD\]")
    lds = _fields(out.stdout, r"LDS Size \[bytes/block\]")
    print(variant, "VGPRs", vgpr, "AGPRs", agpr, "scratch", scratch, "occupancy", occ, "LDS", lds)
    # both entries (one model per launch, and the multi-model entry)
    assert len(vgpr) == 2 and all(v <= DET_VGPRS for v in vgpr), out.stdout
    assert all(a == 0 for a in agpr), out.stdout
    assert len(scratch) == 2 and all(s == 0 for s in scratch), out.stdout
    assert len(occ) == 2 and all(o >= 4 for o in occ), out.stdout
    det_lds[variant] = max(lds)


@pytest.mark.skipif(not HAVE_CLANG, reason="ROCm clang not present")
def test_small_generator_form_fits_beside_the_detector(det_lds):
    out = subprocess.run(["make", "-C", CSRC, "resource"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # gen_fast_kernel<1, 2, kT, false>: every tap-list length the host can choose
    blocks = re.split(r"remark: Function Name: ", out.stderr)
    small = [b for b in blocks if re.match(r"\S*gen_fast_kernelILi1ELi2ELi\d+ELb0E", b)]
    fast = [b for b in blocks if re.match(r"\S*gen_fast_kernelILi1ELi2ELi\d+ELb1E", b)]
    assert len(small) == 6 and len(fast) == 6, [b.split()[0] for b in small + fast]
    det_static = max(det_lds.get(v, 10920) for v in ("k1s_pf", "k1s_ldsf"))
    for b in small:
        v, s = _fields(b, r" VGPRs")[0], _fields(b, r"ScratchSize \[bytes/lane\]")[0]
        lds = _fields(b, r"LDS Size \[bytes/block\]")[0]
        print(b.split()[0], "VGPRs", v, "scratch", s, "LDS", lds)
        assert v <= GEN_VGPRS and s == 0, b
        assert lds <= CU_LDS - (det_static + DET_DYN_LDS), b
    # (the fast form is the one that does not fit in 64: otherwise the small one is not needed)
    assert all(_fields(b, r" VGPRs")[0] > GEN_VGPRS for b in fast)
