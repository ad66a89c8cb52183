"""The bit-sliced m = 6 detector's lockstep loop after the record loads were merged
(cvd_k1s.h BsCursor::mid): per step one 16-byte record load for the wave --
a candidate's slot record or a known row's dense record -- where there were two.  For the
kernels the sweep runs (walk mode compiled out: pre-filter, LDS filter, plain filter), compiled
here as the JIT does (csrc/spec_resource.py): no scratch, at most 112 VGPRs, and the six-step
loop's count of 16-byte global loads, six fewer than before the merge.  The LDS-filter variant
keeps the two sites (cvd_k1s.h kBsOneLoad: the merged form measured slower at p = 0.01 and
0.02), so its count is pinned at the earlier one: a change of either form shows here.

The six-step loop is found by the compiler's own loop annotations: the innermost loop that
holds a non-temporal 16-byte load (the stream chunk, cvd_k1s.h stream_load), with the loops
nested in it (the directory probe loops).  Its 16-byte loads, the stream chunk apart:
  before  36 = 6 steps x (dense record, candidate record, two image halves, two probe image halves)
  after   30 = 6 steps x (record, two image halves, two probe image halves)
(the probe loop's record test is a 4-byte load of c.)  Both instantiations of k1s_wave (the
unchunked and the chunked launch) and both entries hold such a loop; each is checked."""
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
DET_VGPRS = 112
LOOP_X4_LOADS = {"k1s_pf": 30, "k1s_global": 30, "k1s_ldsf": 36}   # 36 before the merge
ENTRIES = ("cvd_k1b_spec", "cvd_k1b_spec_multi")


def six_step_loops(isa, fn):
    """[(header label, 16-byte global loads without the non-temporal one)] of every loop of
    function `fn` that is the innermost loop around a non-temporal 16-byte load."""
    lines = isa.splitlines()
    s = next(i for i, l in enumerate(lines) if l.startswith(fn + ":"))
    e = next(i for i in range(s, len(lines)) if lines[i].lstrip().startswith(".Lfunc_end"))
    # blocks: label -> (innermost loop header or None, that header's parent loops if the block is a header)
    blocks, cur = [], None
    parents = {}
    i = s
    while i < e:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", lines[i])
        if m:
            label, notes = m.group(1), [m.group(2) or ""]
            while i + 1 < e and re.match(r"^\s+;", lines[i + 1]) and not re.match(r"^\s+;;", lines[i + 1]):
                i += 1
                notes.append(lines[i])
            note = " ".join(notes)
            hdr = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if hdr:
                loop = ".L" + hdr.group(1)
            elif "Loop Header" in note:
                loop = label
                parents[label] = [".L" + p for p in re.findall(r"Parent Loop (BB\d+_\d+)", note)]
            else:
                loop = None
            cur = {"label": label, "loop": loop, "insts": []}
            blocks.append(cur)
        elif cur is not None and re.match(r"^\s+[a-z]", lines[i]):
            cur["insts"].append(lines[i].strip())
        i += 1

    def inside(b, header):
        return b["loop"] == header or (b["loop"] is not None and header in parents.get(b["loop"], []))

    def is_x4(inst):
        return inst.startswith("global_load_dwordx4")

    def is_nt(inst):
        return is_x4(inst) and re.search(r"\bnt\b", inst.split(";")[0]) is not None

    headers = sorted({b["loop"] for b in blocks if b["loop"] and any(is_nt(x) for x in b["insts"])})
    # (the work-queue loop around both also loads a wave's first chunk: not innermost)
    headers = [h for h in headers if not any(h in parents.get(o, []) for o in headers)]
    out = []
    for h in headers:
        n = sum(1 for b in blocks if inside(b, h) for x in b["insts"] if is_x4(x) and not is_nt(x))
        out.append((h, n))
    return out


def _fields(text, name):
    return [int(x) for x in re.findall(name + r": (\d+)", text)]


@pytest.mark.skipif(not HAVE_CLANG, reason="ROCm clang not present")
@pytest.mark.parametrize("variant", sorted(K1S))
def test_one_record_load_per_step(variant, tmp_path):
    isa = str(tmp_path / (variant + ".s"))
    out = subprocess.run([sys.executable, SPEC, "m6", *K1S[variant], "--isa", isa], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    vgpr, scratch = _fields(out.stdout, r" VGPRs"), _fields(out.stdout, r"ScratchSize \[bytes/lane\]")
    print(variant, "VGPRs", vgpr, "scratch", scratch)
    assert len(vgpr) == 2 and all(v <= DET_VGPRS for v in vgpr), out.stdout
    assert len(scratch) == 2 and all(x == 0 for x in scratch), out.stdout
    with open(isa) as f:
        text = f.read()
    for fn in ENTRIES:
        loops = six_step_loops(text, fn)
        print(variant, fn, loops)
        # the unchunked and the chunked instantiation of k1s_wave
        assert len(loops) == 2, (fn, loops)
        assert all(n == LOOP_X4_LOADS[variant] for _, n in loops), (fn, loops)
