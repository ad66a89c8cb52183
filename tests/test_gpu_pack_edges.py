"""cvd_pack_windows (csrc/cvd_capture.hip) at every pack_windows_kernel<n, format>, (n = 1,
bytes) included, against test_gpu_capture.py's restatement of include/cvd.h, the whole buffer
for exact equality.  Per instance one case with every funnel offset (win_bit + tile_bits) & 127
from 0 to 127 (an odd stride over 130 windows: test_sweep_cases_host.py), so offset 127 meets the
row's last dword pair and the bytes staging packs every halfword position of a row; sequence
tiles of 64, 64 and 2 rows; a second chunk tile of one chunk whose only word is ragged; q0 = 3
and pitch = nseq + 9 into a sentinel-filled buffer.  For bytes and lsb also n_phase = n, and a
capture whose last window ends exactly on a 128-bit piece (the funnel's second piece lies past
the capture; a piece of ones is allocated behind it)."""
import numpy as np
import pytest
import torch

import sweep_cases as SC
from test_gpu_capture import SENTINEL, capture_bits, pack_restatement, raw_capture

pytestmark = pytest.mark.gpu


def _pack(pkg, c):
    bits = SC.pack_bits(c)
    nbits = len(bits)
    assert c.pad == (nbits % 128 == 0)
    rng = np.random.default_rng(2)
    raw = raw_capture(np.concatenate([bits, np.ones(128, np.uint8)]) if c.pad else bits, c.fmt, rng)
    every = capture_bits(raw, c.fmt, len(raw) if c.fmt == "bytes" else 8 * len(raw))
    assert np.array_equal(every[:nbits], bits) and every[nbits:].all() and len(every) > nbits
    det = pkg.Detector(1, c.n, 2, [[[1, 1, 1]]] * c.n, device=0)
    nseq = c.nwin * c.n_phase
    q0, pitch = SC.PACK_Q0, nseq + SC.PACK_EXTRA_PITCH
    out = torch.full((det.words_per_seq(c.N) // 4, pitch, 4), SENTINEL, dtype=torch.int32, device="cuda")
    buf, nwin = det.pack_capture(torch.from_numpy(raw).cuda(), c.N, start=c.start, stride=c.stride,
                                 n_phase=c.n_phase, nwin=c.nwin, format=c.fmt, nbits=nbits, out=out, q0=q0, pitch=pitch)
    torch.cuda.synchronize()
    assert nwin == c.nwin and buf is out
    # as many windows as fit is exactly nwin: the last one ends on the capture's last bit
    assert det.windows_in(nbits, c.N, c.start, c.stride, c.n_phase) == c.nwin
    want = pack_restatement(bits, c.n, c.N, c.start, c.stride, c.nwin, c.n_phase, pitch, q0, fill=SENTINEL)
    got = buf.cpu().numpy().view(np.uint32)
    wrong = got != want
    assert not wrong.any(), (SC.pack_id(c), int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    return got


@pytest.mark.parametrize("c", SC.PACK_INSTANCE_CASES, ids=SC.pack_id)
def test_every_pack_instance(pkg, c):
    got = _pack(pkg, c)
    assert got.shape[0] == SC.PACK_CHUNKS + 1
    # the columns outside [q0, q0 + nseq) keep the sentinel (part of the whole-buffer comparison)
    assert np.all(got[:, :SC.PACK_Q0] == SENTINEL) and np.all(got[:, SC.PACK_Q0 + c.nwin:] == SENTINEL)


@pytest.mark.parametrize("c", SC.PACK_PHASE_CASES, ids=SC.pack_id)
def test_pack_every_phase(pkg, c):
    _pack(pkg, c)


@pytest.mark.parametrize("c", SC.PACK_PIECE_END_CASES, ids=SC.pack_id)
def test_pack_last_window_ends_on_a_piece(pkg, c):
    _pack(pkg, c)
