"""Command line: the reference's script entry points on the MI355X engine.

  python -m detecting-convolutional-codes-via-markovian-statistics_amd experiment ...
      Pd_plotter.py:242-264 -- run_experiment over (N, p), writes
      <save-dir>/Pd_hybrid_results.csv (columns N, p, Pd, Pc)
  ... parity ...
      comp_parity.py:135-181 -- the parity-template baseline (template of G1,
      basis vector 0 of deg_h = m + 3) on the same trial streams, writes
      <save-dir>/Pd_parity_results.csv: the --baseline CSV of plots_compare.py
  ... exponent ...
      alpha_exponent.py -- learned transition tensors of G1 and G2 streams on
      G1's metric automaton, Eq. 7 per p, writes <save-dir>/error_exponent.csv
  ... compare --hybrid H.csv --baseline B.csv [--outdir plots]
      plots_compare.py:70-148 -- P_err = 1 - Pc of both detectors against p
      (per N) and against N (per p), one PNG each (host only, matplotlib)

  ... scan --code C --p P --N N --input FILE [--format bytes|lsb|msb] [--nbits B]
           [--start S] [--stride BITS] [--phases F] [--parity] [--gamma G] [--learn-len L]
      (nothing in the reference) -- the detector over a captured bitstream: FILE is a
      .npy of uint8 or a raw byte file, one bit per byte or packed LSB-/MSB-first; the
      model of G1 is learned at the one crossover probability P; every window of N steps
      from bit S, BITS apart (default N*n), at F candidate symbol phases, writes
      <save-dir>/scan.csv with one row per (window, phase): window, phase, offset,
      logp1, logref, llr, h1 (and parity_sat, parity_frac with --parity: the
      parity-template baseline on the same windows).  Single-process: under torchrun
      only rank 0 scans.
  ... identify --input FILE --n N --max-span S [--format bytes|lsb|msb] [--nbits B]
               [--start S] [--top K]
      (nothing in the reference) -- which code is in a capture, and at which symbol phase:
      all 2^(N*(S+1)) parity templates over a window of S + 1 symbols are counted at every
      one of the N phases (cvd_parity_sweep: histogram + Walsh-Hadamard transform), the
      significant ones ranked shortest first; writes <save-dir>/identify.csv with one row
      per check: rank, phase, mask (hex), extent, sat, T, z, equation.  For N = 2 the
      first check is the generator pair: printed in octal with the scan --code line that
      takes it.  Single-process, like scan.
  ... decode --code C --input FILE [--format bytes|lsb|msb|soft] [--nbits B] [--start S] [--T T]
             [--out-bits FILE.npy] [--puncture SPEC [--sync T0]]
             [--frame T [--frame-count F] [--frame-stride B | --frame-offsets FILE.npy]
              [--start-state S|any] [--end-state S|any] | [--tail-biting [--laps I]]] [--llr]
             [--list L [--crc SPEC [--crc-first A] [--crc-count C] [--crc-expect X]]]
      (nothing in the reference) -- what was sent: the hard-decision Viterbi decoder of the
      k = 1 code C over the capture from bit S (cvd_viterbi_decode: the Eq. 4-5 recursion with
      its survivor decisions kept, exact whatever the block split); writes the decoded bits to
      <save-dir>/decoded.npy (uint8, packed LSB-first: a --format lsb --nbits T capture that
      identify takes, e.g. for an outer code) and a one-row <save-dir>/decode.csv: T, errors,
      ber, start_state, end_state, blocks, forward_reruns, trace_fixups.  ber = errors / (n T)
      estimates the channel's crossover probability: printed with the scan line that takes
      it, so the workflow is identify -> decode -> scan.  Single-process, like scan.
      --puncture SPEC (dvb:2/3 | dvb:3/4 | dvb:5/6 | dvb:7/8 for oct:171,133, or rows per
      output such as 101/110): the capture carries only the bits the pattern transmits
      (cvd_viterbi_decode_punctured); --sync T0 first tries the K bit offsets of a period over
      T0 steps and decodes from the one with the fewest errors.  The CSV gains capture_bits
      and offset, ber = errors / capture_bits, and no scan line is printed.
      --format soft: the capture is one int8 confidence value per channel bit (a .npy of int8,
      or a raw file read as int8; v > 0 says 1, v < 0 says 0, 0 is an erasure), decoded by
      cvd_viterbi_decode_soft; --nbits and --start count values.  With --puncture the capture
      is depunctured on the device first, and --sync ranks the offsets by the soft distance.
      The CSV gains metric (the soft distance of the decoded path) and erasures; errors
      counts the values whose sign disagrees with the path, ber = errors / non-erased values.
      No scan line is printed: the detector's model is a BSC model.
      --frame T: the capture holds frames of T steps each (802.11a/g PPDUs, GSM bursts, packets),
      decoded in one call (cvd_viterbi_decode_frames and its punctured and soft siblings): frame
      f begins at bit S + f*B (--frame-stride B; default: the frames follow one another), or at
      the int64 offsets of --frame-offsets (a frame that does not lie inside the capture is
      skipped); --frame-count F frames (default: as many as fit).  --start-state / --end-state:
      the encoder's state before / after a frame, or any; the defaults, 0 and 0, are terminated
      frames.  Works with --puncture (the pattern restarts in every frame), with --format soft, and
      with both (cvd_viterbi_decode_frames_soft_punctured: punctured frames of confidence values,
      as a receiver produces them; counted is then the kept values that are not 0); an error
      together with --T or --sync.  Writes <save-dir>/decoded.npy (uint8 [F, 4w],
      w = ceil(T/32): a row per frame, LSB-first) and <save-dir>/decode_frames.csv, a row per
      frame: frame, offset, status (0 decoded, 1 skipped), distance, errors, counted,
      start_state, end_state; prints the totals and p = errors / counted.
      --frame T --tail-biting: the frames are tail-biting (LTE PBCH / PDCCH, 802.16 FCH: the
      encoder starts in the state of the frame's own last m bits and no tail bits are sent),
      decoded by the wrap-around Viterbi algorithm (cvd_viterbi_decode_frames_tailbiting and its
      punctured and soft siblings) with at most --laps I laps (1..8, default 4).  An error
      together with --start-state / --end-state (neither state is known), --T or --sync, and
      with --format soft --puncture together (decode_frames_tailbiting_soft_punctured and
      decode_frames_llr_punctured are reachable from Python and C only).  The
      CSV gains the column laps and status reads 0 tail-biting best path, 1 skipped, 2 best
      tail-biting survivor of the last lap, 3 no tail-biting survivor (start_state !=
      end_state); the summary adds the numbers of such frames and the mean laps.
      --frame T --format soft --llr: soft output (cvd_viterbi_decode_frames_llr): beside
      decoded.npy the run writes <save-dir>/llr.npy (int16 [F, T]), the max-log-MAP value of every
      bit: the cost of the best path with that bit 0 minus that of the best path with it 1,
      positive for a 1, in the units of the input, +-32767 where the other value has no path (the
      tail of a terminated frame).  The CSV's columns are then frame, offset, status, distance,
      zeros (undecided bits), weakest (the smallest |value| of the frame), saturated, end_state.
      An error without --frame, without --format soft, with --tail-biting or with --puncture.
      --frame T --format soft --list L: list decoding (cvd_viterbi_decode_frames_list): the L best
      paths of every frame, 1 <= L <= 8, T <= 8192.  decoded.npy is then uint8 [F, L, 4w] and the CSV
      has a row per (frame, path): frame, path, offset, status, distance, start_state, end_state
      (distance and the states -1 where a frame has fewer than L paths).  With --crc SPEC (crc8-lte,
      crc16-ccitt, crc24a, crc24b, crc32, or WIDTH:POLY[:INIT[:EXPECT]] with the width decimal and the
      others hexadecimal) every path's bits are checked on the device (cvd_frames_crc) over --crc-count
      C bits from bit --crc-first A (defaults: 0, and everything before the CRC and the m tail bits
      of a fixed end state), the bits in the order decoded, the CRC's first bit most significant, and
      the first path of a frame whose value is --crc-expect X (hexadecimal; default: the spec's) is
      chosen: decoded.npy is the chosen rows [F, 4w] (path 0 where none passes) and the CSV has a row
      per frame: frame, offset, status, paths, choice (-1: none), crc_ok, distance (of the chosen
      path), distance0, start_state, end_state; the summary prints decoded, ok and rescued (frames
      whose path 0 fails and a later one passes).  An error without --frame, without --format soft,
      with --tail-biting, --puncture, --llr, --T or --sync, and --crc* without --list.
  ... encode --code C --input FILE.npy [--T T] [--frame T [--frame-count F] [--frame-stride B]
             [--open | --tail-biting]] [--start-state S] [--puncture SPEC]
             [--format bytes|lsb|msb|soft] [--amplitude A] [--output encoded.npy]
      (comp_parity.py:65-83 encode_convolutional, batched) -- the inverse of decode: the k = 1 code C
      (n in 2..3, m <= 16) over information bits, on the device (cvd_encode_frames).  Without --frame
      FILE.npy is one stream of bits packed LSB-first, as decode writes decoded.npy; --T counts the
      steps (default: every bit of the file) and the encoder starts in --start-state (default 0).
      With --frame T it is decoded.npy's rows, uint8 [F, 4w]: a frame per row, terminated (the last
      m inputs taken as 0, whatever the row holds), or --open (no tail is forced), or --tail-biting
      (the encoder starts in the state of the row's own last m bits; an error with --start-state);
      frame f begins at position f*B (--frame-stride B; default: the frames follow one another).
      --puncture SPEC leaves out what the pattern does not transmit, restarting in every frame.
      --format soft writes int8 values, +A for a 1 and -A for a 0 (--amplitude A, 1..127, default
      24; an error with another format).  Writes the capture to <save-dir>/encoded.npy and prints
      the span of a frame, the positions and the frames: decode then encode of a noiseless file
      gives the file back.  Single-process, like scan.

Codes: the BASELINE configurations (m2, m6, r23_m4), the demo presets (example:1,
example:2, demo_script.py:35-52), or oct:G0,G1[,G2] -- k = 1 generators in octal (MSB =
current input), e.g. oct:133,171: n = the number of generators, m from the highest
degree, G2 = the list rotated by one.  Every subcommand but compare
runs on the GPU through libcvd.so.  Under torchrun (one process per GPU) the trials of
experiment and parity are sharded over the ranks, the counts reduced with one all_reduce, and rank 0
writes the CSV.
"""
import argparse
import csv
import os
import re
import sys

from . import (CONFIG_CODES, DEFAULTS, EXAMPLE_CODES, compute_error_exponent, default_template,
               decode_capture, decode_capture_punctured, decode_capture_soft, decode_frames, decode_frames_soft,
               decode_frames_llr, decode_frames_soft_punctured, decode_frames_tailbiting, decode_frames_tailbiting_soft,
               crc_spec, decode_frames_crc, decode_frames_list,
               find_parity_checks,
               learn_transition_tensor, octal_to_taps, parity_experiment, parity_vector_to_equation, parity_vectors,
               puncture_pattern, punctured_bits, run_experiment, scan_capture, sync_punctured, sync_punctured_soft,
               encode_capture, encode_frames)

PROG = "python -m detecting-convolutional-codes-via-markovian-statistics_amd"


def octal_code(spec):
    """(k, n, m, gen1, gen2) of "G0,G1[,G2]": k = 1 generators in octal, MSB = current input."""
    tokens = [t.strip() for t in spec.split(",")]
    if not 1 <= len(tokens) <= 3 or not all(re.fullmatch(r"[0-7]+", t) for t in tokens):
        raise SystemExit(f"oct:{spec}: one to three octal generators, e.g. oct:133,171")
    vals = [int(t, 8) for t in tokens]
    m = max(vals).bit_length() - 1
    if m < 0:
        raise SystemExit(f"oct:{spec}: every generator is zero")
    gen1 = [[octal_to_taps(v, m)] for v in vals]
    return 1, len(vals), m, gen1, gen1[1:] + gen1[:1]


def code_of(name):
    """(k, n, m, gen1, gen2) of a configuration or demo preset name, or of oct:G0,G1[,G2]."""
    if name.startswith("oct:"):
        return octal_code(name.split(":", 1)[1])
    if name.startswith("example:"):
        key = name.split(":", 1)[1]
        if key not in EXAMPLE_CODES:
            raise SystemExit(f"unknown preset {name!r} (example:{' | example:'.join(EXAMPLE_CODES)})")
        c = EXAMPLE_CODES[key]
    elif name in CONFIG_CODES:
        c = CONFIG_CODES[name]
    else:
        raise SystemExit(f"unknown code {name!r}: {', '.join(CONFIG_CODES)}, example:<preset> or oct:G0,G1")
    return c["k"], c["n"], c["m"], c["gen1"], c["gen2"]


def _floats(s):
    return [float(x) for x in s.split(",") if x.strip()]


def _ints(s):
    return [int(x) for x in s.split(",") if x.strip()]


def parser():
    ap = argparse.ArgumentParser(prog=PROG, description="MI355X relative-Viterbi-metric detector")
    sub = ap.add_subparsers(dest="cmd", required=True)
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--code", default="example:1",
                        help="m2 | m6 | r23_m4 (BASELINE configs), example:1 | example:2 (demo presets) or oct:133,171")
    common.add_argument("--p", type=_floats, default=None,
                        help="comma list of BSC crossover probabilities (default: Pd_plotter.py DEFAULTS p_vec)")
    common.add_argument("--seed", type=int, default=DEFAULTS["seed"])
    common.add_argument("--save-dir", default=DEFAULTS["save_dir"])
    common.add_argument("--out", default=None, help="CSV path (default: <save-dir>/<subcommand file>)")

    e = sub.add_parser("experiment", parents=[common], help="Pd/Pc of the Markov detector (Pd_plotter.py)")
    e.add_argument("--num-iter", type=int, default=DEFAULTS["num_iter"])
    e.add_argument("--N", type=_ints, default=None, help="blocklengths (default: N_SPECTRUM_BY_M[m])")
    e.add_argument("--learn-len", type=int, default=DEFAULTS["learn_len"])
    e.add_argument("--learn-burn", type=int, default=DEFAULTS["learn_burn"])
    e.add_argument("--laplace", type=float, default=DEFAULTS["laplace"])

    pa = sub.add_parser("parity", parents=[common], help="parity-template baseline (comp_parity.py)")
    pa.add_argument("--num-iter", type=int, default=DEFAULTS["num_iter"])
    pa.add_argument("--N", type=_ints, default=None, help="blocklengths (default: N_SPECTRUM_BY_M[m])")
    pa.add_argument("--gamma", type=float, default=0.6, help="decision threshold (comp_parity.py:166)")
    pa.add_argument("--deg-h", type=int, default=None, help="parity polynomial degree (default m + 3)")

    x = sub.add_parser("exponent", parents=[common], help="Eq. 7 error exponent (alpha_exponent.py)")
    x.add_argument("--length", type=int, default=300_000, help="learning chain steps per tensor")
    x.add_argument("--burn-in", type=int, default=5_000)
    x.add_argument("--laplace", type=float, default=1.0)
    x.add_argument("--chains", type=int, default=1, help="independent chains (1: the reference's one chain)")
    x.add_argument("--u-grid", type=int, default=401)

    s = sub.add_parser("scan", help="the detector over a captured bitstream")
    s.add_argument("--code", default="example:1",
                   help="m2 | m6 | r23_m4 (BASELINE configs), example:1 | example:2 (demo presets) or oct:133,171")
    s.add_argument("--p", type=float, required=True, help="BSC crossover probability the model is learned at")
    s.add_argument("--N", type=int, required=True, help="steps per window")
    s.add_argument("--input", required=True, help=".npy of uint8, or a raw byte file")
    s.add_argument("--format", choices=["bytes", "lsb", "msb"], default="bytes",
                   help="one bit per byte, or packed with bit 0 / bit 7 of a byte first")
    s.add_argument("--nbits", type=int, default=None, help="capture length in bits (default: the whole file)")
    s.add_argument("--start", type=int, default=0, help="first capture bit of window 0")
    s.add_argument("--stride", type=int, default=None, help="bits between windows (default N*n)")
    s.add_argument("--phases", type=int, default=1, help="candidate symbol phases per window (1..n)")
    s.add_argument("--parity", action="store_true", help="add the parity-template baseline's columns")
    s.add_argument("--gamma", type=float, default=0.6, help="parity decision threshold (comp_parity.py:166)")
    s.add_argument("--learn-len", type=int, default=DEFAULTS["learn_len"])
    s.add_argument("--learn-burn", type=int, default=DEFAULTS["learn_burn"])
    s.add_argument("--laplace", type=float, default=DEFAULTS["laplace"])
    s.add_argument("--seed", type=int, default=DEFAULTS["seed"])
    s.add_argument("--save-dir", default=DEFAULTS["save_dir"])
    s.add_argument("--out", default=None, help="CSV path (default: <save-dir>/scan.csv)")

    i = sub.add_parser("identify", help="blind parity-check search of a captured bitstream")
    i.add_argument("--input", required=True, help=".npy of uint8, or a raw byte file")
    i.add_argument("--n", type=int, required=True, choices=[1, 2, 3], help="outputs per symbol")
    i.add_argument("--max-span", type=int, required=True,
                   help="delays a check may span: the window is n*(max_span+1) <= 22 bits")
    i.add_argument("--format", choices=["bytes", "lsb", "msb"], default="bytes",
                   help="one bit per byte, or packed with bit 0 / bit 7 of a byte first")
    i.add_argument("--nbits", type=int, default=None, help="capture length in bits (default: the whole file)")
    i.add_argument("--start", type=int, default=0, help="capture bit of the first anchor, phase 0")
    i.add_argument("--top", type=int, default=16, help="checks listed")
    i.add_argument("--save-dir", default=DEFAULTS["save_dir"])
    i.add_argument("--out", default=None, help="CSV path (default: <save-dir>/identify.csv)")

    d = sub.add_parser("decode", help="hard-decision Viterbi decoder of a captured bitstream")
    d.add_argument("--code", required=True,
                   help="m2 | m6 (BASELINE configs), example:1 | example:2 (demo presets) or oct:133,171 (k = 1)")
    d.add_argument("--input", required=True, help=".npy of uint8, or a raw byte file")
    d.add_argument("--format", choices=["bytes", "lsb", "msb", "soft"], default="bytes",
                   help="one bit per byte, packed with bit 0 / bit 7 of a byte first, or soft: one int8 confidence "
                        "value per bit (> 0 says 1, < 0 says 0, 0 is an erasure)")
    d.add_argument("--nbits", type=int, default=None,
                   help="capture length in bits (soft: in values; default: the whole file)")
    d.add_argument("--start", type=int, default=0, help="capture bit (soft: value) of output 0 of step 0")
    d.add_argument("--T", type=int, default=None, help="steps to decode (default: as many whole symbols as fit)")
    d.add_argument("--out-bits", default=None, help=".npy path of the decoded bits (default: <save-dir>/decoded.npy)")
    d.add_argument("--save-dir", default=DEFAULTS["save_dir"])
    d.add_argument("--out", default=None, help="CSV path (default: <save-dir>/decode.csv)")
    d.add_argument("--puncture", default=None, metavar="SPEC",
                   help="the capture is punctured: a DVB-S name (dvb:2/3, dvb:3/4, dvb:5/6, dvb:7/8; for oct:171,133) "
                        "or rows per output over a period's columns, e.g. 101/110")
    d.add_argument("--sync", type=int, default=None, metavar="T0",
                   help="with --puncture: try the K bit offsets of a period over the first T0 steps from --start "
                        "and decode from the best")
    d.add_argument("--frame", type=int, default=None, metavar="T",
                   help="the capture holds frames of T steps each, decoded in one call (not with --T or --sync)")
    d.add_argument("--frame-count", type=int, default=None, metavar="F", help="frames (default: as many as fit)")
    d.add_argument("--frame-stride", type=int, default=None, metavar="B",
                   help="capture bits (soft: values) from one frame's start to the next (default: a frame's own)")
    d.add_argument("--frame-offsets", default=None, metavar="FILE.npy",
                   help=".npy of int64: where each frame begins (instead of --start and --frame-stride)")
    d.add_argument("--start-state", type=frame_state, default=0, metavar="S|any", action=BoundaryState,
                   help="with --frame: the encoder's state before a frame, or any (default 0)")
    d.add_argument("--end-state", type=frame_state, default=0, metavar="S|any", action=BoundaryState,
                   help="with --frame: the encoder's state after a frame, or any (default 0: m zero tail bits)")
    d.add_argument("--tail-biting", action="store_true",
                   help="with --frame: the frames are tail-biting, decoded by the wrap-around Viterbi algorithm "
                        "(not with --start-state or --end-state)")
    d.add_argument("--laps", type=int, default=None, metavar="I",
                   help="with --tail-biting: at most I laps over a frame (1..8, default 4)")
    d.add_argument("--llr", action="store_true",
                   help="with --frame and --format soft: also write llr.npy, a max-log-MAP value per bit "
                        "(not with --tail-biting or --puncture)")
    d.add_argument("--out-llr", default=None, help="with --llr: the .npy of values (default <save-dir>/llr.npy)")
    d.add_argument("--list", type=int, default=None, metavar="L",
                   help="with --frame and --format soft: the L best paths of every frame (1..8; not with "
                        "--tail-biting, --puncture or --llr)")
    d.add_argument("--crc", default=None, metavar="SPEC",
                   help="with --list: choose of every frame the first path that passes this CRC (crc8-lte, "
                        "crc16-ccitt, crc24a, crc24b, crc32 or WIDTH:POLY[:INIT[:EXPECT]], the width decimal, "
                        "the others hexadecimal)")
    d.add_argument("--crc-first", type=int, default=None, metavar="A", help="with --crc: the first bit under the CRC (default 0)")
    d.add_argument("--crc-count", type=int, default=None, metavar="C",
                   help="with --crc: the bits under the CRC (default: all before the CRC and a fixed end state's tail)")
    d.add_argument("--crc-expect", type=lambda t: int(t, 16), default=None, metavar="X",
                   help="with --crc: the value (hexadecimal) of a frame that passes (default: the spec's)")
    d.set_defaults(states_given=False)

    en = sub.add_parser("encode", help="convolutional encoder of information bits (the inverse of decode)")
    en.add_argument("--code", required=True,
                    help="m2 | m6 (BASELINE configs), example:1 | example:2 (demo presets) or oct:133,171 (k = 1)")
    en.add_argument("--input", required=True,
                    help=".npy of uint8: bits packed LSB-first (decode's decoded.npy), with --frame a row per frame")
    en.add_argument("--T", type=int, default=None, help="steps of the stream (default: every bit of the file)")
    en.add_argument("--frame", type=int, default=None, metavar="T",
                    help="the input holds a frame of T steps per row, encoded in one call (not with --T)")
    en.add_argument("--frame-count", type=int, default=None, metavar="F", help="frames (default: every row)")
    en.add_argument("--frame-stride", type=int, default=None, metavar="B",
                    help="positions from one frame's start to the next (default: a frame's own)")
    en.add_argument("--open", action="store_true", help="with --frame: no tail is forced (default: terminated frames)")
    en.add_argument("--tail-biting", action="store_true",
                    help="with --frame: the encoder starts in the state of the row's own last m bits")
    en.add_argument("--start-state", type=int, default=None, metavar="S",
                    help="the encoder's state before the stream or a frame (default 0; not with --tail-biting)")
    en.add_argument("--puncture", default=None, metavar="SPEC",
                    help="leave out what the pattern does not transmit: a DVB-S name (dvb:2/3, dvb:3/4, dvb:5/6, "
                         "dvb:7/8; for oct:171,133) or rows per output over a period's columns, e.g. 101/110")
    en.add_argument("--format", choices=["bytes", "lsb", "msb", "soft"], default="bytes",
                    help="one bit per byte, packed with bit 0 / bit 7 of a byte first, or soft: int8 +-amplitude")
    en.add_argument("--amplitude", type=int, default=None, metavar="A", help="with --format soft: 1..127 (default 24)")
    en.add_argument("--output", default=None, help=".npy path of the capture (default: <save-dir>/encoded.npy)")
    en.add_argument("--save-dir", default=DEFAULTS["save_dir"])

    c = sub.add_parser("compare", help="P_err figures of both detectors (plots_compare.py)")
    c.add_argument("--hybrid", required=True, help="CSV of the experiment subcommand")
    c.add_argument("--baseline", required=True, help="CSV of the parity subcommand")
    c.add_argument("--outdir", default="plots")
    return ap


class BoundaryState(argparse.Action):
    """--start-state / --end-state: the value, and that one of them was given."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.states_given = True


def frame_state(text):
    """--start-state / --end-state: a state number, or "any" (None)."""
    if text == "any":
        return None
    try:
        s = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: a state number, or any")
    if s < 0:
        raise argparse.ArgumentTypeError(f"{text!r}: a state number is not negative")
    return s


def parse_args(argv=None):
    """parser().parse_args with the checks between arguments that argparse does not express."""
    ap = parser()
    a = ap.parse_args(argv)
    if a.cmd == "decode":
        if a.frame is None:
            if (a.frame_count is not None or a.frame_stride is not None or a.frame_offsets is not None
                    or a.start_state != 0 or a.end_state != 0):
                ap.error("decode: --frame-count, --frame-stride, --frame-offsets, --start-state and --end-state need --frame")
            if a.tail_biting:
                ap.error("decode: --tail-biting needs --frame")
        else:
            if a.T is not None or a.sync is not None:
                ap.error("decode: --frame decodes frames of T steps each; it does not go with --T or --sync")
            if a.frame_offsets is not None and a.frame_stride is not None:
                ap.error("decode: --frame-offsets and --frame-stride exclude one another")
            if a.tail_biting and a.format == "soft" and a.puncture is not None:
                ap.error("decode: --tail-biting with --format soft does not take --puncture "
                         "(decode_frames_tailbiting_soft_punctured: Python and C only)")
            if a.tail_biting and a.states_given:
                ap.error("decode: --tail-biting does not go with --start-state or --end-state: neither state is known")
        if a.laps is not None and not a.tail_biting:
            ap.error("decode: --laps needs --tail-biting")
        if a.llr:
            if a.frame is None:
                ap.error("decode: --llr needs --frame")
            if a.format != "soft":
                ap.error("decode: --llr needs --format soft")
            if a.tail_biting:
                ap.error("decode: --llr does not go with --tail-biting")
            if a.puncture is not None:
                ap.error("decode: --llr does not take --puncture")
        elif a.out_llr is not None:
            ap.error("decode: --out-llr needs --llr")
        if a.list is not None:
            if a.frame is None:
                ap.error("decode: --list needs --frame")
            if a.format != "soft":
                ap.error("decode: --list needs --format soft")
            if a.tail_biting or a.puncture is not None or a.llr:
                ap.error("decode: --list does not go with --tail-biting, --puncture or --llr")
            if not 1 <= a.list <= 8:
                ap.error("decode: --list takes 1..8 paths")
            if a.crc is not None:
                try:
                    crc_spec(a.crc)
                except ValueError as e:
                    ap.error(f"decode: {e}")
        if a.crc is None and (a.crc_first is not None or a.crc_count is not None or a.crc_expect is not None):
            ap.error("decode: --crc-first, --crc-count and --crc-expect need --crc")
        if a.crc is not None and a.list is None:
            ap.error("decode: --crc needs --list")
    if a.cmd == "encode":
        if a.frame is None:
            if a.frame_count is not None or a.frame_stride is not None or a.open or a.tail_biting:
                ap.error("encode: --frame-count, --frame-stride, --open and --tail-biting need --frame")
        else:
            if a.T is not None:
                ap.error("encode: --frame encodes frames of T steps each; it does not go with --T")
            if a.open and a.tail_biting:
                ap.error("encode: --open and --tail-biting exclude one another")
            if a.tail_biting and a.start_state is not None:
                ap.error("encode: --tail-biting does not go with --start-state: the frame's own bits set the state")
        if a.start_state is not None and a.start_state < 0:
            ap.error("encode: a state number is not negative")
        if a.amplitude is not None and a.format != "soft":
            ap.error("encode: --amplitude needs --format soft")
        if a.amplitude is not None and not 1 <= a.amplitude <= 127:
            ap.error("encode: --amplitude takes 1..127")
    return a


def _init_dist():
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return None
    import torch
    import torch.distributed as dist
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    return dist


def cmd_experiment(a):
    k, n, m, g1, g2 = code_of(a.code)
    df = run_experiment(k, n, m, g1, g2, a.num_iter, a.p or DEFAULTS["p_vec"], a.learn_len, a.learn_burn,
                        a.laplace, a.seed, N_list=a.N)
    return df, "Pd_hybrid_results.csv", "Hybrid Markov-based detector"


def cmd_parity(a):
    k, n, m, g1, g2 = code_of(a.code)
    deg_h = m + 3 if a.deg_h is None else a.deg_h
    eq = parity_vector_to_equation(parity_vectors(g1, deg_h)[0])
    df = parity_experiment(k, n, m, g1, g2, a.num_iter, a.p or DEFAULTS["p_vec"], a.gamma, a.seed,
                           N_list=a.N, template=default_template(g1, m, deg_h))
    return df, "Pd_parity_results.csv", f"Parity-template baseline, equation {eq}"


def cmd_exponent(a):
    import pandas as pd
    k, n, m, g1, g2 = code_of(a.code)
    rows = []
    for p in a.p or DEFAULTS["p_vec"]:
        P1 = learn_transition_tensor(g1, g1, m, p, a.length, a.burn_in, a.laplace, a.seed, k=k, n=n,
                                     chains=a.chains)[0]
        P2 = learn_transition_tensor(g2, g1, m, p, a.length, a.burn_in, a.laplace, a.seed + 1, k=k, n=n,
                                     chains=a.chains)[0]
        I_err, u = compute_error_exponent(P1, P2, u_grid=a.u_grid)
        rows.append({"p": p, "I_err": I_err, "u_star": u, "states": P1.K})
    return pd.DataFrame(rows), "error_exponent.csv", "Error exponent (Eq. 7)"


def load_capture(path):
    """uint8 array of a capture file: a .npy of uint8, or the raw bytes of any other file."""
    import numpy as np
    if path.endswith(".npy"):
        cap = np.load(path)
        if cap.dtype != np.uint8:
            raise SystemExit(f"{path}: a capture is uint8, not {cap.dtype}")
        return cap.reshape(-1)
    return np.fromfile(path, dtype=np.uint8)


def load_soft_capture(path, nvals=None):
    """int8 array of a soft capture file: a .npy of int8, or any other file read as int8; cut to
    its first nvals values."""
    import numpy as np
    if path.endswith(".npy"):
        cap = np.load(path)
        if cap.dtype != np.int8:
            raise SystemExit(f"{path}: a soft capture is int8, not {cap.dtype}")
        cap = cap.reshape(-1)
    else:
        cap = np.fromfile(path, dtype=np.int8)
    if nvals is not None:
        if not 0 <= nvals <= cap.size:
            raise SystemExit(f"decode: --nbits {nvals} outside the capture's {cap.size} values")
        cap = cap[:nvals]
    return cap


def cmd_scan(a):
    """Writes the CSV; floats as repr, so they read back exactly."""
    if int(os.environ.get("RANK", "0")) != 0:   # single-process: under torchrun rank 0 scans
        return 0
    k, n, m, g1, _ = code_of(a.code)
    res = scan_capture(k, n, m, g1, load_capture(a.input), a.N, a.p, a.learn_len, a.learn_burn, a.laplace,
                       a.seed, start=a.start, stride=a.stride, n_phase=a.phases, format=a.format, nbits=a.nbits,
                       parity_template=default_template(g1, m) if a.parity else None, gamma=a.gamma)
    cols = ["logp1", "logref", "llr"]
    out = a.out or os.path.join(a.save_dir, "scan.csv")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    nwin, nph = res["offset"].shape
    with open(out, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["window", "phase", "offset", *cols, "h1"] + (["parity_sat", "parity_frac"] if a.parity else []))
        for i in range(nwin):
            for ph in range(nph):
                row = [i, ph, int(res["offset"][i, ph]), *[repr(float(res[c][i, ph])) for c in cols],
                       int(res["h1"][i, ph])]
                if a.parity:
                    row += [int(res["parity_sat"][i, ph]), repr(float(res["parity_frac"][i, ph]))]
                wr.writerow(row)
    print(f"Scanned {nwin} windows x {nph} phases: {int(res['h1'].sum())} decided H1")
    print("Saved results to", out)
    return 0


def taps_octal(taps):
    """Octal of a delay-ordered tap list, MSB = current input (octal_to_taps' inverse)."""
    return format(int("".join(str(int(b)) for b in taps), 2), "o")


def cmd_identify(a):
    """Writes the CSV; z as repr, so it reads back exactly."""
    if int(os.environ.get("RANK", "0")) != 0:   # single-process: under torchrun rank 0 searches
        return 0
    checks = find_parity_checks(load_capture(a.input), a.n, a.max_span, start=a.start, format=a.format,
                                nbits=a.nbits, top=a.top)
    out = a.out or os.path.join(a.save_dir, "identify.csv")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["rank", "phase", "mask", "extent", "sat", "T", "z", "equation"])
        for rank, c in enumerate(checks):
            h = [[int((j, s) in c["template"]) for s in range(c["extent"])] for j in range(a.n)]
            wr.writerow([rank, c["phase"], hex(c["mask"]), c["extent"], c["sat"], c["T"], repr(c["z"]),
                         parity_vector_to_equation(h)])
    if not checks:
        print("No significant parity check: no code of this shape within the span")
    else:
        c = checks[0]
        print(f"{len(checks)} significant checks listed; the shortest spans {c['extent']} symbols at phase "
              f"{c['phase']} (z = {c['z']:.1f}{', inverted polarity' if c['inverted'] else ''})")
        if a.n == 2:
            m = c["extent"] - 1
            h = [[int((j, s) in c["template"]) for s in range(m + 1)] for j in range(2)]
            code = f"oct:{taps_octal(h[1])},{taps_octal(h[0])}"
            print(f"Generators (octal): {taps_octal(h[1])}, {taps_octal(h[0])}  (k = 1, n = 2, m = {m})")
            print(f"{PROG} scan --code {code} --start {a.start + c['phase']} --input {a.input} --format {a.format}"
                  " --p P --N N")
    print("Saved results to", out)
    return 0


DECODE_COLUMNS = ["T", "errors", "ber", "start_state", "end_state", "blocks", "forward_reruns", "trace_fixups"]
FRAME_COLUMNS = ["frame", "offset", "status", "distance", "errors", "counted", "start_state", "end_state"]
TAILBITING_COLUMNS = FRAME_COLUMNS + ["laps"]
LLR_COLUMNS = ["frame", "offset", "status", "distance", "zeros", "weakest", "saturated", "end_state"]
LIST_COLUMNS = ["frame", "path", "offset", "status", "distance", "start_state", "end_state"]
CRC_COLUMNS = ["frame", "offset", "status", "paths", "choice", "crc_ok", "distance", "distance0", "start_state",
               "end_state"]


def cmd_decode_list(a, n, m, g1, offsets):
    """decode --frame --list: the rows of bits and a CSV row per (frame, path), or with --crc the
    chosen rows and a CSV row per frame."""
    import numpy as np
    kw = dict(F=a.frame_count, start=a.start, stride=a.frame_stride, offsets=offsets, start_state=a.start_state,
              end_state=a.end_state)
    soft = load_soft_capture(a.input, a.nbits)
    try:
        if a.crc is None:
            res = decode_frames_list(n, m, g1, soft, a.frame, a.list, **kw)
        else:
            res = decode_frames_crc(n, m, g1, soft, a.frame, a.list, a.crc, first=a.crc_first or 0, count=a.crc_count,
                                    expect=a.crc_expect, **kw)
    except ValueError as e:
        raise SystemExit(f"decode: {e}")
    if offsets is None:
        stride = a.frame_stride if a.frame_stride is not None else n * a.frame
        offsets = a.start + stride * np.arange(res["F"], dtype=np.int64)
    out = a.out or os.path.join(a.save_dir, "decode_frames.csv")
    out_bits = a.out_bits or os.path.join(a.save_dir, "decoded.npy")
    for path in (out, out_bits):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    bits = (res["bits"] if a.crc is None else res["chosen_bits"]).cpu().numpy()
    with open(out_bits, "wb") as f:             # (np.save would append .npy to another suffix)
        np.save(f, bits)
    dist, s0, sT = (res[k].cpu().numpy() for k in ("distance", "start_states", "end_states"))
    status, paths = res["status"].cpu().numpy(), res["paths"].cpu().numpy()
    with open(out, "w", newline="") as f:
        wr = csv.writer(f)
        if a.crc is None:
            wr.writerow(LIST_COLUMNS)
            for i in range(res["F"]):
                for l in range(res["L"]):
                    wr.writerow([i, l, int(offsets[i]), int(status[i]), int(dist[i, l]), int(s0[i, l]), int(sT[i, l])])
        else:
            wr.writerow(CRC_COLUMNS)
            choice, ok = res["choice"].cpu().numpy(), res["crc_ok"].cpu().numpy()
            for i in range(res["F"]):
                c = max(int(choice[i]), 0)
                wr.writerow([i, int(offsets[i]), int(status[i]), int(paths[i]), int(choice[i]), int(ok[i]),
                             int(dist[i, c]), int(dist[i, 0]), int(s0[i, c]), int(sT[i, c])])
    print(f"Decoded {res['decoded']} frames of {res['T']} steps ({res['skipped']} skipped): {res['total_paths']} paths "
          f"in lists of {res['L']}, distance of the best paths {res['total_distance']}")
    if a.crc is not None:
        print(f"CRC {a.crc}: {res['decoded']} decoded, {res['ok']} ok, {res['rescued']} rescued by a path behind the best")
    print("Saved bits to", out_bits, "(" + " x ".join(str(d) for d in bits.shape) + " bytes)")
    print("Saved results to", out)
    return 0


def cmd_decode_frames(a, n, m, g1):
    """decode --frame: writes the rows of bits and a CSV row per frame."""
    import numpy as np
    offsets = None
    if a.frame_offsets is not None:
        offsets = np.load(a.frame_offsets)
        if offsets.dtype != np.int64:
            raise SystemExit(f"{a.frame_offsets}: frame offsets are int64, not {offsets.dtype}")
        offsets = offsets.reshape(-1)
    if a.list is not None:
        return cmd_decode_list(a, n, m, g1, offsets)
    kw = dict(F=a.frame_count, start=a.start, stride=a.frame_stride, offsets=offsets)
    if a.tail_biting:
        kw["max_laps"] = a.laps
        hard, soft = decode_frames_tailbiting, decode_frames_tailbiting_soft
    else:
        kw.update(start_state=a.start_state, end_state=a.end_state)
        hard, soft = decode_frames, decode_frames_llr if a.llr else decode_frames_soft
    try:
        if a.format == "soft" and a.puncture is not None:    # terminated frames: parse_args saw to it
            res = decode_frames_soft_punctured(n, m, g1, a.puncture, load_soft_capture(a.input, a.nbits), a.frame, **kw)
        elif a.format == "soft":
            res = soft(n, m, g1, load_soft_capture(a.input, a.nbits), a.frame, **kw)
        else:
            res = hard(n, m, g1, load_capture(a.input), a.frame, keep=a.puncture, format=a.format, nbits=a.nbits, **kw)
    except ValueError as e:
        raise SystemExit(f"decode: {e}")
    frames = res["frames"].cpu().numpy()
    if offsets is None:
        span = n * a.frame if a.puncture is None else punctured_bits(a.frame, puncture_pattern(a.puncture, n))
        stride = a.frame_stride if a.frame_stride is not None else span
        offsets = a.start + stride * np.arange(res["F"], dtype=np.int64)
    out = a.out or os.path.join(a.save_dir, "decode_frames.csv")
    out_bits = a.out_bits or os.path.join(a.save_dir, "decoded.npy")
    out_llr = (a.out_llr or os.path.join(a.save_dir, "llr.npy")) if a.llr else None
    for path in (out, out_bits) + ((out_llr,) if a.llr else ()):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(out_bits, "wb") as f:             # (np.save would append .npy to another suffix)
        np.save(f, res["bits"].cpu().numpy())
    if a.llr:
        with open(out_llr, "wb") as f:
            np.save(f, res["llr"].cpu().numpy())
        with open(out, "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(LLR_COLUMNS)
            for i, r in enumerate(frames.tolist()):
                wr.writerow([i, int(offsets[i]), r[3], r[0], r[1], r[4], r[5], r[2]])
        print(f"Decoded {res['decoded']} frames of {res['T']} steps ({res['skipped']} skipped): distance "
              f"{res['total_distance']}, {res['total_zeros']} undecided bits, {res['total_saturated']} saturated")
        print("Saved bits to", out_bits, f"({res['F']} rows of {res['bits'].shape[1]} bytes)")
        print("Saved values to", out_llr, f"({res['F']} rows of {res['T']} int16)")
        print("Saved results to", out)
        return 0
    with open(out, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(TAILBITING_COLUMNS if a.tail_biting else FRAME_COLUMNS)
        for i, r in enumerate(frames.tolist()):
            wr.writerow([i, int(offsets[i]), r[3], r[0], r[4], r[5], r[1], r[2]] + ([r[6]] if a.tail_biting else []))
    print(f"Decoded {res['decoded']} frames of {res['T']} steps ({res['skipped']} skipped): distance "
          f"{res['total_distance']}, {res['total_errors']} channel errors in {res['total_counted']} positions, "
          f"p = {res['ber']!r}")
    if a.tail_biting:
        print(f"Tail-biting: {res['fallback']} frames fell back to the last lap's best tail-biting survivor, "
              f"{res['open']} have none (start_state != end_state); "
              f"{res['total_laps'] / max(res['decoded'], 1):.3f} laps per frame")
    print("Saved bits to", out_bits, f"({res['F']} rows of {res['bits'].shape[1]} bytes)")
    print("Saved results to", out)
    return 0


def cmd_decode(a):
    """Writes the bits and the one-row CSV; ber as repr, so it reads back exactly."""
    if int(os.environ.get("RANK", "0")) != 0:   # single-process: under torchrun rank 0 decodes
        return 0
    import numpy as np
    k, n, m, g1, _ = code_of(a.code)
    if k != 1:
        raise SystemExit(f"decode: {a.code} has k = {k}; the decoder takes k = 1 codes")
    if a.sync is not None and a.puncture is None:
        raise SystemExit("decode: --sync needs --puncture")
    if a.frame is not None:
        return cmd_decode_frames(a, n, m, g1)
    columns = DECODE_COLUMNS
    soft = a.format == "soft"
    if soft:
        capture, offset, keep = load_soft_capture(a.input, a.nbits), 0, None
        if a.puncture is not None:
            try:
                keep = puncture_pattern(a.puncture, n)
            except ValueError as e:
                raise SystemExit(f"decode: {e}")
            if a.sync is not None:
                ranked = sync_punctured_soft(n, m, g1, keep, capture, start=a.start, T=a.sync)
                offset = ranked[0]["offset"]
                print(f"Offsets of a period by soft distance over {a.sync} steps:",
                      ", ".join(f"{r['offset']}: {r['metric']}" for r in ranked))
        res = decode_capture_soft(n, m, g1, capture, start=a.start + offset, T=a.T, keep=keep)
        columns = DECODE_COLUMNS + ["metric", "erasures"]
        if keep is not None:
            res["offset"] = offset
            columns = columns + ["capture_bits", "offset"]
    elif a.puncture is not None:
        try:
            keep = puncture_pattern(a.puncture, n)
        except ValueError as e:
            raise SystemExit(f"decode: {e}")
        capture, offset = load_capture(a.input), 0
        if a.sync is not None:
            ranked = sync_punctured(n, m, g1, keep, capture, start=a.start, T=a.sync, format=a.format, nbits=a.nbits)
            offset = ranked[0]["offset"]
            print(f"Offsets of a period by errors over {a.sync} steps:",
                  ", ".join(f"{r['offset']}: {r['errors']}" for r in ranked))
        res = decode_capture_punctured(n, m, g1, keep, capture, start=a.start + offset, T=a.T, format=a.format,
                                       nbits=a.nbits)
        res["offset"] = offset
        columns = DECODE_COLUMNS + ["capture_bits", "offset"]
    else:
        res = decode_capture(n, m, g1, load_capture(a.input), start=a.start, T=a.T, format=a.format, nbits=a.nbits)
    out = a.out or os.path.join(a.save_dir, "decode.csv")
    out_bits = a.out_bits or os.path.join(a.save_dir, "decoded.npy")
    for path in (out, out_bits):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(out_bits, "wb") as f:             # (np.save would append .npy to another suffix)
        np.save(f, res["bits"].cpu().numpy())
    with open(out, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(columns)
        wr.writerow([repr(res[c]) if c == "ber" else res[c] for c in columns])
    print(f"Decoded {res['T']} steps: {res['errors']} channel errors, p = {res['ber']!r} "
          f"(states {res['start_state']} -> {res['end_state']}; {res['blocks']} blocks, "
          f"{res['forward_reruns']} forward reruns, {res['trace_fixups']} traceback fix-ups)")
    if soft:
        print(f"Soft distance {res['metric']}, {res['erasures']} erasures")
    if a.puncture is not None:
        # no scan line: the detector's model assumes that every output bit is in the capture
        print(f"Punctured {a.puncture}: {res['capture_bits']} capture bits from bit {a.start + res['offset']} "
              f"(offset {res['offset']})")
    elif not soft:                              # (nor for a soft capture: the detector's model is a BSC model)
        print(f"{PROG} scan --code {a.code} --start {a.start} --input {a.input} --format {a.format}"
              + (f" --nbits {a.nbits}" if a.nbits is not None else "") + f" --p {res['ber']!r} --N N")
    print("Saved bits to", out_bits, "(identify --format lsb --nbits", str(res["T"]) + ")")
    print("Saved results to", out)
    return 0


def cmd_encode(a):
    """Writes the capture and prints where the frames lie."""
    if int(os.environ.get("RANK", "0")) != 0:   # single-process: under torchrun rank 0 encodes
        return 0
    import numpy as np
    k, n, m, g1, _ = code_of(a.code)
    if k != 1:
        raise SystemExit(f"encode: {a.code} has k = {k}; the encoder takes k = 1 codes")
    info = np.load(a.input)
    if info.dtype != np.uint8:
        raise SystemExit(f"{a.input}: information bits are uint8 (packed LSB-first), not {info.dtype}")
    kw = dict(start_state=a.start_state or 0, keep=a.puncture, format=a.format, amplitude=a.amplitude)
    try:
        if a.frame is None:
            res = encode_capture(n, m, g1, info.reshape(-1), T=a.T, **kw)
        else:
            if info.ndim != 2:
                raise SystemExit(f"{a.input}: --frame takes rows of bits [F, 4w], not {info.ndim} dimensions")
            mode = "tail-biting" if a.tail_biting else "open" if a.open else "terminated"
            res = encode_frames(n, m, g1, info, a.frame, F=a.frame_count, mode=mode, stride=a.frame_stride, **kw)
    except ValueError as e:
        raise SystemExit(f"encode: {e}")
    out = a.output or os.path.join(a.save_dir, "encoded.npy")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "wb") as f:                  # (np.save would append .npy to another suffix)
        np.save(f, res["capture"].cpu().numpy())
    unit = "values" if a.format == "soft" else "bits"
    print(f"Encoded {res['written']} frames of {res['T']} steps: span {res['span']} {unit}, stride {res['stride']}, "
          f"{res['nbits']} positions ({a.format})")
    if a.frame is None:
        print(f"End state {res['end_state']}")
    print("Saved capture to", out, f"(decode --format {a.format} --nbits {res['nbits']})")
    return 0


def main(argv=None):
    a = parse_args(argv)
    if a.cmd == "encode":
        return cmd_encode(a)
    if a.cmd == "decode":
        return cmd_decode(a)
    if a.cmd == "scan":
        return cmd_scan(a)
    if a.cmd == "identify":
        return cmd_identify(a)
    if a.cmd == "compare":
        from .compare import compare_figures
        for path in compare_figures(a.hybrid, a.baseline, a.outdir):
            print("Saved", path)
        return 0
    dist = _init_dist()
    run = {"experiment": cmd_experiment, "parity": cmd_parity, "exponent": cmd_exponent}[a.cmd]
    df, name, title = run(a)
    if dist is None or dist.get_rank() == 0:
        out = a.out or os.path.join(a.save_dir, name)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        df.to_csv(out, index=False)
        print(title)
        print(df.to_string(index=False))
        print("Saved results to", out)
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
