"""How many segment slots per word the scan-lane sweep EXECUTES, against what its words need: the host
generator's programs (omr_slane_strip_program, csrc/slane_plan.cpp -- no GPU involved) of every strip of every candidate of a
plan, and from their words' own segment counts the mean executed slots per word when the count is decided every 16, 8, 4 rows
(aligned within the turn of 16) or every row; beside it the share of decisions that differ from the one before (what walks a
dispatch stub of the wave program, tools/gen_slane_asm.py).  Every record of the streams counts, virtual rows included: the
wave executes them too.  Also checks the headers the generator wrote against the counts (slane_turn_header, slane.hpp).

Usage: python tools/slane_slot_stats.py [--rows 3508 --cols 2480 --max-angle 10 --step 0.05 --jobs N]"""
import argparse
import ctypes as C
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "omr-img-corrector_amd")]

INTERVALS = (16, 8, 4, 1)
u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)


def strip_counts(rows, cols, M, strip):
    """-> (segment counts [records][2 words], turn headers [records]) of one strip's program"""
    import oics
    L = oics.lib()
    rd, nrec, pre, most, gx, gy = (C.c_int32() for _ in range(6))
    Mc = np.ascontiguousarray(M, np.float64)
    refs = [C.byref(x) for x in (rd, nrec, pre, most, gx, gy)]
    if L.omr_slane_strip_program(rows, cols, Mc.ctypes.data_as(f64p), strip, None, None, *refs) != 0:
        raise SystemExit("strip %d does not fit: %s" % (strip, L.omr_last_error()))
    seg = np.zeros(rd.value * nrec.value, np.uint32)
    fet = np.zeros(4 * nrec.value, np.uint32)
    if L.omr_slane_strip_program(rows, cols, Mc.ctypes.data_as(f64p), strip, seg.ctypes.data_as(u32p), fet.ctypes.data_as(u32p), *refs) != 0:
        raise SystemExit("strip %d: %s" % (strip, L.omr_last_error()))
    S = rd.value // 2
    n = (seg.reshape(nrec.value, 2, S)[:, :, 0] >> 26) & 15
    return n.astype(np.int64), fet.reshape(nrec.value, 4)[:, 3].astype(np.int64)


def candidate_stats(job):
    """one candidate, every strip -> per interval (slots executed summed over words, decisions, decisions that changed), words,
    segments the words hold"""
    rows, cols, M = job
    off = (32 - cols % 32) % 32
    off += 16 if 1 <= off <= 3 else 0
    NS = ((cols + off + 31) // 32 + 1) // 2
    acc = np.zeros((len(INTERVALS), 3), np.int64)
    words = own = 0
    for st in range(NS):
        n, hdr = strip_counts(rows, cols, M, st)
        row_most = n.max(axis=1)
        words += n.size
        for i, iv in enumerate(INTERVALS):
            dec = row_most.reshape(-1, iv).max(axis=1)
            acc[i] += (2 * iv * dec.sum(), dec.size - 1, np.count_nonzero(dec[1:] != dec[:-1]))
        # the headers as the wave program reads them: first record the turn's maximum, second quarter 0's, rows 4 / 8 / 12 their quarter's
        q4 = row_most.reshape(-1, 4, 4).max(axis=2)
        h = hdr.reshape(-1, 16)
        want = np.repeat(q4.max(axis=1)[:, None], 16, axis=1)
        want[:, 1], want[:, 4], want[:, 8], want[:, 12] = q4[:, 0], q4[:, 1], q4[:, 2], q4[:, 3]
        assert (h == want).all(), "turn headers of strip %d differ from the words' counts" % st
        own += int(n.sum())
    return acc, words, own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3508)
    ap.add_argument("--cols", type=int, default=2480)
    ap.add_argument("--max-angle", type=float, default=10)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    from oracle import oracle as orc
    Ms = orc.rotation_matrices(a.rows, a.cols, a.max_angle, a.step)
    with Pool(a.jobs) as pool:
        parts = pool.map(candidate_stats, [(a.rows, a.cols, M) for M in Ms], chunksize=1)
    acc = sum(p[0] for p in parts)
    words = sum(p[1] for p in parts)
    own = sum(p[2] for p in parts)
    print("%d x %d, +-%g @ %g: %d candidates, %d words, %.3f segments per word" % (a.rows, a.cols, a.max_angle, a.step, len(Ms), words, own / words))
    print("| decided every | executed slots per word | decisions that differ from the one before |")
    print("|---|---|---|")
    for i, iv in enumerate(INTERVALS):
        print("| %d rows | %.3f | %.2f %% |" % (iv, acc[i, 0] / words, 100.0 * acc[i, 2] / max(1, acc[i, 1])))


if __name__ == "__main__":
    main()
