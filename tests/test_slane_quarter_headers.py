"""The turn headers of the scan-lane sweep's programs (slane.hpp: slane_turn_header) on the CPU.  The wave
program decides every FOUR rows how many segment slots per word it executes: a turn's first record holds the most segments any
word of its 16 rows needs (what oracle/slane_interp.c reads), its second record the most of rows 0 .. 3, the records at rows 4,
8 and 12 the most of their own four rows, every other record the turn's.  Checked on every strip of every candidate of two
small shapes at +-10 degrees @ 0.5 (the second one's width is 30 modulo 32: the moved grid) and of A4 at -10, 0.05 and +9.95
degrees: each value is the EXACT maximum of its rows' word counts, the interpreter still accepts every program and
reproduces the oracle's sweep, and the small shapes do hold turns whose quarters differ (or none of this would be tested)."""
import ctypes as C

import numpy as np
import pytest

import oics
from oracle import oracle as orc

u32p = C.POINTER(C.c_uint32)
f64p = C.POINTER(C.c_double)
TURN, QUARTER = 16, 4  # SL_TURN, SL_QUARTER (slane.hpp)


def grid(cols):
    """slane_grid_offset / SlaneGeom::set: columns that do not exist in front of column 0, strips"""
    off = (32 - cols % 32) % 32
    if 1 <= off <= 3:
        off += 16
    return off, ((cols + off + 31) // 32 + 1) // 2


def strip_program(rows, cols, M, strip):
    L = oics.lib()
    rd, nrec, pre, most, gx, gy = (C.c_int32() for _ in range(6))
    refs = [C.byref(x) for x in (rd, nrec, pre, most, gx, gy)]
    Mc = np.ascontiguousarray(M, np.float64)
    rc = L.omr_slane_strip_program(rows, cols, Mc.ctypes.data_as(f64p), strip, None, None, *refs)
    assert rc == 0, L.omr_last_error()
    seg = np.zeros(rd.value * nrec.value, np.uint32)
    fet = np.zeros(4 * nrec.value, np.uint32)
    rc = L.omr_slane_strip_program(rows, cols, Mc.ctypes.data_as(f64p), strip, seg.ctypes.data_as(u32p), fet.ctypes.data_as(u32p), *refs)
    assert rc == 0, L.omr_last_error()
    return seg, fet, rd.value, nrec.value, pre.value, gx.value, gy.value


def interleave(scans, gx, gy):
    """[lanes] binary u8 images -> entries[1 + (rows + 2 gy) * colsG][lanes] dwords (entry 0 and the guard zero)"""
    rows, cols = scans[0].shape
    NW = (cols + 31) // 32
    colsG = NW + 2 * gx
    ent = np.zeros((1 + (rows + 2 * gy) * colsG, len(scans)), np.uint32)
    for ln, img in enumerate(scans):
        black = np.zeros((rows, NW * 32), np.uint8)
        black[:, :cols] = img <= 127
        words = np.packbits(black.reshape(rows, NW, 32), axis=2, bitorder="little").view(np.uint32).reshape(rows, NW)
        ent[1:, ln].reshape(rows + 2 * gy, colsG)[gy:gy + rows, gx:gx + NW] = words
    return ent


def check_headers(seg, fet, rd, nrec, what):
    """-> turns whose quarters do not all hold the same value"""
    assert nrec % TURN == 0
    S = rd // 2
    n = ((seg.reshape(nrec, 2, S)[:, :, 0] >> 26) & 15).astype(np.int64)  # the words' own segment counts
    quarters = n.max(axis=1).reshape(-1, TURN // QUARTER, QUARTER).max(axis=2)  # [turn][quarter]: exact maxima
    turn = quarters.max(axis=1)
    hdr = fet.reshape(-1, TURN, 4)[:, :, 3].astype(np.int64)
    assert (hdr[:, 0] == turn).all(), "%s: a turn's first record does not hold the turn's maximum" % what
    assert (hdr[:, 1] == quarters[:, 0]).all(), "%s: the second record does not hold quarter 0's maximum" % what
    for qt in range(1, TURN // QUARTER):
        assert (hdr[:, qt * QUARTER] == quarters[:, qt]).all(), "%s: row %d does not hold its quarter's maximum" % (what, qt * QUARTER)
    assert (quarters <= turn[:, None]).all() and (quarters >= 1).all() and (turn <= S).all()
    others = [r for r in range(TURN) if r != 1 and r % QUARTER]
    assert (hdr[:, others] == turn[:, None]).all(), "%s: a record the kernel does not read differs from the turn's maximum" % what
    return int(np.count_nonzero(quarters.min(axis=1) != turn))


def sweep_and_check(scans, Ms, what):
    """every strip of every candidate: headers, then the interpreter against the oracle's sweep -> turns with differing quarters"""
    orc.build()
    OL = orc.lib()
    OL.orc_slane_run_strip.argtypes = [u32p, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.c_int, u32p, C.c_int64, C.c_int, u32p, u32p]
    OL.orc_slane_run_strip.restype = C.c_int
    lanes = len(scans)
    rows, cols = scans[0].shape
    off, NS = grid(cols)
    ents, mixed = {}, 0
    vp = np.zeros((lanes, len(Ms), cols), np.uint32)
    hp = np.zeros((lanes, len(Ms), rows), np.uint32)
    for a, M in enumerate(Ms):
        hrow = np.zeros((rows, lanes), np.uint32)
        for st in range(NS):
            seg, fet, rd, nrec, pre, gx, gy = strip_program(rows, cols, M, st)
            mixed += check_headers(seg, fet, rd, nrec, "%s candidate %d strip %d" % (what, a, st))
            if (gx, gy) not in ents:
                ents[(gx, gy)] = interleave(scans, gx, gy)
            ent = ents[(gx, gy)]
            vcol = np.zeros((64, lanes), np.uint32)
            rc = OL.orc_slane_run_strip(seg.ctypes.data_as(u32p), rd, fet.ctypes.data_as(u32p), nrec, pre, rows, 2, ent.ctypes.data_as(u32p),
                                        ent.shape[0], lanes, hrow.ctypes.data_as(u32p), vcol.ctypes.data_as(u32p))
            assert rc == 0, "%s: the interpreter rejected the program of candidate %d strip %d" % (what, a, st)
            for b in range(64):
                col = st * 64 - off + b
                if 0 <= col < cols:
                    vp[:, a, col] = vcol[b]
                else:
                    assert (vcol[b] == 0).all()
        hp[:, a, :] = hrow.T
    for ln, img in enumerate(scans):
        evp, ehp, _, _ = orc.sweep_matrices(img, Ms, threads=4, fast=rows > 1000)
        assert (vp[ln] == evp).all(), "%s: column counts differ, lane %d" % (what, ln)
        assert (hp[ln] == ehp).all(), "%s: row counts differ, lane %d" % (what, ln)
    return mixed


@pytest.mark.parametrize("rows,cols", [(70, 100), (200, 94)])
def test_small_shapes_every_strip_of_the_sweep(rows, cols):
    rng = np.random.Generator(np.random.PCG64(rows * 1000 + cols))
    scans = [np.where(rng.random((rows, cols)) < d, 0, 255).astype(np.uint8) for d in (0.5, 0.07)]
    scans += [np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8)]
    mixed = sweep_and_check(scans, orc.rotation_matrices(rows, cols, 10, 0.5), "%d x %d" % (rows, cols))
    assert mixed > 0, "no turn of this shape has two different quarter values: the quarter headers were not exercised"


def test_a4_at_the_sweeps_edges_and_near_zero():
    rows, cols = 3508, 2480
    rng = np.random.Generator(np.random.PCG64(11))
    scans = [np.where(rng.random((rows, cols)) < d, 0, 255).astype(np.uint8) for d in (0.3, 0.02)]
    Mall = orc.rotation_matrices(rows, cols, 10, 0.05)
    pick = [0, 201, 399]  # -10, +0.05 and +9.95 degrees
    assert len(Mall) == 400
    sweep_and_check(scans, Mall[pick], "A4")
