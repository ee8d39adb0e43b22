"""Randomised parity run of omr_lined_picture_device / _batch_device against the restatement of cv::line(.., LINE_AA)
(tests/lined_ref.py): random shapes (1..200 per side, on both sides of the 64-pixel tiles and 128-pixel workgroups),
edge maps of 0 / 255 or of any bytes, 0..400 segments a picture -- anywhere, short, along tile borders, repeated --
odd buffer offsets, pitches and batch strides over a sentinel canvas, batches of 1..5 with a segment list each.  Every
byte is compared; the pitch padding and a guard band behind the last row must stay untouched.  Stops at the first
mismatch, prints the case and exits 1.
Usage: python tests/fuzz/fuzz_lined_picture.py [cases] [seed]"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

import lined_ref as lr
from oics import _lib

SENTINEL = 0xA5
GUARD = 64  # sentinel bytes behind the last row of a picture (and behind the last picture of a batch)


def device_pictures(edges, lines, eo=0, ep=None, egap=0, oo=0, op=None, ogap=0, lead=0, color=lr.COLOR, batch=None):
    """edges: list of (rows, cols) u8 arrays of one shape; lines: one int32 [k, 4] array per edge map -> (list of
    (rows, cols, 3) pictures or None, error text or None).  One map goes through omr_lined_picture_device unless
    batch=True.  Buffers start eo / oo bytes into their allocations, rows ep / op apart, images rows * pitch + gap
    apart; `lead` unused segments sit in front of the first list (line_offsets[0] = lead)."""
    n = len(edges)
    rows, cols = edges[0].shape
    ep = cols if ep is None else ep
    op = 3 * cols if op is None else op
    estride, ostride = rows * ep + egap, rows * op + ogap
    ebuf = np.zeros(eo + n * estride + 4, np.uint8)
    for i, a in enumerate(edges):
        ebuf[eo + i * estride:eo + i * estride + rows * ep].reshape(rows, ep)[:, :cols] = a
    lists = [np.asarray(l, np.int32).reshape(-1, 4) for l in lines]
    off = np.cumsum([lead] + [len(l) for l in lists]).astype(np.int32)
    flat = np.concatenate([np.full((lead, 4), -7, np.int32)] + lists) if off[-1] else np.zeros((0, 4), np.int32)
    d_e = torch.from_numpy(ebuf).cuda()
    d_l = torch.from_numpy(np.ascontiguousarray(flat).reshape(-1)).cuda() if len(flat) else None
    d_o = torch.full((oo + n * ostride + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bgr = (C.c_uint8 * 3)(*color)
    pl = C.c_void_p(d_l.data_ptr()) if d_l is not None else None
    if batch or (batch is None and n > 1):
        rc = _lib.lib().omr_lined_picture_batch_device(C.c_void_p(d_e.data_ptr() + eo), n, estride, ep, rows, cols, pl,
                                                       off.ctypes.data_as(_lib.i32p), bgr, C.c_void_p(d_o.data_ptr() + oo),
                                                       ostride, op, None)
    else:
        assert lead == 0
        rc = _lib.lib().omr_lined_picture_device(C.c_void_p(d_e.data_ptr() + eo), ep, rows, cols, pl, len(lists[0]), bgr,
                                                 C.c_void_p(d_o.data_ptr() + oo), op, None)
    torch.cuda.synchronize()
    if rc != 0:
        return None, "rc %d: %s" % (rc, _lib.lib().omr_last_error().decode())
    if (d_e.cpu().numpy() != ebuf).any():
        return None, "wrote to the edge map"
    buf = d_o.cpu().numpy()
    if (buf[:oo] != SENTINEL).any() or (buf[oo + n * ostride:] != SENTINEL).any():
        return None, "wrote outside the canvas"
    pics = []
    for i in range(n):
        blk = buf[oo + i * ostride:oo + (i + 1) * ostride]
        grid = blk[:rows * op].reshape(rows, op)
        if (grid[:, 3 * cols:] != SENTINEL).any() or (blk[rows * op:] != SENTINEL).any():
            return None, "wrote outside picture %d's rows" % i
        pics.append(grid[:, :3 * cols].reshape(rows, cols, 3).copy())
    return pics, None


def random_lines(rng, rows, cols, k, kind):
    x0, y0 = rng.integers(0, cols, k), rng.integers(0, rows, k)
    if kind == "short":
        x1 = np.clip(x0 + rng.integers(-9, 10, k), 0, cols - 1)
        y1 = np.clip(y0 + rng.integers(-9, 10, k), 0, rows - 1)
    elif kind == "border":  # on and beside the 64-pixel tile borders, axis-parallel and nearly so
        x1, y1 = rng.integers(0, cols, k), rng.integers(0, rows, k)
        for a, b, size in ((x0, x1, cols), (y0, y1, rows)):
            t = np.clip(64 * rng.integers(0, 4, k) + rng.integers(-2, 2, k), 0, size - 1)
            pick = rng.random(k) < 0.5
            a[pick] = t[pick]
            b[pick] = np.clip(t[pick] + rng.integers(-1, 2, int(pick.sum())), 0, size - 1)
    else:
        x1, y1 = rng.integers(0, cols, k), rng.integers(0, rows, k)
    l = np.stack([x0, y0, x1, y1], 1).astype(np.int32)
    if k > 3 and rng.random() < 0.3:
        l[k // 2] = l[0]  # a segment listed twice
    return l


def run_case(rng):
    rows, cols = (int(v) for v in rng.integers(1, 201, 2))
    n = int(rng.integers(1, 6))
    binary = rng.random() < 0.5
    edges = [(rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8) if binary else
             rng.integers(0, 256, (rows, cols), dtype=np.uint8) for _ in range(n)]
    kind = ("any", "short", "border")[int(rng.integers(0, 3))]
    lines = [random_lines(rng, rows, cols, int(rng.integers(0, 401)) if rng.random() < 0.8 else 0, kind) for _ in range(n)]
    eo, oo = (int(v) for v in rng.integers(0, 4, 2))
    ep, op = cols + int(rng.integers(0, 6)), 3 * cols + int(rng.integers(0, 6))
    egap, ogap = (int(v) for v in rng.integers(0, 9, 2))
    batch = n > 1 or rng.random() < 0.3
    lead = int(rng.integers(0, 3)) if batch else 0
    case = (rows, cols, n, binary, kind, [len(l) for l in lines], eo, ep, egap, oo, op, ogap, lead, batch)
    pics, err = device_pictures(edges, lines, eo, ep, egap, oo, op, ogap, lead, batch=batch)
    if err:
        return case, err
    for i in range(n):
        want = lr.lined_picture(edges[i], lines[i])
        if not np.array_equal(pics[i], want):
            return case, "picture %d: %d bytes differ" % (i, int((pics[i] != want).sum()))
    return case, None


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    for i in range(cases):
        case, err = run_case(rng)
        if err:
            print("case", i, case,
                  "(rows, cols, n, binary, kind, segments, eo, ep, egap, oo, op, ogap, lead, batch):", err)
            sys.exit(1)
    print("cases", cases, "mismatches 0")
    sys.exit(0)


if __name__ == "__main__":
    main()
