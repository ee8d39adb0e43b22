"""Randomised parity run of the correct_default batch (omr_correct_batch_*) against the CPU oracle (development aid; a
fixed slice runs in tests/test_gpu_correct_front.py): random sheet shapes and projection limits, weighted toward integer
shrink factors 1..80 (kx = ky and kx != ky) and fractional shrinks, with some enlargements; 1 or 3 channels; random row
padding, guard rows and base offsets; n = 1..70 sheets of random content kinds (tests/correct_sheets.py).
Every case checks omr_correct_batch_front_device's projection-size images byte for byte against
resize_area(erode_cross3(gray)), then runs up to 12 structured sheets (cards, Hough-fallback sheets, blank) of the same
context through omr_correct_batch_run_device and checks scan_rc, the angle bits, need_check and every canvas byte against
the oracle's composition.
Usage: python tests/fuzz/fuzz_correct.py [cases] [seed]"""
import os
import struct
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

import correct_sheets as cs
from oics import omr
from oracle import oracle as orc

MODES = {omr.FRONT_AREA_FUSED: "fused", omr.FRONT_AREA_INT: "int", omr.FRONT_AREA_GENERAL: "general",
         omr.FRONT_LINEAR: "linear"}
PIXELS = 24 << 20  # sheet pixels per case


def bits(x):
    return struct.pack("<d", float(x)).hex()


def pick_shape(rng):
    """-> (rows, cols, max_w, max_h) with a non-empty projection size"""
    while True:
        w = rng.random()
        if w < 0.35:  # one integer factor on both axes
            k = int(rng.choice([1, 2, 3, 5, 17, 64, 65, 80])) if rng.random() < 0.4 else int(rng.integers(1, 81))
            dr, dc = int(rng.integers(1, max(2, 1400 // k))), int(rng.integers(1, max(2, 1400 // k)))
            rows, cols, mw, mh = dr * k, dc * k, dc, dr
        elif w < 0.6:  # kx != ky: the axis with the larger limit rounds down (few output rows or columns)
            kx = int(rng.integers(1, 81))
            dc, dr = int(rng.integers(1, max(2, 1400 // kx))), int(rng.integers(1, 5))
            ky = int(rng.integers(kx, max(kx + 1, (kx * (dr + 1) + dr - 1) // dr)))
            rows, cols, mw, mh = dr * ky, dc * kx, dc, 32000
            if rng.random() < 0.5:  # the same with the axes swapped
                rows, cols, mw, mh = cols, rows, 32000, dc
        elif w < 0.9:  # a fractional shrink
            rows, cols = int(rng.integers(8, 1400)), int(rng.integers(8, 1400))
            mw, mh = int(rng.integers(1, cols + 1)), int(rng.integers(1, rows + 1))
        else:  # an axis enlarges
            rows, cols = int(rng.integers(8, 300)), int(rng.integers(8, 300))
            mw, mh = int(rng.integers(cols, 2 * cols + 2)), int(rng.integers(rows, 2 * rows + 2))
        if 8 <= rows < 4096 and 8 <= cols < 4096 and min(cs.proj_size(rows, cols, mw, mh)) > 0:
            return rows, cols, mw, mh


def run_case(c, rng, ex):
    rows, cols, mw, mh = pick_shape(rng)
    cn = int(rng.choice([1, 3]))
    n = int(rng.integers(1, 71))
    n = max(1, min(n, PIXELS // (rows * cols)))
    pad = int(rng.integers(0, 9))
    guard = int(rng.integers(0, 3))
    off = int(rng.integers(0, 4))
    params = (45, 0.2, mw, mh, 150.0, 50.0)
    cb = omr.CorrectBatch(rows, cols, cn, *params, max_scans=max(n, 12))
    dr, dc, mode, kx, ky = cb.info()
    assert (dr, dc) == cs.proj_size(rows, cols, mw, mh)
    kinds = [str(rng.choice(cs.KINDS[:5])) for _ in range(n)]
    seeds = [int(rng.integers(0, 1 << 30)) for _ in range(n)]
    sheets = list(ex.map(lambda i: cs.sheet(kinds[i], rows, cols, cn, seeds[i]), range(n)))
    # front end
    buf, stride, step = cs.layout(sheets, pad, guard, off)
    d = torch.from_numpy(buf).to("cuda:0")
    sstep, sstride = dc + 1, (dc + 1) * dr + 3
    out = torch.full((n * sstride,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cb.front_device(d.data_ptr() + off, stride, step, n, out.data_ptr(), sstride, sstep)
    host = out.cpu().numpy().reshape(n, sstride)
    exp = list(ex.map(lambda s: cs.front(orc, s, dr, dc), sheets))
    bad_front = [i for i in range(n) if not np.array_equal(host[i, :dr * sstep].reshape(dr, sstep)[:, :dc], exp[i])]
    del d
    # decisions and canvases of structured sheets
    m = min(12, n)
    dk = [str(rng.choice(["card", "bars", "bars", "blank"] if rng.random() < 0.2 else ["card", "bars"])) for _ in range(m)]
    dsheets = list(ex.map(lambda i: cs.sheet(dk[i], rows, cols, cn, seeds[i] + 1), range(m)))
    buf, stride, step = cs.layout(dsheets, pad, guard, off)
    d = torch.from_numpy(buf).to("cuda:0")
    R, Cc = cb.canvas
    ostep = Cc * cn
    o = torch.zeros((m, R * ostep), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ang, chk, src, size = cb.run_device(d.data_ptr() + off, stride, step, m, o.data_ptr(), R * ostep, ostep)
    oh = o.cpu().numpy()
    cb.close()
    ref = list(ex.map(lambda s: cs.correct(orc, s, params), dsheets))
    bad_dec = []
    for i, (erc, ea, ec, eimg) in enumerate(ref):
        ok = src[i] == erc
        if ok and erc == 0:
            r, cc = size[i]
            got = oh[i].reshape(R, ostep)[:r, :cc * cn]
            ok = (bits(ang[i]) == bits(ea) and bool(chk[i]) == ec and (r, cc) == eimg.shape[:2]
                  and np.array_equal(got, eimg.reshape(r, cc * cn)))
        if not ok:
            bad_dec.append(i)
    desc = "%dx%dx%d -> %dx%d %s (%d, %d), n %d, pad %d, guard %d, offset %d" % (rows, cols, cn, dr, dc, MODES[mode], kx, ky, n,
                                                                                pad, guard, off)
    ok = not bad_front and not bad_dec
    print("case %d: %s: %s" % (c, desc, "ok" if ok else "MISMATCH front %s decisions %s" % (bad_front, bad_dec)), flush=True)
    return mode, ok, desc


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    orc.build()
    bad, seen = [], {}
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        for c in range(cases):
            mode, ok, desc = run_case(c, rng, ex)
            seen[MODES[mode]] = seen.get(MODES[mode], 0) + 1
            if not ok:
                bad.append((c, desc))
    print("fuzz_correct: %d cases %s, %d mismatches %s" % (cases, seen, len(bad), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
