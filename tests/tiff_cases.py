"""The bilevel TIFF inputs of test_tiff_ref.py and the GPU TIFF tests, made at run time with Pillow (libtiff) and
tiff_ref.py's assembler: shapes x RowsPerStrip x compressions x contents, each content chosen to force a mode of T.6, with
Photometric, FillOrder and the byte order cycled through the cases."""
import functools

import numpy as np

import tiff_ref

WIDTHS = (1, 7, 8, 9, 31, 32, 33, 100, 257)
ROWS = (1, 2, 37)
CONTENTS = ("white", "black", "checker", "stair", "stair4", "blobs", "text", "endblack")
COMPRESSIONS = (("group4", 4), ("packbits", 32773), ("raw", 1))


def content(kind, rows, cols, seed=0):
    """-> uint8 [rows, cols], 1 = black"""
    rng = np.random.RandomState(1000 + seed)
    a = np.zeros((rows, cols), np.uint8)
    y, x = np.mgrid[0:rows, 0:cols]
    if kind == "black":
        a[:] = 1
    elif kind == "checker":  # horizontal mode throughout
        a = ((x + y) & 1).astype(np.uint8)
    elif kind in ("stair", "stair4"):  # an edge that moves by -3 .. +3 (every vertical code) or by 4 (back to horizontal) a row
        steps = (0, 1, -1, 2, -2, 3, -3) if kind == "stair" else (4, -4, 4, 4, -4)
        e0, e1 = cols // 3, 2 * cols // 3 + 1
        for r in range(rows):
            e0 = int(np.clip(e0 + steps[r % len(steps)], 0, cols))
            e1 = int(np.clip(e1 - steps[(r + 3) % len(steps)], 0, cols))
            a[r, min(e0, e1):max(e0, e1)] = 1
    elif kind == "blobs":  # isolated blobs under white rows: pass mode
        for r in range(0, rows, 3):
            for c in range(int(rng.randint(0, 5)), cols, 11):
                a[r, c:c + int(rng.randint(1, 6))] = 1
    elif kind == "text":  # random runs
        for r in range(rows):
            c, v = 0, 0
            while c < cols:
                n = int(rng.choice((1, 2, 3, 5, 9, 17, 70)))
                a[r, c:c + n] = v
                c, v = c + n, v ^ 1
            if r and rng.rand() < 0.5:
                a[r] = a[r - 1]
    elif kind == "endblack":  # every row ends in black
        for r in range(rows):
            a[r, max(0, cols - 1 - r % 3):] = 1
    return a


@functools.lru_cache(maxsize=None)
def small_cases():
    """[(name, stream)]: every shape, RowsPerStrip, compression and content; case k's Photometric, FillOrder and byte order
    come from the bits of a counter that runs through all eight variants for every (compression, content) pair"""
    out = []
    k = 0
    for comp, _ in COMPRESSIONS:
        for kind in CONTENTS:
            k += 1
            for rows in ROWS:
                for cols in WIDTHS:
                    for rps in sorted({1, min(8, rows), rows}):
                        a = content(kind, rows, cols, seed=rows * 1000 + cols)
                        base = tiff_ref.pillow_tiff(a, comp, rps)
                        photo, fill, order = k & 1, 1 + (k >> 1 & 1), "<>"[k >> 2 & 1]
                        if photo:  # the strips say the same bits; what they mean is turned round
                            base = tiff_ref.pillow_tiff(1 - a, comp, rps)
                        s = tiff_ref.rewrap(base, photometric=photo, fill_order=fill, order=order,
                                            offsets_type=3 if k & 8 else 4, counts_type=3 if k & 16 else 4)
                        out.append(("%s-%s-%dx%d-rps%d-p%d-f%d-%s" % (comp, kind, rows, cols, rps, photo, fill, "II" if order == "<" else "MM"), s))
                        k += 1
    return out


def long_run_cases():
    a = np.zeros((2, 5200), np.uint8)
    a[0, 5000:] = 1
    return [("long-white", tiff_ref.pillow_tiff(a)), ("long-black", tiff_ref.pillow_tiff(1 - a)),
            ("wide-white", tiff_ref.pillow_tiff(np.zeros((1, 2561), np.uint8)))]
