"""tiff_enc_ref.py (the restatement of the Group 4 TIFF encoder) against Pillow's libtiff: its strips are libtiff's, byte for
byte; its files are read back by Pillow and by tiff_ref.decode as the thresholded picture; and no file is longer than
omr_tiff_bound says.  No GPU."""
import numpy as np
import pytest

import tiff_cases
import tiff_enc_ref as enc
import tiff_ref
from oics import tiff

WIDTHS = tiff_cases.WIDTHS + (63, 64, 65, 2561, 2700)
ROWS = (1, 2, 37)
NOISE = (0.01, 0.1, 0.5, 0.9)
MODES = {"H", "P", "V0", "V+1", "V-1", "V+2", "V-2", "V+3", "V-3"}


def _noise(rows, cols, density, seed):
    return (np.random.RandomState(seed).rand(rows, cols) < density).astype(np.uint8)


def _pictures(cols):
    """[(name, bits)] of one width: every content and every noise density at every row count"""
    out = []
    for rows in ROWS:
        for kind in tiff_cases.CONTENTS:
            out.append(("%s-%dx%d" % (kind, rows, cols), tiff_cases.content(kind, rows, cols, seed=rows * 1000 + cols)))
        for d in NOISE:
            out.append(("noise%g-%dx%d" % (d, rows, cols), _noise(rows, cols, d, rows * 7 + cols)))
    return out


def _pillow_strips(bits, rps):
    """-> (the strips Pillow writes for the picture, the plane they code: 1 inside a "black" run).  Pillow may store
    Photometric 1 with the bits turned round; what is compared is the plane libtiff actually coded."""
    s = tiff_ref.pillow_tiff(bits, "group4", rps)
    h = tiff_ref.parse(s)
    assert h["compression"] == 4 and h["rps"] == min(rps, bits.shape[0])
    plane = bits if h["photometric"] == 0 else 1 - bits
    return tiff_ref.strips_of(s), plane


@pytest.mark.parametrize("cols", WIDTHS)
def test_strips_are_libtiffs(cols):
    for name, bits in _pictures(cols):
        rows = bits.shape[0]
        for rps in sorted({1, min(8, rows), rows}):
            want, plane = _pillow_strips(bits, rps)
            got_rps, got = enc.strips(plane, rps)
            assert got_rps == rps and len(got) == len(want), (name, rps)
            for k in range(len(want)):
                assert got[k] == want[k], (name, rps, k)


def test_every_mode_occurs():
    modes = set()
    for kind in ("checker", "stair", "stair4", "blobs", "text", "white"):
        a = tiff_cases.content(kind, 37, 100, seed=37100)
        (s,) = enc.strips(a, 37)[1]
        m = []
        assert (tiff_ref.t6_decode(s, 37, 100, modes=m) == a).all(), kind
        modes |= set(m)
    assert modes >= MODES, modes


@pytest.mark.parametrize("cols", (1, 9, 64, 257, 2561))
def test_files_read_back_and_stay_below_the_bound(cols):
    for name, bits in _pictures(cols):
        rows = bits.shape[0]
        img = np.where(bits != 0, 0, 255).astype(np.uint8)
        for rps, dpi in ((0, 0), (1, 300), (8, 0)):
            s = enc.encode(img, 127, rps, dpi)
            assert (tiff_ref.decode(s) == img).all(), (name, rps)
            assert (tiff_ref.pillow_read(s) == img).all(), (name, rps)
            assert len(s) <= tiff.bound(rows, cols, rps) == enc.bound(rows, cols, rps), (name, rps)
            h = tiff_ref.parse(s)
            assert all(off % 2 == 0 for off, _ in h["strips"]) and h["photometric"] == 0 and h["fill_order"] == 1
    if cols == 257:
        from PIL import Image
        import io
        im = Image.open(io.BytesIO(enc.encode(np.full((3, cols), 255, np.uint8), 127, 0, 300)))
        assert im.info["dpi"] == (300, 300)


def test_worst_rows_stay_below_the_row_bound():
    """checker, vertical stripes of every period up to 8 and noise at 0.5: the longest codes there are"""
    for cols in (1, 2, 3, 64, 257, 1000):
        rows = [np.arange(cols) % 2, 1 - np.arange(cols) % 2, _noise(1, cols, 0.5, cols)[0], np.zeros(cols, int), np.ones(cols, int)]
        rows += [(np.arange(cols) // p) % 2 for p in range(2, 9)]
        worst = 0
        for bp in rows:
            for rp in rows:
                cs, steps = enc.row_codes(bp, rp)
                worst = max(worst, sum(b for _, b in cs))
                assert sum(b for _, b in cs) <= enc.row_bound(cols) and steps <= 2 * cols + 2
        # alternating pixels under a white line are among them: 12 bits a pair, so the bound is not idle
        assert cols < 64 or worst >= 6 * (cols - 2)


def test_threshold_and_gray():
    g = np.arange(256, dtype=np.uint8).reshape(1, 256)
    for thr in (0, 127, 254):
        b = enc.threshold(g, thr)
        assert b[0, thr] == 1 and b[0, thr + 1] == 0 and b.sum() == thr + 1
    # the weights of bgr.hpp: byte 0 takes the R weight; (the device's own conversion: test_gpu_tiff_encode.py)
    bgr = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [10, 20, 30]]], np.uint8)
    assert enc.gray_of(bgr).tolist() == [[76, 150, 29, 255, 18]]
