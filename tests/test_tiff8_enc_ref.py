"""The restatement of the 8-bit TIFF encoder (tests/tiff8_enc_ref.py) against two independent readers -- Pillow's libtiff
and the decoder's restatement tests/tiff8_ref.py -- and omr_tiff8_bound against the restatement's lengths.  No device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tiff8_enc_ref as ref  # noqa: E402
import tiff8_ref  # noqa: E402
from oics import tiff  # noqa: E402

WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)
MODES = ((1, 1), (5, 1), (5, 2))  # (compression, predictor)


def picture(kind, rows, cols, cn, seed=0):
    """gray [rows, cols] or BGR [rows, cols, 3]"""
    return tiff8_ref.content(kind, rows, cols, 1 if cn == 1 else 3, seed)


def as_read(img):
    """what a reader of the file returns for the BGR or gray image: RGB or gray"""
    return img if img.ndim == 2 else img[..., ::-1]


def both_readers(s, img):
    assert (tiff8_ref.pillow_read(s) == as_read(img)).all()
    assert (tiff8_ref.decode(s) == as_read(img)).all()


@pytest.mark.parametrize("cn", [1, 3])
def test_both_readers_return_the_picture(cn):
    k = 0
    for comp, pred in MODES:
        for kind in ("noise", "text", "gradient", "constant", "period2"):
            for rows, cols, rps in ((1, 1, 0), (7, 65, 0), (7, 65, 3), (40, 129, 0), (33, 257, 33), (5, 3, 12)):
                k += 1
                img = picture(kind, rows, cols, cn, k)
                s = ref.encode(img, comp, pred, rps, 300 if k & 1 else 0)
                both_readers(s, img)
                h = tiff8_ref.parse(s)
                assert h["compression"] == comp and h["predictor"] == pred and h["spp"] == cn
                assert all(off % 2 == 0 for off, _ in h["strips"])
                assert h["rps"] == ref.rows_of_strip(rows, cols, cn, rps)


def test_the_table_fills_and_clear_stands_at_3836():
    raw = tiff8_ref.content("noise", 64, 256, 1, 3).tobytes()
    codes = ref.lzw_codes(raw)
    clears = [i for c, i in codes[1:] if c == ref.CLEAR]
    assert len(clears) >= 3 and set(clears) == {ref.CLEAR_AT}
    assert max(i for c, i in codes if i is not None) == ref.CLEAR_AT
    img = np.frombuffer(raw, np.uint8).reshape(64, 256)
    both_readers(ref.encode(img, 5, 1, 64), img)
    # a strip that ends one byte before, at and one byte behind a Clear: the last match has index 3834, 3835, 0
    n = next(n for n in range(3000, len(raw)) if ref.lzw_codes(raw[:n])[-2] == (ref.CLEAR, ref.CLEAR_AT))
    assert ref.lzw_codes(raw[:n])[-1] == (ref.EOI, 0)
    for m in (n - 1, n, n + 1):
        img = np.frombuffer(raw[:m], np.uint8).reshape(1, m)
        both_readers(ref.encode(img, 5, 1, 1), img)
    # long entries: a constant strip, period 2 and period 3
    for img in (np.full((64, 256), 200, np.uint8), np.tile(np.array([0, 255], np.uint8), (64, 128)),
                np.tile(np.array([1, 2, 3], np.uint8), (64, 86))):
        both_readers(ref.encode(img, 5, 1, 64), img)


def test_widths_switch_at_254_766_and_1790():
    raw = ref.pairless_noise(1800, 7)
    for lo in (250, 762, 1786):
        counts = [ref.code_counts(raw[:n].tobytes())[0] for n in range(lo, lo + 11)]
        edge = {250: 254, 762: 766, 1786: 1790}[lo]
        # n codes and EOI: EOI has index n, so the strips take it and their last codes to both sides of the switch
        assert counts == list(range(lo, lo + 11)) and counts[0] < edge - 1 and counts[-1] > edge + 1, (lo, counts)
        for n in range(lo, lo + 11):
            img = raw[:n].reshape(1, n)
            both_readers(ref.encode(img, 5, 1, 1), img)


def test_predictor_pictures():
    ramp = np.tile(np.arange(256, dtype=np.uint8), (3, 2))[:, 3:500]
    cols = np.tile(np.array([0, 255], np.uint8), (5, 33))
    colour = tiff8_ref.content("noise", 9, 70, 3, 5)
    colour[..., 1] = 77  # differences per sample, not per byte: G stays a run of zeros
    for img in (ramp, cols, colour):
        s = ref.encode(img, 5, 2, 2)
        both_readers(s, img)
    raws, _ = ref.raw_strips(colour, 2, 100)
    d = np.frombuffer(raws[0], np.uint8).reshape(9, 70, 3)
    assert (d[:, 1:, 1] == 0).all() and (d[:, 0, 1] == 77).all()
    raws, _ = ref.raw_strips(cols, 2, 100)
    assert set(np.frombuffer(raws[0], np.uint8).reshape(5, 66)[:, 1:].ravel()) == {1, 255}  # 0 - 255 = 1 mod 256


@pytest.mark.parametrize("cn", [1, 3])
def test_bound_holds_and_equals_its_formula(cn):
    for comp, pred in MODES:
        for cols in WIDTHS:
            for rows in (1, 2, 7):
                for rps in (0, 1, rows, rows + 5):
                    b = tiff.bound8(rows, cols, cn, comp, rps)
                    assert b == ref.bound(rows, cols, cn, comp, rps)
                    for kind in ("noise", "constant"):
                        assert len(ref.encode(picture(kind, rows, cols, cn, cols + rows), comp, pred, rps, 300)) <= b
    for kind in ("noise", "constant"):
        img = picture(kind, 64, 256, cn, 1)
        for rps in (0, 64):
            assert len(ref.encode(img, 5, 1, rps, 300)) <= tiff.bound8(64, 256, cn, 5, rps)
