"""The device JPEG encoder (csrc/jpeg.hip, tables of csrc/oics_jpeg.cpp) and decoder (csrc/jpeg_dec.hip) on the crafted
canvases of tests/jpeg_cases.py: every Huffman symbol libjpeg can be made to write -- all 162 entries of both AC tables, DC
categories 0..11 with both signs, one to three ZRLs, blocks without EOB, streams dense with stuffed 0xFF bytes.  What the
canvases reach is asserted on the CPU (tests/test_jpeg_cases.py).  Every comparison is byte for byte, whole stream,
against Pillow (libjpeg-turbo, the arbiter); a difference is reported with the block and the symbol it falls in."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg as fz  # noqa: E402
import fuzz_jpeg_decode as fzd  # noqa: E402
import jpeg_cases as jc  # noqa: E402
from oics import jpeg  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _expected(name, img, q):
    """Pillow's stream, once per (canvas, quality)"""
    if (name, q) not in _REF:
        _REF[name, q] = fz.pillow_bytes(img, q)
    return _REF[name, q]


def _check(name, img, q, got, length, what):
    want = _expected(name, img, q)
    cn = 1 if img.ndim == 2 else 3
    assert len(want) <= jpeg.bound(img.shape[0], img.shape[1], cn), (name, q)
    if got != want or length != len(want):
        pytest.fail("%s at quality %d, %s: out_len %d, %s" % (name, q, what, length, jc.explain(img, q, got, want)))


def _unaligned(rows, cols, cn, q):
    """a base offset of 1..3 bytes and a pad that makes the pitch odd, as test_gpu_jpeg.py's test_batch_equals_pillow"""
    return 1 + (rows + q) % 3, 1 if (cols * cn) % 2 == 0 else 2


def _both_sources(name, img, q):
    rows, cols = img.shape[:2]
    cn = 1 if img.ndim == 2 else 3
    off, pad = _unaligned(rows, cols, cn, q)
    assert 1 <= off <= 3 and (cols * cn + pad) % 2 == 1
    for o, p in ((0, 0), (off, pad)):
        got, lens = fz.encode_on_device([img], rows, cols, cn, q, base_offset=o, pitch_pad=p)
        _check(name, img, q, got[0], int(lens[0]), "base offset %d, pitch pad %d" % (o, p))


@pytest.mark.parametrize("name", jc.names())
def test_crafted_canvas_equals_pillow(name):
    """every crafted canvas at its quality, from an aligned packed source and from an odd base with an odd pitch"""
    _, img, q = jc.case(name)
    _both_sources(name, img, q)


@pytest.mark.parametrize("name,img,q", jc.crops(), ids=[c[0] for c in jc.crops()])
def test_crops_equal_pillow(name, img, q):
    """widths and heights of 8 k + 1 and 16 k + 1: replicated edges of high-contrast blocks and, in BGR, dummy blocks
    beside and below DC differences of category 11 (y_dc's resolution of dummies)"""
    _both_sources(name, img, q)


@pytest.mark.parametrize("q", [100, 75])
def test_gray_canvases_in_one_batch(q):
    """all gray canvases, of different sizes, in one slot shape with a 1 x 1 between them: segments of 256 blocks whose bit
    totals lie far above their neighbours' (the binary canvas beside flat blocks) pass through jpeg_seg_scan_kernel"""
    named = [(n,) + jc.case(n)[1:2] for n in jc.names(colour=False)]
    named.insert(len(named) // 2, ("one-pixel", np.full((1, 1), 200, np.uint8)))
    rows, cols = max(im.shape[0] for _, im in named), max(im.shape[1] for _, im in named)
    assert len({im.shape for _, im in named}) >= 8
    got, lens = fz.encode_on_device([im for _, im in named], rows, cols, 1, q, base_offset=3, pitch_pad=1)
    for i, (n, im) in enumerate(named):
        _check(n, im, q, got[i], int(lens[i]), "image %d of the batch" % i)


@pytest.mark.parametrize("q", [100, 90])
def test_colour_canvases_in_one_batch(q):
    named = [(n,) + jc.case(n)[1:2] for n in jc.names(colour=True)]
    named.insert(1, ("one-pixel-colour", np.full((1, 1, 3), (255, 0, 0), np.uint8)))
    rows, cols = max(im.shape[0] for _, im in named), max(im.shape[1] for _, im in named)
    got, lens = fz.encode_on_device([im for _, im in named], rows, cols, 3, q)
    for i, (n, im) in enumerate(named):
        _check(n, im, q, got[i], int(lens[i]), "image %d of the batch" % i)


def _same(got, want, what):
    """tests/test_gpu_jpeg_decode.py's comparison"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), (what, int((got != want).sum()), "bytes differ")


@pytest.mark.parametrize("channels", [1, 3])
def test_decoder_on_the_crafted_streams(channels):
    """Pillow's streams of every crafted canvas and crop, gray and 4:2:0, through the device decoder's Huffman lookup, in
    one call: equal to Pillow's decode of the same bytes"""
    named = [(n, _expected(n, img, q)) for n, img, q in jc.cases() + jc.crops()]
    rows = max(img.shape[0] for _, img, _ in jc.cases())
    cols = max(img.shape[1] for _, img, _ in jc.cases())
    imgs, size, rc = fzd.decode_on_device([s for _, s in named], rows, cols, channels, pitch_pad=3, base_offset=1)
    assert (rc == 0).all(), [(n, int(r)) for (n, _), r in zip(named, rc) if r != 0]
    for i, (n, s) in enumerate(named):
        _same(imgs[i], fzd.pillow_decode(s, channels), n)
