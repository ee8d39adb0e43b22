"""The device JPEG encoder (csrc/jpeg.hip) on the GPU: omr_jpeg_encode_batch_device, omr_jpeg_encode and
omr_correct_default_batch_jpeg.  Every comparison is byte for byte, whole stream: against Pillow (libjpeg-turbo, the
arbiter) and, on the small shapes, against the numpy restatement tests/jpeg_ref.py too.

The block kernel converts tiles of 128 x 64 pixels (JPEG_TILE_W x JPEG_TILE_H), a workgroup each; 150 x 270 spans three
of them down and three across, the last ones partial both ways.  129 x 131 has a second tile of one pixel column."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg as fz  # noqa: E402
import jpeg_ref  # noqa: E402
from oics import jpeg, omr, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (8, 8), (15, 17), (16, 16), (17, 33), (53, 37), (129, 131), (150, 270)]
QUALITIES = (100, 75, 1)
PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)  # correct_default's, lib.rs:192-205

_REF = {}


def _image(rows, cols, cn, kind, seed=0):
    rng = np.random.Generator(np.random.PCG64(1000 * rows + cols + 7 * cn + seed))
    if kind == "noise":
        return rng.integers(0, 256, (rows, cols) if cn == 1 else (rows, cols, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((rows, cols) if cn == 1 else (rows, cols, 3), 255, np.uint8)
    return (synth.make_card(rows, cols, 5 + seed)[0] if cn == 1 else synth.make_color_card(rows, cols, 5 + seed)[0]).copy()


def _expected(img, q):
    """Pillow's stream, once per (image, quality); small images are held against the restatement as well"""
    key = (img.shape, img.tobytes(), q)
    if key not in _REF:
        want = fz.pillow_bytes(img, q)
        if img.shape[0] * img.shape[1] <= 53 * 37:
            assert jpeg_ref.encode(img, q) == want
        _REF[key] = want
    return _REF[key]


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_batch_equals_pillow(rows, cols, cn):
    """every shape x quality, noise content, from an aligned packed source and from a base offset by 1-3 bytes with an odd
    pitch (the byte-wise loads)"""
    img = _image(rows, cols, cn, "noise")
    for q in QUALITIES:
        want = _expected(img, q)
        for off, pad in ((0, 0), (1 + (rows + q) % 3, 1 if (cols * cn) % 2 == 0 else 2)):
            assert (cols * cn + pad) % 2 == (1 if pad else (cols * cn) % 2)
            got, lens = fz.encode_on_device([img], rows, cols, cn, q, base_offset=off, pitch_pad=pad)
            assert lens[0] == len(want) and got[0] == want, (rows, cols, cn, q, off, pad)
    # an aligned base with a pitch that is a multiple of 4: the dword path with a padded row
    got, _ = fz.encode_on_device([img], rows, cols, cn, 75, base_offset=0, pitch_pad=(-cols * cn) % 4 + 4)
    assert got[0] == _expected(img, 75)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("kind", ["noise", "white", "card"])
def test_content_classes(kind, cn):
    """noise: long codes and stuffed 0xFF bytes, every boundary dword of the bit writer shared; white: every block is an
    EOB, the shortest stream; a card"""
    img = _image(150, 270, cn, kind)
    for q in (100, 75):
        want = _expected(img, q)
        got, _ = fz.encode_on_device([img], 150, 270, cn, q)
        assert got[0] == want, (kind, cn, q)
        if kind == "noise" and q == 100:
            assert b"\xff\x00" in want[623 if cn == 3 else 300:]


@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("cn", [1, 3])
def test_per_image_sizes(n, cn):
    """mixed sizes in one slot shape with a 1 x 1 and a 0 x 0 in the middle; sizes == NULL equals explicit equal sizes"""
    rows, cols = 70, 150
    rng = np.random.Generator(np.random.PCG64(n * 10 + cn))
    imgs = []
    for i in range(n):
        r, c = (rows, cols) if i == 0 else (int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1)))
        imgs.append(_image(r, c, cn, "noise" if i % 2 == 0 else "card", seed=i))
    if n >= 3:
        imgs[n // 2] = _image(1, 1, cn, "noise")
        imgs[n // 2 - 1] = None
    got, lens = fz.encode_on_device(imgs, rows, cols, cn, 90)
    for i, im in enumerate(imgs):
        if im is None:
            assert lens[i] == 0 and got[i] == b""
        else:
            assert got[i] == _expected(im, 90), (i, im.shape)
    full = [_image(rows, cols, cn, "noise", seed=40 + i) for i in range(n)]
    a, la = fz.encode_on_device(full, rows, cols, cn, 90, explicit_sizes=True)
    b, lb = fz.encode_on_device(full, rows, cols, cn, 90, explicit_sizes=False)
    assert a == b and (la == lb).all() and a[0] == _expected(full[0], 90)


def test_a4_colour_noise():
    """one A4 colour canvas of noise at quality 100: the longest stream the shape gives"""
    img = _image(3508, 2480, 3, "noise")
    want = fz.pillow_bytes(img, 100)
    got, lens = fz.encode_on_device([img], 3508, 2480, 3, 100)
    assert lens[0] == len(want) <= jpeg.bound(3508, 2480, 3)
    assert got[0] == want


def test_host_form_equals_device_form():
    for cn in (1, 3):
        img = _image(150, 270, cn, "card")
        dev, _ = fz.encode_on_device([img], 150, 270, cn, 95)
        assert jpeg.encode(img, 95) == dev[0] == _expected(img, 95)
        from oics.transfer import TransformableMatrix
        assert TransformableMatrix(img).encode_jpeg(95) == dev[0]


def test_cap_too_small():
    """omr_jpeg_encode into a buffer that is too short: -4, *len = the length needed, not a byte written; a buffer of exactly
    that length takes the stream.  oics.jpeg.encode's second call (noise does not fit its first buffer) gives the same."""
    import ctypes as C
    import oics
    from oics import _lib
    L = oics.lib()
    for cn in (1, 3):
        img = _image(53, 37, cn, "noise")
        want = _expected(img, 100)
        _, im = oics.transfer.as_image(img)
        for cap in (0, 64, len(want) - 1):
            buf = np.full(max(cap, 1) + 8, 0xA5, np.uint8)
            n = C.c_int64(-7)
            rc = L.omr_jpeg_encode(C.byref(im), 100, buf.ctypes.data_as(_lib.u8p), cap, C.byref(n))
            assert rc == -4 and n.value == len(want) and (buf == 0xA5).all(), (cn, cap, rc, n.value)
            assert L.omr_last_error().decode() == "the stream takes %d bytes, the buffer holds %d" % (len(want), cap)
        buf = np.full(len(want) + 8, 0xA5, np.uint8)
        n = C.c_int64(-7)
        assert L.omr_jpeg_encode(C.byref(im), 100, buf.ctypes.data_as(_lib.u8p), len(want), C.byref(n)) == 0
        assert n.value == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()
        big = _image(150, 270, cn, "noise")
        if cn == 1:  # gray noise at quality 100 is longer than the image: beyond jpeg.encode's first buffer
            assert len(_expected(big, 100)) > big.size + 1024
        assert jpeg.encode(big, 100) == _expected(big, 100)


def test_composite_equals_batch_then_pillow():
    """omr_correct_default_batch_jpeg on 12 sheets of two interleaved shapes and a blank one: angles, need_check and
    scan_rc are omr_correct_default_batch's, every stream is Pillow's encoding of that form's canvas"""
    a = [synth.make_color_card(460, 496, 700 + i, skew=[2.0, -4.5, 7.25][i % 3])[0] for i in range(6)]
    b = [synth.make_color_card(320, 226, 800 + i, skew=[-1.1, 6.6][i % 2])[0] for i in range(5)]
    sheets = [x for pair in zip(a, b) for x in pair] + [a[5]]
    sheets.insert(3, np.full((320, 226, 3), 255, np.uint8))
    assert len(sheets) == 12
    plain = omr.correct_default_batch(sheets, *PARAMS)
    enc = omr.correct_default_batch_jpeg(sheets, *PARAMS, quality=100)
    assert any(p[3] != 0 for p in plain) and sum(p[3] == 0 for p in plain) >= 10
    for i, (p, e) in enumerate(zip(plain, enc)):
        assert np.float64(p[0]).view(np.uint64) == np.float64(e[0]).view(np.uint64) and p[1] == e[1] and p[3] == e[3], i
        if p[3] != 0:
            assert e[2] is None
        else:
            assert e[2] == fz.pillow_bytes(p[2], 100), i


def test_fuzz_40_cases():
    assert fz.run(40, seed=17) is None
