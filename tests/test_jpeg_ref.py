"""tests/jpeg_ref.py, the numpy restatement of libjpeg's baseline encoder, against Pillow (libjpeg-turbo), whole files byte
for byte.  Pillow is the arbiter: csrc/jpeg.hip is held to the restatement stage by stage and to Pillow on the GPU
(tests/test_gpu_jpeg.py).  That OpenCV 4.6's imwrite writes the same bytes (libjpeg with its defaults, quality passed to
jpeg_set_quality(q, TRUE)) is upstream knowledge; it is checked here only where cv2 imports."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_ref  # noqa: E402
from oics import synth  # noqa: E402

SHAPES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 16), (16, 17), (37, 53), (64, 48)]
QUALITIES = (100, 95, 75, 50, 1)


def pillow(img, q):
    b = io.BytesIO()
    Image.fromarray(img[..., ::-1] if img.ndim == 3 else img).save(b, format="JPEG", quality=q)
    return b.getvalue()


def contents(rows, cols, cn):
    shape = (rows, cols) if cn == 1 else (rows, cols, 3)
    rng = np.random.Generator(np.random.PCG64(rows * 100 + cols + cn))
    out = {"u%d" % v: np.full(shape, v, np.uint8) for v in (0, 128, 255)}
    out["noise"] = rng.integers(0, 256, shape, dtype=np.uint8)
    out["card"] = (synth.make_card(rows, cols, 3)[0] if cn == 1 else synth.make_color_card(rows, cols, 3)[0]).copy()
    c = ((np.add.outer(np.arange(rows), np.arange(cols)) & 1) * 255).astype(np.uint8)
    out["checker"] = c if cn == 1 else np.repeat(c[..., None], 3, 2)
    return out


def segments(stream):
    """[(marker, body)] up to and including SOS"""
    out, i = [], 2
    while True:
        assert stream[i] == 0xFF
        m, n = stream[i + 1], (stream[i + 2] << 8) | stream[i + 3]
        out.append((m, stream[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out, i


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_restatement_equals_pillow(rows, cols, cn):
    for name, img in contents(rows, cols, cn).items():
        for q in QUALITIES:
            want = pillow(img, q)
            got = jpeg_ref.encode(img, q)
            assert got == want, (name, q, len(got), len(want))
            dec = Image.open(io.BytesIO(got))
            assert dec.size == (cols, rows) and dec.mode == ("L" if cn == 1 else "RGB")
            dec.load()


def test_noise_streams_hold_stuffed_bytes():
    for cn in (1, 3):
        img = contents(64, 48, cn)["noise"]
        s = jpeg_ref.encode(img, 100)
        _, scan = segments(s)
        assert b"\xff\x00" in s[scan:-2] and s[-2:] == b"\xff\xd9"
        assert s == pillow(img, 100)


def test_quant_tables_equal_pillows_dqt():
    zz = jpeg_ref.ZIGZAG
    img = np.zeros((8, 8, 3), np.uint8)
    for q in range(1, 101):
        dqt = [b for m, b in segments(pillow(img, q))[0] if m == 0xDB]
        assert len(dqt) == 2 and dqt[0][0] == 0 and dqt[1][0] == 1
        luma, chroma = jpeg_ref.quant_tables(q)
        assert bytes(luma[zz].astype(np.uint8)) == dqt[0][1:] and bytes(chroma[zz].astype(np.uint8)) == dqt[1][1:], q
    assert (jpeg_ref.quant_tables(100)[0] == 1).all() and (jpeg_ref.quant_tables(100)[1] == 1).all()
    for a, b in ((0, 1), (-3, 1), (101, 100), (104, 100)):  # libjpeg clamps
        assert all((x == y).all() for x, y in zip(jpeg_ref.quant_tables(a), jpeg_ref.quant_tables(b)))


@pytest.mark.parametrize("rows,cols", [(1, 1), (37, 53), (300, 258)])
def test_header_equals_pillows(rows, cols):
    for cn in (1, 3):
        img = np.zeros((rows, cols) if cn == 1 else (rows, cols, 3), np.uint8)
        want = pillow(img, 75)
        _, scan = segments(want)
        h = jpeg_ref.header(rows, cols, cn, 75)
        assert h == want[:scan] and len(h) <= 623
        segs = segments(want)[0]
        assert segs[0] == (0xE0, bytes.fromhex("4a46494600010100000100010000"))
        assert sum(m == 0xC4 for m, _ in segs) == (4 if cn == 3 else 2)
        if cn == 3:
            assert len(h) == 623
            sof = [b for m, b in segs if m == 0xC0][0]
            assert sof[6:] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])


def test_opencv_writes_the_same_bytes():
    cv2 = pytest.importorskip("cv2")
    for cn in (1, 3):
        for name, img in contents(37, 53, cn).items():
            for q in (100, 75):
                ok, buf = cv2.imencode(".jpg", img, [cv2.IMWRITE_JPEG_QUALITY, q])
                assert ok and buf.tobytes() == jpeg_ref.encode(img, q), (name, q)
