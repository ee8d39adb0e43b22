"""tests/jpeg_dec_ref.py (the numpy restatement of the decoder, which csrc/jpeg_dec.hip follows stage by stage) against
Pillow / libjpeg-turbo, the arbiter: every shape x content x quality x stream variant in all four output forms, dataset
sheets, the streams the encoder's restatement writes; the self-synchronising model at 32, 128 and 1024 bits against the
sequential decoder coefficient for coefficient; every refusal."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg_decode as fz  # noqa: E402
import jpeg_dec_ref as R  # noqa: E402
import jpeg_ref  # noqa: E402

SHAPES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 16), (16, 17), (37, 53), (64, 48)]
VARIANTS = [dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(gray=True), dict(subsampling=2, optimize=True),
            dict(subsampling=2, restart_marker_blocks=1), dict(subsampling=1, restart_marker_blocks=3),
            dict(subsampling=0, restart_marker_rows=1)]
DATASET = os.path.join(HERE, "golden", "dataset")


def content(rows, cols, kind):
    rng = np.random.Generator(np.random.PCG64(1000 * rows + cols))
    if kind == "noise":
        return rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((rows, cols, 3), (31, 140, 222), np.uint8)
    img = np.full((rows, cols, 3), 250, np.uint8)    # a ruled sheet: dark lines every 5 rows, a coloured margin
    img[2::5] = (40, 30, 20)
    img[:, : max(cols // 7, 1)] = (200, 60, 90)
    return img


def check_stream(s, what, lengths=(32, 128, 1024)):
    code, h = R.parse(s)
    assert code == 0, what
    data, ivals, rst_ok = R.unstuff(s, h.data)
    assert rst_ok, what
    coef, code = R.huff_decode(h, data, ivals)
    assert code == 0, what
    for sub in lengths:
        c2, code2, rounds = R.selfsync(h, data, ivals, sub)
        assert code2 == 0 and (c2 == coef).all(), (what, sub)
    for channels in (1, 3):
        got = R.render(h, coef, channels)
        want = fz.pillow_decode(s, channels)
        assert got.shape == want.shape and (got == want).all(), (what, channels)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_restatement_equals_pillow(rows, cols):
    """gray and colour streams in both output forms: the four forms of DESIGN 4.19"""
    for kind in ("noise", "flat", "ruled"):
        img = content(rows, cols, kind)
        for q in (100, 90, 25):
            for v in VARIANTS:
                check_stream(fz.make_stream(img, q, **v), (rows, cols, kind, q, v))


def test_many_rounds_at_32_bits():
    """32-bit subsequences on noise: lanes start in the middle of codes, and some need several rounds"""
    s = fz.make_stream(content(64, 48, "noise"), 100, subsampling=2)
    code, h = R.parse(s)
    data, ivals, _ = R.unstuff(s, h.data)
    _, code, rounds = R.selfsync(h, data, ivals, 32)
    assert code == 0 and rounds > 2


def test_fill_bytes_before_a_stuffed_ff_are_refused():
    """0xFF 0xFF 0x00 inside a scan: libjpeg's C decoder keeps one data 0xFF, libjpeg-turbo (Pillow) returns another
    picture; the decoder gives neither: OMR_ERR_ASSERT"""
    s = fz.make_stream(content(64, 48, "noise"), 100, subsampling=2)
    at = s.index(b"\xff\x00", s.index(b"\xff\xda"))
    for fill in (b"\xff", b"\xff\xff"):
        assert R.decode(s[:at] + fill + s[at:], 3)[0] == R.ASSERT
    assert R.decode(s, 3)[0] == 0


@pytest.mark.parametrize("name", ["image001.jpg", "image040.jpg", "SCN00025_2.jpg"])
def test_dataset_sheets(name):
    check_stream(open(os.path.join(DATASET, name), "rb").read(), name)


def test_streams_of_the_encoders_restatement():
    for rows, cols in ((16, 16), (15, 17), (37, 53)):
        img = content(rows, cols, "noise")
        for q in (100, 75):
            check_stream(jpeg_ref.encode(img, q), (rows, cols, q, "bgr"))
            check_stream(jpeg_ref.encode(img[..., 1].copy(), q), (rows, cols, q, "gray"))


def _segment(s, marker):
    i = s.index(bytes([0xFF, marker]))
    return i, (s[i + 2] << 8) | s[i + 3]


def test_refusals():
    from PIL import Image
    img = content(37, 53, "noise")
    good = fz.make_stream(img, 90, subsampling=2)
    assert R.parse(good)[0] == 0
    sof, _ = _segment(good, 0xC0)
    sos, sos_len = _segment(good, 0xDA)
    dqt, _ = _segment(good, 0xDB)

    def patched(at, value):
        b = bytearray(good)
        b[at] = value
        return bytes(b)

    def with_segment(marker, body):
        seg = bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
        return good[:sof] + seg + good[sof:]

    cmyk = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(cmyk, "JPEG")
    exif6 = b"Exif\x00\x00MM\x00*\x00\x00\x00\x08\x00\x01\x01\x12\x00\x03\x00\x00\x00\x01\x00\x06\x00\x00\x00\x00\x00\x00"
    exif1 = exif6.replace(b"\x00\x01\x00\x06", b"\x00\x01\x00\x01")
    two_scans = good[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + good[sos + 2 + sos_len:]
    notimpl = {
        "progressive": fz.make_stream(img, 90, progressive=True),
        "SOF1": patched(sof + 1, 0xC1), "SOF9 arithmetic": patched(sof + 1, 0xC9), "12 bit": patched(sof + 4, 12),
        "CMYK": cmyk.getvalue(), "two scans": two_scans,
        "sampling 4x1": patched(sof + 11, 0x41), "chroma 2x1": patched(sof + 14, 0x21),
        "Adobe": with_segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01"),
        "16-bit DQT": patched(dqt + 4, 0x10), "DNL": with_segment(0xDC, b"\x00\x25"),
        "orientation 6": with_segment(0xE1, exif6),
    }
    for what, s in notimpl.items():
        code, h = R.parse(s)
        assert code == R.NOTIMPL, what
        assert R.decode(s, 3) == (R.NOTIMPL, None)
    code, h = R.parse(notimpl["progressive"])
    assert (h.rows, h.cols) == (37, 53)      # the size is there whenever SOF was readable
    # component ids R G B without a JFIF segment
    app0, app0_len = _segment(good, 0xE0)
    rgb = bytearray(good[:app0] + good[app0 + 2 + app0_len:])
    sof2 = bytes(rgb).index(b"\xff\xc0")
    sos2 = bytes(rgb).index(b"\xff\xda")
    for k, ident in enumerate(b"RGB"):
        rgb[sof2 + 10 + 3 * k] = ident
        rgb[sos2 + 5 + 2 * k] = ident
    assert R.parse(bytes(rgb))[0] == R.NOTIMPL
    assert R.parse(with_segment(0xE1, exif1))[0] == 0 and R.parse(with_segment(0xFE, b"a comment"))[0] == 0
    badarg = {
        "no SOI": b"\x00" + good[1:], "empty": b"", "segment past the end": good[:sof + 6],
        "ends before SOS": good[:sos], "rows 0": patched(sof + 5, 0)[:sof + 6] + b"\x00" + good[sof + 7:],
        "cols 0": good[:sof + 7] + b"\x00\x00" + good[sof + 9:],
        "undefined Huffman table": patched(sos + 6, 0x13), "undefined quantisation table": patched(sof + 12, 3),
    }
    for what, s in badarg.items():
        assert R.parse(s)[0] == R.BADARG, what
    # entropy data: cut short, and with RSTn out of order
    assert R.decode(good[:sos + (len(good) - sos) // 2], 3)[0] == R.ASSERT
    for sub in (32, 1024):
        assert R.decode(good[:sos + (len(good) - sos) // 2], 3, sub)[0] == R.ASSERT
    rst = bytearray(fz.make_stream(img, 90, subsampling=2, restart_marker_blocks=1))
    first = bytes(rst).index(b"\xff\xd1")
    rst[first + 1] = 0xD3
    assert R.decode(bytes(rst), 3)[0] == R.ASSERT
