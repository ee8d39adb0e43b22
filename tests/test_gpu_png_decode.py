"""The device PNG decoder (csrc/png_dec.hip) on the GPU: omr_png_decode_batch_device, omr_png_decode and PNG sheets in
omr_correct_default_batch_streams.  Every comparison is byte for byte, against Pillow (what imread returns) or, for
streams no compressor writes, against the restatement in png_ref.py.

The inflate kernel stages 4096 bytes of an image's input and 512 literal and 512 match records a batch; the unfilter
kernel sweeps bands of 64 rows, eight filter units a step."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_png_decode as fz  # noqa: E402
import png_ref as P  # noqa: E402
import test_png_ref as cases  # noqa: E402
from oics import omr, png  # noqa: E402
from oics.transfer import TransformableMatrix  # noqa: E402

pytestmark = pytest.mark.gpu

DATASET = os.path.join(HERE, "golden", "dataset")
_VARIANTS = []


def _variants():
    if not _VARIANTS:
        _VARIANTS.extend(cases.variants())
    return _VARIANTS


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), (what, int((got != want).sum()), "bytes differ")


def _noise(rows, cols, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


@pytest.mark.parametrize("channels", [3, 1])
def test_every_shape_type_and_filter_in_one_call(channels):
    """shapes x colour type / depth x filter choice, contents rotating, in slots larger than the images with a pitch pad
    and a base offset; the helper checks every slack byte untouched"""
    chosen = [(name, s) for name, s, ct in _variants() if channels == 3 or ct in (0, 4)]
    assert len(chosen) == 9 * 10 * (11 if channels == 3 else 5)
    streams = [s for _, s in chosen]
    imgs, size, rc = fz.decode_on_device(streams, 132, 60, channels, pitch_pad=5, base_offset=1)
    assert (rc == 0).all(), [(chosen[i][0], int(rc[i])) for i in np.nonzero(rc)[0][:10]]
    for i, (name, s) in enumerate(chosen):
        _same(imgs[i], fz.pillow_decode(s, channels), name)


def test_deflate_forms():
    """stored, fixed, dynamic, a full flush every few rows, a 512-byte window, the crafted blocks, distance 1 at length 258
    throughout, matches at distance 32768, a literal stream 4.5 times the input window and 36 times the literal records, a stream of
    3040 short matches (six times the match records), IDAT in
    1-byte chunks and with empty chunks"""
    ruled = cases.content(37, 53, 2, 8, "ruled")
    streams, want = [], []
    for z in (dict(level=0), dict(strategy=zlib.Z_FIXED), dict(), dict(flush_every=3 * (1 + 53 * 3)), dict(wbits=9)):
        for cuts in (None, 1, [0, 1, 0, 7, 0]):
            streams.append(P.write(ruled, 2, 8, filters="rotate", cuts=cuts, **z))
            want.append(ruled[..., ::-1])
    # the crafted blocks on gray rows with filter byte 0: 14 pixel values and the 0 make 15 literals
    rng = np.random.default_rng(3)
    for craft, vals in ((P.crafted_15bit, rng.integers(0, 14, (20, 15), dtype=np.uint8) * 16 + 3),
                        (P.crafted_crossing, rng.integers(0, 256, (12, 25), dtype=np.uint8))):
        raw = b"".join(b"\x00" + vals[r].tobytes() for r in range(vals.shape[0]))
        streams.append(P.assemble(vals.shape[0], vals.shape[1], 0, 8, craft(raw)))
        want.append(np.repeat(vals[..., None], 3, axis=2))
    flat = np.full((96, 128, 3), (31, 140, 222), np.uint8)
    streams.append(P.write(flat, 2, 8))
    want.append(flat[..., ::-1])
    # the bytes from 32768 on repeat the first ones: zlib never reaches back that far, so the matches are written here
    raw = bytearray(P.filter_rows(P.pack_rows(_noise(96, 128, 5), 2, 8), 3, 0))
    for at in range(0, len(raw), 385):
        if at >= 32768:
            raw[at - 32768] = 0           # what lands on a filter byte
    raw[32768:] = raw[:len(raw) - 32768]
    w, at = P.BitWriter(), 32768
    symbols = list(raw[:32768])
    while at < len(raw):
        n = min(258, len(raw) - at) if len(raw) - at not in (259, 260) else 200
        symbols.append((n, 32768))
        at += n
    P.fixed_block(w, symbols)
    streams.append(P.assemble(96, 128, 2, 8, P.zlib_wrap(w.done(), bytes(raw))))
    far = np.frombuffer(bytes(raw), np.uint8).reshape(96, 385)[:, 1:].reshape(96, 128, 3)
    want.append(far[..., ::-1])
    # 3040 matches of length 4 and not one literal behind the first row: the match records wrap six times.  Gray rows of
    # 127 pixels are 128 bytes with their filter byte, so the group that holds a filter byte copies one from whole rows back
    rng = np.random.default_rng(17)
    raw = bytearray(b"\x00" + bytes(rng.integers(0, 256, 127, dtype=np.uint8)))
    symbols = list(raw)
    for at in range(128, 96 * 128, 4):
        d = 128 * int(rng.integers(1, min(at // 128, 200) + 1)) if at % 128 == 0 else int(rng.integers(4, min(at, 32768) + 1))
        symbols.append((4, d))
        raw += raw[at - d:at - d + 4]
    w = P.BitWriter()
    P.fixed_block(w, symbols)
    streams.append(P.assemble(96, 127, 0, 8, P.zlib_wrap(w.done(), bytes(raw))))
    assert len(symbols) - 128 >= 4 * 512 and P.decode(streams[-1])[0] == 0
    want.append(P.decode(streams[-1])[1])
    long = _noise(64, 96, 9)
    streams.append(P.write(long, 2, 8, strategy=zlib.Z_HUFFMAN_ONLY))
    assert len(P.parse(streams[-1])[1].idat) >= 4 * 4096
    want.append(long[..., ::-1])
    for s, w in zip(streams, want):
        assert np.array_equal(fz.pillow_decode(s, 3), w)
    imgs, size, rc = fz.decode_on_device(streams, 96, 128, 3, pitch_pad=3)
    assert (rc == 0).all(), rc
    for i, w in enumerate(want):
        _same(imgs[i], w, i)


def test_refused_and_malformed_streams_between_good_ones():
    imgs, size, rc = fz.decode_on_device([], 16, 16, 3)
    assert imgs == []
    a, b = cases.content(37, 53, 2, 8, "noise"), cases.content(15, 17, 0, 4, "ruled")
    good0, good1 = P.write(a, 2, 8, filters=4), P.write(b, 0, 4, filters=3)
    zs = P.deflate(P.filter_rows(P.pack_rows(a, 2, 8), 3, 0))
    interlaced = P.assemble(37, 53, 2, 8, zs, interlace=1)
    deep = P.assemble(8, 8, 0, 16, P.deflate(bytes(8 * 17)))
    malformed = good0[:40]
    imgs, size, rc = fz.decode_on_device([good0, interlaced, good1, deep, malformed, good0], 37, 53, 3, pitch_pad=3)
    assert list(rc) == [0, -213, 0, -213, -5, 0] and (size[[1, 3, 4]] == 0).all()
    _same(imgs[0], a[..., ::-1], 0)
    _same(imgs[2], fz.pillow_decode(good1, 3), 2)
    _same(imgs[5], imgs[0], 5)
    # an image larger than the slot: its own code, the others unaffected; a colour stream asked for as gray
    imgs, size, rc = fz.decode_on_device([good1, good0], 15, 17, 3)
    assert list(rc) == [0, -5]
    _same(imgs[0], fz.pillow_decode(good1, 3), 0)
    imgs, size, rc = fz.decode_on_device([good0, good1], 37, 53, 1)
    assert list(rc) == [-213, 0]
    _same(imgs[1], fz.pillow_decode(good1, 1), "gray")


def test_single_decode_equals_the_batch_form():
    for ct, depth in ((2, 8), (0, 8), (4, 8), (3, 2)):
        arr = cases.content(53, 37, ct, depth, "ruled")
        s = P.write(arr, ct, depth, cases.palette_of(depth) if ct == 3 else None, filters="rotate")
        for channels in (1, 3):
            if channels == 1 and ct not in (0, 4):
                with pytest.raises(Exception) as e:
                    png.decode(s, 1)
                assert e.value.code == -213
                continue
            one = png.decode(s, channels)
            (many,), _, rc = fz.decode_on_device([s], 53, 37, channels)
            assert rc[0] == 0
            _same(one, many, (ct, channels))
            _same(one, fz.pillow_decode(s, channels), (ct, channels))
            _same(TransformableMatrix.from_png_bytes(s, channels).get_mat(), one, "from_png_bytes")


PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)  # correct_default's, lib.rs:192-205


def _as_png(jpg, mode=None):
    from PIL import Image
    im = Image.open(io.BytesIO(jpg))
    if mode:
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, format="PNG")
    return b.getvalue()


def _sheets():
    from oics import jpeg
    by_shape = {}
    for f in sorted(os.listdir(DATASET)):
        if f.lower().endswith(".jpg"):
            s = open(os.path.join(DATASET, f), "rb").read()
            by_shape.setdefault(jpeg.info(s)[:2], []).append(s)
    return sorted(by_shape.values(), key=len, reverse=True)[:2]


def _decoded(s):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))[..., ::-1])


def _compare(streams):
    got = omr.correct_default_batch_streams(streams, *PARAMS)
    want = omr.correct_default_batch_jpeg([_decoded(s) for s in streams], *PARAMS)
    assert len(got) == len(want) == len(streams)
    for i, (g, w) in enumerate(zip(got, want)):
        assert w[3] == 0 and w[2] is not None, i
        assert g[0] == w[0] and g[1] == w[1] and g[3] == w[3], (i, g[:2], w[:2], g[3])
        assert g[2] == w[2], (i, "the output streams differ")
    return want


def test_correct_default_from_a_mixed_batch_of_png_and_jpeg_sheets():
    """four dataset sheets of one shape, two re-written as PNG by Pillow (one gray, one RGB), two left as JPEG: one bucket
    holds both kinds; angles, flags and output streams are omr_correct_default_batch_jpeg's on Pillow's decode"""
    a, _ = _sheets()
    want = _compare([_as_png(a[0]), a[1], _as_png(a[2], "RGB"), a[3]])
    assert len({w[2] for w in want}) == 4      # four different sheets: the comparison says something


def test_correct_default_from_png_sheets_alone_in_two_shapes():
    a, b = _sheets()
    bad = P.assemble(8, 8, 0, 16, P.deflate(bytes(8 * 17)))
    streams = [_as_png(a[0]), _as_png(b[0], "P"), _as_png(a[1], "1")]
    got = omr.correct_default_batch_streams(streams[:1] + [bad] + streams[1:], *PARAMS)
    assert got[1] == (0.0, False, None, -213)
    _compare(streams)


def test_fuzz_cases():
    assert fz.run(12, seed=1) is None


def test_stats_count_groups_and_stages():
    s = P.write(_noise(64, 96, 9), 2, 8, filters=4)
    png.stats(True)
    try:
        imgs, _, rc = fz.decode_on_device([s, s], 64, 96, 3)
        groups, ms = png.stats(False)
    finally:
        png.stats(False)
    assert rc[0] == 0 and groups == 1 and all(v > 0 for v in ms) and len(ms) == 4
    _same(imgs[1], fz.pillow_decode(s, 3), "with the collection on")
    fz.decode_on_device([s], 64, 96, 3)
    assert png.stats(False) == (0, [0.0] * 4)


def test_decode_stats_are_not_the_tiff_encoders():
    """the two codecs have as many stages; their statistics are still two objects: with the PNG decoder's collection on,
    a TIFF encode on the same thread collects nothing and leaves the decoder's figures alone"""
    import threading
    from oics import tiff
    s = P.write(_noise(64, 96, 9), 2, 8, filters=4)
    seen = {}

    def work():
        png.stats(True)
        try:
            imgs, _, rc = fz.decode_on_device([s], 64, 96, 3)
            seen["before"] = png.stats(True)
            tiff.encode(imgs[0])
            seen["tiff"] = tiff.encode_stats(False)
            seen["after"] = png.stats(False)
        finally:
            png.stats(False), tiff.encode_stats(False)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert seen["before"][0] == 1 and sum(seen["before"][1]) > 0
    assert seen["tiff"] == (0, [0.0] * len(tiff.STAGES_ENC))
    assert seen["after"] == seen["before"]


def test_zz_damaged_data_between_two_good_streams():
    """Last in the file.  Each damaged stream sits between two good ones and answers -215; the good ones stay exact.  None
    of them asks the kernels for anything outside their bounds checks: a flipped bit in a stored block's LEN, a zlib stream
    cut in half, a match that reaches before the start, a wrong Adler-32, one surplus row, a filter byte 5, a palette index
    beyond PLTE, a critical chunk's CRC."""
    img = cases.content(37, 53, 2, 8, "noise")
    packed = P.pack_rows(img, 2, 8)
    raw = P.filter_rows(packed, 3, "rotate")
    good = P.assemble(37, 53, 2, 8, P.deflate(raw))

    def with_zs(zs, rows=37):
        return P.assemble(rows, 53, 2, 8, zs)

    stored = bytearray(P.deflate(raw, level=0))
    stored[3] ^= 0x10                                        # LEN of the first stored block
    dynamic = P.deflate(raw)
    w = P.BitWriter()
    P.fixed_block(w, [0, 1, 2, (40, 4)] + [7] * (len(raw) - 43))
    before_start = P.zlib_wrap(w.done(), bytes([0, 1, 2]) + bytes(40) + bytes([7]) * (len(raw) - 43))
    wrong_adler = dynamic[:-4] + struct.pack(">I", (zlib.adler32(raw) ^ 1) & 0xffffffff)
    surplus = P.deflate(raw + raw[:1 + 53 * 3])
    five = bytearray(raw)
    five[(1 + 53 * 3) * 20] = 5
    pal = cases.palette_of(4)[:5]
    idx = cases.content(15, 17, 3, 4, "noise") % 5
    idx[7, 9] = 5
    crc = bytearray(good)
    crc[good.index(b"IDAT") + 10] ^= 1
    damaged = [with_zs(bytes(stored)), with_zs(dynamic[:len(dynamic) // 2]), with_zs(before_start), with_zs(wrong_adler),
               with_zs(surplus), with_zs(P.deflate(bytes(five))), P.write(idx, 3, 4, pal), bytes(crc)]
    for s in damaged:
        assert P.decode(s) == (P.ASSERT, None)
    streams = [good]
    for s in damaged:
        streams += [s, good]
    imgs, size, rc = fz.decode_on_device(streams, 37, 53, 3, pitch_pad=1)
    assert list(rc) == [0] + [-215, 0] * len(damaged), rc
    for i in range(0, len(streams), 2):
        _same(imgs[i], img[..., ::-1], i)
