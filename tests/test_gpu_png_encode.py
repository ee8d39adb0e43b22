"""The device PNG encoder (omr_png_encode*, omr_correct_default_batch_png, omr_correct_default_batch_streams_png) on the
GPU.  PNG has no canonical stream: the arbiters are Pillow, tests/png_ref.py and the project's own device decoder, which
must all return the image; every chunk's CRC; and the restatement tests/png_enc_ref.py, byte for byte."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_png_encode as fz  # noqa: E402
import png_enc_ref as ref  # noqa: E402
import png_ref  # noqa: E402
import oics  # noqa: E402
from oics import omr, png, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 300), (300, 1), (2, 2), (15, 17), (53, 37), (150, 270), (257, 259)]
PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)


def three_blocks(cn):
    """the smallest-rowed shape whose raw data spans three blocks with a last block of less than one piece"""
    for rows in range(2, 400):
        for cols in range(1, 400):
            if 2 * ref.BLOCK < ref.raw_bytes(rows, cols, cn) < 2 * ref.BLOCK + ref.PIECE and cols * cn > 60:
                return rows, cols
    raise AssertionError


def long_row(cn):
    return 5, ref.PIECE // cn + 40  # 1 + row bytes > PIECE: the row above lies two pieces back


def check(stream, img):
    err = fz.host_arbiters(stream, img) or fz.device_arbiters(stream, img)
    assert err is None, (img.shape, err)


BIG = (150, 270)   # the largest shape the restatement is held to, beside the block-spanning one


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_every_shape_and_content_decodes_and_equals_the_restatement(cn):
    """every content at every small shape, byte for byte; 257 x 259 is held to the decoders alone (as the issue sets it);
    150 x 270 and the block-spanning shape have a case per content below"""
    k = 0
    for rows, cols in [sh for sh in SHAPES if sh != BIG] + [long_row(cn)]:
        imgs = []
        for kind in fz.KINDS:
            k += 1
            imgs.append(fz.content(kind, rows, cols, cn, seed=k))
        streams, _ = fz.encode_on_device(imgs, rows, cols, cn)
        for kind, img, s in zip(fz.KINDS, imgs, streams):
            check(s, img)
            if rows * cols <= BIG[0] * BIG[1]:
                assert s == ref.encode(img, 1), (rows, cols, cn, kind)


@pytest.mark.parametrize("kind", fz.KINDS)
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_multi_block_shapes_equal_the_restatement(cn, kind):
    """150 x 270 (3 to 10 blocks) and the shape of three blocks with a last block below one piece: every content decodes
    and equals the restatement byte for byte -- fixed and stored blocks with the empty stored block behind them, runs of
    258 cut at piece and block ends, scaled frequencies"""
    for j, (rows, cols) in enumerate([BIG, three_blocks(cn)]):
        img = fz.content(kind, rows, cols, cn, seed=100 + 7 * j + cn)
        (s,), _ = fz.encode_on_device([img], rows, cols, cn)
        check(s, img)
        assert s == ref.encode(img, 1), (rows, cols, cn, kind)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_source_layouts_give_one_stream(cn):
    imgs = [fz.content("card", 53, 37, cn, 3), fz.content("noise", 20, 37, cn, 4)]
    a, _ = fz.encode_on_device(imgs, 53, 37, cn)
    odd = 1 if (37 * cn) % 2 == 0 else 2   # makes the pitch odd
    b, _ = fz.encode_on_device(imgs, 53, 37, cn, base_offset=1 + cn % 3, pitch_pad=odd)
    assert (37 * cn + odd) % 2 == 1
    pad4 = (-37 * cn) % 4 + 4
    c, _ = fz.encode_on_device(imgs, 53, 37, cn, pitch_pad=pad4)
    assert (37 * cn + pad4) % 4 == 0
    assert a == b == c


def test_batches_sizes_and_determinism():
    cn, rows, cols = 3, 40, 50
    pool = [fz.content(fz.KINDS[i % len(fz.KINDS)], 1 + (7 * i) % rows, 1 + (11 * i) % cols, cn, i + 1) for i in range(17)]
    pool[0] = fz.content("card", rows, cols, cn, 9)
    alone = {}

    def key(img):
        return img.tobytes() + bytes(img.shape)

    for n in (1, 3, 17):
        imgs = pool[:n]
        if n >= 3:
            imgs = imgs[:1] + [fz.content("noise", 1, 1, cn, 2), None] + imgs[1:n - 2]
        streams, lens = fz.encode_on_device(imgs, rows, cols, cn)
        for img, s in zip(imgs, streams):
            if img is None:
                assert s == b""
                continue
            check(s, img)
            assert alone.setdefault(key(img), s) == s
    # the same image at every position of a call and beside every neighbour: three images at several slots each, then the
    # call reversed, then rotated, with another base offset and pitch
    a, b, c = pool[0], pool[4], pool[9]
    order = [a, b, a, c, None, c, b, a, c, b, b, a]
    for imgs, off, pad in ((order, 0, 0), (order[::-1], 3, 1), (order[5:] + order[:5], 1, 4)):
        streams, _ = fz.encode_on_device(imgs, rows, cols, cn, base_offset=off, pitch_pad=pad)
        for img, s in zip(imgs, streams):
            assert s == (b"" if img is None else alone[key(img)])
    full = [fz.content("sheet", rows, cols, cn, 1), fz.content("gradient", rows, cols, cn, 2)]
    a, _ = fz.encode_on_device(full, rows, cols, cn, explicit_sizes=True)
    b, _ = fz.encode_on_device(full, rows, cols, cn, explicit_sizes=False)
    assert a == b == [ref.encode(im, 1) for im in full]
    assert fz.encode_on_device([], rows, cols, cn)[0] == []


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_compression_0_writes_stored_blocks_only(cn):
    rows, cols = three_blocks(cn)
    imgs = [fz.content("white", rows, cols, cn), fz.content("card", 15, 17, cn)]
    streams, lens = fz.encode_on_device(imgs, rows, cols, cn, compression=0)
    for img, s in zip(imgs, streams):
        check(s, img)
        assert set(ref.block_types(s)) == {0} and len(s) <= png.bound(*img.shape[:2], cn)
        assert s == ref.encode(img, 0)
    assert fz.encode_on_device(imgs, rows, cols, cn, compression=-2)[0] == streams
    levels = [fz.encode_on_device(imgs[1:], 15, 17, cn, compression=q)[0] for q in (1, 5, 9, 50)]
    assert levels[0] == levels[1] == levels[2] == levels[3] == [ref.encode(imgs[1], 1)]
    assert ref.block_types(levels[0][0])[-1] == "compressed"


def test_size_caps():
    rows, cols = 150, 270
    for cn in (1, 3):
        raw = ref.raw_bytes(rows, cols, cn)
        kinds = [k for k in fz.KINDS]
        streams, _ = fz.encode_on_device([fz.content(k, rows, cols, cn) for k in kinds], rows, cols, cn)
        size = {k: len(s) for k, s in zip(kinds, streams)}
        print("cn", cn, "raw", raw, size)
        assert all(v <= png.bound(rows, cols, cn) for v in size.values())
        blocks = (raw + ref.BLOCK - 1) // ref.BLOCK
        assert size["noise"] <= raw + 43 + 5 * blocks + 20   # the bound's documented overhead: every block stored
        assert size["white"] <= raw / 30
        assert size["repeated row"] <= raw / 20
        assert size["constant rows"] <= raw / 20
        assert size["four-valued"] <= 0.45 * raw


def test_host_form_and_front_doors():
    img = fz.content("card", 53, 37, 3, 5)
    s = png.encode(img, 1)
    assert s == ref.encode(img, 1) == oics.transfer.TransformableMatrix(img).encode_png()
    import ctypes as C
    from oics import _lib
    _, im = oics.transfer.as_image(img)
    n = C.c_int64(-7)
    buf = np.full(64, 0xA5, np.uint8)
    assert oics.lib().omr_png_encode(C.byref(im), 1, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == -4
    assert oics.lib().omr_last_error().decode() == "the stream takes %d bytes, the buffer holds 64" % len(s)
    assert n.value == len(s) and (buf == 0xA5).all()
    assert oics.lib().omr_png_encode(C.byref(im), 1, None, 0, C.byref(n)) == -4 and n.value == len(s)
    png.encode_stats(True)
    png.encode(img, 1)
    groups, ms = png.encode_stats(False)
    assert groups == 1 and len(ms) == len(png.STAGES_ENC) and all(v >= 0 for v in ms) and sum(ms) > 0


def _sheets():
    a = [synth.make_color_card(150, 200, 20 + i, skew=float(-2 + i))[0].copy() for i in range(3)]
    b = [synth.make_color_card(120, 90, 30 + i, skew=1.5)[0].copy() for i in range(2)]
    blank = np.full((150, 200, 3), 255, np.uint8)
    return [a[0], b[0], blank, a[1], b[1], a[2]]


def _decode_bgr(stream):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))[..., ::-1]


def test_correct_default_batch_png_equals_the_canvases():
    sheets = _sheets()
    want = omr.correct_default_batch(sheets, *PARAMS)
    got = omr.correct_default_batch_png(sheets, *PARAMS)
    assert len(got) == len(want) == 6 and any(w[3] != 0 for w in want) and sum(w[3] == 0 for w in want) >= 4
    for (ang, chk, data, rc), w in zip(got, want):
        w_ang, w_chk, w_img, w_rc = w
        assert (ang, chk, rc) == (w_ang, w_chk, w_rc)
        if rc != 0:
            assert data is None
            continue
        check(data, np.ascontiguousarray(w_img))


def test_correct_default_batch_streams_png_takes_mixed_inputs():
    from PIL import Image
    sheets = [s for i, s in enumerate(_sheets()) if i != 2][:4]
    streams = []
    for i, s in enumerate(sheets):
        b = io.BytesIO()
        Image.fromarray(s[..., ::-1]).save(b, format="JPEG" if i % 2 else "PNG", quality=95)
        streams.append(b.getvalue())
    streams.insert(2, streams[0][:60])  # a PNG stream cut short: refused, the others unaffected
    decoded = [_decode_bgr(s) for i, s in enumerate(streams) if i != 2]
    want = omr.correct_default_batch([np.ascontiguousarray(d) for d in decoded], *PARAMS)
    got = omr.correct_default_batch_streams_png(streams, *PARAMS)
    assert got[2][3] != 0 and got[2][2] is None and got[2][0] == 0.0
    for g, w in zip(got[:2] + got[3:], want):
        assert (g[0], g[1], g[3]) == (w[0], w[1], w[3]) and g[3] == 0
        check(g[2], np.ascontiguousarray(w[2]))


def test_short_fuzz_pass():
    assert fz.run(12, seed=20) is None
