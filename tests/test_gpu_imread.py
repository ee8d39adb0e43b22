"""The imread layer on the GPU: omr_imread_batch_device and omr_imread on JPEG streams that carry an EXIF orientation,
mixed with unturned streams and a PNG.  The reference of every comparison is Pillow's decode of the stream turned by
ImageOps.exif_transpose (BGR) and tests/orient_ref.py's restatement of it on Pillow's stored decode (BGR and gray)."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg_decode as fz  # noqa: E402
import fuzz_png_decode as fp  # noqa: E402
import orient_ref as O  # noqa: E402
import png_ref as P  # noqa: E402
from oics import _lib, imread  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
VARIANTS = [dict(gray=True), dict(subsampling=0, restart_marker_blocks=3), dict(subsampling=1), dict(subsampling=2)]
_CACHE = {}


def _img(seed=0):
    return np.random.Generator(np.random.PCG64(700 + seed)).integers(0, 256, (37, 53, 3), dtype=np.uint8)


def _batch():
    """[(stream, stored decode's source, code)]: every variant x codes 2..8 x both byte orders, a code-1 stream, an
    untagged one and an RGB PNG"""
    if "batch" not in _CACHE:
        out = []
        for v, kw in enumerate(VARIANTS):
            plain = fz.make_stream(_img(v), (100, 90, 75, 95)[v], **kw)
            for code in range(2, 9):
                for le in (True, False):
                    out.append((O.tag_jpeg(plain, code, le), plain, code))
        plain = fz.make_stream(_img(9), 90, subsampling=2)
        out += [(O.tag_jpeg(plain, 1), plain, 1), (plain, plain, 1)]
        png = P.write(_img(10)[..., ::-1], 2, 8)
        out.append((png, png, 1))
        _CACHE["batch"] = out
    return _CACHE["batch"]


def _stored(stream, channels):
    return (fp if stream[:8] == P.SIGNATURE else fz).pillow_decode(stream, channels)


def _pillow_transposed(stream):
    from PIL import Image, ImageOps
    im = ImageOps.exif_transpose(Image.open(io.BytesIO(stream)))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def _decode(streams, rows, cols, channels, flags=0, pitch_pad=5, base_offset=1):
    """-> (images, out_size, rc); every byte of a slot outside its image still holds FILL"""
    import torch
    n = len(streams)
    step = cols * channels + pitch_pad
    stride = rows * step + pitch_pad
    out = torch.full((base_offset + max(n, 1) * stride + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    size, rc = imread.decode_batch_device(streams, channels, out.data_ptr() + base_offset, stride, step, rows, cols, flags)
    got = out.cpu().numpy()
    assert (got[:base_offset] == FILL).all() and (got[base_offset + n * stride:] == FILL).all()
    imgs = []
    for i in range(n):
        slot = got[base_offset + i * stride: base_offset + (i + 1) * stride]
        body = slot[:rows * step].reshape(rows, step)
        r, c = (int(size[i, 0]), int(size[i, 1])) if rc[i] == 0 else (0, 0)
        mask = np.ones((rows, step), bool)
        mask[:r, :c * channels] = False
        assert (body[mask] == FILL).all() and (slot[rows * step:] == FILL).all(), "slot %d written outside its image" % i
        im = body[:r, :c * channels].copy()
        imgs.append(im.reshape(r, c) if channels == 1 else im.reshape(r, c, 3))
    return imgs, size, rc


@pytest.mark.parametrize("channels", [3, 1])
def test_mixed_batch_equals_pillow_turned(channels):
    items = _batch()
    if channels == 1:
        items = [it for it in items if it[0][:8] != P.SIGNATURE]      # gray from an RGB PNG is the PNG decoder's -213
    streams = [s for s, _, _ in items]
    imgs, size, rc = _decode(streams, 53, 53, channels)
    assert (rc == 0).all(), rc
    for i, (s, plain, code) in enumerate(items):
        want = O.apply(_stored(plain, channels), code)
        assert tuple(size[i]) == want.shape[:2], (i, code)
        assert imgs[i].shape == want.shape and (imgs[i] == want).all(), (i, code, int((imgs[i] != want).sum()))
        if channels == 3 and s[:8] != P.SIGNATURE:
            assert (imgs[i] == _pillow_transposed(s)).all(), (i, code)
    assert len({im.tobytes() for im in imgs}) >= 7 * len(VARIANTS)      # the turns differ: the comparison says something


def test_slot_fit_is_judged_on_the_turned_size():
    plain = fz.make_stream(_img(1), 90, subsampling=2)
    six, three = O.tag_jpeg(plain, 6), O.tag_jpeg(plain, 3)
    imgs, size, rc = _decode([six, three, plain], 37, 53, 3)
    assert list(rc) == [-5, 0, 0] and list(size[0]) == [0, 0]
    assert (imgs[1] == O.apply(_stored(plain, 3), 3)).all() and (imgs[2] == _stored(plain, 3)).all()
    imgs, size, rc = _decode([six, three, plain], 53, 37, 3)
    assert list(rc) == [0, -5, -5] and list(size[0]) == [53, 37]
    assert (imgs[0] == O.apply(_stored(plain, 3), 6)).all()


def test_ignore_orientation_gives_the_stored_picture():
    plain = fz.make_stream(_img(2), 95, subsampling=1)
    streams = [O.tag_jpeg(plain, code) for code in (6, 3, 9, 1)]
    imgs, size, rc = _decode(streams, 37, 53, 3, flags=imread.IGNORE_ORIENTATION)
    assert (rc == 0).all(), rc
    for im in imgs:
        assert (im == _stored(plain, 3)).all()
    assert (imread.decode(streams[0], 3, imread.IGNORE_ORIENTATION) == _stored(plain, 3)).all()


def test_a_refused_stream_leaves_its_neighbours_alone():
    plain = fz.make_stream(_img(3), 90, subsampling=2)
    prog = fz.make_stream(_img(3), 90, progressive=True)
    streams = [O.tag_jpeg(plain, 8), O.tag_jpeg(prog, 6), O.tag_jpeg(plain, 9), O.tag_jpeg(plain, 5), prog, plain]
    imgs, size, rc = _decode(streams, 53, 53, 3)
    assert list(rc) == [0, -213, -213, 0, -213, 0]
    for i, code in ((0, 8), (3, 5), (5, 1)):
        assert (imgs[i] == O.apply(_stored(plain, 3), code)).all(), i
    # a turned stream whose entropy data is cut short: its own code, the others unaffected
    cut = O.tag_jpeg(plain, 6)[:-40]
    imgs, size, rc = _decode([cut, O.tag_jpeg(plain, 6)], 53, 53, 3)
    assert list(rc) == [-215, 0] and list(size[0]) == [0, 0]
    assert (imgs[1] == O.apply(_stored(plain, 3), 6)).all()


@pytest.mark.parametrize("channels", [3, 1])
def test_one_buffer_form(channels):
    for v, kw in enumerate(VARIANTS):
        plain = fz.make_stream(_img(v), 90, **kw)
        for code in (1, 3, 6, 7):
            got = imread.decode(O.tag_jpeg(plain, code, le := code % 2 == 0), channels)
            want = O.apply(_stored(plain, channels), code)
            assert got.shape == want.shape and (got == want).all(), (v, code, le)
    png = P.write(_img(10)[..., ::-1], 2, 8)
    assert (imread.decode(png, 3) == _stored(png, 3)).all()
    with pytest.raises(_lib.OmrError) as e:
        imread.decode(O.tag_jpeg(fz.make_stream(_img(0), 90), 0), channels)
    assert e.value.code == -213
