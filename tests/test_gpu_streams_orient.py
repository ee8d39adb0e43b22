"""The files-to-files deskew flow on sheets that carry an EXIF orientation: omr_deskew_with_projections_batch_streams (JPEG
and PNG outputs, and the angles alone) returns what the host-image flow (omr_deskew_with_projections_batch +
omr_jpeg_encode) returns for omr_imread's images of the same files: angles as f64 bits, streams byte for byte.  The
correct_default streams flows keep refusing such a sheet (an existing test pins that).  omr_imread itself is checked against Pillow in
tests/test_gpu_imread.py.

One batch: a 120 x 90 sheet tagged 1, two 90 x 120 sheets tagged 6 and 8 (120 x 90 after the turn: the same bucket, next
to the unturned sheet), a 120 x 90 sheet tagged 3, an untagged PNG of that shape and a progressive JPEG (-213)."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import correct_sheets as S  # noqa: E402
import fuzz_jpeg_decode as fz  # noqa: E402
import orient_ref as O  # noqa: E402
import png_ref as P  # noqa: E402
from oics import imread, jpeg, omr, projection, transfer  # noqa: E402
from oics.types import RotateClipStrategy  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEP = (10, 0.5, 0.5)
LINEAR = 1
_CACHE = {}


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _batch():
    """[(stream, scan_rc expected)]"""
    if "b" not in _CACHE:
        tall = [S.sheet("card", 120, 90, 3, 40 + i) for i in range(3)]
        wide = [S.sheet("card", 90, 120, 3, 50 + i) for i in range(2)]
        _CACHE["b"] = [(O.tag_jpeg(fz.make_stream(tall[0], 95, subsampling=2), 1), 0),
                       (O.tag_jpeg(fz.make_stream(wide[0], 95, subsampling=2), 6), 0),
                       (O.tag_jpeg(fz.make_stream(wide[1], 90, subsampling=0, restart_marker_blocks=3), 8, False), 0),
                       (O.tag_jpeg(fz.make_stream(tall[1], 100, gray=True), 3), 0),
                       (P.write(np.ascontiguousarray(tall[2][..., ::-1]), 2, 8), 0),
                       (O.tag_jpeg(fz.make_stream(tall[0], 90, progressive=True), 6), -213)]
    return _CACHE["b"]


def _images():
    """omr_imread's image of every accepted sheet (None for the refused one)"""
    if "i" not in _CACHE:
        _CACHE["i"] = [imread.decode(s, 3) if code == 0 else None for s, code in _batch()]
        assert [im.shape for im in _CACHE["i"] if im is not None] == [(120, 90, 3)] * 5
    return _CACHE["i"]


def _host_flow():
    if "h" not in _CACHE:
        good = [im for im in _images() if im is not None]
        _CACHE["h"] = projection.get_angles_and_deskew(good, *SWEEP, interp=LINEAR, want_idx=True)
    return _CACHE["h"]


def test_imread_turned_the_sheets():
    streams = [s for s, _ in _batch()]
    assert [imread.info(s)[:2] for s in streams[:5]] == [(120, 90)] * 5
    assert imread.info(streams[1])[3] == 6 and imread.info(streams[2])[3] == 8
    assert (_images()[1] == O.apply(fz.pillow_decode(streams[1], 3), 6)).all()


def test_deskew_streams_jpeg_outputs_equal_the_host_image_flow():
    streams, want_rc = [s for s, _ in _batch()], [c for _, c in _batch()]
    ang, idx, rc, out = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, quality=95, want_idx=True)
    assert list(rc) == want_rc and out[5] is None and ang[5] == 0.0 and idx[5] == -1
    h_ang, h_idx, h_img = _host_flow()
    for k, i in enumerate(range(5)):
        assert _bits(ang[i]) == _bits(h_ang[k]) and idx[i] == h_idx[k], (i, ang[i], h_ang[k])
        assert out[i] == jpeg.encode(h_img[k], 95), (i, "the output streams differ")
    assert len(set(out[:5])) == 5
    # every sheet as if sent alone
    for i in (1, 2, 3):
        a1, i1, r1, o1 = projection.deskew_streams([streams[i]], *SWEEP, interp=LINEAR, quality=95, want_idx=True)
        assert r1[0] == 0 and _bits(a1[0]) == _bits(ang[i]) and o1[0] == out[i], i


def test_deskew_streams_png_outputs_decode_to_the_canvas_and_the_angles_alone():
    from PIL import Image
    streams, want_rc = [s for s, _ in _batch()], [c for _, c in _batch()]
    ang, idx, rc, out = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, quality=1, png=True, want_idx=True)
    assert list(rc) == want_rc and out[5] is None
    h_ang, h_idx, h_img = _host_flow()
    for i in range(5):
        assert _bits(ang[i]) == _bits(h_ang[i]) and idx[i] == h_idx[i], i
        back = np.asarray(Image.open(io.BytesIO(out[i])).convert("RGB"))[..., ::-1]
        assert back.shape == h_img[i].shape and (back == h_img[i]).all(), i
    a2, i2, r2 = projection.get_angles_from_streams(streams, *SWEEP, want_idx=True)
    assert list(r2) == want_rc and (_bits(a2[:5]) == _bits(h_ang)).all() and (i2[:5] == h_idx).all()


def test_deskew_streams_gray_form():
    """channels = 1: the Y plane, turned"""
    streams = [s for s, c in _batch() if c == 0 and s[:8] != P.SIGNATURE]
    ang, idx, rc, out = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, border=(255,), quality=95, channels=1, want_idx=True)
    assert list(rc) == [0] * 4
    imgs = [imread.decode(s, 1) for s in streams]
    assert [im.shape for im in imgs] == [(120, 90)] * 4
    h_ang, h_idx, h_img = projection.get_angles_and_deskew(imgs, *SWEEP, interp=LINEAR, border=(255,), want_idx=True)
    for i in range(4):
        assert _bits(ang[i]) == _bits(h_ang[i]) and out[i] == jpeg.encode(h_img[i], 95), i


def test_correct_default_streams_keep_their_refusal():
    """omr_correct_default_batch_streams / _streams_png are not part of this layer: tests/test_jpeg_decode_abi.py pins -213
    for an orientation other than 1 there, so a tagged sheet keeps that code and its untagged neighbours are corrected as
    omr_correct_default_batch_jpeg corrects omr_imread's images of them"""
    streams = [s for s, _ in _batch()]
    got = omr.correct_default_batch_streams(streams, *S.PARAMS, quality=95)
    assert [t[3] for t in got][1:4] == [-213] * 3 and got[5][3] == -213
    assert all(t[:3] == (0.0, False, None) for t in got[1:4])
    imgs = _images()
    want = omr.correct_default_batch_jpeg([imgs[0], imgs[4]], *S.PARAMS, quality=95)
    for i, w in zip((0, 4), want):
        assert got[i][3] == w[3] and got[i][1] == w[1] and _bits(got[i][0]) == _bits(w[0]) and got[i][2] == w[2], i
    as_png = omr.correct_default_batch_streams_png(streams, *S.PARAMS, compression=1)
    assert [t[3] for t in as_png][1:4] == [-213] * 3
