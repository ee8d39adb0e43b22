"""The three files-to-files deskew flows with 8-bit TIFF outputs (omr_deskew_with_projections_batch_streams_tiff8,
omr_deskew_with_hough_batch_streams_tiff8, omr_deskew_with_fft_batch_streams_tiff8) on the GPU: a small batch of gray LZW
TIFF, RGB TIFF, JPEG and PNG inputs with one refused member; angles and scan_rc are the _png form's, every output is byte
for byte omr_tiff8_encode of the host-image flow's canvas and decodes to the canvas the _png form's output decodes to; a
gray TIFF sheet fed in at angle 0 comes out with its gray levels."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tiff8_ref  # noqa: E402
from oics import fft, hough, imread, projection, synth, tiff  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS = 150, 199
HOUGH = (40.0, 5.0)
FFT = (30.0, 90.0, 40.0, 5.0)
PROJ = (45, 0.2, 1.0)
TIFF8 = dict(compression=5, predictor=2, rows_per_strip=0, dpi=300)
ARGS = (5, 2, 0, 300)
_STREAMS = []


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _save(img, fmt, **kw):
    bio = io.BytesIO()
    Image.fromarray(img if img.ndim == 2 else img[..., ::-1].copy()).save(bio, format=fmt, **kw)
    return bio.getvalue()


def streams():
    """a gray LZW TIFF and an RGB TIFF of one shape, a gray JPEG, an RGB PNG, a progressive JPEG (refused, -213) and a
    smaller gray PNG"""
    if not _STREAMS:
        g1 = synth.make_card(ROWS, COLS, 61, 3.0)[0]
        c2 = synth.make_color_card(ROWS, COLS, 62, -7.0)[0]
        g3 = synth.make_card(ROWS, COLS, 63, 5.0)[0]
        c4 = synth.make_color_card(ROWS, COLS, 64, -4.0)[0]
        g5 = synth.make_card(120, 163, 65, 8.0)[0]
        _STREAMS.extend([tiff8_ref.pillow_tiff(g1, "tiff_lzw", rps=16), tiff8_ref.pillow_tiff(c2[..., ::-1], "tiff_lzw", predictor=2),
                         _save(g3, "JPEG", quality=95), _save(c4, "PNG"), _save(g1, "JPEG", quality=90, progressive=True), _save(g5, "PNG")])
    return _STREAMS


GOOD = (0, 1, 2, 3, 5)


def png_canvas(s, channels):
    a = np.asarray(Image.open(io.BytesIO(s)))
    return a if channels == 1 else a[..., ::-1].copy()


def check_outputs(out, out_png, rc, channels):
    for i, s in enumerate(out):
        if rc[i] != 0:
            assert s is None
            continue
        canvas = png_canvas(out_png[i], channels)
        assert s == tiff.encode8(canvas, *ARGS), i
        h = tiff8_ref.parse(s)
        assert (h["rows"], h["cols"], h["spp"], h["predictor"]) == canvas.shape[:2] + (channels, 2)
        assert (tiff8_ref.pillow_read(s) == (canvas if channels == 1 else canvas[..., ::-1])).all()
        assert (tiff.decode(s, channels) == canvas).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_projection_flow(channels):
    ss = streams()
    ang_p, rc_p, out_p = projection.deskew_streams(ss, *PROJ, png=True, quality=1, channels=channels)
    ang, rc, out = projection.deskew_streams_tiff8(ss, *PROJ, channels=channels, **TIFF8)
    assert (bits(ang) == bits(ang_p)).all() and list(rc) == list(rc_p)
    # a colour TIFF or PNG asked for as gray is refused by its decoder (-213), like the progressive JPEG
    assert [int(c) for c in rc] == ([0, 0, 0, 0, -213, 0] if channels == 3 else [0, -213, 0, -213, -213, 0])
    check_outputs(out, out_p, rc, channels)
    # the host-image flow's canvases
    good = [i for i in GOOD if rc[i] == 0]
    imgs = [imread.decode(ss[i], channels) for i in good]
    ang_h, rot = projection.get_angles_and_deskew(imgs, *PROJ)
    for k, i in enumerate(good):
        assert bits(ang_h[k]) == bits(ang[i])
        assert out[i] == tiff.encode8(rot[k], *ARGS), i


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_detector_flows(which):
    ss = streams()
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    ang_p, rc_p, out_p = mod.deskew_streams(ss, *args, png=True, level=1)
    ang, rc, out = mod.deskew_streams_tiff8(ss, *args, **TIFF8)
    assert (bits(ang) == bits(ang_p)).all() and list(rc) == list(rc_p)
    assert int(rc[4]) == -213 and sum(int(c) == 0 for c in rc) >= 3
    check_outputs(out, out_p, rc, 3)
    imgs = [imread.decode(ss[i], 3) for i in GOOD]
    rot = mod.deskew(imgs, *args)[-1]
    for k, i in enumerate(GOOD):
        if rc[i] == 0:
            assert out[i] == tiff.encode8(rot[k], *ARGS), i
    ang_n, rc_n, none = mod.deskew_streams_tiff8(ss, *args, want_out=False, **TIFF8)
    assert none is None and (bits(ang_n) == bits(ang)).all() and list(rc_n) == list(rc)


def test_a_gray_sheet_at_angle_0_keeps_its_gray_levels():
    """the point of the change: a straight gray TIFF sheet goes through the projection flow and leaves as TIFF with every
    gray level it came with (Group 4 would leave two, JPEG would change them)"""
    # ruled lines across the whole width (the sweep's sharpest profile is at 0), paper and ink shaded from left to right
    x = np.arange(COLS)
    sheet = np.tile(190 + x * 60 // COLS, (ROWS, 1)) + np.random.RandomState(3).randint(0, 6, (ROWS, COLS))
    sheet[10::12] = sheet[11::12] = (x * 50 // COLS)[None, :]
    sheet = sheet.astype(np.uint8)
    assert len(np.unique(sheet)) > 100
    src = tiff8_ref.pillow_tiff(sheet, "tiff_lzw")
    for kw in (dict(compression=5, predictor=1), dict(compression=5, predictor=2), dict(compression=1, predictor=1)):
        # candidates -45, 0 and 45 degrees: at a step of 0.2 a sheet this small has the same profile at -0.2 and at 0
        ang, rc, out = projection.deskew_streams_tiff8([src], 45, 45.0, 1.0, channels=1, **kw)
        assert int(rc[0]) == 0 and float(ang[0]) == 0.0
        back = tiff8_ref.pillow_read(out[0])
        assert back.shape == sheet.shape and (back == sheet).all()
        assert (tiff.decode(out[0], 1) == sheet).all()
