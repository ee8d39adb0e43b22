"""The three files-to-files deskew flows with Group 4 TIFF outputs (omr_deskew_with_projections_batch_streams_tiff,
omr_deskew_with_hough_batch_streams_tiff, omr_deskew_with_fft_batch_streams_tiff) on the GPU: a small batch of JPEG, PNG
and Group 4 inputs with one refused member; angles and scan_rc are the _png form's, every output is byte for byte
omr_tiff_encode of the host-image flow's canvas (and of the canvas the _png form's output decodes to), NULL outputs give
the angles alone."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tiff_ref  # noqa: E402
from oics import fft, hough, imread, projection, synth, tiff  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS = 150, 199
HOUGH = (40.0, 5.0)
FFT = (30.0, 90.0, 40.0, 5.0)
PROJ = (45, 0.2, 1.0)
TIFF = dict(threshold=140, rows_per_strip=64, dpi=300)
_STREAMS = []


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _save(img, fmt, **kw):
    bio = io.BytesIO()
    Image.fromarray(img if img.ndim == 2 else img[..., ::-1].copy()).save(bio, format=fmt, **kw)
    return bio.getvalue()


def streams():
    """a gray JPEG, an RGB PNG, two Group 4 TIFFs of one shape (one bucket of two), a progressive JPEG (refused, -213), a
    truncated TIFF header (malformed) and a smaller gray PNG"""
    if not _STREAMS:
        g1 = synth.make_card(ROWS, COLS, 61, 3.0)[0]
        c2 = synth.make_color_card(ROWS, COLS, 62, -7.0)[0]
        g3 = synth.make_card(ROWS, COLS, 63, 5.0)[0]
        g4 = synth.make_card(ROWS, COLS, 64, -4.0)[0]
        g5 = synth.make_card(120, 163, 65, 8.0)[0]
        _STREAMS.extend([_save(g1, "JPEG", quality=95), _save(c2, "PNG"), tiff_ref.pillow_tiff(g3 <= 127), tiff_ref.pillow_tiff(g4 <= 127, rps=8),
                         _save(g1, "JPEG", quality=90, progressive=True), b"II*\0" + bytes(6), _save(g5, "PNG")])
    return _STREAMS


GOOD = (0, 1, 2, 3, 6)


def check_outputs(out, canvases, rc):
    for i, s in enumerate(out):
        if rc[i] != 0:
            assert s is None
            continue
        canvas = canvases[i]
        assert s == tiff.encode(canvas, TIFF["threshold"], TIFF["rows_per_strip"], TIFF["dpi"]), i
        h = tiff_ref.parse(s)
        assert (h["rows"], h["cols"]) == canvas.shape[:2] and h["rps"] == min(64, canvas.shape[0])
        gray = canvas if canvas.ndim == 2 else tiff_enc_gray(canvas)
        assert (tiff_ref.pillow_read(s) == np.where(gray <= TIFF["threshold"], 0, 255)).all()


def tiff_enc_gray(bgr):
    import tiff_enc_ref
    return tiff_enc_ref.gray_of(bgr)


def png_canvas(s, channels):
    a = np.asarray(Image.open(io.BytesIO(s)))
    return a if channels == 1 else a[..., ::-1].copy()


def test_projection_flow(channels=3):
    ss = streams()
    ang_p, rc_p, out_p = projection.deskew_streams(ss, *PROJ, png=True, quality=1, channels=channels)
    ang, rc, out = projection.deskew_streams_tiff(ss, *PROJ, channels=channels, **TIFF)
    assert (bits(ang) == bits(ang_p)).all() and list(rc) == list(rc_p)
    assert [int(c) for c in rc] == [0, 0, 0, 0, -213, -5, 0]
    check_outputs(out, [None if s is None else png_canvas(s, channels) for s in out_p], rc)
    # the host-image flow's canvases
    imgs = [imread.decode(ss[i], channels) for i in GOOD]
    ang_h, rot = projection.get_angles_and_deskew(imgs, *PROJ)
    for k, i in enumerate(GOOD):
        assert bits(ang_h[k]) == bits(ang[i])
        assert out[i] == tiff.encode(rot[k], TIFF["threshold"], TIFF["rows_per_strip"], TIFF["dpi"]), i
    ang_n, rc_n = projection.get_angles_from_streams(ss, *PROJ, channels=channels)
    assert (bits(ang_n) == bits(ang)).all() and list(rc_n) == list(rc)


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_detector_flows(which):
    ss = streams()
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    ang_p, rc_p, out_p = mod.deskew_streams(ss, *args, png=True, level=1)
    ang, rc, out = mod.deskew_streams_tiff(ss, *args, **TIFF)
    assert (bits(ang) == bits(ang_p)).all() and list(rc) == list(rc_p)
    assert int(rc[4]) == -213 and int(rc[5]) == -5 and sum(int(c) == 0 for c in rc) >= 3
    check_outputs(out, [None if s is None else png_canvas(s, 3) for s in out_p], rc)
    # the host-image flow's canvases
    imgs = [imread.decode(ss[i], 3) for i in GOOD]
    res = mod.deskew(imgs, *args)
    rot = res[-1]
    for k, i in enumerate(GOOD):
        if rc[i] == 0:
            assert out[i] == tiff.encode(rot[k], TIFF["threshold"], TIFF["rows_per_strip"], TIFF["dpi"]), i
    ang_n, rc_n, none = mod.deskew_streams_tiff(ss, *args, want_out=False, **TIFF)
    assert none is None and (bits(ang_n) == bits(ang)).all() and list(rc_n) == list(rc)
