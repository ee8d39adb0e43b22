"""The three files-to-files deskew flows on bilevel TIFF sheets: omr_deskew_with_projections / _hough / _fft_batch_streams on a
batch of two Group 4 sheets of different shapes and one JPEG return what the host-image flows return for Pillow's decode of
the same files -- angles as f64 bits, output streams byte for byte."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg_decode as fz  # noqa: E402
import tiff_ref  # noqa: E402
from oics import fft, hough, jpeg, omr, projection, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEP = (10, 0.5, 0.5)
HOUGH = (40.0, 5.0)
FFT = (30.0, 90.0, 40.0, 5.0)
LINEAR, CONTAIN = 1, 1
BORDER = (255, 255, 255, 0)
_CACHE = {}


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _batch():
    """[(stream, Pillow's decode of it as BGR)]: G4 sheets of 120 x 90 and 150 x 199 (ruled cards, skewed, thresholded), one JPEG"""
    if "b" not in _CACHE:
        out = []
        for rows, cols, seed, skew in ((120, 90, 80, 4.0), (150, 199, 64, -6.0)):
            g = synth.make_color_card(rows, cols, seed, skew)[0][..., 1]
            s = tiff_ref.pillow_tiff(g < 128, "group4", rows if seed == 80 else 32)
            out.append((s, np.repeat(tiff_ref.pillow_read(s)[..., None], 3, axis=2)))
        j = fz.make_stream(synth.make_color_card(120, 90, 81, 9.0)[0], 95, subsampling=2)
        out.append((j, fz.pillow_decode(j, 3)))
        _CACHE["b"] = out
    return _CACHE["b"]


def test_projection_flow():
    streams, imgs = [s for s, _ in _batch()], [im for _, im in _batch()]
    ang, idx, rc, out = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, quality=95, want_idx=True)
    assert list(rc) == [0, 0, 0]
    h_ang, h_idx, h_img = projection.get_angles_and_deskew(imgs, *SWEEP, interp=LINEAR, want_idx=True)
    for i in range(3):
        assert _bits(ang[i]) == _bits(h_ang[i]) and idx[i] == h_idx[i], (i, ang[i], h_ang[i])
        assert out[i] == jpeg.encode(h_img[i], 95), (i, "the output streams differ")
    a2, i2, r2, o2 = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, quality=1, png=True, want_idx=True)
    assert list(r2) == [0, 0, 0] and (_bits(a2) == _bits(ang)).all()
    from oics import png
    for i in range(3):
        assert (png.decode(o2[i], 3) == h_img[i]).all(), i


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_detector_flows(which):
    streams, imgs = [s for s, _ in _batch()], [im for _, im in _batch()]
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    ang, rc, out = mod.deskew_streams(streams, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN, level=95)
    h = mod.deskew(imgs, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN)
    h_ang, h_img = h[0], h[-1]
    made = 0
    for i in range(3):
        assert _bits(ang[i]) == _bits(h_ang[i]), (i, ang[i], h_ang[i])
        if h_img[i] is None:
            assert which == "hough" and rc[i] == -215 and out[i] is None
            continue
        made += 1
        assert rc[i] == 0 and out[i] == jpeg.encode(h_img[i], 95), (i, "the output streams differ")
    assert made >= 2
    a_png, rc_png, out_png = mod.deskew_streams(streams, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN, png=True, level=1)
    assert list(rc_png) == list(rc) and (_bits(a_png) == _bits(ang)).all()


def test_correct_default_streams_stay_out_of_scope():
    """omr_correct_default_batch_streams has its own dispatch: a TIFF sheet is refused there as before, its neighbour corrected"""
    import correct_sheets as S
    streams = [s for s, _ in _batch()]
    got = omr.correct_default_batch_streams([streams[0], streams[2]], *S.PARAMS, quality=95)
    assert got[0][3] != 0 and got[0][2] is None and got[1][3] == 0
