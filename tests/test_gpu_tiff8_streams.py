"""The three files-to-files deskew flows on 8-bit gray and RGB TIFF sheets: omr_deskew_with_projections / _hough /
_fft_batch_streams on a batch of small gray and RGB TIFF sheets (LZW, LZW with Predictor 2, raw, PackBits) mixed with a
JPEG return what the host-image flows return for Pillow's decode of the same files -- angles as f64 bits, output streams
byte for byte; Group 4 outputs from gray TIFF; an RGB TIFF in a gray call is refused alone."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg_decode as fz  # noqa: E402
import tiff8_ref as R  # noqa: E402
from oics import fft, hough, jpeg, projection, synth, tiff  # noqa: E402

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
    """[(stream, Pillow's decode of it as BGR)]: an RGB LZW sheet of 120 x 90, a gray LZW + Predictor 2 sheet of 150 x 199 in
    strips of 32 rows, a gray raw and an RGB PackBits sheet of 120 x 90, one JPEG"""
    if "b" not in _CACHE:
        out = []
        for rows, cols, seed, skew, gray, form in ((120, 90, 80, 4.0, False, ("tiff_lzw", None, 1)), (150, 199, 64, -6.0, True, ("tiff_lzw", 32, 2)),
                                                   (120, 90, 82, -3.0, True, ("raw", None, 1)), (120, 90, 83, 7.0, False, ("packbits", 16, 1))):
            bgr = synth.make_color_card(rows, cols, seed, skew)[0]
            s = R.pillow_tiff(np.ascontiguousarray(bgr[..., 1]) if gray else np.ascontiguousarray(bgr[..., ::-1]), *form)
            out.append((s, R.as_output(R.pillow_read(s), 3)))
        j = fz.make_stream(synth.make_color_card(120, 90, 81, 9.0)[0], 95, subsampling=2)
        out.append((j, fz.pillow_decode(j, 3)))
        _CACHE["b"] = out
    return _CACHE["b"]


def test_projection_flow():
    streams, imgs = [s for s, _ in _batch()], [im for _, im in _batch()]
    n = len(streams)
    ang, idx, rc, out = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, quality=95, want_idx=True)
    assert list(rc) == [0] * n
    h_ang, h_idx, h_img = projection.get_angles_and_deskew(imgs, *SWEEP, interp=LINEAR, want_idx=True)
    for i in range(n):
        assert _bits(ang[i]) == _bits(h_ang[i]) and idx[i] == h_idx[i], (i, ang[i], h_ang[i])
        assert out[i] == jpeg.encode(h_img[i], 95), (i, "the output streams differ")


def test_projection_flow_group4_outputs_from_gray_tiff_and_rgb_refused_in_a_gray_call():
    streams, imgs = [s for s, _ in _batch()], [im for _, im in _batch()]
    ang, idx, rc, out = projection.deskew_streams_tiff(streams, *SWEEP, interp=LINEAR, threshold=127, channels=1, want_idx=True)
    assert list(rc) == [-213, 0, 0, -213, 0] and out[0] is None and out[3] is None
    keep = [1, 2]
    gray = [np.ascontiguousarray(imgs[i][..., 0]) for i in keep]
    h_ang, h_idx, h_img = projection.get_angles_and_deskew(gray, *SWEEP, interp=LINEAR, want_idx=True)
    for k, i in enumerate(keep):
        assert _bits(ang[i]) == _bits(h_ang[k]) and idx[i] == h_idx[k], (i, ang[i], h_ang[k])
        assert out[i] == tiff.encode(h_img[k], 127), (i, "the Group 4 files differ")
    # each as if sent alone: the refused neighbours change nothing
    a1, r1, o1 = projection.deskew_streams_tiff([streams[1]], *SWEEP, interp=LINEAR, threshold=127, channels=1)
    assert r1[0] == 0 and _bits(a1[0]) == _bits(ang[1]) and o1[0] == out[1]


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_detector_flows(which):
    streams, imgs = [s for s, _ in _batch()], [im for _, im in _batch()]
    n = len(streams)
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    ang, rc, out = mod.deskew_streams(streams, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN, level=95)
    h = mod.deskew(imgs, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN)
    h_ang, h_img = h[0], h[-1]
    made = 0
    for i in range(n):
        assert _bits(ang[i]) == _bits(h_ang[i]), (i, ang[i], h_ang[i])
        if h_img[i] is None:
            assert which == "hough" and rc[i] == -215 and out[i] is None
            continue
        made += 1
        assert rc[i] == 0 and out[i] == jpeg.encode(h_img[i], 95), (i, "the output streams differ")
    assert made >= 3
