"""omr_lined_picture / _device / _batch_device and the two *_ex detectors on the GPU, byte for byte against the
restatement of cv::line(.., 1, LINE_AA, 0) (tests/lined_ref.py).

The shapes and segments sit on both sides of what the kernel (csrc/lined.hip) does differently: a wavefront owns a tile
of 64 x 64 pixels, a workgroup 2 x 2 of them; a workgroup collects the segments that reach it in a list of 1024 entries
and drains the list whenever fewer than 256 are free.  Every picture is drawn onto a canvas of 0xA5 with a guard band;
any byte written outside the pictures' pixels fails the case (tests/fuzz/fuzz_lined_picture.py: device_pictures)."""
import math
import os
import sys

import numpy as np
import pytest

import lined_ref as lr
from oics import _lib, fft, hough, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_lined_picture as fz  # noqa: E402

pytestmark = pytest.mark.gpu

TILE, GROUP = 64, 128
CROSS = [(10, 20, 50, 24), (30, 5, 33, 45)]  # tests/test_lined_ref.py shows that this pair is order-sensitive


def _edges(rng, rows, cols, binary=True):
    if binary:
        return (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (rows, cols), dtype=np.uint8)


def _check(e, lines, **layout):
    lines = np.asarray(lines, np.int32).reshape(-1, 4)
    pics, err = fz.device_pictures([e], [lines], **layout)
    assert err is None, (e.shape, layout, err)
    want = lr.lined_picture(e, lines)
    assert np.array_equal(pics[0], want), (e.shape, layout, lines[:4].tolist(), int((pics[0] != want).sum()))
    return pics[0]


def _corner_lines(rows, cols):
    """end points on each border and in each corner"""
    r, c = rows - 1, cols - 1
    return [(0, 0, c, r), (c, 0, 0, r), (0, 0, c, 0), (0, r, c, r), (0, 0, 0, r), (c, 0, c, r), (c // 2, 0, c // 3, r),
            (0, r // 2, c, r // 3), (0, 0, 0, 0), (c, r, c, r), (c, 0, c, 0), (0, r, 0, r)]


@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 7), (TILE, TILE), (TILE + 1, TILE + 1), (TILE, TILE + 1), (TILE + 1, TILE),
                                       (GROUP, GROUP), (GROUP + 1, GROUP + 1), (70, 131), (33, 150)])
def test_picture_sizes(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    e = _edges(rng, rows, cols)
    _check(e, [])
    lines = _corner_lines(rows, cols)
    _check(e, lines)
    # an output pitch larger than 3 * cols, odd bases and pitches: the padding stays as it was (device_pictures checks)
    _check(e, lines, op=3 * cols + 4, oo=4, ep=cols + 4)
    _check(e, lines, op=3 * cols + 5, oo=1, ep=cols + 3, eo=3)
    for l in lines:
        _check(e, [l])


def test_single_segments_in_every_octant_and_both_end_point_orders():
    rng = np.random.default_rng(7)
    rows, cols = 90, 100
    e = _edges(rng, rows, cols)
    cx, cy = 50, 45
    segs = []
    for dx, dy in ((40, 0), (0, 40), (33, 33), (33, -33), (40, 3), (40, -3), (40, 17), (40, -17), (3, 40), (-3, 40),
                   (17, 40), (-17, 40), (40, 39), (39, 40), (1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (0, 0)):
        segs.append((cx - dx // 2, cy - dy // 2, cx - dx // 2 + dx, cy - dy // 2 + dy))
    for x0, y0, x1, y1 in segs:
        _check(e, [(x0, y0, x1, y1)])
        _check(e, [(x1, y1, x0, y0)])


def test_segments_along_tile_borders_and_through_tile_corners():
    rng = np.random.default_rng(8)
    rows, cols = 150, 200
    e = _edges(rng, rows, cols, binary=False)
    segs = []
    for t in (TILE - 2, TILE - 1, TILE, TILE + 1, GROUP - 1, GROUP, GROUP + 1):
        segs += [(0, t, cols - 1, t), (5, t, cols - 7, t + 1), (cols - 1, t + 1, 0, t - 1)]
        if t < cols:
            segs += [(t, 0, t, rows - 1), (t, 3, t + 1, rows - 4), (t + 1, rows - 1, t - 1, 0)]
    # through the corners (64, 64), (128, 64), (128, 128), (64, 128): diagonals and near-diagonals
    for cx, cy in ((TILE, TILE), (GROUP, TILE), (GROUP, GROUP), (TILE, GROUP)):
        for d in (20, 21):
            segs += [(cx - d, cy - d, cx + d, cy + d), (cx - d, cy + d, cx + d, cy - d), (cx - d, cy - d + 1, cx + d, cy + d),
                     (cx - 1, cy - 1, cx, cy), (cx, cy, cx, cy)]
    for s in segs:
        _check(e, [s])
    _check(e, segs)
    _check(e, segs[::-1])


def test_crossing_segments_in_both_orders():
    e = np.zeros((50, 60), np.uint8)
    ab = _check(e, CROSS)
    ba = _check(e, CROSS[::-1])
    assert (ab != ba).any()  # the order shows, and the device keeps it
    _check(e, [CROSS[0], CROSS[0]])  # the same segment twice: blended twice
    assert (_check(e, [CROSS[0], CROSS[0]]) != _check(e, [CROSS[0]])).any()


def test_star_of_300_segments_through_one_pixel():
    rng = np.random.default_rng(9)
    rows, cols = 140, 180
    e = _edges(rng, rows, cols)
    cx, cy = 70, 66  # beside a tile corner: the star spreads over several tiles and both workgroups
    segs = []
    for i in range(300):
        a = math.pi * i / 300.0
        dx, dy = int(round(60 * math.cos(a))), int(round(60 * math.sin(a)))
        segs.append((cx - dx, cy - dy, cx + dx, cy + dy))
    p = _check(e, segs)
    q = _check(e, segs[::-1])
    assert (p != q).any()


def test_2000_short_segments_overflow_the_tile_list():
    rng = np.random.default_rng(10)
    rows, cols = 128, 160
    e = _edges(rng, rows, cols)
    lines = fz.random_lines(rng, rows, cols, 2000, "short")
    # the first workgroup (columns 0..127) gets more segments than its list holds: it drains at least once on the way
    assert (lines[:, [0, 2]].max(axis=1) < GROUP - 12).sum() > 1024
    _check(e, lines)
    dense = lines.copy()
    dense[:, [0, 2]] = 130 + dense[:, [0, 2]] % 30  # all 2000 in the second workgroup's 32 columns
    _check(e, dense)


def test_any_background():
    rng = np.random.default_rng(11)
    e = _edges(rng, 77, 93, binary=False)
    lines = fz.random_lines(rng, 77, 93, 120, "any")
    _check(e, lines)
    pics, err = fz.device_pictures([e], [lines], color=(0, 255, 7))
    assert err is None and np.array_equal(pics[0], lr.lined_picture(e, lines, color=(0, 255, 7)))


@pytest.mark.parametrize("n", [1, 3, 17])
def test_batch_equals_per_call_device_form_equals_host_form(n):
    rng = np.random.default_rng(50 + n)
    rows, cols = 70, 131
    edges = [_edges(rng, rows, cols, binary=i % 2 == 0) for i in range(n)]
    counts = [int(rng.integers(1, 200)) for _ in range(n)]
    if n > 1:
        counts[n // 2] = 0  # an empty list in the middle
    lines = [fz.random_lines(rng, rows, cols, k, ("any", "short", "border")[i % 3]) for i, k in enumerate(counts)]
    # a scan stride larger than the image, odd bases and pitches, unused segments in front of the first list
    batch, err = fz.device_pictures(edges, lines, eo=1, ep=cols + 1, egap=13, oo=3, op=3 * cols + 2, ogap=7, lead=2, batch=True)
    assert err is None, err
    for i in range(n):
        one, err = fz.device_pictures([edges[i]], [lines[i]], batch=False)
        assert err is None, err
        assert np.array_equal(batch[i], one[0]), i
        assert np.array_equal(one[0], hough.lined_picture(edges[i], lines[i])), i
        assert np.array_equal(batch[i], lr.lined_picture(edges[i], lines[i])), i
    assert np.array_equal(fft.lined_picture(edges[0], lines[0]), batch[0])


def test_device_forms_refuse_an_end_point_outside_the_picture():
    rng = np.random.default_rng(12)
    e = _edges(rng, 40, 50)
    good = fz.random_lines(rng, 40, 50, 20, "any")
    for bad in ((50, 3, 4, 5), (3, 40, 4, 5), (3, 4, 50, 5), (3, 4, 5, 40), (-1, 3, 4, 5)):
        lines = np.concatenate([good, np.asarray([bad], np.int32)])
        for batch in (False, True):
            pics, err = fz.device_pictures([e], [lines], batch=batch)
            assert pics is None and err.startswith("rc -5"), (bad, batch, err)


def _sheet(rules):
    """a 160 x 128 synthetic sheet, optionally with a few long rules"""
    g = synth.make_card(128, 160, 3, skew=2.0)[0].copy()
    if rules:
        for y in (20, 60, 100):
            for x in range(8, 152):
                yy = y + int(round((x - 80) * math.tan(math.radians(2.0))))
                g[yy:yy + 2, x] = 0
        g[10:118, 30:32] = 0
    return g


HOUGH_ARGS = (30.0, 5.0)
FFT_ARGS = (50.0, 150.0, 10.0, 5.0)


def test_hough_detector_hands_back_the_reference_picture():
    g = _sheet(True)
    angle = hough.get_angle_with_hough(g, *HOUGH_ARGS)
    got, pic = hough.get_angle_with_hough(g, *HOUGH_ARGS, want_picture=True)
    assert np.float64(got).view(np.uint64) == np.float64(angle).view(np.uint64)
    edges = hough.canny(g, 50.0, 150.0)
    lines = hough.hough_lines_p(edges, 1.0, math.pi / 180.0, 0, *HOUGH_ARGS)
    assert len(lines) > 3
    assert pic.shape == (128, 160, 3) and np.array_equal(pic, lr.lined_picture(edges, lines))


def test_fft_detector_hands_back_the_reference_picture():
    g = _sheet(True)
    angle = fft.get_angle_with_fft(g, *FFT_ARGS)
    got, pic = fft.get_angle_with_fft(g, *FFT_ARGS, want_picture=True)
    assert np.float64(got).view(np.uint64) == np.float64(angle).view(np.uint64)
    edges = hough.canny(fft.get_fft_image(g)[1], FFT_ARGS[0], FFT_ARGS[1])
    lines = hough.hough_lines_p(edges, 1.0, math.pi / 180.0, 100, FFT_ARGS[2], FFT_ARGS[3])
    assert len(lines) >= 1
    assert pic.shape == (128, 160, 3) and np.array_equal(pic, lr.lined_picture(edges, lines))


def test_detectors_without_a_segment():
    flat = np.full((128, 160), 200, np.uint8)  # no edge, no segment
    with pytest.raises(_lib.OmrError) as e:
        hough.get_angle_with_hough(flat, *HOUGH_ARGS)
    assert e.value.code == -215
    with pytest.raises(_lib.OmrError) as e:
        hough.get_angle_with_hough(flat, *HOUGH_ARGS, want_picture=True)  # the reference panics before its imwrite
    assert e.value.code == -215
    # FFT: a minimum length no segment of a 160 x 128 picture reaches -> angle 0 and the bare edge picture
    g = _sheet(True)
    args = (FFT_ARGS[0], FFT_ARGS[1], 1000.0, 5.0)
    assert fft.get_angle_with_fft(g, *args) == 0.0
    got, pic = fft.get_angle_with_fft(g, *args, want_picture=True)
    edges = hough.canny(fft.get_fft_image(g)[1], args[0], args[1])
    assert got == 0.0 and (edges > 0).any() and np.array_equal(pic, lr.gray2bgr(edges))


def test_fuzz_slice(monkeypatch):
    """A fixed slice of tests/fuzz/fuzz_lined_picture.py: random shapes, backgrounds, segment lists, pitches, batches."""
    import runpy
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz", "fuzz_lined_picture.py")
    monkeypatch.setattr(sys, "argv", [tool, "40", "7"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(tool, run_name="__main__")
    assert e.value.code == 0
