"""tests/lined_ref.py -- the restatement of cv::line(.., 1, LINE_AA, 0) that the GPU line pictures are tested against:
properties that hold whatever the filter tables contain, the statement-by-statement walk against the closed form the
kernel implements, and -- where a cv2 can be imported -- OpenCV itself, byte for byte."""
import numpy as np
import pytest

import lined_ref as lr

CROSS = [(10, 20, 50, 24), (30, 5, 33, 45)]  # a shallow and a steep segment that cross near (30, 22)


def _random_lines(rng, rows, cols, n, max_len=None):
    x0 = rng.integers(0, cols, n)
    y0 = rng.integers(0, rows, n)
    if max_len is None:
        x1, y1 = rng.integers(0, cols, n), rng.integers(0, rows, n)
    else:
        x1 = np.clip(x0 + rng.integers(-max_len, max_len + 1, n), 0, cols - 1)
        y1 = np.clip(y0 + rng.integers(-max_len, max_len + 1, n), 0, rows - 1)
    return np.stack([x0, y0, x1, y1], 1).astype(np.int32)


def test_no_lines_is_gray2bgr():
    rng = np.random.default_rng(1)
    e = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    pic = lr.lined_picture(e, np.zeros((0, 4), np.int32))
    assert pic.shape == (9, 13, 3) and pic.dtype == np.uint8
    for c in range(3):
        assert np.array_equal(pic[:, :, c], e)
    assert np.array_equal(lr.gray2bgr(e), pic)


def test_literal_walk_equals_closed_form():
    rng = np.random.default_rng(2)
    rows, cols = 37, 53
    bg = lr.gray2bgr(rng.integers(0, 256, (rows, cols), dtype=np.uint8))
    lines = np.concatenate([
        _random_lines(rng, rows, cols, 150),
        np.array([(0, 0, cols - 1, rows - 1), (cols - 1, 0, 0, rows - 1), (5, 5, 5, 5), (0, 0, 0, 0),
                  (cols - 1, rows - 1, cols - 1, rows - 1), (0, 7, cols - 1, 7), (9, rows - 1, 9, 0),
                  (3, 3, 20, 20), (20, 3, 3, 20), (20, 20, 3, 3), (3, 20, 20, 3)], np.int32)])
    for l in lines:  # one by one: a difference names its segment
        a = lr.draw_lines_aa(bg, [l], literal=True)
        b = lr.draw_lines_aa(bg, [l])
        assert np.array_equal(a, b), l
    assert np.array_equal(lr.draw_lines_aa(bg, lines, literal=True), lr.draw_lines_aa(bg, lines))


def test_far_pixels_are_untouched_and_painted_ones_move_towards_the_colour():
    rng = np.random.default_rng(3)
    rows, cols = 60, 80
    e = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    bg = lr.gray2bgr(e)
    lines = _random_lines(rng, rows, cols, 6)
    pic = lr.draw_lines_aa(bg, lines)
    far = lr.chebyshev_far_mask((rows, cols), lines, 2.0)
    assert far.any() and not far.all()
    assert np.array_equal(pic[far], bg[far])
    assert (pic != bg).any()
    # a single segment: every channel ends between its old value and the colour's
    for l in lines:
        one = lr.draw_lines_aa(bg, [l]).astype(int)
        lo = np.minimum(bg.astype(int), np.asarray(lr.COLOR))
        hi = np.maximum(bg.astype(int), np.asarray(lr.COLOR))
        assert (one >= lo).all() and (one <= hi).all(), l


def test_crossing_segments_depend_on_their_order():
    """tests/test_gpu_lined_picture.py relies on this case being order-sensitive"""
    bg = lr.gray2bgr(np.zeros((50, 60), np.uint8))
    ab = lr.draw_lines_aa(bg, CROSS)
    ba = lr.draw_lines_aa(bg, CROSS[::-1])
    diff = (ab != ba).any(axis=2)
    assert diff.any()
    ys, xs = np.nonzero(diff)
    assert (abs(xs - 31) <= 3).all() and (abs(ys - 22) <= 3).all()  # only at the crossing


def test_color_argument():
    bg = lr.gray2bgr(np.full((8, 8), 7, np.uint8))
    assert np.array_equal(lr.draw_lines_aa(bg, [(1, 1, 6, 5)], color=(7, 7, 7)), bg)
    p = lr.draw_lines_aa(bg, [(1, 1, 6, 5)], color=(7, 200, 7))
    assert np.array_equal(p[:, :, 0], bg[:, :, 0]) and np.array_equal(p[:, :, 2], bg[:, :, 2]) and (p[:, :, 1] > 7).any()


def test_against_cv2_line_when_there_is_one():
    cv2 = pytest.importorskip("cv2", reason="no OpenCV on this machine: the restatement is pinned against the GPU only")
    print("OpenCV", cv2.__version__)
    rng = np.random.default_rng(4)
    rows, cols = 64, 96
    e = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    lines = _random_lines(rng, rows, cols, 200)
    pic = cv2.cvtColor(e, cv2.COLOR_GRAY2BGR)
    for x0, y0, x1, y1 in lines.tolist():
        cv2.line(pic, (x0, y0), (x1, y1), (186, 88, 255, 0), 1, cv2.LINE_AA, 0)
    assert np.array_equal(pic, lr.lined_picture(e, lines)), "restatement != cv2.line of OpenCV %s" % cv2.__version__
