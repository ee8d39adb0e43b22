"""The numpy restatement of erode / dilate (tests/morph_ref.py) pinned against sources that share nothing with it:
scipy.ndimage's grey morphology, the oracle's erode_cross3 (the front end's 3 x 3 cross), and masks written out by
hand from OpenCV 4.6.0's getStructuringElement."""
import numpy as np
import pytest

import morph_ref as mr


def _mask(rows):
    return np.array([[int(ch) for ch in r] for r in rows], np.uint8)


def test_restatement_equals_scipy_grey_morphology():
    """~300 random cases: shape, size 1..8, anchor, 1..3 iterations.  scipy's erosion origin is
    (ay - kh//2, ax - kw//2); its dilation mirrors the footprint, so dilation takes m[::-1, ::-1] and the origin
    ((kh-1-ay) - kh//2, (kw-1-ax) - kw//2).  scipy must be present: this test runs, it does not skip, where the
    project is developed (scipy 1.15.3 there)."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    done = 0
    for _ in range(300):
        rows, cols = (int(v) for v in rng.integers(1, 20, 2))
        kw, kh = (int(v) for v in rng.integers(1, 9, 2))
        shape = int(rng.integers(0, 3))
        ax, ay = int(rng.integers(0, kw)), int(rng.integers(0, kh))
        anchor = (-1, -1) if rng.random() < 0.3 else (ax, ay)
        ax, ay = mr.normalize_anchor(kw, kh, anchor)
        m = mr.get_structuring_element(shape, (kw, kh), anchor)
        assert m.any()
        a = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        it = int(rng.integers(1, 4))
        se = sd = a
        for _ in range(it):
            se = ndi.grey_erosion(se, footprint=m, origin=(ay - kh // 2, ax - kw // 2), mode="constant", cval=255)
            sd = ndi.grey_dilation(sd, footprint=m[::-1, ::-1], origin=((kh - 1 - ay) - kh // 2, (kw - 1 - ax) - kw // 2),
                                   mode="constant", cval=0)
        case = (rows, cols, kw, kh, shape, anchor, it)
        assert (mr.erode(a, shape, (kw, kh), anchor, it) == se).all(), case
        assert (mr.dilate(a, shape, (kw, kh), anchor, it) == sd).all(), case
        done += 1
    assert done == 300


@pytest.mark.parametrize("it", [1, 2, 3, 4])
def test_restatement_equals_oracle_erode_cross3(oracle, it):
    rng = np.random.default_rng(10 + it)
    for rows, cols in ((1, 1), (2, 3), (17, 31), (64, 70)):
        gray = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        exp = oracle.erode_cross3(gray, it)
        for shape in (mr.ELLIPSE, mr.CROSS):
            assert (mr.erode(gray, shape, (3, 3), (-1, -1), it) == exp).all(), (rows, cols, shape)


def test_literal_masks():
    e = lambda w, h: mr.get_structuring_element(mr.ELLIPSE, (w, h))
    assert (e(5, 5) == _mask(["00100", "11111", "11111", "11111", "00100"])).all()
    assert (e(7, 7) == _mask(["0001000", "0111110", "1111111", "1111111", "1111111", "0111110", "0001000"])).all()
    assert (e(3, 3) == _mask(["010", "111", "010"])).all()
    assert (e(3, 3) == mr.get_structuring_element(mr.CROSS, (3, 3))).all()
    assert (e(4, 6) == _mask(["0010", "0111", "1111", "1111", "1111", "0111"])).all()
    assert (mr.get_structuring_element(mr.CROSS, (5, 3), (4, 0)) == _mask(["11111", "00001", "00001"])).all()
    assert (mr.get_structuring_element(mr.RECT, (4, 2)) == 1).all()
    assert (mr.get_structuring_element(mr.CROSS, (1, 1)) == 1).all() and (e(1, 1) == 1).all()
    # ELLIPSE ignores the anchor
    assert (mr.get_structuring_element(mr.ELLIPSE, (5, 5), (0, 4)) == e(5, 5)).all()


def test_zero_iterations_and_unit_element_copy():
    a = np.random.default_rng(3).integers(0, 256, (5, 6, 3), dtype=np.uint8)
    assert (mr.erode(a, mr.RECT, (3, 3), (-1, -1), 0) == a).all()
    assert (mr.dilate(a, mr.ELLIPSE, (1, 1), (-1, -1), 4) == a).all()
