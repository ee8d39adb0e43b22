"""tests/projpic_ref.py against itself: the statement-by-statement restatement of transfer.rs:337-376 / :409-455 equals
the closed forms the kernels implement, on random images of the three value classes and on hand-written cases."""
import numpy as np
import pytest

import projpic_ref as pr


@pytest.mark.parametrize("cls", sorted(pr.VALUE_CLASSES))
def test_literal_equals_closed_form(cls):
    rng = np.random.default_rng({"binary": 1, "six": 2, "any": 3}[cls])
    for _ in range(150):
        rows, cols = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        a = pr.random_image(rng, rows, cols, cls)
        keep = a.copy()
        assert np.array_equal(pr.horizontal_literal(a), pr.horizontal(a)), a.tolist()
        assert np.array_equal(pr.vertical_literal(a), pr.vertical(a)), a.tolist()
        assert np.array_equal(a, keep)  # the reference is left unchanged


def _h(row):
    a = np.array([row], np.uint8)
    lit, closed = pr.horizontal_literal(a), pr.horizontal(a)
    assert np.array_equal(lit, closed)
    return closed[0].tolist()


def test_horizontal_hand_cases():
    assert _h([100, 255, 7, 255, 0]) == [100, 0, 0, 255, 255]
    assert _h([3, 0, 254, 128]) == [3, 0, 254, 128]                # a row with no 255: untouched
    assert _h([255, 0, 9, 255, 254]) == [0, 0, 0, 255, 255]        # a row that starts with 255: nothing kept
    assert _h([255, 255, 255]) == [255, 255, 255]
    assert _h([0, 0, 255]) == [0, 0, 255]                          # k0 == K: no fill
    assert _h([254]) == [254] and _h([255]) == [255]


def test_vertical_hand_cases():
    a = np.array([[127], [128], [255], [0]], np.uint8)             # 127 counts, 128 does not
    assert pr.vertical(a)[:, 0].tolist() == [255, 255, 0, 0] == pr.vertical_literal(a)[:, 0].tolist()
    a = np.array([[128, 127, 0], [200, 129, 1]], np.uint8)
    exp = [[255, 255, 0], [255, 0, 0]]
    assert pr.vertical(a).tolist() == exp == pr.vertical_literal(a).tolist()
    white = np.full((3, 4), 255, np.uint8)
    assert (pr.vertical(white) == 255).all() and (pr.vertical(np.zeros((3, 4), np.uint8)) == 0).all()


def test_the_three_predicates_agree_only_on_binary_images():
    """on 0 / 255 the run and the bar are the == 0 counts of get_horizontal_projection / get_vertical_projection"""
    rng = np.random.default_rng(4)
    a = pr.random_image(rng, 9, 11, "binary")
    h, v = pr.horizontal(a), pr.vertical(a)
    assert ((h == 0).sum(axis=1) == (a == 0).sum(axis=1)).all() and ((v == 0).sum(axis=0) == (a == 0).sum(axis=0)).all()
    g = np.array([[100, 255, 200]], np.uint8)  # gray ink: != 255 counts it, == 0 and <= 127 do not
    assert pr.horizontal(g).tolist() == [[100, 0, 255]] and pr.vertical(g).tolist() == [[0, 255, 255]]
