"""omr_projection_pictures / _device / _batch_device on the GPU, byte for byte against the restatement of the
reference's loops (tests/projpic_ref.py).

The shapes sit on both sides of what the kernels (csrc/projpic.hip) do differently:
  * a wavefront takes a row 256 bytes a step, four loads in flight once a row has more than 1024 bytes: widths 1 .. 64,
    259, 1030, 1300 and the longest row there is (32 766);
  * column counts are taken on tiles of 256 columns x 256 rows and added across workgroups: 1100 x 1300 has 5 x 6 tiles;
  * dword accesses need base and pitch to be multiples of 4; a row's last partial dword and every other layout go
    byte by byte: pitches 260 / 1032 / 80 over widths 259 / 1030 / 77, tightly packed odd widths, bases offset by 1..3.
Every destination is a canvas of 0xA5 with a guard band; any byte written outside the pictures' pixels fails the case
(tests/fuzz/fuzz_projection_pictures.py: device_pictures)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import projpic_ref as pr
from oics import _lib, synth, transfer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_projection_pictures as fz  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 7), (7, 1), (3, 5), (33, 61), (64, 64)]
PITCHED = [((70, 259), 260), ((129, 1030), 1032), ((200, 77), 80)]
PACKED_ODD = [(5, 3), (31, 33), (67, 129), (40, 257), (9, 1023)]
BIG = (1100, 1300)


def _values(rng, rows, cols, kind):
    if kind in pr.VALUE_CLASSES:
        return pr.random_image(rng, rows, cols, kind)
    if kind == "white":
        return np.full((rows, cols), 255, np.uint8)
    if kind == "black":
        return np.zeros((rows, cols), np.uint8)
    assert kind == "sheet"
    return np.ascontiguousarray(synth.make_binary_card(rows, cols, 5, skew=1.3)[0])


KINDS = ["binary", "six", "any", "white", "black"]


def _check(a, **layout):
    """both pictures of `a` through the device form, against the restatement"""
    h, v, err = fz.device_pictures([a], **layout)
    assert err is None, (a.shape, layout, err)
    eh, ev = pr.horizontal(a), pr.vertical(a)
    assert np.array_equal(h[0], eh), (a.shape, layout, int((h[0] != eh).sum()))
    assert np.array_equal(v[0], ev), (a.shape, layout, int((v[0] != ev).sum()))
    return h[0], v[0]


@pytest.mark.parametrize("kind", KINDS)
def test_small_shapes_every_base_offset(kind):
    rng = np.random.default_rng(20 + KINDS.index(kind))
    for k, (rows, cols) in enumerate(SMALL):
        a = _values(rng, rows, cols, kind)
        _check(a)
        for so, ho, vo in ((1, 2, 3), (3, 1, 2), (2, 3, 1), (0, 1, 0), (1, 0, 0)):
            _check(a, so=so, ho=ho, vo=vo, sp=cols + (k + so) % 4, hp=cols + (k + ho) % 5, vp=cols + (k + vo) % 3)


@pytest.mark.parametrize("kind", KINDS)
def test_awkward_pitches_and_packed_odd_widths(kind):
    rng = np.random.default_rng(30 + KINDS.index(kind))
    for (rows, cols), pitch in PITCHED:
        a = _values(rng, rows, cols, kind)
        _check(a, sp=pitch, hp=pitch, vp=pitch)                       # dword path, byte tail
        _check(a, sp=pitch, hp=pitch, vp=pitch, so=1, ho=3, vo=2)     # the same pitches from odd bases
        _check(a, sp=pitch + 1, hp=pitch + 3, vp=pitch + 2)           # pitches that are no multiple of 4
    for rows, cols in PACKED_ODD:
        a = _values(rng, rows, cols, kind)
        _check(a)
        _check(a, so=3, ho=2, vo=1)


def test_synthetic_sheet():
    a = _values(None, 301, 437, "sheet")
    assert set(np.unique(a)) <= {0, 255} and (a == 0).any() and (a == 255).any()
    _check(a)
    _check(a, so=1, sp=440, ho=2, hp=439, vo=3, vp=441)


@pytest.mark.parametrize("kind", ["binary", "six", "any"])
def test_more_than_one_tile_in_both_directions(kind):
    rows, cols = BIG
    assert rows > 4 * 256 and cols > 4 * 256  # several column-count tiles each way, rows of several wave steps
    rng = np.random.default_rng(40)
    a = _values(rng, rows, cols, kind)
    a[:, 700] = 0      # a full-height bar
    a[:, 701] = 128    # and a column the vertical predicate does not count at all
    a[500, :] = 254    # a row with no 255: kept as it is
    _check(a)
    _check(a, so=2, sp=cols + 3, ho=1, hp=cols + 1, vo=3, vp=cols + 2)


def test_longest_row():
    rng = np.random.default_rng(41)
    a = pr.random_image(rng, 3, 32766, "six")
    a[1, :32765] = 254                      # k0 at the very last pixel
    a[1, 32765] = 255
    a[2, :] = 7                             # no 255 at all
    _check(a)
    _check(a, so=1, ho=3, vo=2, sp=32766 + 1, hp=32766 + 2, vp=32766 + 3)
    tall = pr.random_image(rng, 32766, 2, "six")
    _check(tall)


def test_each_picture_alone_equals_both_together():
    rng = np.random.default_rng(42)
    for rows, cols in ((33, 61), (70, 259), (300, 520)):
        a = pr.random_image(rng, rows, cols, "any")
        layout = dict(so=1, sp=cols + 3, ho=2, hp=cols + 1, vo=3, vp=cols + 2)
        h, v = _check(a, **layout)
        h1, none, err = fz.device_pictures([a], want_v=False, **layout)
        assert err is None and none is None and np.array_equal(h1[0], h)
        none, v1, err = fz.device_pictures([a], want_h=False, **layout)
        assert err is None and none is None and np.array_equal(v1[0], v)


def _host(a, want_h=True, want_v=True, pad=5):
    wide = np.zeros((a.shape[0], a.shape[1] + pad), np.uint8)  # a padded host pitch
    wide[:, :a.shape[1]] = a
    im = _lib.OmrImage(wide.ctypes.data, a.shape[0], a.shape[1], 1, wide.strides[0])
    oh, ov = _lib.OmrImageOwned(), _lib.OmrImageOwned()
    assert _lib.lib().omr_projection_pictures(C.byref(im), C.byref(oh) if want_h else None,
                                              C.byref(ov) if want_v else None) == 0
    return (transfer._take_owned(oh) if want_h else None), (transfer._take_owned(ov) if want_v else None)


@pytest.mark.parametrize("n", [1, 3, 65])
def test_batch_equals_per_call_device_form_equals_host_form(n):
    rng = np.random.default_rng(50 + n)
    rows, cols = (70, 259) if n < 65 else (37, 131)
    imgs = [pr.random_image(rng, rows, cols, ("binary", "six", "any")[i % 3]) for i in range(n)]
    # strides larger than an image, odd bases and pitches
    bh, bv, err = fz.device_pictures(imgs, so=1, sp=cols + 1, sgap=13, ho=3, hp=cols + 2, hgap=7, vo=2, vp=cols + 5, vgap=11,
                                     batch=True)
    assert err is None, err
    for i, a in enumerate(imgs):
        h, v, err = fz.device_pictures([a], batch=False)
        assert err is None, err
        assert np.array_equal(bh[i], h[0]) and np.array_equal(bv[i], v[0]), i
        hh, hv = _host(a)
        assert np.array_equal(h[0], hh) and np.array_equal(v[0], hv), i
        assert np.array_equal(bh[i], pr.horizontal(a)) and np.array_equal(bv[i], pr.vertical(a)), i
    # each picture of the batch alone
    h1, none, err = fz.device_pictures(imgs, sp=cols + 3, hgap=5, want_v=False, batch=True)
    assert err is None and none is None and all(np.array_equal(h1[i], bh[i]) for i in range(n))
    none, v1, err = fz.device_pictures(imgs, sp=cols + 3, vgap=5, want_h=False, batch=True)
    assert err is None and none is None and all(np.array_equal(v1[i], bv[i]) for i in range(n))


def test_python_functions_equal_the_restatement():
    rng = np.random.default_rng(60)
    a = pr.random_image(rng, 50, 61, "any")
    t = transfer.TransformableMatrix(a)
    h = transfer.transfer_thresh_binary_to_horizontal_projection(t)
    v = transfer.transfer_thresh_binary_to_vertical_projection(t)
    both = transfer.projection_pictures(a)
    assert isinstance(h, transfer.TransformableMatrix) and np.array_equal(t.get_mat(), a)
    assert np.array_equal(h.get_mat(), pr.horizontal(a)) and np.array_equal(v.get_mat(), pr.vertical(a))
    assert np.array_equal(both[0].get_mat(), h.get_mat()) and np.array_equal(both[1].get_mat(), v.get_mat())
    hh, hv = _host(a, want_v=False)
    assert hv is None and np.array_equal(hh, h.get_mat())
    hh, hv = _host(a, want_h=False)
    assert hh is None and np.array_equal(hv, v.get_mat())


def test_binary_images_agree_with_the_projections():
    """strictly 0 / 255: the black run of row r is get_horizontal_projection[r] long, the bar of column c
    get_vertical_projection[c] high"""
    rng = np.random.default_rng(61)
    for a in (pr.random_image(rng, 90, 131, "binary"), _values(None, 230, 248, "sheet")):
        h, v = _host(a)
        hp, vp = transfer.get_horizontal_projection(a), transfer.get_vertical_projection(a)
        rows, cols = a.shape
        for r in range(rows):
            k = int(hp[r])
            assert (h[r, :k] == 0).all() and (h[r, k:] == 255).all(), r
        for c in range(cols):
            k = int(vp[c])
            assert (v[:rows - k, c] == 255).all() and (v[rows - k:, c] == 0).all(), c


def test_fuzz_slice(monkeypatch):
    """A fixed slice of tests/fuzz/fuzz_projection_pictures.py: random shapes, values, pitches, offsets, batch sizes."""
    import runpy
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz", "fuzz_projection_pictures.py")
    monkeypatch.setattr(sys, "argv", [tool, "150", "7"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(tool, run_name="__main__")
    assert e.value.code == 0
