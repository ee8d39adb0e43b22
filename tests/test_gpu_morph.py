"""omr_morph / omr_morph_device / omr_morph_batch_device on the GPU, byte for byte against the numpy restatement of
erode / dilate (tests/morph_ref.py).

The library picks one of three kernels (csrc/oics_morph.cpp), and the cases sit on both sides of each choice:
  * rectangle or spans: a full rectangle (RECT, or a CROSS / ELLIPSE one cell high or wide) folds its iterations into
    one element and runs separably; anything else runs as row spans;
  * one rectangle launch or a chain: a launch reaches 30 cells in all per axis (a 31 x 31 element), so RECT 3 x 3
    takes one launch up to 15 iterations and two from 16, and RECT 31 / 32 / 33 straddle it directly; an element that
    reaches past the image is clamped to it;
  * LDS or global spans: elements up to 31 x 31 stay in LDS, 32 on either axis goes to the global loop;
  * fused or ping-pong passes: the LDS span kernel fuses passes while their accumulated halo stays within 32 rows
    and 32 dwords: 3 x 3 on 1 channel fuses 16 (17 takes two launches), 7 x 7 fuses 5 (6 takes two), 15 x 15 fuses
    2 (3 takes two)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import morph_ref as mr
from oics import _lib, transfer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_morph as fz  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 3), (5, 5), (7, 3), (4, 6), (1, 9), (9, 1), (15, 15), (31, 31), (64, 5)]
ITERS = [0, 1, 2, 3, 5]
# (rows, cols): 1 x 1 up to 70 x 90, widths that are not multiples of 4, images smaller than the elements
IMAGES = [(1, 1), (2, 3), (5, 7), (13, 33), (31, 30), (64, 64), (70, 90), (33, 257)]


def _anchors(kw, kh):
    return [(-1, -1), (0, 0), (kw - 1, kh - 1), (kw // 3, kh - 1 - kh // 3)]


def _img(rng, rows, cols, cn, op=0):
    a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    a[rng.random((rows, cols)) < 0.5] = 255 if op == mr.ERODE else 0
    return a


def _check(a, op, shape, size, anchor, it, **buf):
    rc, got, err = fz.device_morph(a, op, shape, size, anchor, it, **buf)
    case = (a.shape, op, shape, size, anchor, it, buf)
    assert err is None, (case, err)
    exp = mr.morph(a, op, shape, size, anchor, it)
    assert np.array_equal(got, exp), (case, int((got != exp).sum()))


@pytest.mark.parametrize("op", [mr.ERODE, mr.DILATE])
@pytest.mark.parametrize("shape", [mr.RECT, mr.CROSS, mr.ELLIPSE])
def test_per_image_cases(op, shape):
    """op x shape x every size, with anchors, iterations, channels, image sizes and pitches walked in step (a pruned
    product: each value of each axis meets each size at least once)"""
    rng = np.random.default_rng(100 + 10 * op + shape)
    n = 0
    for (kw, kh) in SIZES:
        for k in range(8):
            anchor = _anchors(kw, kh)[k % 4]
            it = ITERS[(k + kw) % 5]
            cn = 1 + (k + kh) % 4
            rows, cols = IMAGES[(k * 3 + kw + kh) % len(IMAGES)]
            pad_s, pad_d = (k * 5) % 4, (k * 7 + 1) % 4
            a = _img(rng, rows, cols, cn, op)
            _check(a, op, shape, (kw, kh), anchor, it, so=k % 4, sp=cols * cn + pad_s, do=(k + 1) % 4, dp=cols * cn + pad_d)
            n += 1
    assert n == 80


@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_every_iteration_count_and_anchor_on_small_elements(cn):
    rng = np.random.default_rng(7 + cn)
    a = _img(rng, 37, 45, cn)
    for shape, (kw, kh) in itertools.product((mr.RECT, mr.CROSS, mr.ELLIPSE), ((3, 3), (5, 5), (7, 3), (4, 6))):
        for i, anchor in enumerate(_anchors(kw, kh)):
            for it in ITERS:
                _check(a, (i + it) % 2, shape, (kw, kh), anchor, it)


def test_path_boundaries():
    """both sides of every choice listed in the module docstring"""
    rng = np.random.default_rng(11)
    a1, a3 = _img(rng, 70, 90, 1), _img(rng, 70, 90, 3)
    for op in (mr.ERODE, mr.DILATE):
        # fused | ping-pong passes of the LDS span kernel
        for size, its in (((3, 3), (16, 17)), ((7, 7), (5, 6)), ((15, 15), (2, 3))):
            for it in its:
                _check(a1, op, mr.ELLIPSE, size, (-1, -1), it)
                _check(a3, op, mr.CROSS, size, (size[0] - 1, 0), it)
        # LDS | global spans
        for size in ((31, 31), (32, 31), (31, 32), (33, 33), (32, 3), (3, 32)):
            _check(a1, op, mr.ELLIPSE, size, (-1, -1), 1)
            _check(a3, op, mr.CROSS, size, (size[0] // 3, size[1] - 1), 2)
        # rectangle | spans at one size, one rectangle launch | a chain
        for shape in (mr.RECT, mr.CROSS, mr.ELLIPSE):
            _check(a3, op, shape, (5, 4), (1, 2), 3)
        for it in (15, 16):
            _check(a1, op, mr.RECT, (3, 3), (-1, -1), it)
            _check(a3, op, mr.RECT, (3, 3), (0, 2), it)
        for k in (30, 31, 32, 33, 61, 62):
            _check(a1, op, mr.RECT, (k, k), (-1, -1), 1)
            _check(a3, op, mr.RECT, (k, 2), (k - 1, 0), 1)
        # elements and iteration counts that reach past the image on every side
        small = _img(rng, 2, 3, 3, op)
        for shape in (mr.RECT, mr.CROSS, mr.ELLIPSE):
            _check(small, op, shape, (7, 7), (-1, -1), 1)
            _check(small, op, shape, (7, 7), (6, 0), 3)
        _check(a1, op, mr.RECT, (200, 150), (10, 140), 2)
        _check(a1, op, mr.RECT, (3, 3), (-1, -1), 2000 if op == mr.ERODE else 500)
        _check(a1, op, mr.CROSS, (200, 150), (10, 140), 1)


def test_odd_base_address_and_padded_pitch_over_a_sentinel():
    """device_morph fills the destination with a sentinel and fails on any byte written past cols * channels"""
    rng = np.random.default_rng(12)
    for cn, (rows, cols) in itertools.product((1, 2, 3, 4), ((5, 7), (33, 61), (64, 64))):
        a = _img(rng, rows, cols, cn)
        for so, do, pad in ((1, 3, 1), (3, 1, 7), (2, 2, 2), (0, 1, 0), (1, 0, 5)):
            _check(a, mr.ERODE, mr.ELLIPSE, (5, 5), (-1, -1), 2, so=so, sp=cols * cn + pad, do=do, dp=cols * cn + pad + 1)
            _check(a, mr.DILATE, mr.RECT, (9, 4), (2, 3), 2, so=so, sp=cols * cn + pad, do=do, dp=cols * cn + pad + 1)
            _check(a, mr.DILATE, mr.CROSS, (33, 3), (-1, -1), 1, so=so, sp=cols * cn + pad, do=do, dp=cols * cn + pad + 1)


def _a4_gray():
    rng = np.random.default_rng(13)
    a = rng.integers(0, 256, (3508, 2480, 1), dtype=np.uint8)
    a[rng.random((3508, 2480)) < 0.6] = 255
    a[100:3400:57, 50:2400] = 0   # rules
    a[200:3300, 80:2300:91] = 0
    return a


def _sheet():
    import dataset_pin
    return dataset_pin.imread_color(sorted(os.listdir(dataset_pin.DATASET))[1])


@pytest.mark.parametrize("which", ["a4_gray", "colour_sheet", "colour_sheet_distinct_channels"])
def test_large_inputs_on_all_rows(which):
    if which == "a4_gray":
        a = _a4_gray()
        assert a.shape == (3508, 2480, 1)
    else:
        a = _sheet()
        assert a.ndim == 3 and a.shape[2] == 3 and a.shape[0] > 1000
        if which.endswith("distinct_channels"):
            a = a.copy()
            a[:, :, 1] = np.roll(a[:, :, 1], 5, axis=1)
            a[:, :, 2] = 255 - a[:, :, 2]
    for op in (mr.ERODE, mr.DILATE):
        _check(a, op, mr.ELLIPSE, (5, 5), (-1, -1), 2)
        _check(a, op, mr.RECT, (3, 3), (-1, -1), 10)


def test_ellipse3_three_passes_equal_erode3_device_and_the_oracle(oracle):
    rng = np.random.default_rng(14)
    for rows, cols in ((1, 1), (7, 9), (64, 70), (230, 248), (301, 437)):
        g = _img(rng, rows, cols, 1)
        rc, got, err = fz.device_morph(g, mr.ERODE, mr.ELLIPSE, (3, 3), (-1, -1), 3)
        assert err is None, err
        d_s = torch.from_numpy(g[:, :, 0].copy()).cuda()
        d_d = torch.zeros_like(d_s)
        assert _lib.lib().omr_erode3_device(C.c_void_p(d_s.data_ptr()), cols, rows, cols, C.c_void_p(d_d.data_ptr()), cols,
                                            None) == 0
        torch.cuda.synchronize()
        old = d_d.cpu().numpy()
        assert np.array_equal(got[:, :, 0], old), (rows, cols)
        assert np.array_equal(old, oracle.erode_cross3(g[:, :, 0].copy(), 3)), (rows, cols)


def test_duality():
    rng = np.random.default_rng(15)
    a = rng.integers(0, 256, (61, 77, 3), dtype=np.uint8)
    for shape, size, anchor, it in ((mr.ELLIPSE, (5, 5), (-1, -1), 2), (mr.CROSS, (7, 3), (0, 2), 3), (mr.RECT, (4, 6), (3, 0), 2),
                                    (mr.ELLIPSE, (33, 9), (-1, -1), 1), (mr.RECT, (40, 3), (5, 1), 1)):
        _, d, err = fz.device_morph(a, mr.DILATE, shape, size, anchor, it)
        assert err is None, err
        _, e, err = fz.device_morph(255 - a, mr.ERODE, shape, size, anchor, it)
        assert err is None, err
        assert np.array_equal(d, 255 - e), (shape, size, anchor, it)


def test_host_form_equals_device_form():
    rng = np.random.default_rng(16)
    for cn, (rows, cols) in itertools.product((1, 3, 4), ((3, 5), (70, 90))):
        a = _img(rng, rows, cols, cn)
        for op, shape, size, anchor, it in ((0, 2, (5, 5), (-1, -1), 2), (1, 0, (3, 3), (0, 0), 20), (1, 1, (40, 3), (-1, -1), 1),
                                            (0, 2, (7, 7), (-1, -1), 0), (0, 2, (7, 7), (-1, -1), 7)):
            wide = np.zeros((rows, cols * cn + 5), np.uint8)  # a padded host pitch
            wide[:, :cols * cn] = a.reshape(rows, -1)
            im = _lib.OmrImage(wide.ctypes.data, rows, cols, cn, wide.strides[0])
            out = _lib.OmrImageOwned()
            assert _lib.lib().omr_morph(C.byref(im), op, shape, size[0], size[1], anchor[0], anchor[1], it, C.byref(out)) == 0
            host = transfer._take_owned(out).reshape(rows, cols, cn)
            _, dev, err = fz.device_morph(a, op, shape, size, anchor, it)
            assert err is None, err
            assert np.array_equal(host, dev), (cn, rows, cols, op, shape, size, it)


@pytest.mark.parametrize("case", [(0, 2, (5, 5), (-1, -1), 2, 3), (1, 0, (9, 4), (2, 3), 12, 1), (1, 1, (35, 3), (-1, -1), 2, 2),
                                  (0, 2, (7, 7), (-1, -1), 6, 4), (0, 0, (3, 3), (-1, -1), 0, 3)])
def test_batch_of_37_equals_37_calls(case):
    op, shape, size, anchor, it, cn = case
    rng = np.random.default_rng(17)
    n, rows, cols = 37, 41, 53
    sp, dp = cols * cn + 3, cols * cn + 2
    sstride, dstride = rows * sp + 13, rows * dp + 7  # padded strides, odd image bases
    imgs = [_img(rng, rows, cols, cn, op) for _ in range(n)]
    sbuf = np.zeros(n * sstride, np.uint8)
    for i, a in enumerate(imgs):
        sbuf[i * sstride:i * sstride + rows * sp].reshape(rows, sp)[:, :cols * cn] = a.reshape(rows, -1)
    d_s = torch.from_numpy(sbuf).cuda()
    d_d = torch.full((n * dstride,), fz.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert _lib.lib().omr_morph_batch_device(C.c_void_p(d_s.data_ptr()), n, sstride, sp, rows, cols, cn, op, shape, size[0],
                                             size[1], anchor[0], anchor[1], it, C.c_void_p(d_d.data_ptr()), dstride, dp,
                                             None) == 0
    torch.cuda.synchronize()
    out = d_d.cpu().numpy()
    for i, a in enumerate(imgs):
        blk = out[i * dstride:(i + 1) * dstride]
        grid = blk[:rows * dp].reshape(rows, dp)
        assert (grid[:, cols * cn:] == fz.SENTINEL).all() and (blk[rows * dp:] == fz.SENTINEL).all(), i
        _, one, err = fz.device_morph(a, op, shape, size, anchor, it)
        assert err is None, err
        assert np.array_equal(grid[:, :cols * cn].reshape(rows, cols, cn), one), i
        if i % 9 == 0:
            assert np.array_equal(one, mr.morph(a, op, shape, size, anchor, it)), i


def test_transformable_matrix_methods_equal_the_restatement():
    rng = np.random.default_rng(18)
    for a in (rng.integers(0, 256, (50, 61), dtype=np.uint8), rng.integers(0, 256, (50, 61, 3), dtype=np.uint8)):
        t = transfer.TransformableMatrix(a)
        for shape, size, anchor, it in ((transfer.MORPH_ELLIPSE, (3, 3), (-1, -1), 3), (transfer.MORPH_CROSS, (5, 7), (4, 0), 2),
                                        (transfer.MORPH_RECT, (4, 4), (-1, -1), 9), (transfer.MORPH_ELLIPSE, (9, 9), (-1, -1), 0)):
            e, d = t.erode(shape, size, anchor, it), t.dilate(shape, size, anchor, it)
            assert isinstance(e, transfer.TransformableMatrix) and e is not t and np.array_equal(t.get_mat(), a)
            assert np.array_equal(e.get_mat(), mr.erode(a, shape, size, anchor, it))
            assert np.array_equal(d.get_mat(), mr.dilate(a, shape, size, anchor, it))


def test_fuzz_morph_slice(monkeypatch):
    """A fixed slice of tests/fuzz/fuzz_morph.py: random images, channels, elements, anchors, iterations, pitches."""
    import runpy
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz", "fuzz_morph.py")
    monkeypatch.setattr(sys, "argv", [tool, "300", "7"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(tool, run_name="__main__")
    assert e.value.code == 0
