"""omr_rotate_ex / omr_rotate_device_ex / omr_warp_coeff_table without a GPU: the numpy restatement of warpAffine
(tests/warp_ref.py) against the oracle, the library's weight tables against the restatement's, and every argument
error -- each returned before any device work (a device call on a machine without a GPU would be -217)."""
import ctypes as C

import numpy as np
import pytest

import warp_ref as wr
from oics import _lib, transfer
from oics._lib import OmrImage, OmrImageOwned


def _img(rng, rows, cols, cn):
    a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    a[::3, ::2] = 255
    return a if cn > 1 else a[:, :, 0]


@pytest.mark.parametrize("interp", [0, 1])
def test_restatement_equals_oracle_for_nearest_and_linear(oracle, interp):
    rng = np.random.default_rng(7 + interp)
    cases = [(1, 1, 1, 13.0, 0), (2, 3, 3, -41.0, 1), (7, 8, 4, 90.0, 1), (31, 45, 1, 7.3, 0), (40, 33, 3, -0.05, 1),
             (64, 70, 2, 180.0, 0), (25, 90, 1, 3.3, 1), (9, 4, 3, -90.0, 0)]
    border = (17, 200, 91, 5)
    for rows, cols, cn, angle, clip in cases:
        for scale in (1.0, 0.37, 2.5):
            a = _img(rng, rows, cols, cn)
            exp = oracle.rotate_mat(a, angle, scale, interp, border, clip)
            got = wr.rotate_ex(a, angle, scale, interp, wr.CONSTANT, border, clip)
            assert got.shape == exp.shape and (got == exp).all(), (rows, cols, cn, angle, clip, scale)


@pytest.mark.parametrize("interp,k", [(2, 4), (4, 8)])
def test_weight_tables_equal_the_restatement(interp, k):
    n = C.c_int32()
    assert _lib.lib().omr_warp_coeff_table(interp, None, 0, C.byref(n)) == 0 and n.value == 1024 * k * k
    t = np.zeros(n.value, np.int16)
    p = t.ctypes.data_as(C.POINTER(C.c_int16))
    assert _lib.lib().omr_warp_coeff_table(interp, p, n.value - 1, C.byref(n)) == -5
    assert _lib.lib().omr_warp_coeff_table(interp, p, n.value, C.byref(n)) == 0
    t = t.reshape(1024, k * k).astype(np.int64)
    assert (t == wr.coeff_table(interp)).all()
    assert (t.sum(axis=1) == 32768).all()
    # fraction 0: the centre tap alone.  saturate_cast<short>(1.0f * 32768) is 32767 and initInterTab2D's sum fix
    # searches the 2 x 2 from tap (k/2, k/2), one past the centre, so the missing 1 lands there -- the output is still
    # the centre texel: (32767 S + S' + 2^14) >> 15 == S for all bytes S, S'
    ident = np.zeros(k * k, np.int64)
    ident[(k // 2 - 1) * (k + 1)] = 32767
    ident[(k // 2) * (k + 1)] = 1
    assert (t[0] == ident).all()
    S = np.arange(256)[:, None]
    assert (((32767 * S + S.T + (1 << 14)) >> 15) == S).all()
    assert (t < 0).any() and (t.max() > 32768 // 2)  # negative lobes: cubic and Lanczos overshoot
    for bad in (0, 1, 3, 5, -1):
        assert _lib.lib().omr_warp_coeff_table(bad, None, 0, C.byref(n)) == -5


def test_border_interpolate_loop_and_modular_forms_agree():
    # the kernel folds REFLECT / REFLECT_101 in closed form and WRAP as a floor modulus; the restatement runs the loop
    for n in (1, 2, 3, 7, 10):
        p = np.arange(-60, 61)
        for mode, per, fold in ((wr.REFLECT, 2 * n, lambda m: 2 * n - 1 - m), (wr.REFLECT_101, 2 * n - 2, lambda m: 2 * n - 2 - m)):
            got = wr.border_interpolate(p, n, mode)
            if n == 1:
                assert (got == 0).all()
                continue
            m = p % per
            assert (got == np.where(m < n, m, fold(m))).all(), (n, mode)
        assert (wr.border_interpolate(p, n, wr.WRAP) == p % n).all()
        assert (wr.border_interpolate(p, n, wr.REPLICATE) == np.clip(p, 0, n - 1)).all()
        assert (wr.border_interpolate(p, n, wr.CONSTANT) == np.where((p >= 0) & (p < n), p, -1)).all()


def test_rotate_mat_constants():
    assert (transfer.INTER_NEAREST, transfer.INTER_LINEAR, transfer.INTER_CUBIC, transfer.INTER_AREA,
            transfer.INTER_LANCZOS4) == (0, 1, 2, 3, 4)
    assert (transfer.WARP_FILL_OUTLIERS, transfer.WARP_INVERSE_MAP) == (8, 16)
    assert (transfer.BORDER_CONSTANT, transfer.BORDER_REPLICATE, transfer.BORDER_REFLECT, transfer.BORDER_WRAP,
            transfer.BORDER_REFLECT_101, transfer.BORDER_TRANSPARENT) == (0, 1, 2, 3, 4, 5)


def _dev_call(flags=1, border_mode=0, rows=20, cols=30, cn=3, clip=0, src=1 << 20, dst=1 << 21, src_step=None,
              dst_step=None, dst_rows=None, dst_cols=None, border=True):
    lib = _lib.lib()
    dr, dc = C.c_int32(), C.c_int32()
    assert lib.omr_rotate_size(max(rows, 1), cols, 10.0, clip if clip in (0, 1) else 0, C.byref(dr), C.byref(dc)) == 0
    b = (C.c_uint8 * 4)(1, 2, 3, 4)
    return lib.omr_rotate_device_ex(
        C.c_void_p(src) if src else None, cols * cn if src_step is None else src_step, rows, cols, cn, 10.0, 1.0, flags,
        border_mode, C.cast(b, _lib.u8p) if border else None, clip, C.c_void_p(dst) if dst else None,
        dc.value * cn if dst_step is None else dst_step, dr.value if dst_rows is None else dst_rows,
        dc.value if dst_cols is None else dst_cols, None)


def _host_call(flags=1, border_mode=0, img=True, out=True, border=True):
    a = np.zeros((12, 9, 3), np.uint8)
    im = OmrImage(a.ctypes.data, 12, 9, 3, 27)
    o = OmrImageOwned()
    b = (C.c_uint8 * 4)(1, 2, 3, 4)
    return _lib.lib().omr_rotate_ex(C.byref(im) if img else None, 5.0, 1.0, flags, border_mode,
                                    C.cast(b, _lib.u8p) if border else None, 1, C.byref(o) if out else None)


def test_argument_errors_before_any_device_work():
    # the device form is given addresses that were never allocated: every call must fail in its checks
    for call in (_dev_call, _host_call):
        for f in (5, 6, 7, 5 | 16, 7 | 8):
            assert call(flags=f) == -213, f
        for f in (32, 64, 1 | 128, -1, 1 << 20, 2 | 32):
            assert call(flags=f) == -5, f
        for bm in (-1, 6, 16, 16 | 1):
            assert call(border_mode=bm) == -5, bm
        assert call(border=False) == -5
    assert _dev_call(src=0) == -5 and _dev_call(dst=0) == -5
    assert _dev_call(src_step=3 * 30 - 1) == -5
    assert _dev_call(cn=4, src_step=3 * 30) == -5
    assert _dev_call(dst_step=3 * 30 - 1, flags=2) == -5
    assert _dev_call(dst_rows=19) == -215 and _dev_call(dst_cols=31, clip=1) == -215
    assert _dev_call(cn=0) == -215 and _dev_call(cn=5) == -215 and _dev_call(rows=0) == -215
    assert _dev_call(clip=2) == -5
    assert _host_call(img=False) == -5 and _host_call(out=False) == -5


def test_python_rotate_mat_refuses_only_unimplemented_flags():
    a = np.zeros((6, 5), np.uint8)
    for f in (5, 6, 7):
        with pytest.raises(_lib.OmrError) as e:
            transfer.rotate_mat(a, 3.0, 1.0, f, transfer.BORDER_REPLICATE)
        assert e.value.code == -213
    with pytest.raises(_lib.OmrError) as e:
        transfer.rotate_mat(a, 3.0, 1.0, 1, 7)
    assert e.value.code == -5


@pytest.mark.parametrize("interp", [0, 1, 2, 4])
def test_restatement_against_opencv_when_present(interp):
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(3)
    a = _img(rng, 23, 31, 3)
    for mode in range(6):
        for inv in (0, 16):
            M, dr, dc = wr.rotate_geometry(23, 31, 7.3, 1.2, 1)
            init = np.zeros((dr, dc, 3), np.uint8)
            got = wr.rotate_ex(a, 7.3, 1.2, interp | inv, mode, (9, 200, 40, 0), 1, init=init)
            exp = init.copy()
            cv2.warpAffine(a, M.reshape(2, 3), (dc, dr), exp, interp | inv, mode, (9, 200, 40, 0))
            assert (got == exp).all(), (interp, mode, inv)
