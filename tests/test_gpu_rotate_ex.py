"""omr_rotate_ex / omr_rotate_device_ex on the device, byte for byte against the numpy restatement of warpAffine
(tests/warp_ref.py): every interpolation (NEAREST, LINEAR, CUBIC, AREA = LINEAR, LANCZOS4) x border mode (CONSTANT ..
TRANSPARENT) x channels 1..4 x clip, with and without WARP_INVERSE_MAP, on shapes at the w - 1 / w - 3 / w - 7 interior
thresholds and REFLECT_101's length-1 case, scales that take the LDS-staged path (1, 2.5) and the global fallback
(0.37), a medium sheet and a full A4 scan.  The device form runs on buffers at odd addresses with odd pitches and a
sentinel canvas: bytes past each canvas row stay untouched, BORDER_TRANSPARENT pixels keep the sentinel."""
import ctypes as C

import numpy as np
import pytest

import warp_ref as wr
from oics import _lib, transfer
from oics._lib import OmrImage, OmrImageOwned

pytestmark = pytest.mark.gpu

ANGLES = [0.0, 90.0, -90.0, 180.0, 0.05, 7.3, -41.0]
SCALES = [1.0, 0.37, 2.5]
SHAPES = [(1, 1), (1, 7), (2, 2), (3, 3), (4, 4), (7, 8)]
BORDER = (23, 201, 87, 140)
SENTINEL = 0xA5


def _content(rng, rows, cols, cn):
    a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    yy, xx = np.mgrid[:rows, :cols]
    board = ((yy // 2 + xx // 2) % 2 * 255).astype(np.uint8)
    half = xx < cols // 2  # left half: 0/255 checkerboard, so cubic and Lanczos overshoot and saturate
    a[half] = board[half][:, None]
    return a


def _size(rows, cols, angle, clip):
    dr, dc = C.c_int32(), C.c_int32()
    assert _lib.lib().omr_rotate_size(rows, cols, angle, clip, C.byref(dr), C.byref(dc)) == 0
    return dr.value, dc.value


def _device(a, angle, scale, flags, mode, clip):
    """omr_rotate_device_ex at odd base addresses and odd pitches over a sentinel canvas -> (canvas, pad bytes)"""
    import torch
    rows, cols, cn = a.shape
    dr, dc = _size(rows, cols, angle, clip)
    sp, dp = cols * cn + 3, dc * cn + 5
    sbuf = torch.zeros(1 + rows * sp + 8, dtype=torch.uint8)
    sv = sbuf[1:1 + rows * sp].view(rows, sp)
    sv[:, :cols * cn] = torch.from_numpy(a.reshape(rows, cols * cn))
    d_s = sbuf.cuda()
    d_d = torch.full((3 + dr * dp + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = (C.c_uint8 * 4)(*BORDER)
    rc = _lib.lib().omr_rotate_device_ex(C.c_void_p(d_s.data_ptr() + 1), sp, rows, cols, cn, angle, scale, flags, mode,
                                         C.cast(b, _lib.u8p), clip, C.c_void_p(d_d.data_ptr() + 3), dp, dr, dc, None)
    assert rc == 0, _lib.lib().omr_last_error()
    torch.cuda.synchronize()
    out = d_d.cpu().numpy()
    assert (out[:3] == SENTINEL).all() and (out[3 + dr * dp:] == SENTINEL).all()
    rows_ = out[3:3 + dr * dp].reshape(dr, dp)
    return rows_[:, :dc * cn].reshape(dr, dc, cn), rows_[:, dc * cn:]


def _host(a, angle, scale, flags, mode, clip):
    rows, cols, cn = a.shape
    a = np.ascontiguousarray(a)
    im = OmrImage(a.ctypes.data, rows, cols, cn, cols * cn)
    o = OmrImageOwned()
    b = (C.c_uint8 * 4)(*BORDER)
    rc = _lib.lib().omr_rotate_ex(C.byref(im), angle, scale, flags, mode, C.cast(b, _lib.u8p), clip, C.byref(o))
    assert rc == 0, _lib.lib().omr_last_error()
    try:
        n = o.rows * o.step_bytes
        return np.frombuffer((C.c_uint8 * n).from_address(o.data), np.uint8).reshape(o.rows, o.cols, cn).copy()
    finally:
        _lib.lib().omr_image_free(C.byref(o))


def _old(a, angle, scale, interp, clip):
    rows, cols, cn = a.shape
    a = np.ascontiguousarray(a)
    im = OmrImage(a.ctypes.data, rows, cols, cn, cols * cn)
    o = OmrImageOwned()
    b = (C.c_uint8 * 4)(*BORDER)
    assert _lib.lib().omr_rotate(C.byref(im), angle, scale, interp, C.cast(b, _lib.u8p), clip, C.byref(o)) == 0
    try:
        n = o.rows * o.step_bytes
        return np.frombuffer((C.c_uint8 * n).from_address(o.data), np.uint8).reshape(o.rows, o.cols, cn).copy()
    finally:
        _lib.lib().omr_image_free(C.byref(o))


def _check(a, angle, scale, flags, mode, clip, rows=None, host=False):
    got, pad = _device(a, angle, scale, flags, mode, clip)
    assert (pad == SENTINEL).all(), "bytes past the canvas row were written"
    init = np.full(got.shape, SENTINEL, np.uint8)
    exp = wr.rotate_ex(a, angle, scale, flags, mode, BORDER, clip, init=init, rows=rows)
    sel = slice(None) if rows is None else rows
    ok = (got[sel] == exp[sel])
    assert ok.all(), (a.shape, angle, scale, flags, mode, clip, np.argwhere(~ok)[:5].tolist())
    if host:
        h = _host(a, angle, scale, flags, mode, clip)
        dev0 = got
        if mode == wr.TRANSPARENT:  # the host form's skipped pixels are 0
            skipped = (wr.rotate_ex(a, angle, scale, flags, mode, BORDER, clip, init=np.zeros_like(init), rows=rows) !=
                       wr.rotate_ex(a, angle, scale, flags, mode, BORDER, clip, init=np.full_like(init, 255), rows=rows))
            dev0 = np.where(skipped, 0, got)
        assert (h[sel] == dev0[sel]).all(), (a.shape, angle, scale, flags, mode, clip)
    return got


def test_small_shapes_every_interp_border_channel_clip():
    rng = np.random.default_rng(11)
    i = 0
    for rows, cols in SHAPES:
        for cn in (1, 2, 3, 4):
            a = _content(rng, rows, cols, cn)
            for interp in (0, 1, 2, 3, 4):
                for mode in range(6):
                    for clip in (0, 1):
                        angle, scale = ANGLES[i % 7], SCALES[(i // 7) % 3]
                        inv = 16 if (i // 21) % 2 else 0
                        _check(a, angle, scale, interp | inv, mode, clip, host=(i % 17 == 0))
                        i += 1


@pytest.mark.parametrize("rows,cols", [(4, 4), (7, 8), (1, 7)])
def test_small_shapes_every_angle_scale_and_matrix_mode(rows, cols):
    rng = np.random.default_rng(rows * 100 + cols)
    a = _content(rng, rows, cols, 3)
    for interp in (1, 2, 4):
        for mode in (1, 2, 4, 5):
            for angle in ANGLES:
                for scale in SCALES:
                    for inv in (0, 16):
                        _check(a, angle, scale, interp | inv | 8, mode, 1)


def test_medium_sheet_sample():
    rng = np.random.default_rng(5)
    rows_sel = np.arange(0, 600, 7)
    i = 0
    for interp in (0, 1, 2, 4):
        for mode in range(6):
            cn = 1 + i % 4
            a = _content(rng, 301, 437, cn)
            angle, scale = (7.3, -41.0, 0.05)[i % 3], SCALES[i % 3]
            clip = i % 2
            dr, _ = _size(301, 437, angle, clip)
            _check(a, angle, scale, interp | (16 if i % 5 == 4 else 0), mode, clip, rows=rows_sel[rows_sel < dr],
                   host=(i % 4 == 1))
            i += 1


@pytest.mark.parametrize("interp", [2, 4])
def test_a4_scan_replicate(interp):
    rng = np.random.default_rng(interp)
    a = _content(rng, 3508, 2480, 3)
    dr, _ = _size(3508, 2480, 3.3, 1)
    _check(a, 3.3, 1.0, interp, wr.REPLICATE, 1, rows=np.linspace(0, dr - 1, 160).astype(int))


def test_old_pairs_are_omr_rotate_bit_for_bit():
    rng = np.random.default_rng(9)
    for rows, cols, cn in ((301, 437, 3), (64, 90, 1), (33, 17, 4), (5, 9, 2)):
        a = _content(rng, rows, cols, cn)
        for flags in (0, 1, 3, 1 | 8):
            for angle, clip in ((7.3, 1), (-2.2, 0)):
                exp = _old(a, angle, 1.0, 1 if flags & 7 == 3 else flags & 7, clip)
                assert (_host(a, angle, 1.0, flags, 0, clip) == exp).all(), (rows, cols, cn, flags)
                got, _ = _device(a, angle, 1.0, flags, 0, clip)
                assert (got == exp).all(), (rows, cols, cn, flags)


def test_constant_border_pairs_at_sheet_size():
    """NEAREST / LINEAR with BORDER_CONSTANT on the 301 x 437 content, both clips, at scales that stage a tile's source
    box in LDS (1.0, 2.5) and one whose boxes do not fit (0.37: taps from global memory).  2 and 4 channels: the device
    form at odd addresses and pitches against warp_ref, and omr_rotate against the same warp_ref image.  1 and 3
    channels with WARP_INVERSE_MAP: the kernel choice does not look at the flag."""
    rng = np.random.default_rng(21)
    for cn in (2, 4):
        a = _content(rng, 301, 437, cn)
        for interp in (0, 1):
            for clip in (0, 1):
                for scale in SCALES:
                    exp = _check(a, 7.3, scale, interp, wr.CONSTANT, clip)  # == warp_ref's image, every byte (no skips)
                    assert (_old(a, 7.3, scale, interp, clip) == exp).all(), (cn, interp, clip, scale)
    for cn in (1, 3):
        a = _content(rng, 301, 437, cn)
        for interp in (0, 1):
            for clip in (0, 1):
                for scale in SCALES:
                    _check(a, -41.0, scale, interp | 16, wr.CONSTANT, clip)


def test_python_rotate_mat_every_flag_and_border():
    rng = np.random.default_rng(4)
    a = _content(rng, 40, 57, 3)
    for interp in (0, 1, 2, 3, 4):
        for mode in range(6):
            got = transfer.rotate_mat(a, 11.0, 1.0, interp, mode, tuple(float(v) for v in BORDER),
                                      transfer.RotateClipStrategy.CONTAIN).matrix
            exp = wr.rotate_ex(a, 11.0, 1.0, interp, mode, BORDER, 1)
            assert (np.asarray(got) == exp).all(), (interp, mode)


def test_fuzz_rotate_ex_slice(monkeypatch):
    """A fixed slice of tests/fuzz/fuzz_rotate_ex.py: random shapes, channels, flags, border modes, angles, scales."""
    import os
    import runpy
    import sys
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz", "fuzz_rotate_ex.py")
    monkeypatch.setattr(sys, "argv", [tool, "300", "7"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(tool, run_name="__main__")
    assert e.value.code == 0
