"""The warp, resize and gray kernels against float64 first-principles math (tests/geom_exact.py), with the bounds
derived there and the inputs of tests/geom_cases.py; tests/test_geom_exact.py holds the restatements to the same bounds
on the same inputs.  The byte-for-byte tests compare kernel and restatement, which were written from one reading of
the published algorithm; here a shared misreading (a half-pixel centre, a wrong cubic A, a Lanczos window off by a
tap, a border index off by one, a transposed matrix term, swapped gray weights) or a drifting fixed-point table shows.

  exact-coordinate warps   quarter turns at scales whose destination-to-source map is a multiple of 1 / 32: NEAREST
                           equal, LINEAR equal to floor(exact + 0.5), CUBIC / LANCZOS4 within 0.5 + wq(K)
  general warps            smooth content: within 0.5 + wq(K) + S A (Lx + Ly) delta; NEAREST with the tie rule
through omr_rotate_device_ex (test_gpu_rotate_ex's device helper: odd base address, odd pitch, sentinel canvas),
omr_rotate_batch_device_ex, omr_rotate_device and the projection batch's deskew; then the area resize, the enlarging
resize and the gray conversion.  Every pixel is counted.

Worst |kernel - exact| / bound measured on an MI355X: exact-coordinate LINEAR 1.000, CUBIC 0.87, LANCZOS4 0.70;
general LINEAR 0.83, CUBIC 0.56, LANCZOS4 0.36; area 1.000, enlarging 0.62, gray 0.96 -- the restatements' own
figures (tests/test_geom_exact.py), as the byte-for-byte tests lead one to expect."""
import ctypes as C

import numpy as np
import pytest

import geom_cases as gc
import geom_exact as gx
import test_geom_exact as cpu
import test_gpu_rotate_ex as rx
from oics import _lib, projection, transfer

pytestmark = pytest.mark.gpu

assert rx.BORDER == gc.BORDER


def _canvas(a, flags, mode, clip, angle, scale):
    got, pad = rx._device(a, angle, scale, flags, mode, clip)
    assert (pad == rx.SENTINEL).all(), "bytes past the canvas row were written"
    return got


# ---- omr_rotate_device_ex -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", gc.EVEN_SHAPES + gc.ODD_SHAPES)
def test_warp_at_exact_coordinates(rows, cols):
    rng = np.random.default_rng(rows * 7 + cols)
    for case in gc.exact_cases(rows, cols):
        cn, flags, mode, clip, angle, scale = case
        a = gc.board(rng, rows, cols, cn)
        cpu.check_exact_case(a, _canvas(a, flags, mode, clip, angle, scale), cpu._kept(a, flags, mode, clip, angle, scale), case)


@pytest.mark.parametrize("rows,cols", gc.GENERAL_SHAPES)
def test_warp_at_general_angles(rows, cols):
    a = gc.smooth(rows, cols)
    for case in gc.general_cases(rows, cols):
        flags, mode, clip, angle, scale = case
        cpu.check_general_case(a, _canvas(a, flags, mode, clip, angle, scale), case)


@pytest.mark.parametrize("rows,cols", gc.GENERAL_SHAPES)
def test_nearest_at_general_angles(rows, cols):
    a = gc.smooth(rows, cols)
    for case in gc.nearest_cases(rows, cols):
        mode, clip, angle, scale = case
        cpu.check_nearest_case(a, _canvas(a, 0, mode, clip, angle, scale), case)


# ---- omr_rotate_batch_device_ex: four angles in one call, one source ------------------------------------------------
def _batch(a, angles, scale, flags, mode, clip):
    import torch
    rows, cols, cn = a.shape
    mr, mc, sizes = transfer.rotate_batch_canvas(rows, cols, angles, clip)
    d_src = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    dstep = mc * cn + 3
    d_dst = torch.full((len(angles), mr, dstep), rx.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = transfer.rotate_batch_device_ex(d_src.data_ptr(), len(angles), 0, cols * cn, rows, cols, cn, angles, scale, flags, mode,
                                          gc.BORDER, clip, d_dst.data_ptr(), mr * dstep, dstep, mr, mc)
    torch.cuda.synchronize()
    assert (got == sizes).all()
    out = d_dst.cpu().numpy()
    return [out[i, :dr, :dc * cn].reshape(dr, dc, cn) for i, (dr, dc) in enumerate(sizes)]


def test_batch_warp_both_tiers():
    rng = np.random.default_rng(31)
    for (rows, cols), cn, flags, mode, clip, scale in (((38, 54), 3, 1, 0, 0, 2.0), ((38, 54), 1, 2 | 16, 2, 1, 17 / 16),
                                                      ((64, 96), 4, 4 | 16, 3, 1, 5 / 2), ((37, 53), 3, 0, 4, 1, 1 / 2),
                                                      ((8, 8), 2, 2, 1, 0, 32 / 33), ((64, 96), 3, 1 | 16, 0, 0, 4.0)):
        a = gc.board(rng, rows, cols, cn)
        for angle, got in zip(gc.QUARTER_TURNS, _batch(a, gc.QUARTER_TURNS, scale, flags, mode, clip)):
            cpu.check_exact_case(a, got, None, (cn, flags, mode, clip, angle, scale))
    for (rows, cols), flags, mode, clip, scale in (((37, 53), 1, 0, 1, 1.0), ((64, 96), 2, 3, 0, 2.5), ((64, 96), 4, 1, 1, 0.37),
                                                  ((8, 7), 2, 4, 1, 1.0)):
        a = gc.smooth(rows, cols)
        for angle, got in zip(gc.GENERAL_ANGLES, _batch(a, gc.GENERAL_ANGLES, scale, flags, mode, clip)):
            cpu.check_general_case(a, got, (flags, mode, clip, angle, scale))
    a = gc.smooth(64, 96)
    by_geometry = {c[1:]: c[0] for c in gc.nearest_cases(64, 96)}
    angles = [ang for ang in gc.GENERAL_ANGLES if (1, ang, 1.0) in by_geometry]
    assert len(angles) >= 3
    for angle, got in zip(angles, _batch(a, angles, 1.0, 0, 1, 1)):
        cpu.check_nearest_case(a, got, (1, 1, angle, 1.0))


# ---- omr_rotate_device: the NEAREST / LINEAR + BORDER_CONSTANT path -------------------------------------------------
def _rotate_device(a, angle, scale, interp, clip):
    import torch
    rows, cols, cn = a.shape
    dr, dc = rx._size(rows, cols, angle, clip)
    sp, dp = cols * cn + 3, dc * cn + 5
    sbuf = np.zeros((rows, sp), np.uint8)
    sbuf[:, :cols * cn] = a.reshape(rows, cols * cn)
    d_s = torch.from_numpy(sbuf).cuda()
    d_d = torch.full((dr, dp), rx.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = (C.c_uint8 * 4)(*gc.BORDER)
    rc = _lib.lib().omr_rotate_device(C.c_void_p(d_s.data_ptr()), sp, rows, cols, cn, float(angle), float(scale), interp,
                                      C.cast(b, _lib.u8p), clip, C.c_void_p(d_d.data_ptr()), dp, dr, dc, None)
    assert rc == 0, _lib.lib().omr_last_error()
    torch.cuda.synchronize()
    out = d_d.cpu().numpy()
    assert (out[:, dc * cn:] == rx.SENTINEL).all()
    return out[:, :dc * cn].reshape(dr, dc, cn)


def test_rotate_device_both_tiers():
    rng = np.random.default_rng(32)
    for (rows, cols), cn, clip in (((38, 54), 1, 0), ((37, 53), 3, 1), ((64, 96), 3, 0), ((4, 6), 1, 1), ((64, 96), 1, 1)):
        a = gc.board(rng, rows, cols, cn)
        for interp in (0, 1):
            for angle, scale in zip(gc.QUARTER_TURNS, gc.EXACT_SCALES[0]):
                cpu.check_exact_case(a, _rotate_device(a, angle, scale, interp, clip), None, (cn, interp, 0, clip, angle, scale))
    for rows, cols in gc.GENERAL_SHAPES:
        a = gc.smooth(rows, cols)
        for i, (angle, scale) in enumerate(zip(gc.GENERAL_ANGLES, gc.GENERAL_SCALES + (1.0,))):
            cpu.check_general_case(a, _rotate_device(a, angle, scale, 1, i % 2), (1, 0, i % 2, angle, scale))
        for mode, clip, angle, scale in gc.nearest_cases(rows, cols):
            if mode == 0:
                cpu.check_nearest_case(a, _rotate_device(a, angle, scale, 0, clip), (0, clip, angle, scale))


# ---- the projection batch's deskew (deskew.hip's tile-record kernel) ------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1])
def test_projection_batch_deskew(interp):
    """three smooth 64 x 96 scans: the returned canvas against the float64 warp at the returned angle (CONTAIN, scale 1,
    BORDER_CONSTANT); NEAREST with the tie rule at whatever share of ties that angle has"""
    import torch
    rows, cols, cn, n = 64, 96, 3, 3
    imgs = [gc.smooth(rows, cols, 3, seed=s) for s in (1, 2, 3)]
    d = torch.from_numpy(np.stack(imgs)).cuda()
    pb = projection.ProjectionBatch(rows, cols, cn, 10, 0.25, 1.0, n)
    try:
        DR, DC = pb.deskew_canvas()
        step = DC * cn + 5
        out = torch.full((n, DR + 1, step), rx.SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ang, idx, size = pb.deskew_device(d.data_ptr(), rows * cols * cn, cols * cn, n, interp, gc.BORDER[:3], out.data_ptr(),
                                          (DR + 1) * step, step)
        torch.cuda.synchronize()
    finally:
        pb.close()
    out = out.cpu().numpy()
    for i, a in enumerate(imgs):
        angle = float(ang[i])
        M, dr, dc = gx.rotate_geometry(rows, cols, angle, 1.0, 1)
        assert tuple(size[i]) == (dr, dc), (i, angle, size[i], dr, dc)
        got = out[i, :dr, :dc * cn].reshape(dr, dc, cn)
        if interp == 1:
            cpu.check_general_case(a, got, (1, 0, 1, angle, 1.0))
        else:
            ref, alts, amb = gx.nearest_candidates(a, M, dr, dc, 0, gc.BORDER)
            ok = (got == ref).all(-1) | (amb & (got[None] == alts).all(-1).any(0))
            assert ok.all(), (i, angle, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


# ---- resize and gray ------------------------------------------------------------------------------------------------
def _resize_area_device(a, drows, dcols):
    import torch
    rows, cols, cn = a.shape
    sp, dp = cols * cn + 3, dcols * cn + 5
    sbuf = np.zeros((rows, sp), np.uint8)
    sbuf[:, :cols * cn] = a.reshape(rows, cols * cn)
    d_s = torch.from_numpy(sbuf).cuda()
    d_d = torch.full((drows, dp), rx.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = _lib.lib().omr_resize_area_device(C.c_void_p(d_s.data_ptr()), sp, rows, cols, cn, C.c_void_p(d_d.data_ptr()), dp, drows,
                                           dcols, None)
    assert rc == 0, _lib.lib().omr_last_error()
    torch.cuda.synchronize()
    out = d_d.cpu().numpy()
    assert (out[:, dcols * cn:] == rx.SENTINEL).all()
    return out[:, :dcols * cn].reshape(drows, dcols, cn)


@pytest.mark.parametrize("rows,cols,drows,dcols", gc.AREA_CASES)
def test_area_resize(rows, cols, drows, dcols):
    rng = np.random.default_rng(rows + dcols)
    for cn in (1, 3):
        for a in (rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8), gc.board(rng, rows, cols, cn)):
            cpu._hold(_resize_area_device(a, drows, dcols), gx.area_resize(a, drows, dcols),
                      gx.area_bound(rows, cols, drows, dcols), (rows, cols, drows, dcols, cn), clip=False, key="area")


@pytest.mark.parametrize("rows,cols,scale", gc.ENLARGE_CASES)
def test_enlarging_resize(rows, cols, scale):
    rng = np.random.default_rng(rows)
    for a in (gc.smooth(rows, cols), gc.board(rng, rows, cols, 3), gc.board(rng, rows, cols, 1)):
        got = transfer.TransformableMatrix(a).scale_self(scale).matrix
        dr, dc = int(rows * scale), int(cols * scale)
        assert got.shape[:2] == (dr, dc)
        cpu._hold(got, gx.linear_resize(a, dr, dc), gx.linear_resize_bound(), (rows, cols, scale), clip=False, key="enlarge")


def test_gray_conversion():
    """the 65 536 random triples, the cube's corners and the one-channel triples, per call and through the batch form
    on a padded pitch; the bytes are COLOR_RGB2GRAY's R, G, B in memory order (see test_geom_exact.test_restated_gray)"""
    import torch
    a = gc.gray_triples()
    exact = gx.gray(a[:, :, ::-1])
    cpu._hold(transfer.transfer_rgb_image_to_gray_image(a).matrix, exact, gx.gray_bound(), "per call", clip=False, key="gray")
    rows, cols = a.shape[:2]
    sp, dp = cols * 3 + 7, cols + 3
    sbuf = np.zeros((2, rows, sp), np.uint8)
    sbuf[0, :, :cols * 3] = a.reshape(rows, cols * 3)
    sbuf[1, :, :cols * 3] = a[::-1].reshape(rows, cols * 3)
    d_s = torch.from_numpy(sbuf).cuda()
    d_d = torch.full((2, rows, dp), rx.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    transfer.rgb_to_gray_batch(d_s.data_ptr(), 2, rows * sp, sp, rows, cols, 3, d_d.data_ptr(), rows * dp, dp)
    torch.cuda.synchronize()
    out = d_d.cpu().numpy()
    assert (out[:, :, cols:] == rx.SENTINEL).all()
    cpu._hold(out[0, :, :cols], exact, gx.gray_bound(), "batch 0", clip=False, key="gray")
    cpu._hold(out[1, :, :cols], exact[::-1], gx.gray_bound(), "batch 1", clip=False, key="gray")
