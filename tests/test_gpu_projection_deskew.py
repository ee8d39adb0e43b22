"""omr_projection_batch_deskew_device / omr_deskew_with_projections_batch on the device.

Scans: a synthetic ruled sheet -- dark horizontal rules and three boxes on white, drawn in numpy -- turned by -7, 0, 4.5,
33 and -38 degrees; colour 320 x 400, colour 333 x 453 tightly packed (nothing a multiple of 4: the warp's unstaged
path), gray 256 x 384, and one batch that is the same padded scan five times (scan stride 0).

Per (layout, front mode, sweep), for NEAREST and LINEAR and two borders each:
  (i)   angle[i] has the f64 bits of omr_get_angle_with_projections and best_idx agrees; out_size and every canvas byte
        equal omr_rotate_device on the same scan with that angle; the slot's other bytes stay as they were pre-filled
  (ii)  oracle.get_angle_with_projections gives the same angle; oracle.rotate_mat: NEAREST exact, LINEAR within 1 level
        (the tolerance tests/test_gpu_deskew.py has for the same kernels: the device builds warpAffine's fixed-point
        tables in its own kernel)
  and under +-45 @ 0.5 the winners of the 33 and -38 degree scans are at least 30 degrees, where a tile's source box no
  longer fits LDS and the warp taps global memory (staging such tiles by quadrants was measured and dropped,
  profiles/r16_projection_deskew.md, and its own test with it).
Then (iv) the same steep scans through omr_batch_deskew_device_cn, (v) the host form and (vi) reuse of one context."""
import ctypes as C

import numpy as np
import pytest

from oics import _lib, projection, transfer
from oics._lib import OmrImage, OmrImageOwned
from oics.types import RotateClipStrategy

import test_projection_deskew_abi as abi

pytestmark = pytest.mark.gpu

NONE, AREA_INT, AREA_GENERAL, LINEAR_FRONT = 0, 1, 2, 3
NEAREST, LINEAR = 0, 1
SENTINEL = 0xA5
ANGLES = (-7.0, 0.0, 4.5, 33.0, -38.0)
STEEP = (3, 4)  # the scans turned by 33 and -38 degrees
FRONTS = [(1.0, NONE), (0.5, AREA_INT), (0.3, AREA_GENERAL), (1.5, LINEAR_FRONT)]
SWEEPS = [(45, 0.5), (10, 0.25)]
BORDERS = [(255, 255, 255), (10, 200, 77)]
LAYOUTS = {  # rows, cols, channels, how the batch lies in memory
    "colour": (320, 400, 3, "packed"),
    "colour_odd": (333, 453, 3, "packed"),  # rows of 1359 bytes: nothing is a multiple of 4
    "gray": (256, 384, 1, "packed"),
    "same_scan_padded": (320, 400, 3, "stride0"),
}


def ruled_sheet(rows, cols, cn, angle):
    """rules 8 thick every 24 and three box outlines inside a sheet of 84 % of the frame, turned by `angle` about the centre"""
    yy, xx = np.mgrid[:rows, :cols].astype(np.float64)
    t = np.deg2rad(angle)
    x, y = xx - cols / 2.0, yy - rows / 2.0
    u = x * np.cos(t) + y * np.sin(t)
    v = -x * np.sin(t) + y * np.cos(t)
    dark = (np.mod(v, 24.0) < 8.0) & (np.abs(u) < 0.42 * cols) & (np.abs(v) < 0.42 * rows)
    for bu, bv in ((-0.3, -0.25), (0.1, 0.05), (0.28, 0.3)):
        d = np.maximum(np.abs(u - bu * cols), np.abs(v - bv * rows))
        dark |= (d < 20.0) & (d >= 14.0)
    g = np.where(dark, 25, 255).astype(np.uint8)
    if cn == 1:
        return g
    a = np.stack([g, g, g], 2)
    a[dark] = (25, 60, 40)
    return np.ascontiguousarray(a)


_SHEETS = {}


def _sheets(rows, cols, cn):
    key = (rows, cols, cn)
    if key not in _SHEETS:
        _SHEETS[key] = [ruled_sheet(rows, cols, cn, a) for a in ANGLES]
    return _SHEETS[key]


class Dev:
    """n same-shape scans on the device: tightly packed one after the other, or ONE scan with padded rows at stride 0"""

    def __init__(self, imgs, kind):
        import torch
        a0 = imgs[0]
        self.rows, self.cols = a0.shape[:2]
        self.cn = 1 if a0.ndim == 2 else a0.shape[2]
        row = self.cols * self.cn
        if kind == "stride0":
            assert all(a is a0 for a in imgs)
            self.step, self.stride = row + 8, 0
            buf = np.full((self.rows, self.step), 0x3C, np.uint8)
            buf[:, :row] = a0.reshape(self.rows, row)
        else:
            self.step, self.stride = row, self.rows * row
            buf = np.stack([a.reshape(self.rows, row) for a in imgs])
        self.host = buf.reshape(-1)
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = self.dev.data_ptr()
        self.n = len(imgs)

    def scan_ptr(self, i):
        return self.ptr + i * self.stride

    def untouched(self):
        return (self.dev.cpu().numpy() == self.host).all()


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _border4(border):
    return (C.c_uint8 * 4)(*(tuple(border) + (0,) * (4 - len(border))))


def _rotate_device(src, i, angle, interp, border):
    """omr_rotate_device on scan i as it lies in the batch: CONTAIN, scale 1"""
    import torch
    L = _lib.lib()
    r, c = C.c_int32(), C.c_int32()
    assert L.omr_rotate_size(src.rows, src.cols, angle, 1, C.byref(r), C.byref(c)) == 0
    d = torch.empty((r.value, c.value * src.cn), dtype=torch.uint8, device="cuda")
    rc = L.omr_rotate_device(src.scan_ptr(i), src.step, src.rows, src.cols, src.cn, angle, 1.0, interp, _border4(border), 1,
                             d.data_ptr(), c.value * src.cn, r.value, c.value, None)
    assert rc == 0, L.omr_last_error()
    torch.cuda.synchronize()
    return d.cpu().numpy()


def _deskew(pb, src, n, interp, border):
    """(angles, best_idx, out_size, slots [n, DR + 1, step]): every slot a row and 5 bytes a row larger than the canvas"""
    import torch
    DR, DC = pb.deskew_canvas()
    step = DC * src.cn + 5
    stride = (DR + 1) * step
    d = torch.full((n, DR + 1, step), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ang, idx, size = pb.deskew_device(src.ptr, src.stride, src.step, n, interp, border, d.data_ptr(), stride, step)
    return ang, idx, size, d.cpu().numpy()


def _check_slot(slot, size, ref, cn):
    dr, dcb = ref.shape
    assert tuple(size) == (dr, dcb // cn), (size, ref.shape)
    assert (slot[:dr, :dcb] == ref).all(), "%d bytes differ from omr_rotate_device" % int((slot[:dr, :dcb] != ref).sum())
    assert (slot[dr:, :] == SENTINEL).all() and (slot[:, dcb:] == SENTINEL).all(), "bytes outside the canvas were written"


def _check_batch(oracle, pb, imgs, kind, max_angle, step, scale, n=None):
    """(i) and (ii) for one batch on one context, both interpolations and both borders; returns the angles"""
    n = len(imgs) if n is None else n
    src = Dev(imgs[:n], kind)
    cn = src.cn
    N, _ = projection.candidate_count(max_angle, step)
    per_call, orc = {}, {}
    for i, a in enumerate(imgs[:n]):  # the same array object: the same scan
        if id(a) not in per_call:
            per_call[id(a)] = projection.get_angle_with_projections(a, max_angle, step, scale, 1)
            orc[id(a)] = oracle.get_angle_with_projections(a, max_angle, step, scale)
    angles = None
    for interp in (NEAREST, LINEAR):
        for border in BORDERS:
            bv = border[:cn]
            ang, idx, size, slots = _deskew(pb, src, n, interp, bv)
            assert src.untouched()
            if angles is not None:
                assert (_bits(ang) == _bits(angles)).all()
            angles = ang
            refs = {}
            for i, a in enumerate(imgs[:n]):
                oang, oidx = orc[id(a)]
                assert _bits(ang[i]) == _bits(per_call[id(a)]), (i, ang[i], per_call[id(a)])
                assert _bits(ang[i]) == _bits(oang) and idx[i] == oidx, (i, ang[i], oang, idx[i], oidx)
                assert _bits((idx[i] - N) * step) == _bits(ang[i])
                if id(a) not in refs:
                    refs[id(a)] = (_rotate_device(src, i, float(ang[i]), interp, bv),
                                   oracle.rotate_mat(a, float(ang[i]), 1.0, interp, tuple(bv) + (0,) * (4 - cn), 1))
                ref, exp = refs[id(a)]
                assert tuple(size[i]) == exp.shape[:2], (i, size[i], exp.shape)
                _check_slot(slots[i], size[i], ref, cn)
                got = slots[i][:exp.shape[0], :exp.shape[1] * cn].reshape(exp.shape)
                if interp == NEAREST:
                    assert (got == exp).all(), (i, int((got != exp).sum()))
                else:
                    assert np.abs(got.astype(np.int16) - exp.astype(np.int16)).max() <= 1, i
    return angles


@pytest.mark.parametrize("max_angle,step", SWEEPS)
@pytest.mark.parametrize("scale,mode", FRONTS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_batch_equals_the_per_call_pair_and_the_oracle(oracle, layout, scale, mode, max_angle, step):
    rows, cols, cn, kind = LAYOUTS[layout]
    sheets = _sheets(rows, cols, cn)
    imgs = [sheets[3]] * 5 if kind == "stride0" else sheets
    pb = projection.ProjectionBatch(rows, cols, cn, max_angle, step, scale, 5)
    try:
        # (333 x 453 does not halve exactly: its 0.5 is a fractional shrink, the other layouts' the integer one)
        assert pb.front_mode == (AREA_GENERAL if (layout, scale) == ("colour_odd", 0.5) else mode)
        angles = _check_batch(oracle, pb, imgs, kind, max_angle, step, scale)
    finally:
        pb.close()
    if max_angle == 45:  # the steep scans' winners are steep
        steep = range(5) if kind == "stride0" else STEEP
        assert all(abs(angles[i]) >= 30.0 for i in steep), angles


@pytest.mark.parametrize("rows,cols,cn,max_angle,step,scale", [(3508, 2480, 3, 45, 0.2, 0.2), (320, 400, 3, 45, 0.5, 1.0),
                                                               (333, 453, 3, 10, 0.25, 0.3), (256, 384, 1, 45, 0.5, 1.5)])
def test_canvas_is_rotate_sizes_maximum_and_the_context_refuses_before_device_work(rows, cols, cn, max_angle, step, scale):
    """omr_projection_batch_deskew_canvas == omr_rotate_size maximised over the candidates at the FULL shape, columns
    rounded up to 4; null pointers, n outside 1..3, pitches and slots a byte too small: -5; interp 2, 3, 4, -1: -213; all
    with host pointers and the outputs untouched"""
    pb = projection.ProjectionBatch(rows, cols, cn, max_angle, step, scale, 3)
    try:
        abi.check_context_refusals(pb.handle, rows, cols, cn, max_angle, step)
        assert pb.deskew_canvas() == abi.expected_canvas(rows, cols, max_angle, step)
    finally:
        pb.close()


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_existing_batch_deskew_keeps_its_results_at_steep_winners(interp):
    """(iv): the steep scans through omr_batch_deskew_device_cn with a +-45 context, against omr_rotate_device"""
    import torch
    rows, cols, cn, _ = LAYOUTS["colour"]
    imgs = [_sheets(rows, cols, cn)[i] for i in STEEP]
    src = Dev(imgs, "packed")
    b = projection.Batch(rows, cols, 45, 0.5, device=0, n_streams=1)
    try:
        DR, DC = b.deskew_canvas()
        out = torch.full((2, DR, DC * cn), SENTINEL, dtype=torch.uint8, device="cuda")
        size = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        best = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b.deskew_device_cn(src.ptr, src.stride, src.step, cn, 2, 127, interp, (10, 200, 77), out.data_ptr(), DR * DC * cn, DC * cn,
                           size.data_ptr(), best.data_ptr())
        b.sync()
        N = b.N
    finally:
        b.close()
    out, size, best = out.cpu().numpy(), size.cpu().numpy(), best.cpu().numpy()
    for i in range(2):
        angle = (int(best[i]) - N) * 0.5
        assert abs(angle) >= 30.0, angle
        _check_slot(out[i], size[i], _rotate_device(src, i, angle, interp, (10, 200, 77)), cn)


def test_host_form_mixed_shapes_with_a_four_channel_image():
    """(v): 7 images of three shapes, one of them 4 channels (the per-call path inside the batch); results at the
    images' own positions, identical to omr_get_angle_with_projections + omr_rotate"""
    c3 = _sheets(320, 400, 3)
    g1 = _sheets(256, 384, 1)
    four = np.ascontiguousarray(np.concatenate([_sheets(333, 453, 3)[2], np.full((333, 453, 1), 200, np.uint8)], 2))
    imgs = [c3[0], g1[3], c3[4], four, g1[1], c3[2], g1[4]]
    border = (10, 200, 77, 5)
    L = _lib.lib()
    keep = [transfer.as_image(a) for a in imgs]
    arr = (OmrImage * 7)(*[im for _, im in keep])
    ang, idx = np.zeros(7), np.zeros(7, np.int32)
    owned = (OmrImageOwned * 7)()
    rc = L.omr_deskew_with_projections_batch(arr, 7, 45, 0.5, 0.5, LINEAR, _border4(border), ang.ctypes.data_as(_lib.f64p),
                                             idx.ctypes.data_as(_lib.i32p), owned)
    assert rc == 0, L.omr_last_error()
    N, _ = projection.candidate_count(45, 0.5)
    for i, a in enumerate(imgs):
        ref = projection.get_angle_with_projections(a, 45, 0.5, 0.5, 1)
        assert _bits(ang[i]) == _bits(ref) and _bits((idx[i] - N) * 0.5) == _bits(ref), (i, ang[i], ref)
        exp = transfer.rotate_mat(a, ref, 1.0, LINEAR, 0, border, RotateClipStrategy.CONTAIN).get_mat()
        o = owned[i]
        cn = 1 if a.ndim == 2 else a.shape[2]
        assert (o.rows, o.cols, o.channels, o.step_bytes) == (exp.shape[0], exp.shape[1], cn, exp.shape[1] * cn), i
        got = np.ctypeslib.as_array(C.cast(o.data, C.POINTER(C.c_uint8)), shape=(o.rows * o.step_bytes,)).reshape(exp.shape)
        assert (got == exp).all(), (i, int((got != exp).sum()))
        L.omr_image_free(C.byref(owned[i]))
        assert not owned[i].data
    # the Python front door gives the same
    a2, pics = projection.get_angles_and_deskew(imgs[:3], 45, 0.5, 0.5, interp=NEAREST, border=border)
    assert (_bits(a2) == _bits(ang[:3])).all()
    for i in range(3):
        exp = transfer.rotate_mat(imgs[i], a2[i], 1.0, NEAREST, 0, border, RotateClipStrategy.CONTAIN).get_mat()
        assert pics[i].shape == exp.shape and (pics[i] == exp).all()


def test_one_context_two_batch_sizes_and_a_refused_call_in_between(oracle):
    """(vi): runs of 5, then 2 scans (the second run's results are the second run's), a refused call, a valid call"""
    rows, cols, cn, _ = LAYOUTS["colour"]
    sheets = _sheets(rows, cols, cn)
    pb = projection.ProjectionBatch(rows, cols, cn, 45, 0.5, 0.5, 5)
    try:
        _check_batch(oracle, pb, sheets, "packed", 45, 0.5, 0.5)
        second = [sheets[4], sheets[1]]
        a2 = _check_batch(oracle, pb, second, "packed", 45, 0.5, 0.5)
        assert a2[0] == -38.0 and abs(a2[1]) <= 0.5
        src = Dev(second, "packed")
        DR, DC = pb.deskew_canvas()
        L = _lib.lib()
        ang, size = np.full(2, 7.0), np.full(4, -9, np.int32)
        args = (ang.ctypes.data_as(_lib.f64p), None)
        sp = size.ctypes.data_as(_lib.i32p)
        w = _border4((255, 255, 255))
        for rc, call in ((-5, (src.ptr, src.stride, src.step, 6, LINEAR, w, src.ptr, DR * DC * cn, DC * cn, sp)),
                         (-5, (src.ptr, src.stride, src.step, 2, LINEAR, w, src.ptr, DR * DC * cn, DC * cn - 1, sp)),
                         (-5, (src.ptr, src.stride, src.step, 2, LINEAR, w, src.ptr, DR * DC * cn - 1, DC * cn, sp)),
                         (-5, (src.ptr, src.stride, src.step, 2, LINEAR, w, None, DR * DC * cn, DC * cn, sp)),
                         (-213, (src.ptr, src.stride, src.step, 2, 2, w, src.ptr, DR * DC * cn, DC * cn, sp))):
            assert L.omr_projection_batch_deskew_device(pb.handle, *call, *args) == rc, call
        assert (ang == 7.0).all() and (size == -9).all() and src.untouched()
        _check_batch(oracle, pb, sheets, "packed", 45, 0.5, 0.5, n=3)
        # the angle-only entry point still runs on the same context
        ang3, idx3, _, _ = pb.run_device(src.ptr, src.stride, src.step, 2)
        assert (_bits(ang3) == _bits(a2)).all()
    finally:
        pb.close()
