"""omr_projection_batch_* / omr_get_angles_with_projections_batch on the device.  All parity is bit for bit.

front_device: every scan's working image against the per-call chain (omr_scale) and against oracle.scale_self, for the
four front-end modes, 1 and 3 channels, odd shapes, three source layouts (tightly packed: byte-wise staging for odd
widths; dword-aligned pitches: dword staging; padded steps and strides at odd addresses), into a sentinel-filled
destination whose every byte outside the working images must survive, with the source untouched.
run_device: angle (as f64 bits), best_idx and, when asked for, all A scores of every scan against
omr_get_angle_with_projections and oracle.get_angle_with_projections (scores: the per-call stages omr_scale ->
omr_rgb_to_gray -> sweep at black_max 127, and the oracle's scale_self -> rgb2gray -> threshold -> sweep).
Then the host form and a slice of tests/fuzz/fuzz_projection_batch.py.  Every GPU step runs once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import dataset_pin as dp
from oics import _lib, projection, transfer
from oics._lib import OmrImage

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NONE, AREA_INT, AREA_GENERAL, LINEAR = 0, 1, 2, 3
SENTINEL = 0xA5


def _scan(rng, rows, cols, cn, skew=0.0):
    """a noisy sheet: light paper, dark bars along a slightly tilted grid, full-range noise in one corner"""
    yy, xx = np.mgrid[:rows, :cols].astype(np.float64)
    t = np.deg2rad(skew)
    u = xx * np.cos(t) + yy * np.sin(t)
    v = -xx * np.sin(t) + yy * np.cos(t)
    g = np.where(((u % 23) < 4) | ((v % 31) < 5), 30, 225).astype(np.int64)
    a = np.clip(g[:, :, None] + rng.integers(-25, 26, (rows, cols, cn)), 0, 255).astype(np.uint8)
    a[:rows // 5, :cols // 5] = rng.integers(0, 256, (rows // 5, cols // 5, cn), dtype=np.uint8)
    return a if cn > 1 else a[:, :, 0]


class Src:
    """n same-shape scans on the device in one of three layouts"""

    def __init__(self, imgs, kind):
        import torch
        a0 = imgs[0]
        self.rows, self.cols = a0.shape[:2]
        self.cn = 1 if a0.ndim == 2 else a0.shape[2]
        row = self.cols * self.cn
        if kind == "packed":
            self.off, self.step = 0, row
            self.stride = self.rows * self.step
        elif kind == "dword":
            self.off, self.step = 0, (row + 3) & ~3
            self.stride = self.rows * self.step + 8
        else:  # padded rows, gaps between scans, an odd base address
            self.off, self.step = 1, row + 5
            self.stride = self.rows * self.step + 11
        buf = np.full(self.off + (len(imgs) - 1) * self.stride + (self.rows - 1) * self.step + row, 0x3C, np.uint8)
        for i, a in enumerate(imgs):
            o = self.off + i * self.stride
            for y in range(self.rows):
                buf[o + y * self.step:o + y * self.step + row] = a[y].reshape(-1)
        self.host = buf
        self.dev = torch.from_numpy(buf).cuda()
        self.ptr = self.dev.data_ptr() + self.off

    def untouched(self):
        return (self.dev.cpu().numpy() == self.host).all()


def _per_call_scale(a, scale):
    return np.asarray(transfer.TransformableMatrix(a.copy()).scale_self(scale).matrix)


def _check_front(oracle, imgs, scale, kind, mode):
    import torch
    src = Src(imgs, kind)
    n = len(imgs)
    pb = projection.ProjectionBatch(src.rows, src.cols, src.cn, 5, 0.5, scale, n)
    try:
        assert pb.front_mode == mode, (pb.front_mode, mode)
        wr, wc = pb.wrows, pb.wcols
        wrow = wc * src.cn
        off, step = 2, wrow + 3
        stride = wr * step + 7
        d = torch.full((off + n * stride + 5,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pb.front_device(src.ptr, src.stride, src.step, n, d.data_ptr() + off, stride, step)
        got = d.cpu().numpy()
    finally:
        pb.close()
    inside = np.zeros(got.size, bool)
    for i, a in enumerate(imgs):
        o = off + i * stride
        inside[o:o + wr * step].reshape(wr, step)[:, :wrow] = True
        w = got[o:o + wr * step].reshape(wr, step)[:, :wrow].reshape((wr, wc) if src.cn == 1 else (wr, wc, src.cn))
        ref1 = _per_call_scale(a, scale).reshape(w.shape)
        ref2 = oracle.scale_self(a, scale).reshape(w.shape)
        assert (w == ref1).all(), "scan %d differs from omr_scale in %d bytes" % (i, int((w != ref1).sum()))
        assert (w == ref2).all(), "scan %d differs from oracle.scale_self in %d bytes" % (i, int((w != ref2).sum()))
    assert (got[~inside] == SENTINEL).all(), "bytes outside the working images were written"
    assert src.untouched()


FRONT = [  # rows, cols, scale, mode
    (453, 641, 0.5, AREA_GENERAL), (453, 641, 0.37, AREA_GENERAL), (453, 641, 1.5, LINEAR), (453, 641, 1.0, NONE),
    (452, 640, 0.5, AREA_INT), (450, 640, 0.2, AREA_INT), (451, 644, 0.05, AREA_GENERAL), (970, 3000, 0.011, AREA_GENERAL),
]


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("kind", ["packed", "dword", "odd"])
def test_front_device_matches_the_per_call_chain_and_the_oracle(oracle, cn, kind):
    rng = np.random.Generator(np.random.PCG64(100 + cn))
    for rows, cols, scale, mode in FRONT:
        imgs = [_scan(rng, rows, cols, cn, skew=i - 1.0) for i in range(3)]
        _check_front(oracle, imgs, scale, kind, mode)


def test_front_device_a4_colour_batch(oracle):
    rng = np.random.Generator(np.random.PCG64(7))
    base = _scan(rng, 3508, 2480, 3, skew=0.7)
    imgs = [base, np.ascontiguousarray(base[::-1]), np.ascontiguousarray(base[:, ::-1])]
    _check_front(oracle, imgs, 0.2, "packed", AREA_GENERAL)


def test_front_device_segment_wider_than_the_staging_budget(oracle):
    """one destination pixel spans more than 5461 x 3 source bytes, more than the tile kernel stages, so the direct
    kernels run: 5600 x 5600 -> 1 x 1 (factor 5600 both ways) and 5600 x 11001 -> 1 x 2 (5500.5 across)"""
    rng = np.random.Generator(np.random.PCG64(9))
    a = rng.integers(0, 256, (5600, 11001, 3), dtype=np.uint8)
    _check_front(oracle, [np.ascontiguousarray(a[:, :5600])], 0.0002, "packed", AREA_INT)
    _check_front(oracle, [a], 0.0002, "packed", AREA_GENERAL)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _oracle_scores(oracle, a, max_angle, step, scale):
    w = oracle.scale_self(a, scale)
    gray = oracle.rgb2gray(w) if w.ndim == 3 else w
    _, _, vs, hs = oracle.sweep(oracle.threshold_binary(gray), max_angle, step, want_proj=False)
    return vs, hs


def _per_call_scores(a, max_angle, step, scale):
    w = _per_call_scale(a, scale) if scale != 1.0 else a
    gray = np.asarray(transfer.transfer_rgb_image_to_gray_image(w).matrix) if w.ndim == 3 else w
    plan = projection.SweepPlan(gray.shape[0], gray.shape[1], max_angle, step)
    try:
        _, _, vs, hs, _ = plan.run(gray, black_max=127, want_proj=False)
    finally:
        plan.close()
    return vs, hs


def _check_run(oracle, pb, imgs, kind, max_angle, step, scale, want_sd):
    src = Src(imgs, kind)
    n = len(imgs)
    N, A = projection.candidate_count(max_angle, step)
    ang, idx, vs, hs = pb.run_device(src.ptr, src.stride, src.step, n, want_sd=want_sd)
    assert src.untouched()
    for i, a in enumerate(imgs):
        ref = projection.get_angle_with_projections(a, max_angle, step, scale, 1)
        oang, oidx = oracle.get_angle_with_projections(a, max_angle, step, scale)
        assert _bits(ang[i]) == _bits(ref), (i, ang[i], ref)
        assert _bits(ang[i]) == _bits(oang) and idx[i] == oidx, (i, ang[i], oang, idx[i], oidx)
        assert _bits((idx[i] - N) * step) == _bits(ang[i])
        if want_sd:
            for rv, rh in (_per_call_scores(a, max_angle, step, scale), _oracle_scores(oracle, a, max_angle, step, scale)):
                assert (_bits(vs[i]) == _bits(rv)).all() and (_bits(hs[i]) == _bits(rh)).all(), i
    return ang, idx


def test_run_device_dataset_sheets_with_the_references_parameters(oracle):
    """sheets of tests/golden/dataset rotated by known angles, (45, 0.2, 0.2): core/src/main.rs:70"""
    by_shape = {}
    for name in dp.sheets()[:12]:
        a = dp.imread_color(name)
        by_shape.setdefault(a.shape, []).append(a)
    sheets = max(by_shape.values(), key=len)[:3]
    inject = [3.4, -7.8, 0.6]
    imgs = [oracle.rotate_mat(a, -t, 1.0, interp=1, border=(255, 255, 255, 0), clip=0) for a, t in zip(sheets, inject)]
    rows, cols = imgs[0].shape[:2]
    pb = projection.ProjectionBatch(rows, cols, 3, 45, 0.2, 0.2, 4)
    try:
        _check_run(oracle, pb, imgs, "packed", 45, 0.2, 0.2, want_sd=True)
    finally:
        pb.close()


@pytest.mark.parametrize("cn", [1, 3])
def test_run_device_small_range_batch_sizes_and_reuse(oracle, cn):
    """(2, 0.05, 0.5) as DESIGN section 3; a batch of max_scans, a batch of 1 and a batch in between on one context"""
    rng = np.random.Generator(np.random.PCG64(31 + cn))
    rows, cols, max_scans = 453, 641, 5
    imgs = [_scan(rng, rows, cols, cn, skew=0.3 * i - 0.6) for i in range(max_scans)]
    pb = projection.ProjectionBatch(rows, cols, cn, 2, 0.05, 0.5, max_scans)
    try:
        _check_run(oracle, pb, imgs, "dword", 2, 0.05, 0.5, want_sd=True)
        _check_run(oracle, pb, imgs[3:4], "packed", 2, 0.05, 0.5, want_sd=False)
        _check_run(oracle, pb, imgs[1:4], "odd", 2, 0.05, 0.5, want_sd=True)
        # argument errors between valid runs, each before any device work
        L = _lib.lib()
        src = Src(imgs[:2], "packed")
        out = np.zeros(8)
        op = out.ctypes.data_as(_lib.f64p)
        for args in ((0, src.stride, src.step, 1, op), (src.ptr, src.stride, src.step, 0, op),
                     (src.ptr, src.stride, src.step, max_scans + 1, op), (src.ptr, src.stride, cols * cn - 1, 2, op),
                     (src.ptr, -1, src.step, 2, op), (src.ptr, src.stride, src.step, 2, None)):
            assert L.omr_projection_batch_run_device(pb.handle, args[0], args[1], args[2], args[3], args[4], None, None, None) == -5
        assert L.omr_projection_batch_front_device(pb.handle, src.ptr, src.stride, src.step, 2, None, 1 << 20, 4096) == -5
        assert L.omr_projection_batch_front_device(pb.handle, src.ptr, src.stride, src.step, 2, src.ptr, 1 << 20, pb.wcols * cn - 1) == -5
        assert L.omr_projection_batch_front_device(pb.handle, src.ptr, src.stride, src.step, 2, src.ptr, pb.wrows * 4096 - 1, 4096) == -5
        _check_run(oracle, pb, imgs[:2], "packed", 2, 0.05, 0.5, want_sd=False)
    finally:
        pb.close()


@pytest.mark.parametrize("scale,mode", [(0.37, AREA_GENERAL), (1.5, LINEAR), (0.25, AREA_INT)])
def test_run_device_other_modes(oracle, scale, mode):
    rng = np.random.Generator(np.random.PCG64(57))
    rows, cols = (452, 640) if mode == AREA_INT else (301, 427)
    imgs = [_scan(rng, rows, cols, 3, skew=1.1 * i - 1.0) for i in range(3)]
    pb = projection.ProjectionBatch(rows, cols, 3, 5, 0.5, scale, 3)
    try:
        assert pb.front_mode == mode
        _check_run(oracle, pb, imgs, "packed", 5, 0.5, scale, want_sd=True)
    finally:
        pb.close()


def test_run_device_scale_one_is_the_colour_batch_sweep(oracle):
    """scale 1.0: no resize stage; the answers of omr_batch_run_device_cn followed by the arg-max"""
    import torch
    rng = np.random.Generator(np.random.PCG64(77))
    rows, cols, n = 300, 404, 4
    imgs = [_scan(rng, rows, cols, 3, skew=0.8 * i - 1.0) for i in range(n)]
    pb = projection.ProjectionBatch(rows, cols, 3, 5, 0.5, 1.0, n)
    try:
        assert pb.front_mode == NONE and (pb.wrows, pb.wcols) == (rows, cols)
        ang, idx = _check_run(oracle, pb, imgs, "dword", 5, 0.5, 1.0, want_sd=True)
        src = Src(imgs, "dword")
        _, _, vs, hs = pb.run_device(src.ptr, src.stride, src.step, n, want_sd=True)[0:4]
    finally:
        pb.close()
    N, A = projection.candidate_count(5, 0.5)
    b = projection.Batch(rows, cols, 5, 0.5)
    try:
        d_best = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_v = torch.zeros(n * A, dtype=torch.float64, device="cuda")
        d_h = torch.zeros(n * A, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        b.run_device_cn(src.ptr, src.stride, src.step, 3, n, 127, d_best.data_ptr(), d_v.data_ptr(), d_h.data_ptr())
        b.sync()
    finally:
        b.close()
    bv, bh = d_v.cpu().numpy().reshape(n, A), d_h.cpu().numpy().reshape(n, A)
    assert (_bits(bv) == _bits(vs)).all() and (_bits(bh) == _bits(hs)).all()
    assert (d_best.cpu().numpy() == idx).all()
    for i in range(n):
        assert projection.argmax_projection(bv[i], bh[i]) == idx[i]


def test_host_form_mixed_shapes_and_channels(oracle):
    rng = np.random.Generator(np.random.PCG64(91))
    shapes = [(300, 404, 3), (213, 317, 1), (300, 404, 3), (120, 96, 4), (213, 317, 1), (300, 404, 3), (301, 404, 3),
              (120, 96, 4)]
    imgs = [_scan(rng, r, c, cn, skew=0.4 * i - 1.5) for i, (r, c, cn) in enumerate(shapes)]
    for scale in (0.5, 1.0):
        ang, idx = projection.get_angles_with_projections(imgs, 5, 0.5, scale, want_idx=True)
        N, _ = projection.candidate_count(5, 0.5)
        for i, a in enumerate(imgs):
            ref = projection.get_angle_with_projections(a, 5, 0.5, scale, 1)
            assert _bits(ang[i]) == _bits(ref), (scale, i, ang[i], ref)
            assert _bits((idx[i] - N) * 0.5) == _bits(ref)
            if a.ndim == 2 or a.shape[2] != 4:
                assert _bits(oracle.get_angle_with_projections(a, 5, 0.5, scale)[0]) == _bits(ref)
    # a padded step (a view into a wider array) is taken as it is
    wide = np.full((300, 420, 3), 9, np.uint8)
    wide[:, :404] = imgs[0]
    a, im = transfer.as_image(imgs[0])
    arr = (OmrImage * 2)(OmrImage(wide.ctypes.data, 300, 404, 3, wide.strides[0]), im)
    out = np.zeros(2)
    assert _lib.lib().omr_get_angles_with_projections_batch(arr, 2, 5, 0.5, 0.5, out.ctypes.data_as(_lib.f64p), None) == 0
    assert _bits(out[0]) == _bits(out[1]) and _bits(out[0]) == _bits(projection.get_angle_with_projections(imgs[0], 5, 0.5, 0.5, 1))


def test_host_form_invalid_image_in_the_middle_leaves_no_partial_result():
    rng = np.random.Generator(np.random.PCG64(93))
    good = _scan(rng, 120, 96, 3)
    keep = [good, np.zeros((40, 40, 2), np.uint8), good]
    arr = (OmrImage * 3)(*[transfer.as_image(k)[1] for k in keep])
    ang, idx = np.full(3, 7.0), np.full(3, -9, np.int32)
    rc = _lib.lib().omr_get_angles_with_projections_batch(arr, 3, 5, 0.5, 0.5, ang.ctypes.data_as(_lib.f64p),
                                                          idx.ctypes.data_as(_lib.i32p))
    assert rc == -215 and (ang == 7.0).all() and (idx == -9).all()
    arr[1] = OmrImage(good.ctypes.data, 1, 96, 3, 288)  # 1 * 0.5 truncates to 0, as per call
    rc = _lib.lib().omr_get_angles_with_projections_batch(arr, 3, 5, 0.5, 0.5, ang.ctypes.data_as(_lib.f64p),
                                                          idx.ctypes.data_as(_lib.i32p))
    assert rc == -215 and (ang == 7.0).all() and (idx == -9).all()
    with pytest.raises(_lib.OmrError) as e:
        projection.get_angle_with_projections(good[:1], 5, 0.5, 0.5, 1)
    assert e.value.code == -215


def test_fuzz_projection_batch_slice(monkeypatch):
    """A fixed slice of tests/fuzz/fuzz_projection_batch.py: random shapes, scales, channels, strides and sweeps."""
    import runpy
    tool = os.path.join(HERE, "fuzz", "fuzz_projection_batch.py")
    monkeypatch.setattr(sys, "argv", [tool, "40", "11"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(tool, run_name="__main__")
    assert e.value.code == 0
