"""omr_rotate_batch_device_ex / omr_rotate_batch_ex on the device.  The batch form promises omr_rotate_device_ex's
bytes, so the yardstick is the per-call entry point: each batch runs once into a pattern-filled block of slots, the
same images run one call each into an identical block, and the two blocks are compared whole -- canvases, the guard
bytes of every slot outside its canvas, and the gaps between rows and slots.  Three layouts (tightly packed odd widths:
the byte-wise staging; dword-aligned pitches: the dword staging; padded steps and strides at odd addresses) x every
interpolation x every border mode x {forward, WARP_INVERSE_MAP} x channels {1, 3, 4} x clip x scale {1.0, 0.2}.  A subset
is checked against the numpy restatement of warpAffine (tests/warp_ref.py) with test_gpu_rotate_ex.py's rule: every
byte equal, for every interpolation.  Then BORDER_TRANSPARENT, the acceptance protocol's shape (64 golden sheets, one
call), the Hough batch's angles fed straight in, the host form with mixed shapes, more images than one launch's
blockIdx.z holds, and argument errors between valid calls.  Every GPU step runs once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import warp_ref as wr
from oics import _lib, omr, synth, transfer
from oics._lib import OmrImage, OmrImageOwned

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BORDER = (23, 201, 87, 140)
ANGLES7 = [0.0, 0.05, -0.05, 7.3, -10.0, 41.0, -90.0]  # distinct, 0, both signs, a quarter turn


def _content(rng, rows, cols, cn):
    a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    yy, xx = np.mgrid[:rows, :cols]
    board = ((yy // 2 + xx // 2) % 2 * 255).astype(np.uint8)
    half = xx < cols // 2  # left half: 0/255 checkerboard, so cubic and Lanczos overshoot and saturate
    a[half] = board[half][:, None]
    return a


class Layout:
    """n images of rows x cols x cn on the device: where the sources lie and how the slots are laid out"""

    def __init__(self, imgs, angles, clip, kind):
        import torch
        self.imgs, self.angles, self.clip = imgs, np.asarray(angles, np.float64), clip
        self.n = len(imgs)
        self.rows, self.cols, self.cn = imgs[0].shape
        rows, cols, cn, n = self.rows, self.cols, self.cn, self.n
        self.mr, self.mc, self.sizes = transfer.rotate_batch_canvas(rows, cols, self.angles, clip)
        if kind == "packed":
            self.so, self.sstep, self.do, self.dstep = 0, cols * cn, 0, self.mc * cn
            self.sstride, self.dstride = rows * self.sstep, self.mr * self.dstep
        elif kind == "dword":
            self.so, self.sstep, self.do, self.dstep = 0, (cols * cn + 3) & ~3, 0, (self.mc * cn + 3) & ~3
            self.sstride, self.dstride = rows * self.sstep, self.mr * self.dstep
        else:  # padded rows, gaps between images, odd base addresses
            self.so, self.sstep, self.do, self.dstep = 1, cols * cn + 5, 3, self.mc * cn + 7
            self.sstride, self.dstride = rows * self.sstep + 11, self.mr * self.dstep + 13
        sbuf = np.zeros(self.so + n * self.sstride + 8, np.uint8)
        for i, a in enumerate(imgs):
            v = sbuf[self.so + i * self.sstride:self.so + i * self.sstride + rows * self.sstep].reshape(rows, self.sstep)
            v[:, :cols * cn] = a.reshape(rows, cols * cn)
        self.d_src = torch.from_numpy(sbuf).cuda()
        self.dlen = self.do + n * self.dstride + 8
        self.pattern = ((torch.arange(self.dlen, device="cuda") * 7 + 3) % 251).to(torch.uint8)
        inside = np.zeros(self.dlen, bool)
        for i in range(n):
            dr, dc = self.sizes[i]
            s = inside[self.do + i * self.dstride:self.do + i * self.dstride + self.mr * self.dstep].reshape(self.mr, self.dstep)
            s[:dr, :dc * cn] = True
        self.outside = torch.from_numpy(~inside).cuda()

    def src_ptr(self, i=0):
        return self.d_src.data_ptr() + self.so + i * self.sstride

    def batch(self, scale, flags, mode, fill=None):
        """one call of the batch form -> (device block, sizes)"""
        import torch
        d = self.pattern.clone() if fill is None else torch.full((self.dlen,), fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sizes = transfer.rotate_batch_device_ex(self.src_ptr(), self.n, self.sstride, self.sstep, self.rows, self.cols, self.cn,
                                                self.angles, scale, flags, mode, BORDER, self.clip, d.data_ptr() + self.do,
                                                self.dstride, self.dstep, self.mr, self.mc)
        torch.cuda.synchronize()
        return d, sizes

    def per_call(self, scale, flags, mode):
        """the same work, one omr_rotate_device_ex call per image into an identical block"""
        import torch
        d = self.pattern.clone()
        torch.cuda.synchronize()
        b = (C.c_uint8 * 4)(*BORDER)
        for i in range(self.n):
            dr, dc = C.c_int32(), C.c_int32()
            assert _lib.lib().omr_rotate_size(self.rows, self.cols, self.angles[i], self.clip, C.byref(dr), C.byref(dc)) == 0
            rc = _lib.lib().omr_rotate_device_ex(C.c_void_p(self.src_ptr(i)), self.sstep, self.rows, self.cols, self.cn,
                                                 float(self.angles[i]), scale, flags, mode, C.cast(b, _lib.u8p), self.clip,
                                                 C.c_void_p(d.data_ptr() + self.do + i * self.dstride), self.dstep, dr.value,
                                                 dc.value, None)
            assert rc == 0, _lib.lib().omr_last_error()
            assert (dr.value, dc.value) == tuple(self.sizes[i])
        torch.cuda.synchronize()
        return d

    def canvas(self, block, i):
        dr, dc = self.sizes[i]
        s = block[self.do + i * self.dstride:self.do + i * self.dstride + self.mr * self.dstep].reshape(self.mr, self.dstep)
        return s[:dr, :dc * self.cn].reshape(dr, dc, self.cn)

    def check(self, scale, flags, mode):
        import torch
        got, sizes = self.batch(scale, flags, mode)
        assert (sizes == self.sizes).all()
        assert torch.equal(got[self.outside], self.pattern[self.outside]), ("guard bytes written", scale, flags, mode)
        exp = self.per_call(scale, flags, mode)
        if not torch.equal(got, exp):
            g, e = got.cpu().numpy(), exp.cpu().numpy()
            bad = [i for i in range(self.n) if not np.array_equal(self.canvas(g, i), self.canvas(e, i))]
            raise AssertionError(("batch != per call", self.rows, self.cols, self.cn, scale, flags, mode, self.clip, bad,
                                  int((g != e).sum())))
        return got


BATCHES = [("packed", 453, 311), ("dword", 452, 312), ("padded", 201, 333)]


@pytest.mark.parametrize("kind,rows,cols", BATCHES)
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_batch_equals_per_call_every_flag_border_clip_scale(kind, rows, cols, cn):
    rng = np.random.default_rng(rows + cn)
    imgs = [_content(rng, rows, cols, cn) for _ in ANGLES7]
    for clip in (0, 1):
        lay = Layout(imgs, ANGLES7, clip, kind)
        if kind == "packed":
            assert lay.sstride == rows * cols * cn and lay.dstep == lay.mc * cn
        if kind == "dword":
            assert lay.sstep % 4 == 0 and lay.sstride % 4 == 0 and lay.dstep % 4 == 0 and lay.src_ptr() % 4 == 0
        for interp in (0, 1, 2, 3, 4):
            for mode in range(6):
                for inv in (0, 16):
                    for scale in (1.0, 0.2):
                        lay.check(scale, interp | inv, mode)


@pytest.mark.parametrize("kind,rows,cols", BATCHES)
def test_batch_equals_the_restatement(kind, rows, cols):
    """test_gpu_rotate_ex.py compares the per-call entry point with warp_ref.rotate_ex byte for byte, every interpolation
    included; the same rule here"""
    rng = np.random.default_rng(rows)
    cases = [(0, wr.CONSTANT, 1, 1, 1.0), (1, wr.CONSTANT, 3, 1, 1.0), (1 | 16, wr.REPLICATE, 1, 0, 1.0),
             (2, wr.REFLECT_101, 3, 1, 1.0), (4, wr.WRAP, 1, 1, 1.0), (2 | 16, wr.REFLECT, 4, 0, 0.2),
             (0, wr.TRANSPARENT, 3, 1, 0.2), (4, wr.CONSTANT, 4, 0, 1.0), (3, wr.TRANSPARENT, 1, 1, 1.0)]
    for flags, mode, cn, clip, scale in cases:
        imgs = [_content(rng, rows, cols, cn) for _ in ANGLES7]
        lay = Layout(imgs, ANGLES7, clip, kind)
        got = lay.batch(scale, flags, mode)[0].cpu().numpy()
        pat = lay.pattern.cpu().numpy()
        for i in range(lay.n):
            exp = wr.rotate_ex(imgs[i], ANGLES7[i], scale, flags, mode, BORDER, clip, init=lay.canvas(pat, i).copy())
            ok = lay.canvas(got, i) == exp
            assert ok.all(), (kind, flags, mode, cn, clip, scale, i, np.argwhere(~ok)[:5].tolist())


def test_border_transparent_device_keeps_and_host_zeroes():
    rng = np.random.default_rng(77)
    imgs = [_content(rng, 120, 161, 3) for _ in ANGLES7]
    for interp in (0, 1, 2, 4):
        lay = Layout(imgs, ANGLES7, 1, "padded")
        a, _ = lay.batch(1.0, interp, wr.TRANSPARENT, fill=0x11)
        b, _ = lay.batch(1.0, interp, wr.TRANSPARENT, fill=0xEE)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        host = transfer.rotate_batch_ex(imgs, ANGLES7, 1.0, interp, wr.TRANSPARENT, BORDER, 1)
        for i in range(lay.n):
            ca, cb = lay.canvas(a, i), lay.canvas(b, i)
            skipped = ca != cb  # a written pixel does not depend on what was there
            exp0 = wr.rotate_ex(imgs[i], ANGLES7[i], 1.0, interp, wr.TRANSPARENT, BORDER, 1, init=np.zeros(ca.shape, np.uint8))
            exp1 = wr.rotate_ex(imgs[i], ANGLES7[i], 1.0, interp, wr.TRANSPARENT, BORDER, 1, init=np.full(ca.shape, 255, np.uint8))
            assert (skipped == (exp0 != exp1)).all(), (interp, i)
            assert (ca[skipped] == 0x11).all() and (cb[skipped] == 0xEE).all()
            h = host[i].matrix
            assert h.shape == ca.shape and (h[skipped] == 0).all() and (h[~skipped] == ca[~skipped]).all(), (interp, i)
            assert (h == exp0).all()


def _rotate_device_per_call(d_src_ptr, sstep, rows, cols, cn, angle, interp, border, clip):
    """omr_rotate_device into a packed canvas of its own -> numpy canvas"""
    import torch
    dr, dc = C.c_int32(), C.c_int32()
    assert _lib.lib().omr_rotate_size(rows, cols, angle, clip, C.byref(dr), C.byref(dc)) == 0
    out = torch.zeros((dr.value, dc.value, cn), dtype=torch.uint8, device="cuda")
    b = (C.c_uint8 * 4)(*border)
    rc = _lib.lib().omr_rotate_device(C.c_void_p(d_src_ptr), sstep, rows, cols, cn, float(angle), 1.0, interp,
                                      C.cast(b, _lib.u8p), clip, C.c_void_p(out.data_ptr()), dc.value * cn, dr.value, dc.value,
                                      None)
    assert rc == 0, _lib.lib().omr_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_protocol_shape_64_golden_sheets_one_call():
    """lib.rs:55 / :161: every sheet by its own angle, INTER_LINEAR, BORDER_CONSTANT, white, CONTAIN, 3 channels"""
    import torch
    import dataset_pin as dp
    names = dp.sheets()[:64]
    assert len(names) == 64
    sheets = [dp.imread_color(nm) for nm in names]
    rows, cols = max(s.shape[0] for s in sheets), max(s.shape[1] for s in sheets)
    batch = np.full((64, rows, cols, 3), 255, np.uint8)  # padded with paper white to one shape
    for i, s in enumerate(sheets):
        batch[i, :s.shape[0], :s.shape[1]] = s
    angles = np.random.Generator(np.random.PCG64(55)).uniform(-10.0, 10.0, 64)
    white = (255, 255, 255, 0)
    mr, mc, sizes = transfer.rotate_batch_canvas(rows, cols, angles, 1)
    d_src = torch.from_numpy(batch).cuda()
    dstep = mc * 3
    d_dst = torch.full((64, mr, dstep), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got_sizes = transfer.rotate_batch_device_ex(d_src.data_ptr(), 64, rows * cols * 3, cols * 3, rows, cols, 3, angles, 1.0,
                                                transfer.INTER_LINEAR, transfer.BORDER_CONSTANT, white, 1, d_dst.data_ptr(),
                                                mr * dstep, dstep, mr, mc)
    torch.cuda.synchronize()
    assert (got_sizes == sizes).all()
    out = d_dst.cpu().numpy()
    for i in range(64):
        exp = _rotate_device_per_call(d_src.data_ptr() + i * rows * cols * 3, cols * 3, rows, cols, 3, angles[i], 1, white, 1)
        dr, dc = sizes[i]
        assert exp.shape == (dr, dc, 3)
        assert (out[i, :dr, :dc * 3].reshape(dr, dc, 3) == exp).all(), (i, names[i], angles[i])
        assert (out[i, dr:] == 0x5A).all() and (out[i, :dr, dc * 3:] == 0x5A).all(), i


def test_chained_hough_batch_angles_into_rotate_batch():
    import torch
    rows, cols, n = 300, 420, 16
    imgs = [synth.make_card(rows, cols, 40 + i)[0] for i in range(n)]
    d = torch.from_numpy(np.stack(imgs)).cuda()
    angles, status, nl = omr.edges_detection_batch_device(d.data_ptr(), n, rows * cols, rows, cols, 1, cols, 60.0, 10.0)
    assert np.isfinite(angles).all() and len(set(angles.tolist())) > 4
    white = (255, 255, 255, 0)
    mr, mc, sizes = transfer.rotate_batch_canvas(rows, cols, angles, 1)
    d_dst = torch.full((n, mr, mc), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    transfer.rotate_batch_device_ex(d.data_ptr(), n, rows * cols, cols, rows, cols, 1, angles, 1.0, transfer.INTER_LINEAR,
                                    transfer.BORDER_CONSTANT, white, 1, d_dst.data_ptr(), mr * mc, mc, mr, mc)
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    for i in range(n):
        exp = _rotate_device_per_call(d.data_ptr() + i * rows * cols, cols, rows, cols, 1, angles[i], 1, white, 1)
        dr, dc = sizes[i]
        assert (out[i, :dr, :dc] == exp[:, :, 0]).all(), (i, angles[i])


def _host_single(a, angle, scale, flags, mode, clip):
    a = np.ascontiguousarray(a)
    rows, cols, cn = a.shape
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


def test_host_form_mixed_shapes_and_channels_land_at_their_positions():
    rng = np.random.default_rng(3)
    shapes = [(120, 161, 3), (64, 90, 1), (120, 161, 3), (33, 17, 4), (64, 90, 1), (5, 9, 2), (120, 161, 1), (64, 90, 1),
              (1, 1, 1), (120, 161, 3)]
    imgs = [_content(rng, *s) for s in shapes]
    angles = [7.3, -2.2, 0.0, 41.0, 0.05, -90.0, 3.3, 180.0, 12.0, -7.3]
    for flags, mode, clip, scale in ((1, 0, 1, 1.0), (0, 0, 0, 1.0), (2 | 16, wr.REFLECT, 1, 0.5), (4, wr.TRANSPARENT, 1, 1.0),
                                     (3, wr.WRAP, 0, 2.5)):
        got = transfer.rotate_batch_ex(imgs, angles, scale, flags, mode, BORDER, clip)
        assert len(got) == len(imgs)
        for i, a in enumerate(imgs):
            exp = _host_single(a, angles[i], scale, flags, mode, clip)
            g = got[i].matrix.reshape(exp.shape)
            assert (g == exp).all(), (i, shapes[i], flags, mode, clip, scale)
    # 2-D inputs come back 2-D, like rotate_mat's
    g = transfer.rotate_batch_ex([imgs[1][:, :, 0]], [5.0], 1.0, 1)[0].matrix
    assert g.ndim == 2 and (g == transfer.rotate_mat(imgs[1][:, :, 0], 5.0, 1.0, 1).matrix).all()


def test_more_images_than_one_launch_holds():
    """65537 angles for one 6 x 5 image (src_stride_bytes 0): the batch is cut at 65535 images per launch"""
    import torch
    rng = np.random.default_rng(8)
    a = _content(rng, 6, 5, 1)
    n = 65537
    angles = np.linspace(-180.0, 180.0, n)
    mr, mc, sizes = transfer.rotate_batch_canvas(6, 5, angles, 1)
    d_src = torch.from_numpy(a.reshape(-1).copy()).cuda()
    d_dst = torch.full((n, mr, mc), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = transfer.rotate_batch_device_ex(d_src.data_ptr(), n, 0, 5, 6, 5, 1, angles, 1.0, 1, 0, BORDER, 1, d_dst.data_ptr(),
                                          mr * mc, mc, mr, mc)
    torch.cuda.synchronize()
    assert (got == sizes).all()
    out = d_dst.cpu().numpy()
    for i in (0, 1, 30000, 65534, 65535, 65536):
        exp = _rotate_device_per_call(d_src.data_ptr(), 5, 6, 5, 1, angles[i], 1, BORDER, 1)
        dr, dc = sizes[i]
        assert (out[i, :dr, :dc] == exp[:, :, 0]).all(), i
        assert (out[i, dr:] == 0x5A).all() and (out[i, :dr, dc:] == 0x5A).all(), i


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_small_batches_on_both_sides_of_the_table_threshold(n):
    """up to 3 images are launched one by one, from 4 on through the table: the same bytes either way"""
    rng = np.random.default_rng(n)
    imgs = [_content(rng, 97, 131, 3) for _ in range(n)]
    for kind in ("packed", "dword", "padded"):
        lay = Layout(imgs, [7.3, -0.05, 0.0, -33.0][:n], 1, kind)
        for flags, mode in ((0, 0), (1, 0), (2, wr.REFLECT), (4 | 16, wr.TRANSPARENT)):
            lay.check(1.0, flags, mode)


def test_argument_errors_leave_the_device_usable():
    import torch
    rng = np.random.default_rng(12)
    imgs = [_content(rng, 60, 75, 3) for _ in range(4)]
    angles = [4.0, 0.0, -9.0, 0.05]
    lay = Layout(imgs, angles, 1, "dword")
    good = lay.check(1.0, 1, 0)
    b = (C.c_uint8 * 4)(*BORDER)
    d = lay.pattern.clone()
    torch.cuda.synchronize()

    def call(**kw):
        p = dict(src=lay.src_ptr(), n=lay.n, sstride=lay.sstride, sstep=lay.sstep, rows=lay.rows, cols=lay.cols, cn=lay.cn,
                 angles=lay.angles, scale=1.0, flags=1, mode=0, border=C.cast(b, _lib.u8p), clip=1, dst=d.data_ptr() + lay.do,
                 dstride=lay.dstride, dstep=lay.dstep, sr=lay.mr, sc=lay.mc)
        p.update(kw)
        ang = None if p["angles"] is None else np.asarray(p["angles"], np.float64)
        return _lib.lib().omr_rotate_batch_device_ex(
            C.c_void_p(p["src"]), p["n"], p["sstride"], p["sstep"], p["rows"], p["cols"], p["cn"],
            None if ang is None else ang.ctypes.data_as(_lib.f64p), p["scale"], p["flags"], p["mode"], p["border"], p["clip"],
            C.c_void_p(p["dst"]), p["dstride"], p["dstep"], p["sr"], p["sc"], None, None)

    refused = [(dict(flags=5), -213), (dict(flags=7 | 16), -213), (dict(flags=32), -5), (dict(mode=6), -5), (dict(mode=-1), -5),
               (dict(n=0), -5), (dict(angles=None), -5), (dict(angles=[1.0, float("nan"), 2.0, 3.0]), -5),
               (dict(angles=[1.0, 2.0, 3.0, float("inf")]), -5), (dict(sr=lay.mr - 1), -5), (dict(sc=lay.mc - 1), -5),
               (dict(dstep=lay.mc * 3 - 1), -5), (dict(dstride=lay.mr * lay.dstep - 1), -5), (dict(dst=lay.src_ptr()), -5),
               (dict(dst=lay.src_ptr() + 100), -5), (dict(border=None), -5), (dict(clip=2), -5), (dict(cn=5), -215)]
    for kw, code in refused:
        assert call(**kw) == code, kw
        torch.cuda.synchronize()
        assert torch.equal(d, lay.pattern), ("a refused call wrote", kw)
        # the device and the library are as they were: the valid call still gives the same block
        again, _ = lay.batch(1.0, 1, 0)
        assert torch.equal(again, good), kw
    with pytest.raises(_lib.OmrError):
        transfer.rotate_batch_ex(imgs, [1.0, float("nan"), 2.0, 3.0], 1.0, 1)
    assert (transfer.rotate_batch_ex(imgs, angles, 1.0, 1, 0, BORDER, 1)[1].matrix == imgs[1]).all()  # angle 0: the image


def test_fuzz_rotate_batch_slice(monkeypatch):
    """A fixed slice of tests/fuzz/fuzz_rotate_batch.py: random n, shapes, angles, flags, borders, channels, pitches."""
    import runpy
    tool = os.path.join(HERE, "fuzz", "fuzz_rotate_batch.py")
    monkeypatch.setattr(sys, "argv", [tool, "60", "7"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(tool, run_name="__main__")
    assert e.value.code == 0
