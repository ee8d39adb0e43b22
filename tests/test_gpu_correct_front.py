"""correct_default for batches of sheets (omr_correct_batch_*, omr_correct_default_batch) against the CPU oracle.

The front end: omr_correct_batch_front_device's projection-size images equal, byte for byte,
oracle.resize_area(oracle.erode_cross3(gray)) at the oracle.c:839-850 size, for every branch of the dispatch
(asserted through omr_correct_batch_info) with 3 channels and 1, on content that makes halo, rounding and channel-order
errors visible (tests/correct_sheets.py), in padded layouts at an odd base address.
End to end: scan_rc, the angle's f64 bits, need_check, the canvas size and every canvas byte equal the oracle's
composition of omr.rs:339-448 (projection result, edges result, correct_default_decision, rotate_mat NEAREST CONTAIN),
not the per-call GPU function."""
import os
import struct
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oics import _lib, omr
from oics._lib import OmrError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import correct_sheets as cs  # noqa: E402
import dataset_pin as dp  # noqa: E402

PARAMS = cs.PARAMS
WORKERS = min(16, os.cpu_count() or 1)
SENTINEL = 0xA5


def _bits(x):
    return struct.pack("<d", float(x)).hex()


def _pmap(fn, items):
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        return list(ex.map(fn, items))


def _upload(buf):
    import torch
    d = torch.from_numpy(buf).to("cuda:0")
    torch.cuda.synchronize()
    return d


def _front_images(cb, sheets, pitch_pad, guard_rows, offset):
    """front_device on the sheets laid out as asked -> [n] projection-size images; the bytes around them untouched"""
    import torch
    n = len(sheets)
    dr, dc = cb.info()[:2]
    buf, stride, step = cs.layout(sheets, pitch_pad, guard_rows, offset)
    d = _upload(buf)
    sstep = dc + 3
    sstride = dr * sstep + 7
    out = torch.full((n * sstride + 1,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cb.front_device(d.data_ptr() + offset, stride, step, n, out.data_ptr() + 1, sstride, sstep)
    host = out.cpu().numpy()
    assert host[0] == SENTINEL
    slots = host[1:].reshape(n, sstride)
    assert (slots[:, dr * sstep:] == SENTINEL).all()
    grid = slots[:, :dr * sstep].reshape(n, dr, sstep)
    assert (grid[:, :, dc:] == SENTINEL).all()
    return [grid[i, :, :dc] for i in range(n)]


def _check_front(oracle, cb, sheets, dr, dc, pitch_pad=0, guard_rows=0, offset=0):
    got = _front_images(cb, sheets, pitch_pad, guard_rows, offset)
    exp = _pmap(lambda s: cs.front(oracle, s, dr, dc), sheets)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert e.shape == (dr, dc)
        if not np.array_equal(g, e):
            ys, xs = np.nonzero(g != e)
            pytest.fail("sheet %d: %d of %d bytes differ, first at (%d, %d): %d, oracle %d"
                        % (i, len(ys), g.size, ys[0], xs[0], g[ys[0], xs[0]], e[ys[0], xs[0]]))


def _sheets(kinds, rows, cols, cn, n, seed):
    return _pmap(lambda i: cs.sheet(kinds[i % len(kinds)], rows, cols, cn, seed + i), range(n))


FUSED, INT, GENERAL, LINEAR = omr.FRONT_AREA_FUSED, omr.FRONT_AREA_INT, omr.FRONT_AREA_GENERAL, omr.FRONT_LINEAR

# (rows, cols, max_w, max_h) -> (dr, dc, mode, kx, ky)
BRANCHES = [
    ((17, 257, 257, 17), (17, 257, FUSED, 1, 1)),        # identity; one column into a second 256-wide tile
    ((33, 513, 513, 33), (33, 513, FUSED, 1, 1)),        # identity; one row into a third 16-row tile
    ((460, 496, 248, 230), (230, 248, FUSED, 2, 2)),     # (sum + 2) >> 2
    ((462, 258, 129, 231), (231, 129, FUSED, 2, 2)),     # (sum + 2) >> 2, partial last tiles (dc % 128 = 1)
    ((690, 744, 248, 230), (230, 248, FUSED, 3, 3)),     # rintf(sum / 9), THo clamped to 16
    ((18, 1240, 248, 230), (3, 248, FUSED, 5, 6)),       # kx != ky
    ((5, 1240, 248, 230), (1, 248, FUSED, 5, 5)),        # one output row
    ((1088, 1088, 64, 64), (64, 64, FUSED, 17, 17)),     # TWo = 15, THo = 3
    ((1024, 1024, 16, 16), (16, 16, FUSED, 64, 64)),     # THo = 1, TWo = 4
    ((2048, 128, 4, 32), (32, 2, FUSED, 64, 64)),        # the largest fused factors, two output columns
    ((700, 40, 10, 20), (20, 1, FUSED, 40, 35)),         # one output column
    ((1280, 1280, 16, 16), (16, 16, INT, 80, 80)),       # beyond the fused kernel
    ((300, 320, 5, 300), (4, 5, INT, 64, 75)),           # one factor on each side of the limit
    ((1754, 1240, 248, 230), (230, 162, GENERAL, 0, 0)),  # resizeArea_ tap tables
    ((1150, 1241, 248, 230), (229, 248, GENERAL, 0, 0)),
    ((1089, 1088, 64, 64), (64, 63, GENERAL, 0, 0)),
    ((120, 100, 248, 230), (230, 191, LINEAR, 0, 0)),    # enlargement (quirk B7)
]
FRONT_KINDS = ("random", "border", "boundary", "frame", "card")


@pytest.mark.parametrize("cn", [3, 1])
@pytest.mark.parametrize("shape,expect", BRANCHES, ids=["%dx%d-%dx%d" % b[0] for b in BRANCHES])
def test_front_end_branch_against_the_oracle(oracle, shape, expect, cn):
    """Every byte of every sheet's projection-size image, in a layout with an odd row pitch, guard rows and an odd base
    address, after asserting the branch the context takes."""
    rows, cols, mw, mh = shape
    assert cs.proj_size(rows, cols, mw, mh) == expect[:2]
    cb = omr.CorrectBatch(rows, cols, cn, 45, 0.2, mw, mh, 150.0, 50.0, max_scans=5)
    assert cb.info() == expect
    sheets = _sheets(FRONT_KINDS, rows, cols, cn, 5, 7 * rows + cols + cn)
    _check_front(oracle, cb, sheets, expect[0], expect[1], cs.odd_pad(cols, cn), 3, 1)
    cb.close()


@pytest.mark.parametrize("shape,expect", [
    ((60, 50, 19, 23), (22, 19, GENERAL, 0, 0)),
    ((130, 130, 2, 2), (2, 2, INT, 65, 65)),
    ((60, 50, 248, 230), (230, 191, LINEAR, 0, 0)),
], ids=["general", "int", "linear"])
def test_front_end_more_than_one_chunk(oracle, shape, expect):
    """300 sheets: the full-size modes go through their 256-sheet chunk loop twice."""
    rows, cols, mw, mh = shape
    cb = omr.CorrectBatch(rows, cols, 3, 45, 0.2, mw, mh, 150.0, 50.0, max_scans=320)
    assert cb.info() == expect
    sheets = _sheets(FRONT_KINDS, rows, cols, 3, 300, 40000 + rows)
    _check_front(oracle, cb, sheets, expect[0], expect[1], 0, 1, 1)
    cb.close()


def test_front_device_rejects_bad_arguments():
    import torch
    cb = omr.CorrectBatch(460, 496, 3, *PARAMS, max_scans=2)
    dr, dc = cb.info()[:2]
    d = torch.zeros(2 * 460 * 496 * 3, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(2 * dr * dc, dtype=torch.uint8, device="cuda:0")
    p, q, st, sp = d.data_ptr(), out.data_ptr(), 460 * 496 * 3, 496 * 3
    for args in ((p, st, sp, 2, q, dr * (dc - 1), dc - 1),  # small_step < proj_cols
                 (p, st, sp, 2, q, dr * dc - 1, dc),        # small_stride < proj_rows x small_step
                 (p, st, sp, 2, None, dr * dc, dc),         # no output
                 (p, st, sp, 3, q, dr * dc, dc),            # n > max_scans
                 (p, st, sp, 0, q, dr * dc, dc),
                 (p, st, sp - 1, 2, q, dr * dc, dc),        # step < cols x channels
                 (p, st - 1, sp, 2, q, dr * dc, dc),        # scan stride < rows x step
                 (None, st, sp, 2, q, dr * dc, dc)):
        with pytest.raises(OmrError) as e:
            cb.front_device(*args)
        assert e.value.code == -5, args
    cb.front_device(p, st, sp, 2, q, dr * dc, dc)  # the smallest valid layout
    cb.close()


# ---- end to end ---------------------------------------------------------------------------------------------------
def _run_device(cb, sheets, pitch_pad=0, guard_rows=0, offset=0):
    """run_device with canvases -> (angles, need_check, scan_rc, sizes, [canvas or None]); every slot's bytes outside its
    canvas are left as they were"""
    import torch
    n = len(sheets)
    buf, stride, step = cs.layout(sheets, pitch_pad, guard_rows, offset)
    d = _upload(buf)
    R, Cc = cb.canvas
    cn = cb.channels
    out_step = Cc * cn + 9
    out_stride = out_step * (R + 1)
    out = torch.full((n, out_stride), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ang, chk, rc, size = cb.run_device(d.data_ptr() + offset, stride, step, n, out.data_ptr(), out_stride, out_step)
    host = out.cpu().numpy()
    canv = []
    for i in range(n):
        slot = host[i].reshape(R + 1, out_step)
        r, c = size[i]
        assert (slot[r:] == 7).all() and (slot[:, c * cn:] == 7).all(), i
        canv.append(slot[:r, :c * cn].reshape((r, c) if cn == 1 else (r, c, cn)) if rc[i] == 0 else None)
    return ang, chk, rc, size, canv


def _check_against_oracle(oracle, sheets, res, params=PARAMS):
    ang, chk, rc, size, canv = res
    exp = _pmap(lambda s: cs.correct(oracle, s, params), sheets)
    for i, (erc, ea, ec, eimg) in enumerate(exp):
        assert rc[i] == erc, (i, rc[i], erc)
        if erc:
            assert tuple(size[i]) == (0, 0) and canv[i] is None, i
            continue
        assert _bits(ang[i]) == _bits(ea) and bool(chk[i]) == ec, (i, ang[i], ea, chk[i], ec)
        assert canv[i].shape == eimg.shape, (i, canv[i].shape, eimg.shape)
        assert np.array_equal(canv[i], eimg), (i, int((canv[i] != eimg).sum()))
    return exp


def _mixed(rows, cols, cn, n, seed):
    kinds = ["card", "bars", "bars"]
    s = _sheets(kinds, rows, cols, cn, n, seed)
    s[n // 2] = cs.sheet("blank", rows, cols, cn, 0)
    return s


@pytest.mark.parametrize("cn", [3, 1])
def test_device_form_mixed_batch(oracle, cn):
    """Believed cards, sheets that take the Hough fallback and a blank sheet (-215), from an odd base address with an odd
    row pitch: every result equals the oracle's composition."""
    sheets = _mixed(230, 248, cn, 45, 500 + cn)
    cb = omr.CorrectBatch(230, 248, cn, *PARAMS, max_scans=48)
    exp = _check_against_oracle(oracle, sheets, _run_device(cb, sheets, cs.odd_pad(248, cn), 2, 1))
    cb.close()
    assert exp[len(sheets) // 2][0] == -215 and sum(1 for e in exp if e[0] == 0) == len(sheets) - 1
    assert len({_bits(e[1]) for e in exp if e[0] == 0}) >= 20  # varied decisions
    assert {e[2] for e in exp if e[0] == 0} == {False, True}


def test_two_hough_chunks(oracle):
    """300 sheets that are not Believed among 310: the Hough pass runs twice (256 + 44) and both warp phases run."""
    rows, cols = 230, 248
    sheets = _sheets(["bars"] * 30 + ["card"], rows, cols, 3, 310, 9000)
    cb = omr.CorrectBatch(rows, cols, 3, *PARAMS, max_scans=310)
    exp = _check_against_oracle(oracle, sheets, _run_device(cb, sheets))
    cb.close()
    assert sum(1 for i in range(310) if i % 31 != 30) == 300
    assert sum(1 for e in exp if e[0] == 0) >= 290


def test_dataset_cases_against_the_oracle(oracle):
    """The 10 Hough cases of the dataset pin and 20 Believed ones, one context per sheet shape: decisions and canvases
    against the oracle."""
    exp = dp.load_expected()["cases"]
    hough = [c for c in exp if c["proj_status"] != 0]
    believed = [c for c in exp if c["proj_status"] == 0][::47][:20]
    cases = hough + believed
    assert len(hough) == 10 and len(believed) == 20

    def prepare(c):
        return dp.inject(dp.imread_color(c["sheet"]), c["idx"] * 0.1, oracle)

    sheets = _pmap(prepare, cases)
    by_shape = {}
    for j, s in enumerate(sheets):
        by_shape.setdefault(s.shape, []).append(j)
    for shape, js in by_shape.items():
        cb = omr.CorrectBatch(shape[0], shape[1], 3, *PARAMS, max_scans=len(js))
        sub = [sheets[j] for j in js]
        res = _run_device(cb, sub)
        _check_against_oracle(oracle, sub, res)
        for t, j in enumerate(js):  # and the committed expectations
            assert _bits(res[0][t]) == cases[j]["angle_bits"] and bool(res[1][t]) == cases[j]["need_check"]
        cb.close()


def _host_batch(images, want_image=True):
    """omr_correct_default_batch on [(array of rows x step bytes, rows, cols, cn)] -> [(rc, angle, need_check, image)]"""
    from oics.hough import _take
    L = omr.lib()
    n = len(images)
    arr = (_lib.OmrImage * n)(*[_lib.OmrImage(a.ctypes.data, r, c, cn, a.strides[0]) for a, r, c, cn in images])
    ang = np.zeros(n, np.float64)
    chk = np.zeros(n, np.int32)
    rc = np.zeros(n, np.int32)
    owned = (_lib.OmrImageOwned * n)() if want_image else None
    ma, st, mw, mh, ml, mg = PARAMS
    assert L.omr_correct_default_batch(arr, n, ma, st, mw, mh, ml, mg, ang.ctypes.data_as(_lib.f64p),
                                       chk.ctypes.data_as(_lib.i32p), rc.ctypes.data_as(_lib.i32p), owned) == 0
    imgs = [_take(owned[i]) if want_image and owned[i].data else None for i in range(n)]
    return [(int(rc[i]), float(ang[i]), bool(chk[i]), imgs[i]) for i in range(n)]


def _pitched(s, pad):
    """a host image with rows `pad` bytes longer than packed"""
    rows, cols = s.shape[:2]
    cn = 1 if s.ndim == 2 else s.shape[2]
    buf = np.full((rows, cols * cn + pad), 0, np.uint8)
    buf[:, :cols * cn] = s.reshape(rows, cols * cn)
    return buf, rows, cols, cn


def test_host_form_against_the_oracle(oracle):
    """omr_correct_default_batch: six shapes in one call (more than the 4 kept contexts), one bucket of 270 sheets
    (two runs of at most 256), padded rows, and a repeat call that gives the same results."""
    rng = np.random.Generator(np.random.PCG64(77))
    shapes = [(230, 248, 3), (460, 496, 3), (231, 249, 1), (300, 200, 3), (120, 100, 3), (690, 744, 1)]
    sheets = []
    for k, (r, c, cn) in enumerate(shapes):
        sheets += _sheets(["card", "bars"], r, c, cn, 3, 6000 + 10 * k)
    sheets += _sheets(["bars", "card", "bars"], 230, 248, 3, 266, 7000)  # the first shape: 3 + 266 + 1 sheets
    sheets.append(cs.sheet("blank", 230, 248, 3, 0))
    order = rng.permutation(len(sheets))
    sheets = [sheets[i] for i in order]
    assert sum(1 for s in sheets if s.shape == (230, 248, 3)) == 270
    images = [_pitched(s, int(rng.integers(0, 4)) * 3 if i % 2 else 0) for i, s in enumerate(sheets)]
    assert any(a.strides[0] > c * cn for a, r, c, cn in images)
    got = _host_batch(images)
    exp = _pmap(lambda s: cs.correct(oracle, s), sheets)
    for i, ((rc, a, chk, img), (erc, ea, ec, eimg)) in enumerate(zip(got, exp)):
        assert rc == erc, (i, rc, erc)
        if erc:
            assert img is None, i
            continue
        assert _bits(a) == _bits(ea) and chk == ec, (i, a, ea, chk, ec)
        assert img.shape == eimg.shape and np.array_equal(img, eimg), i
    again = _host_batch(images)
    for (rc, a, chk, img), (rc2, a2, chk2, img2) in zip(got, again):
        assert (rc, _bits(a), chk) == (rc2, _bits(a2), chk2)
        assert (img is None and img2 is None) or np.array_equal(img, img2)


def test_fuzz_correct_slice(oracle, monkeypatch):
    """A fixed slice of tests/fuzz/fuzz_correct.py: random shapes and factors, 1 or 3 channels, padding and content
    kinds; front-end images and decisions against the oracle."""
    import runpy
    tool = os.path.join(HERE, "fuzz", "fuzz_correct.py")
    monkeypatch.setattr(sys, "argv", [tool, "100", "3"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(tool, run_name="__main__")
    assert e.value.code == 0
