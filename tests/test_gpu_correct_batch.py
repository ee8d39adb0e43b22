"""correct_default for batches of sheets on the device: omr_correct_batch_run_device / omr_correct_default_batch.

The contract is the per-call function: for every sheet, rotate_angle (as f64 bits), need_check, scan_rc and the rotated
canvas (size and every byte) equal omr_correct_default's.  Covered: the dataset pin (936 cases of several sheet shapes,
10 of them through the Hough fallback) against the committed expectations; colour and gray sheets with a fractional shrink, with a row pitch and
a scan stride larger than packed; sheets that enlarge (quirk B7); a blank sheet in the middle of a batch; d_out = NULL;
context reuse; the host-image entry point over two interleaved shapes."""
import os
import struct
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oics import omr, synth
from oics._lib import OmrError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_pin as dp  # noqa: E402

PARAMS = dp.PARAMS  # (45, 0.2, 248, 230, 150.0, 50.0), lib.rs:192-205


def _bits(x):
    return struct.pack("<d", float(x)).hex()


def _per_call(img, params=PARAMS, want_image=True):
    """omr_correct_default -> (rc, angle, need_check, image)"""
    try:
        a, c, im = omr.correct_default(img, *params, want_image=want_image)
        return 0, a, c, im
    except OmrError as e:
        return e.code, None, None, None


def _to_device(sheets, pitch_pad=0, stride_pad_rows=0):
    """host sheets [n, rows, cols(, cn)] -> (tensor, ptr, scan_stride, step) with the given padding"""
    import torch
    a = np.asarray(sheets)
    n, rows, cols = a.shape[:3]
    cn = 1 if a.ndim == 3 else a.shape[3]
    step = cols * cn + pitch_pad
    buf = np.zeros((n, rows + stride_pad_rows, step), np.uint8)
    buf[:, :rows, :cols * cn] = a.reshape(n, rows, cols * cn)
    d = torch.from_numpy(buf).to("cuda:0")
    torch.cuda.synchronize()
    return d, d.data_ptr(), (rows + stride_pad_rows) * step, step


def _run(cb, sheets, want_image=True, pitch_pad=0, stride_pad_rows=0):
    """run a batch -> (angles, need_check, scan_rc, sizes, canvases or None)"""
    import torch
    n = len(sheets)
    d, ptr, stride, step = _to_device(sheets, pitch_pad, stride_pad_rows)
    R, Cc = cb.canvas
    cn = cb.channels
    if want_image:
        out_step = Cc * cn + 32 * want_image
        out_stride = out_step * (R + 1)
        out = torch.full((n, out_stride), 7, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ang, chk, rc, size = cb.run_device(ptr, stride, step, n, out.data_ptr(), out_stride, out_step)
        host = out.cpu().numpy()
        canv = []
        for i in range(n):
            r, c = size[i]
            slot = host[i].reshape(R + 1, out_step)
            canv.append(slot[:r, :c * cn].reshape((r, c) if cn == 1 else (r, c, cn)) if rc[i] == 0 else None)
    else:
        ang, chk, rc, size = cb.run_device(ptr, stride, step, n)
        canv = None
    del d
    return ang, chk, rc, size, canv


def _compare(sheets, res, params=PARAMS, check_images=True):
    ang, chk, rc, size, canv = res
    for i, s in enumerate(sheets):
        erc, ea, ec, eimg = _per_call(s, params, want_image=check_images)
        assert rc[i] == erc, (i, rc[i], erc)
        if erc != 0:
            assert tuple(size[i]) == (0, 0), (i, size[i])
            continue
        assert _bits(ang[i]) == _bits(ea) and bool(chk[i]) == ec, (i, ang[i], ea, chk[i], ec)
        if check_images and canv is not None:
            assert canv[i].shape == eimg.shape, (i, canv[i].shape, eimg.shape)
            assert np.array_equal(canv[i], eimg), (i, int((canv[i] != eimg).sum()))


def _inject_cases(cases, oracle):
    by_sheet = {}
    for k, c in enumerate(cases):
        by_sheet.setdefault(c["sheet"], []).append((k, c))

    def prepare(item):
        name, cs = item
        bgr = dp.imread_color(name)
        return [(k, dp.inject(bgr, c["idx"] * 0.1, oracle)) for k, c in cs]

    out = [None] * len(cases)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        for batch in ex.map(prepare, sorted(by_sheet.items())):
            for k, x in batch:
                out[k] = x
    return out


def test_dataset_pin_through_the_batch(oracle):
    """All 936 cases, in three parts, each bucketed by sheet shape into one context per shape (most calls carry an n that
    is not a multiple of 64): every angle_bits / need_check equals the committed expectations; then all 10 Hough cases
    and 30 Believed ones again with canvases, against omr_correct_default's images."""
    exp = dp.load_expected()["cases"]
    assert len(exp) == 936
    ctx = {}
    mism, got = [], {}
    hough = [k for k, c in enumerate(exp) if c["proj_status"] != 0]
    assert len(hough) == 10
    believed = [k for k, c in enumerate(exp) if c["proj_status"] == 0][::31][:30]
    keep = set(hough) | set(believed)
    kept = {}
    for lo, hi in ((0, 300), (300, 600), (600, 936)):
        cases = exp[lo:hi]
        sheets = _inject_cases(cases, oracle)
        shapes = {}
        for j, x in enumerate(sheets):
            shapes.setdefault(x.shape, []).append(j)
        for shape, js in shapes.items():
            if shape not in ctx:
                ctx[shape] = omr.CorrectBatch(shape[0], shape[1], 3, *PARAMS, max_scans=336)
            ang, chk, rc, _, _ = _run(ctx[shape], [sheets[j] for j in js], want_image=False)
            for t, j in enumerate(js):
                c = cases[j]
                assert rc[t] == 0, (c["sheet"], c["idx"])
                got[lo + j] = (ang[t], chk[t])
                if _bits(ang[t]) != c["angle_bits"] or bool(chk[t]) != c["need_check"]:
                    mism.append((c["sheet"], c["idx"], ang[t], c["angle"], bool(chk[t]), c["need_check"]))
                if lo + j in keep:
                    kept[lo + j] = sheets[j]
    assert len(got) == 936
    assert not mism, mism[:5]
    by_shape = {}
    for k in sorted(keep):
        by_shape.setdefault(kept[k].shape, []).append(k)
    for shape, ks in by_shape.items():
        sub = [kept[k] for k in ks]
        res = _run(ctx[shape], sub, want_image=True)
        for j, k in enumerate(ks):  # d_out makes no difference to the decisions
            assert _bits(res[0][j]) == _bits(got[k][0]) and res[1][j] == got[k][1]
        _compare(sub, res)
    for cb in ctx.values():
        cb.close()


def _cards(rows, cols, n, seed0, skews):
    return [synth.make_color_card(rows, cols, seed0 + i, skew=skews[i % len(skews)])[0] for i in range(n)]


def test_fractional_shrink_colour_and_gray_with_padded_layout(oracle):
    """A4 1754 x 1240 (scale 0.1311: resizeArea_'s tap tables), 3 channels and 1, row pitch and scan stride larger than
    packed: every sheet equals the per-call function (angle bits, need_check, canvas)."""
    skews = [2.4, -7.3, 0.0, 11.1, -0.6, 33.3, -44.0, 5.05]
    cards = _cards(1754, 1240, 12, 100, skews)
    cb = omr.CorrectBatch(1754, 1240, 3, *PARAMS, max_scans=16)
    _compare(cards, _run(cb, cards, pitch_pad=36, stride_pad_rows=5))
    cb.close()
    gray = [oracle.rgb2gray(c) for c in cards[:7]]
    cb1 = omr.CorrectBatch(1754, 1240, 1, *PARAMS, max_scans=8)
    _compare(gray, _run(cb1, gray, pitch_pad=12, stride_pad_rows=2))
    cb1.close()


def test_enlarging_sheets():
    """120 x 100 sheets against 248 x 230: the resize enlarges (quirk B7, the bilinear kernel)."""
    cards = _cards(120, 100, 6, 300, [1.2, -3.0, 8.8])
    cb = omr.CorrectBatch(120, 100, 3, *PARAMS, max_scans=6)
    _compare(cards, _run(cb, cards))
    cb.close()


def test_blank_sheet_in_the_middle_and_context_reuse():
    """A blank sheet gets scan_rc -215 and 0 x 0, its neighbours equal the per-call function; runs of different n on one
    context, and a run after an argument error, equal a fresh context."""
    cards = _cards(1150, 1240, 9, 500, [3.3, -1.7, 0.4, 9.9])
    blank = np.full((1150, 1240, 3), 255, np.uint8)
    sheets = cards[:4] + [blank] + cards[4:]
    cb = omr.CorrectBatch(1150, 1240, 3, *PARAMS, max_scans=10)
    res = _run(cb, sheets)
    assert res[2][4] == -215 and tuple(res[3][4]) == (0, 0)
    _compare(sheets, res)
    # a smaller run, then an argument error (n above max_scans), then the first run again
    small = _run(cb, sheets[2:5])
    for j in range(3):
        assert _bits(small[0][j]) == _bits(res[0][2 + j]) and small[2][j] == res[2][2 + j]
    with pytest.raises(OmrError) as e:
        _run(cb, sheets + sheets[:2], want_image=False)
    assert e.value.code == -5
    again = _run(cb, sheets)
    fresh_cb = omr.CorrectBatch(1150, 1240, 3, *PARAMS, max_scans=10)
    fresh = _run(fresh_cb, sheets)
    for a, b in ((again, res), (fresh, res)):
        assert [_bits(x) for x in a[0]] == [_bits(x) for x in b[0]]
        assert (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all()
        for x, y in zip(a[4], b[4]):
            assert (x is None and y is None) or np.array_equal(x, y)
    cb.close()
    fresh_cb.close()


def test_host_batch_two_interleaved_shapes():
    """omr_correct_default_batch over sheets of two shapes, interleaved, one of them blank: per position the per-call
    results and images."""
    a = _cards(1150, 1240, 4, 700, [2.0, -4.5])
    b = _cards(640, 452, 4, 800, [-1.1, 6.6])
    sheets = [x for pair in zip(a, b) for x in pair]
    sheets.insert(3, np.full((640, 452, 3), 255, np.uint8))
    out = omr.correct_default_batch(sheets, *PARAMS)
    assert len(out) == len(sheets)
    for i, s in enumerate(sheets):
        erc, ea, ec, eimg = _per_call(s)
        ang, chk, img, rc = out[i]
        assert rc == erc, (i, rc, erc)
        if erc:
            assert img is None
            continue
        assert _bits(ang) == _bits(ea) and chk == ec, (i, ang, ea)
        assert img.shape == eimg.shape and np.array_equal(img, eimg), i
    nod = omr.correct_default_batch(sheets, *PARAMS, want_image=False)
    assert [(_bits(x[0]), x[1], x[3]) for x in nod] == [(_bits(x[0]), x[1], x[3]) for x in out]


@pytest.mark.parametrize("rows,cols,cn,params", [
    (460, 496, 3, PARAMS),                            # factor 2 on both axes: the (sum + 2) >> 2 rounding, BGR weights fused
    (230, 248, 3, PARAMS),                            # the projection size is the sheet's: no resize (identity)
    (1150, 1240, 1, PARAMS),                          # factor 5, 1 channel through the fused kernel
    (18, 1240, 3, PARAMS),                            # factors 5 across and 6 down (kx != ky)
    (1280, 1280, 3, (45, 0.2, 16, 16, 150.0, 50.0)),  # factor 80: beyond the fused kernel, the per-call resize per sheet
])
def test_front_end_branches(oracle, rows, cols, cn, params):
    """Every branch of the front end against the per-call function: angle bits, need_check, scan_rc, canvas."""
    cards = _cards(rows, cols, 5, 1000 + rows, [2.2, -6.4, 0.0, 17.5, -31.0])
    if cn == 1:
        cards = [oracle.rgb2gray(c) for c in cards]
    cb = omr.CorrectBatch(rows, cols, cn, *params, max_scans=5)
    _compare(cards, _run(cb, cards), params)
    cb.close()


def test_host_batch_sheet_without_projection_size():
    """A sheet whose projection size truncates to 0 rows fails alone with -215, as per call; the others stand."""
    a = _cards(460, 496, 2, 1100, [3.0, -2.0])
    tiny = _cards(3, 1240, 1, 1200, [0.0])[0]
    sheets = [a[0], tiny, a[1]]
    out = omr.correct_default_batch(sheets, *PARAMS)
    assert _per_call(tiny)[0] == -215 and out[1][3] == -215 and out[1][2] is None
    for i in (0, 2):
        erc, ea, ec, eimg = _per_call(sheets[i])
        assert out[i][3] == erc == 0 and _bits(out[i][0]) == _bits(ea) and out[i][1] == ec
        assert np.array_equal(out[i][2], eimg)
