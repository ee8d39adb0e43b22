"""omr_hough_angles_batch_device / omr_get_angles_with_hough_batch on the GPU.  All parity is bit for bit: the batch
against the per-call get_angle_with_hough (angle bits, -215 for a scan without a segment, segment counts, pictures byte
for byte), against the CPU oracle's Canny -> HoughLinesP -> hough.rs vote, and the vote-and-select kernel on its own
against a NumPy restatement in float32.

Shapes: 256 x 320 (rows x cols: two by three workgroups of the picture kernel, dword picture rows) and 200 x 253 (a
picture row of 759 bytes, scan and picture pitches and strides that are no multiple of 4).  The Hough parameters
(160, 5) were picked on the CPU oracle so that the seven scans of a batch hold a blank scan, a steeply rotated card with
one to three segments and at least four cards with two or more; the tests assert that mix from n_lines."""
import ctypes as C

import numpy as np
import pytest
import torch

from oics import _lib, hough, synth

pytestmark = pytest.mark.gpu

MLL, MLG = 160.0, 5.0
SHAPES = {"even": (256, 320), "odd": (200, 253)}
# (seed, skew): None = the card's own skew within +-9.5 degrees; "blank" = a white sheet
BATCH = ["blank", (47, 44.0), (42, None), (43, None), (44, None), (45, 30.0), (48, 35.0)]


def make_scan(rows, cols, cn, what):
    if what == "blank":
        g = np.full((rows, cols), 255, np.uint8)
    else:
        g = synth.make_card(rows, cols, what[0], what[1])[0]
    if cn == 1:
        return g
    rng = np.random.Generator(np.random.PCG64((0 if what == "blank" else what[0]) + 100))
    bgr = np.stack([g] * cn, axis=2).astype(np.int16)
    if what != "blank":
        bgr[:, :, :3] += rng.integers(-12, 13, size=(rows, cols, 3), dtype=np.int16)  # the channels differ: the max-channel rule
    return np.clip(bgr, 0, 255).astype(np.uint8)


_REF = {}


def reference(shape, cn, mll=MLL, mlg=MLG):
    """the batch's scans and, per scan, the per-call answer (angle or None, picture or None, segment count): computed
    once per (shape, channels, parameters) and shared by the tests"""
    key = (shape, cn, mll, mlg)
    if key not in _REF:
        rows, cols = SHAPES[shape]
        scans, per = [], []
        for what in BATCH:
            img = make_scan(rows, cols, cn, what)
            count = len(hough.hough_lines_p(hough.canny(img), 1.0, np.pi / 180.0, 0, mll, mlg))
            try:
                ang, pic = hough.get_angle_with_hough(img, mll, mlg, want_picture=True)
                assert hough.get_angle_with_hough(img, mll, mlg) == ang
            except _lib.OmrError as e:
                assert e.code == -215 and count == 0
                ang, pic = None, None
            scans.append(img)
            per.append((ang, pic, count))
        for a in scans:
            a.setflags(write=False)
        _REF[key] = (scans, per)
    return _REF[key]


def assert_mix(n_lines):
    """the batch cannot pass with every scan empty, or without the shapes of list the kernels treat differently"""
    n_lines = list(n_lines)
    blank = sum(1 for c in n_lines if c == 0)
    assert blank >= 1 and 3 * blank <= len(n_lines), n_lines
    assert any(1 <= c <= 3 for c in n_lines), n_lines
    assert sum(1 for c in n_lines if c >= 2) >= 4, n_lines


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def run_device(scans, cn, mll, mlg, pictures, odd_layout):
    """the device form on `scans` (one shape); returns angles, rc, n_lines and the whole picture buffer with its layout"""
    n = len(scans)
    rows, cols = scans[0].shape[:2]
    row = cols * cn
    step = row + (3 if odd_layout else 0)
    stride = rows * step + (5 if odd_layout else 0)
    base = 1 if odd_layout else 0
    host = np.full(base + n * stride, 0x5A, np.uint8)
    for i, a in enumerate(scans):
        v = host[base + i * stride: base + i * stride + rows * step].reshape(rows, step)
        v[:, :row] = a.reshape(rows, row)
    d = torch.from_numpy(host).to("cuda:0")
    lstep = 3 * cols + (4 if odd_layout else 8)
    lstride = rows * lstep + (7 if odd_layout else 16)
    lbase = 3 if odd_layout else 0
    out = torch.full((lbase + n * lstride + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ang, rc, nl = hough.hough_angles_batch_device(d.data_ptr() + base, n, stride, rows, cols, cn, step, mll, mlg,
                                                  d_lined=out.data_ptr() + lbase if pictures else None,
                                                  lined_stride_bytes=lstride, lined_step=lstep)
    assert np.array_equal(d.cpu().numpy(), host)  # the scans are read-only
    return ang, rc, nl, out.cpu().numpy(), (lbase, lstride, lstep)


def check_against_per_call(scans, per, cn, pictures, odd_layout, mll=MLL, mlg=MLG):
    ang, rc, nl, out, (lbase, lstride, lstep) = run_device(scans, cn, mll, mlg, pictures, odd_layout)
    rows, cols = scans[0].shape[:2]
    n = len(scans)
    assert nl.tolist() == [p[2] for p in per]
    for i, (e_ang, e_pic, count) in enumerate(per):
        if e_ang is None:
            assert rc[i] == -215 and ang[i] == 0.0 and bits(ang[i]) == 0, i
        else:
            assert rc[i] == 0 and bits(ang[i]) == bits(e_ang), (i, ang[i], e_ang)
    assert (out[:lbase] == 0xA5).all() and (out[lbase + n * lstride:] == 0xA5).all()
    for i, (e_ang, e_pic, count) in enumerate(per):
        slot = out[lbase + i * lstride: lbase + (i + 1) * lstride]
        if not pictures or e_ang is None:
            assert (slot == 0xA5).all(), "slot %d was written" % i  # no segment: no picture, as per call
            continue
        pic = slot[: rows * lstep].reshape(rows, lstep)
        assert np.array_equal(pic[:, : 3 * cols].reshape(rows, cols, 3), e_pic), (i, count)
        assert (pic[:, 3 * cols:] == 0xA5).all() and (slot[rows * lstep:] == 0xA5).all(), i
    return ang, rc, nl


@pytest.mark.parametrize("shape,cn", [("even", 1), ("even", 3), ("odd", 1), ("odd", 3)])
def test_device_form_is_the_per_call_form(shape, cn):
    scans, per = reference(shape, cn)
    assert_mix([p[2] for p in per])
    ang, rc, nl = check_against_per_call(scans, per, cn, True, shape == "odd")
    assert_mix(nl)
    # n = 1: a card with segments, the blank sheet
    for i in (2, 0):
        check_against_per_call(scans[i:i + 1], per[i:i + 1], cn, True, shape == "odd")


def test_device_form_with_many_segments_per_scan():
    """(60, 4): dozens of segments per card, crossing each other -- the pictures show the order of the packed list"""
    scans, per = reference("odd", 1, 60.0, 4.0)
    counts = [p[2] for p in per]
    assert counts[0] == 0 and sum(1 for c in counts if c >= 16) >= 4, counts
    check_against_per_call(scans, per, 1, True, True, 60.0, 4.0)


@pytest.mark.parametrize("shape,cn", [("even", 3), ("odd", 1)])
def test_without_pictures_the_angles_are_the_same(shape, cn):
    scans, per = reference(shape, cn)
    ang, rc, nl = check_against_per_call(scans, per, cn, False, shape == "odd")
    assert_mix(nl)
    ang1, rc1, nl1 = check_against_per_call(scans[3:4], per[3:4], cn, False, shape == "odd")
    assert rc1[0] == 0 and bits(ang1[0]) == bits(ang[3])


def vote_reference(a):
    """hough.rs:72-89 in float32: the first index with the most angles within 0.1 of it; -1 for an empty list"""
    a = np.asarray(a, np.float32)
    if len(a) == 0:
        return -1, None
    counts = np.zeros(len(a), np.int64)
    for lo in range(0, len(a), 512):
        d = np.abs(a[lo:lo + 512, None] - a[None, :])
        assert d.dtype == np.float32
        counts[lo:lo + 512] = (d < np.float32(0.1)).sum(axis=1)
    return int(np.argmax(counts)), counts  # argmax returns the first maximum


def test_vote_and_select_kernel_alone():
    """segment counts on both sides of a wavefront (63, 64, 65), of the 1024-angle LDS tile (1025) and several tiles
    with a partial last one (5000), an empty list first, in the middle and last, in one launch"""
    rng = np.random.Generator(np.random.PCG64(77))
    tenth = np.float32(0.1)
    sizes = [0, 1, 63, 64, 65, 0, 1025, 5000, 0]
    lists = []
    for k, m in enumerate(sizes):
        if k % 2:  # multiples of a tenth: many exact ties, and differences that round to either side of 0.1f
            a = (rng.integers(-449, 450, m).astype(np.float32) * tenth).astype(np.float32)
        else:      # clusters as a card gives them: some angles repeated exactly, the rest scattered
            a = rng.uniform(-45.0, 45.0, m).astype(np.float32)
            if m >= 8:
                a[rng.integers(0, m, m // 2)] = a[:4][rng.integers(0, 4, m // 2)]
        lists.append(a)
    # a list whose winner depends on the rounding of single differences: x, x + 0.1f and its two float neighbours
    x = np.float32(12.5)
    edge = np.array([x, x + tenth, np.nextafter(x + tenth, np.float32(0)), np.nextafter(x + tenth, np.float32(99)),
                     x - tenth, np.nextafter(x - tenth, np.float32(99)), np.float32(-30.0)], np.float32)
    lists.append(edge)
    sizes.append(len(edge))
    exp, tie_lists, below, at_or_above = [], 0, 0, 0
    for a in lists:
        w, counts = vote_reference(a)
        exp.append(w)
        if counts is not None and len(a) <= 1025:
            tie_lists += int((counts == counts.max()).sum() > 1 and len(a) > 1)
            d = np.abs(a[:, None] - a[None, :])
            below += int(((d < tenth) & (d >= np.nextafter(tenth, np.float32(0)) - np.float32(4e-6))).sum())
            at_or_above += int(((d >= tenth) & (d <= tenth + np.float32(4e-6))).sum())
    assert tie_lists >= 3 and below > 0 and at_or_above > 0  # first maxima matter; differences sit on both sides of 0.1f
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    flat = np.concatenate(lists).astype(np.float32)
    d_a = torch.from_numpy(flat).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    d_win = torch.full((len(lists),), -7, dtype=torch.int32, device="cuda:0")
    _lib.check(_lib.lib().omr_hough_vote_select_device(d_a.data_ptr(), d_off.data_ptr(), len(lists), d_win.data_ptr(), None))
    torch.cuda.synchronize()
    assert d_win.cpu().numpy().tolist() == exp
    # one list alone, and with an offset that is no multiple of 4 floats in front of it
    d_off2 = torch.from_numpy(np.array([off[6], off[7]], np.int32)).to("cuda:0")
    d_win2 = torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
    _lib.check(_lib.lib().omr_hough_vote_select_device(d_a.data_ptr(), d_off2.data_ptr(), 1, d_win2.data_ptr(), None))
    torch.cuda.synchronize()
    assert off[6] % 4 != 0 and d_win2.cpu().numpy().tolist() == [exp[6]]


def test_host_form_lands_every_result_at_its_own_index():
    a1, p_a1 = reference("even", 1)
    a3, p_a3 = reference("even", 3)
    b1, p_b1 = reference("odd", 1)
    b3, p_b3 = reference("odd", 3)
    picks = [(a1, p_a1, 2), (b3, p_b3, 3), (a1, p_a1, 0), (a3, p_a3, 4), (b1, p_b1, 4), (a1, p_a1, 5), (b3, p_b3, 0),
             (a3, p_a3, 1), (b1, p_b1, 2)]
    imgs = [s[i] for s, p, i in picks]
    per = [p[i] for s, p, i in picks]
    assert sum(1 for p in per if p[0] is None) == 2 and sum(1 for p in per if p[2] >= 2) >= 4
    for want_pictures in (True, False):
        got = hough.get_angles_with_hough(imgs, MLL, MLG, want_pictures=want_pictures)
        ang, rc = got[0], got[1]
        for i, (e_ang, e_pic, count) in enumerate(per):
            if e_ang is None:
                assert rc[i] == -215 and ang[i] == 0.0
                assert not want_pictures or got[2][i] is None
            else:
                assert rc[i] == 0 and bits(ang[i]) == bits(e_ang), i
                assert not want_pictures or np.array_equal(got[2][i], e_pic), i
    # a batch of one, and a row pitch wider than the row (a view into a larger image)
    wide = np.full((SHAPES["odd"][0], SHAPES["odd"][1] + 9), 7, np.uint8)
    wide[:, :SHAPES["odd"][1]] = b1[3]
    view = wide[:, :SHAPES["odd"][1]]
    im = _lib.OmrImage(view.ctypes.data, view.shape[0], view.shape[1], 1, view.strides[0])
    ang, rc = np.zeros(1), np.zeros(1, np.int32)
    pics = (_lib.OmrImageOwned * 1)()
    _lib.check(_lib.lib().omr_get_angles_with_hough_batch(C.byref(im), 1, MLL, MLG, ang.ctypes.data_as(_lib.f64p),
                                                          rc.ctypes.data_as(_lib.i32p), pics))
    assert rc[0] == 0 and bits(ang[0]) == bits(p_b1[3][0])
    assert np.array_equal(hough._take(pics[0]), p_b1[3][1])


@pytest.mark.parametrize("shape,cn", [("even", 1), ("odd", 3)])
def test_against_the_cpu_oracle(oracle, shape, cn):
    scans, per = reference(shape, cn)
    ang, rc, nl, _, _ = run_device(scans, cn, MLL, MLG, False, shape == "odd")
    assert_mix(nl)
    for i, img in enumerate(scans):
        edges = oracle.canny(img, 50.0, 150.0)
        lines = oracle.hough_lines_p(edges, MLL, MLG)
        assert nl[i] == len(lines), i
        if len(lines) == 0:
            assert rc[i] == -215
            continue
        e_ang, e_n = oracle.get_angle_with_hough(img, MLL, MLG)
        assert e_n == len(lines) and rc[i] == 0 and bits(ang[i]) == bits(e_ang), (i, ang[i], e_ang)
