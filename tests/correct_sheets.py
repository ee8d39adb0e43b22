"""Sheets and CPU-oracle references for the correct_default batch tests (tests/test_gpu_correct_front.py,
tests/fuzz/fuzz_correct.py).

Content kinds, each chosen to make some front-end error visible:
  random    uniform bytes: every pixel's minimum and every area sum matters
  border    uniform bytes, the first and last three rows and columns black: a wrong 255 halo at the sheet border shows
  boundary  BGR triples whose gray value sits on the rounding boundary, (9798 b + 19235 g + 3735 r + 16384) mod 32768 in
            {0, 32767}: a swapped channel order or rounding constant shows (1 channel: uniform bytes)
  frame     uniform bytes inside a white frame 4 pixels wide: the eroded border rows and columns are the minimum of the
            frame and the 255 halo outside the sheet, so a wrong halo value shows
  card      synth.make_color_card (its gray for 1 channel): large flat regions, Believed by the projection
  bars      white, with two long light-gray lines (invisible to the threshold, found by Canny + HoughLinesP): not Believed,
            so it takes the Hough fallback; below 150 pixels it has no segment
  blank     white: no Hough segment, OMR_ERR_ASSERT (-215)
The oracle references are computed without the device's dispatch: front() restates omr.rs:88-126 (gray, erode x3,
INTER_AREA to the oracle.c:839-850 size), correct() composes omr.rs:339-448 from the oracle's parts."""
import numpy as np

from oics import synth

PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)  # lib.rs:192-205
KINDS = ("random", "border", "boundary", "frame", "card", "bars", "blank")

_BOUNDARY = None


def boundary_triples():
    """every (b, g, r) byte triple on the gray rounding boundary, [m, 3] u8"""
    global _BOUNDARY
    if _BOUNDARY is None:
        inv = pow(3735, -1, 32768)
        b, g = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
        b, g = b.ravel(), g.ravel()
        out = []
        for k in (0, 32767):
            r = ((k - 9798 * b - 19235 * g - 16384) * inv) % 32768
            ok = r < 256
            out.append(np.stack([b[ok], g[ok], r[ok]], axis=1))
        t = np.concatenate(out).astype(np.uint8)
        w = t.astype(np.int64)
        v = (9798 * w[:, 0] + 19235 * w[:, 1] + 3735 * w[:, 2] + 16384) % 32768
        assert np.isin(v, (0, 32767)).all() and len(t) > 1000
        _BOUNDARY = t
    return _BOUNDARY


def bars(rows, cols, rng):
    """white sheet with two long light-gray lines at random angles (gray, rows x cols)"""
    img = np.full((rows, cols), 255, np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for _ in range(2):
        a = np.deg2rad(rng.uniform(-25, 25))
        cy, cx = rng.uniform(0.3, 0.7) * rows, rng.uniform(0.3, 0.7) * cols
        length = rng.uniform(0.67, 0.87) * min(rows, cols) if min(rows, cols) > 250 else rng.uniform(165, 215)
        d = -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
        t = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a)
        img[(np.abs(d) < 1.5) & (np.abs(t) < length / 2)] = int(rng.integers(150, 215))
    return img


def sheet(kind, rows, cols, cn, seed):
    """one sheet of a content kind: [rows, cols] (cn = 1) or [rows, cols, 3] u8"""
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = (rows, cols) if cn == 1 else (rows, cols, cn)
    if kind in ("random", "border", "frame") or (kind == "boundary" and cn == 1):
        s = rng.integers(0, 256, shape, dtype=np.uint8)
        if kind == "border":
            s[:3], s[-3:], s[:, :3], s[:, -3:] = 0, 0, 0, 0
        elif kind == "frame":
            s[:4], s[-4:], s[:, :4], s[:, -4:] = 255, 255, 255, 255
        return s
    if kind == "boundary":
        t = boundary_triples()
        return np.ascontiguousarray(t[rng.integers(0, len(t), rows * cols)].reshape(rows, cols, 3))
    if kind == "blank":
        return np.full(shape, 255, np.uint8)
    if kind == "card":
        c = synth.make_color_card(rows, cols, seed % 100000, skew=float(rng.uniform(-20, 20)))[0]
    elif kind == "bars":
        g = bars(rows, cols, rng)
        c = np.ascontiguousarray(np.stack([g, g, g], axis=2))
    else:
        raise ValueError(kind)
    if cn == 1:
        from oracle import oracle as orc
        return orc.rgb2gray(c)
    return c


def proj_size(rows, cols, max_w, max_h):
    """(dr, dc): omr.rs:60-82, :114-126 (oracle.c:839-850)"""
    ws = 1.0 if max_w <= 0 else max_w / cols
    hs = 1.0 if max_h <= 0 else max_h / rows
    s = ws if ws < hs else hs
    return int(rows * s), int(cols * s)


def front(orc, s, dr, dc):
    """the projection-size image before the threshold: resize_area(erode_cross3(gray))"""
    gray = orc.rgb2gray(s) if s.ndim == 3 else s
    return orc.resize_area(orc.erode_cross3(gray), dr, dc)


def _rc_of(e):
    return int(str(e).split()[-1])


def correct(orc, s, params=PARAMS, want_image=True):
    """omr_correct_default from the oracle's parts -> (scan_rc, angle, need_check, canvas or None)"""
    ma, st, mw, mh, ml, mg = params
    try:
        pa, pst, pc = orc.get_result_from_projection(s, ma, st, mw, mh)
        if pst == 0:
            ang, chk = pa, False
        else:
            ea = orc.get_result_from_edges_detection(s, ml, mg)[0]
            ang, chk = orc.correct_default_decision(pa, pst, pc, ea)
    except RuntimeError as e:  # "oracle error <rc>": no Hough segment, or a projection size of 0 (-215)
        return _rc_of(e), None, None, None
    img = orc.rotate_mat(s, ang, 1.0, 0, (255, 255, 255, 0), 1) if want_image else None
    return 0, ang, chk, img


def layout(sheets, pitch_pad=0, guard_rows=0, offset=0, fill=0):
    """host sheets -> (flat u8 buffer, scan_stride, step): sheet i at offset + i * scan_stride, rows step apart; padding,
    guard rows and the bytes before offset hold `fill`"""
    a = np.asarray(sheets)
    n, rows, cols = a.shape[:3]
    cn = 1 if a.ndim == 3 else a.shape[3]
    step = cols * cn + pitch_pad
    stride = (rows + guard_rows) * step
    buf = np.full(offset + n * stride, fill, np.uint8)
    body = buf[offset:].reshape(n, rows + guard_rows, step)
    body[:, :rows, :cols * cn] = a.reshape(n, rows, cols * cn)
    return buf, stride, step


def odd_pad(cols, cn):
    """a row pad that makes the pitch larger than packed and not a multiple of 4"""
    return 5 if (cols * cn + 5) % 4 else 6
