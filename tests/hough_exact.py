"""The Hough-line path from first principles, for holding the kernels and both restatements (oracle/oracle_hough.c,
oracle_np.canny_np / hough_lines_p_py) to something that was not read off OpenCV's source: numpy and scipy only,
nothing from oracle/ and nothing from the library.

  canny()           Canny from its definition, byte-exact (the fixed-point sector test of the kernel equals the sector
                    of the true angle for every gradient an 8-bit image can give: sector_fixed / sector_exact,
                    enumerated in tests/test_hough_exact.py)
  check_segments()  P1-P5: what every HoughLinesP answer satisfies whatever its random draws were
  line_angles() / vote_hough_rs() / vote_omr_rs() / check_vote()
                    hough.rs:50-89 and omr.rs:231-302 in float64, and the check of a float32 answer against them
  strips() / truth_bound()
                    two-level images of straight strips at one known angle, and how far from it the detector may land

What stays unpinned: which segments the progressive probabilistic transform returns (its random draws decide), and
OpenCV's tie convention of the non-maximum test (stated in canny())."""
import math

import numpy as np
from scipy import ndimage

TAN_22_5 = math.tan(math.pi / 8)
TAN_67_5 = math.tan(3 * math.pi / 8)


# ---- direction sectors ---------------------------------------------------------------------------------------------
def sector_exact(ax, ay):
    """0 horizontal, 1 diagonal, 2 vertical, from exact float64 tangents of 22.5 and 67.5 degrees; ax = |gx|, ay = |gy|
    (tan 22.5 = sqrt(2) - 1 is irrational: no integer pair lies on a boundary)"""
    ax, ay = np.asarray(ax, np.float64), np.asarray(ay, np.float64)
    return np.where(ay < TAN_22_5 * ax, 0, np.where(ay > TAN_67_5 * ax, 2, 1))


def sector_atan2(ax, ay):
    """the same from the angle itself"""
    a = np.degrees(np.arctan2(np.asarray(ay, np.float64), np.asarray(ax, np.float64)))
    return np.where(a < 22.5, 0, np.where(a > 67.5, 2, 1))


def sector_fixed(ax, ay):
    """the kernels' and OpenCV's fixed-point test: |gy| << 15 against |gx| * 13573 and that plus |gx| << 16"""
    ax, ay = np.asarray(ax, np.int64), np.asarray(ay, np.int64)
    t22 = ax * 13573
    return np.where((ay << 15) < t22, 0, np.where((ay << 15) > t22 + (ax << 16), 2, 1))


# ---- Canny ---------------------------------------------------------------------------------------------------------
def _shift(m, dy, dx):
    """m[y + dy, x + dx], zero outside the image"""
    p = np.pad(m, 1)
    r, c = m.shape
    return p[1 + dy:1 + dy + r, 1 + dx:1 + dx + c]


def canny(img, low=50.0, high=150.0):
    """Canny(img, low, high, apertureSize 3, L2gradient false) from its definition -> uint8 0 / 255.

    3x3 Sobel of each channel with replicated borders; L1 magnitude |gx| + |gy|; per pixel the channel with the largest
    magnitude, the first one on a tie; the direction sector from atan2 of that channel's gradient.  A pixel survives
    when its magnitude exceeds floor(low) and is a maximum along its gradient direction, magnitudes outside the image
    being zero; the answer is every 8-connected component of survivors that holds a pixel above floor(high).  Swapped
    thresholds are ordered first.

    The one thing taken from OpenCV, not derived: the tie convention of the maximum.  In the horizontal and vertical
    sectors a pixel must be strictly greater than its left / upper neighbour and greater or equal to its right / lower
    one (of a two-pixel plateau across the gradient the left / upper one survives); in the diagonal sectors strictly
    greater on both sides.  The diagonal pair is the one the gradient points along: equal signs of gx and gy give
    (-1, -1) / (+1, +1), otherwise (+1, -1) / (-1, +1), as (dx, dy) with y running down."""
    a = np.asarray(img).astype(np.int64)
    if a.ndim == 2:
        a = a[:, :, None]
    rows, cols, cn = a.shape
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
    smooth_y = p[:-2] + 2 * p[1:-1] + p[2:]          # [rows, cols + 2, cn]: 1 2 1 down the column
    smooth_x = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]  # [rows + 2, cols, cn]: 1 2 1 along the row
    gx_c = smooth_y[:, 2:] - smooth_y[:, :-2]
    gy_c = smooth_x[2:] - smooth_x[:-2]
    mag_c = np.abs(gx_c) + np.abs(gy_c)
    gx = np.zeros((rows, cols), np.int64)
    gy = np.zeros((rows, cols), np.int64)
    mag = np.full((rows, cols), -1, np.int64)
    for k in range(cn):                               # a later channel wins only when strictly larger
        better = mag_c[:, :, k] > mag
        gx[better], gy[better], mag[better] = gx_c[:, :, k][better], gy_c[:, :, k][better], mag_c[:, :, k][better]
    lo, hi = math.floor(min(low, high)), math.floor(max(low, high))
    sec = sector_atan2(np.abs(gx), np.abs(gy))
    left, right, up, down = _shift(mag, 0, -1), _shift(mag, 0, 1), _shift(mag, -1, 0), _shift(mag, 1, 0)
    horizontal = (mag > left) & (mag >= right)
    vertical = (mag > up) & (mag >= down)
    along_main = (mag > _shift(mag, -1, -1)) & (mag > _shift(mag, 1, 1))
    along_anti = (mag > _shift(mag, -1, 1)) & (mag > _shift(mag, 1, -1))
    same_sign = (gx > 0) == (gy > 0)                  # a diagonal sector has gx != 0 and gy != 0
    is_max = np.select([sec == 0, sec == 2], [horizontal, vertical], np.where(same_sign, along_main, along_anti))
    survive = (mag > lo) & is_max
    lab, n = ndimage.label(survive, structure=np.ones((3, 3), int))
    keep = np.zeros(n + 1, bool)
    keep[lab[survive & (mag > hi)]] = True
    keep[0] = False
    return np.where(keep[lab], 255, 0).astype(np.uint8)


# ---- HoughLinesP properties ----------------------------------------------------------------------------------------
def rounded(v):
    """cvRound of a parameter: nearest, ties to even"""
    return int(np.rint(v))


def chord(x0, y0, x1, y1):
    """the chord between two pixels, one pixel per major-axis step, rounded to the nearest on the minor axis ->
    (xs, ys, x_is_major)"""
    dx, dy = x1 - x0, y1 - y0
    t = max(abs(dx), abs(dy))
    k = np.arange(t + 1)
    if t == 0:
        return np.array([x0]), np.array([y0]), True
    if abs(dx) >= abs(dy):
        return x0 + k * (1 if dx > 0 else -1), np.floor(y0 + k * (dy / t) + 0.5).astype(np.int64), True
    return np.floor(x0 + k * (dx / t) + 0.5).astype(np.int64), y0 + k * (1 if dy > 0 else -1), False


def longest_gap(E, x0, y0, x1, y1):
    """P5's figure: the longest run of major-axis steps of the chord whose band of +-1 px on the minor axis holds no
    set pixel of E"""
    rows, cols = E.shape
    xs, ys, xmajor = chord(x0, y0, x1, y1)
    hit = np.zeros(len(xs), bool)
    for d in (-1, 0, 1):
        bx, by = (xs, ys + d) if xmajor else (xs + d, ys)
        ok = (bx >= 0) & (bx < cols) & (by >= 0) & (by < rows)
        hit[ok] |= E[by[ok], bx[ok]] != 0
    run = best = 0
    for h in hit:
        run = 0 if h else run + 1
        best = max(best, run)
    return best


def check_segments(E, lines, rho, theta, min_line_length, max_line_gap):
    """The properties every HoughLinesP(E, rho, theta, threshold, min_line_length, max_line_gap) answer has, whatever
    the random draws: `lines` int32 [n, 4] (x0, y0, x1, y1) in order -> list of violations, one string each.

    The algorithm: draw a set pixel, vote it into the accumulator, take the best angle n, walk from the pixel both ways
    along (-sin, cos)(n theta) one major-axis step at a time over the not yet erased pixels (the mask, a subset of E),
    stop a side at the border or after more than G = round(max_line_gap) steps without a mask pixel; the ends are the
    last mask pixels seen; erase what the walk met between them; report when max(|dx|, |dy|) >= L =
    round(min_line_length).

    P1  both endpoints are inside the image and set in E (they are mask pixels)
    P2  max(|dx|, |dy|) >= L
    P3  for L >= 1 all 2 n endpoints are distinct pixels: an endpoint is erased with its segment, and no later walk
        ends on an erased pixel; the two ends of one segment differ by P2
    P4  for some accumulator angle n the minor-axis displacement is within 1 px of T slope_n, T the major-axis length,
        slope_n from float64 cos and sin of n theta: both ends are floors of one straight walk of that slope
    P5  the gap rule against the original map: in the band of +-1 px on the minor axis around the chord, rounded to the
        nearest pixel per major-axis step, no run of steps without a set pixel of E is longer than G.  The walk's pixel
        is floor(w(t)) for a straight w, and both ends are such floors, so w minus the chord is linear and in [0, 1) at
        both ends, hence throughout: walk and chord differ by less than 1, walk and rounded chord by less than 1.5 and
        so, being integers, by at most 1.  The walk saw no run without a mask pixel longer than G between its ends; the
        mask is a subset of E; so a run without a pixel of E in the band is no longer than the walk's."""
    E = np.asarray(E)
    rows, cols = E.shape
    lines = np.asarray(lines, np.int64).reshape(-1, 4)
    L, G = rounded(min_line_length), rounded(max_line_gap)
    numangle = rounded(np.pi / np.float32(theta))
    ang = np.arange(numangle) * float(theta)
    a, b = -np.sin(ang), np.cos(ang)                 # walk direction of angle n
    bad = []
    seen = {}
    for i, (x0, y0, x1, y1) in enumerate(lines.tolist()):
        inside = 0 <= x0 < cols and 0 <= x1 < cols and 0 <= y0 < rows and 0 <= y1 < rows
        if not inside or not E[y0, x0] or not E[y1, x1]:
            bad.append("P1 segment %d %r: endpoint outside the image or not set" % (i, (x0, y0, x1, y1)))
            continue
        dx, dy = x1 - x0, y1 - y0
        T = max(abs(dx), abs(dy))
        if T < L:
            bad.append("P2 segment %d %r: length %d < %d" % (i, (x0, y0, x1, y1), T, L))
        if L >= 1:
            for pt in ((x0, y0), (x1, y1)):
                if pt in seen:
                    bad.append("P3 segment %d: endpoint %r already an endpoint of segment %d" % (i, pt, seen[pt]))
                seen.setdefault(pt, i)
        near = np.abs(np.abs(a) - np.abs(b)) < 1e-6   # 45 degrees: float32 decides the major axis
        ok = False
        with np.errstate(divide="ignore", invalid="ignore"):
            if abs(dx) == T:
                xm = (np.abs(a) > np.abs(b)) | near
                ok |= bool((xm & (np.abs(dy - dx * (b / a)) <= 1.0)).any())
            if abs(dy) == T:
                ym = (np.abs(a) <= np.abs(b)) | near
                ok |= bool((ym & (np.abs(dx - dy * (a / b)) <= 1.0)).any())
        if not ok:
            bad.append("P4 segment %d %r: no accumulator angle has this slope" % (i, (x0, y0, x1, y1)))
        g = longest_gap(E, x0, y0, x1, y1)
        if g > G:
            bad.append("P5 segment %d %r: %d steps without an edge pixel > %d" % (i, (x0, y0, x1, y1), g, G))
    return bad


# ---- angles and votes ----------------------------------------------------------------------------------------------
def rust_rem(a, m):
    """Rust's % on floats: the remainder keeps the dividend's sign"""
    return math.fmod(a, m)


def line_angles(lines):
    """hough.rs:65-68 / omr.rs:263-266 in float64: atan2(y2 - y1, x2 - x1) in degrees, % 45"""
    l = np.asarray(lines, np.float64).reshape(-1, 4)
    return np.array([rust_rem(math.degrees(math.atan2(y1 - y0, x1 - x0)), 45.0) for x0, y0, x1, y1 in l.tolist()])


def window_counts(values, members, width):
    """per value v: #{members m : |v - m| < width}"""
    s = np.sort(np.asarray(members, np.float64))
    v = np.asarray(values, np.float64)
    return np.searchsorted(s, v + width, "left") - np.searchsorted(s, v - width, "right")


def vote_hough_rs(angles, width=0.1):
    """hough.rs:72-89: the first angle with the strictly largest count of angles within +-width (`<`)"""
    c = window_counts(angles, angles, width)
    return float(angles[int(np.argmax(c))])          # argmax: the first maximum


BELIEVED, NEED_CHECK, NOT_A_RESULT = 0, 1, 2  # ResultStatus as the C ABI numbers it


def vote_omr_rs(angles, width=0.1):
    """omr.rs:268-301 -> (angle, status, candidates): a strictly larger count restarts the candidates with its angle, an
    equal one appends; status NOT_A_RESULT (no candidate), BELIEVED (one) or NEED_CHECK (more)"""
    c = window_counts(angles, angles, width)
    best, target, cand = 0, float(angles[0]), []
    for i in range(len(angles)):
        if c[i] > best:
            best, target, cand = int(c[i]), float(angles[i]), [float(angles[i])]
        elif c[i] == best:
            cand.append(float(angles[i]))
    return target, (NOT_A_RESULT if not cand else BELIEVED if len(cand) == 1 else NEED_CHECK), np.array(cand, np.float64)


EPS = 1e-4  # degrees: far above what float32 atan2, * 180 / pi and % 45 lose near 45 (4e-6), far below the window


def _admissible(lines):
    """per segment the folded float64 angle, plus the other fold where the unfolded angle is within EPS of a nonzero
    multiple of 45: there float32 rounding decides on which side of the fold the code under test lands (a segment at
    exactly 45 degrees is 44.999996 in float32 and 0 in float64).  Axis-parallel segments are not among them: atan2 with
    a zero argument is 0, +-pi/2 or pi in either precision, and float32's pi/2 * 180 / pi and pi * 180 / pi are 90 and
    180 exactly.  -> (values, owner index, two_valued per segment)"""
    l = np.asarray(lines, np.float64).reshape(-1, 4)
    vals, own, two = [], [], np.zeros(len(l), bool)
    for i, (x0, y0, x1, y1) in enumerate(l.tolist()):
        raw = math.degrees(math.atan2(y1 - y0, x1 - x0))
        r = rust_rem(raw, 45.0)
        vals.append(r)
        own.append(i)
        k = round(raw / 45.0)
        if k != 0 and abs(raw - 45.0 * k) < EPS and x0 != x1 and y0 != y1:
            vals.append(r + math.copysign(45.0, raw) if abs(r) < 1.0 else r - math.copysign(45.0, raw))
            own.append(i)
            two[i] = True
    return np.array(vals), np.array(own), two


def check_vote(lines, reported, eps=EPS):
    """A float32 winner held to the float64 vote -> (ok, ambiguous, message).

    The code under test computes the angles and the window in float32, which can flip a pair within rounding of the
    window's edge.  So: `reported` must be, to eps, the float64 angle of a segment whose count with window 0.1 + eps is
    at least every segment's count with window 0.1 - eps; where exactly one angle qualifies it must be that one.  Where
    no pair is within eps of the window's edge at all, the counts are certain and the winner must be the first segment
    of the strictly largest count.  ambiguous: more than one distinct angle qualifies."""
    vals, own, two = _admissible(lines)
    single = vals[~two[own]]                          # a two-valued segment is in no certain count
    hi = window_counts(vals, vals, 0.1 + eps)
    lo = window_counts(vals, single, 0.1 - eps)
    if (hi == lo).all():                              # certain counts: hough.rs exactly
        want = vote_hough_rs(vals)
        ok = abs(reported - want) <= eps
        return ok, False, "reported %.6f, the certain float64 winner is %.6f" % (reported, want)
    q = vals[hi >= lo.max()]
    distinct = np.unique(np.round(q / eps).astype(np.int64))
    ok = bool((np.abs(q - reported) <= eps).any())
    return ok, len(distinct) > 1, "reported %.6f, qualifying float64 angles %r" % (reported, np.unique(q)[:8].tolist())


def certain_omr_vote(lines, eps=EPS):
    """omr.rs's (angle, status, candidates) in float64 where float32 cannot change a count (no pair within eps of the
    window's edge, no segment within eps of a fold), else None"""
    vals, own, two = _admissible(lines)
    hi = window_counts(vals, vals, 0.1 + eps)
    lo = window_counts(vals, vals[~two[own]], 0.1 - eps)
    return vote_omr_rs(vals) if (hi == lo).all() else None


def check_omr_vote(lines, angle, status, candidates, eps=EPS):
    """omr.rs's result held to the float64 vote -> (ok, ambiguous, message).  With certain counts (no pair within eps
    of the window's edge, no segment within eps of a fold): angle, status and every candidate to eps.  Otherwise the
    angle as in check_vote, every candidate a qualifying angle, and status the rule applied to the candidates' number."""
    vals, own, two = _admissible(lines)
    single = vals[~two[own]]
    hi = window_counts(vals, vals, 0.1 + eps)
    lo = window_counts(vals, single, 0.1 - eps)
    candidates = np.asarray(candidates, np.float64)
    want_status = NOT_A_RESULT if len(candidates) == 0 else BELIEVED if len(candidates) == 1 else NEED_CHECK
    if int(status) != want_status:
        return False, False, "status %d with %d candidates" % (int(status), len(candidates))
    if (hi == lo).all():
        a, s, c = vote_omr_rs(vals)
        ok = abs(angle - a) <= eps and int(status) == s and len(c) == len(candidates) and \
            bool((np.abs(c - candidates) <= eps).all())
        return ok, False, "got (%.6f, %d, %d candidates), float64 (%.6f, %d, %d candidates)" % (
            angle, int(status), len(candidates), a, s, len(c))
    q = vals[hi >= lo.max()]
    near = lambda v: bool((np.abs(q - v) <= eps).any())  # noqa: E731
    ok = near(angle) and all(near(v) for v in candidates.tolist()) and len(candidates) >= 1
    return ok, True, "got %.6f with %d candidates, qualifying float64 angles %r" % (
        angle, len(candidates), np.unique(q)[:8].tolist())


# ---- truth images --------------------------------------------------------------------------------------------------
def strips(rows, cols, psi_deg, count, length, width, pitch):
    """`count` parallel straight strips at angle psi (degrees, y down, near-horizontal), rendered in float64: a pixel is
    black (0, on 255) when its centre lies within width / 2 of a strip's axis and within length / 2 of the strip's
    middle along it.  Axes are `pitch` apart (perpendicular distance), the stack centred on the image.  -> uint8"""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    y -= (rows - 1) / 2.0
    x -= (cols - 1) / 2.0
    c, s = math.cos(math.radians(psi_deg)), math.sin(math.radians(psi_deg))
    along = x * c + y * s
    across = -x * s + y * c
    img = np.full((rows, cols), 255, np.uint8)
    for k in range(count):
        off = (k - (count - 1) / 2.0) * pitch
        img[(np.abs(across - off) <= width / 2.0) & (np.abs(along) <= length / 2.0)] = 0
    return img


def truth_bound(min_line_length):
    """How far (degrees) get_angle_with_hough may land from the true angle psi of a strips() image whose strips are
    wider than G + 4, more than G + 4 apart and longer than 3 L (L, G the rounded parameters).

    The argument the bound was set by: a strip's Canny response is the closed outline of a two-level shape, one pixel
    per column of a long side, next to the boundary line.  A walk cannot pass from one long side to the other or to
    another strip: that takes more than G steps without an edge pixel (a walk of slope up to 1 against the strip's own
    tan psi crosses a band v px thick in v / (1 + tan |psi|) steps, so tests/hough_cases.py keeps widths and distances
    above 1.25 (G + 4)).  It can reach an end cap only next to a corner, within G steps of leaving its side, after
    running along the side for L - G steps or more.  So both endpoints of a segment lie within d px, vertically, of one
    line of slope tan psi, T >= L columns apart: |tan a - tan psi| <= 2 d / L for the segment's angle a, and |a - psi|
    <= atan(2 d / L) when a and psi have one sign (tan(a - psi) = (tan a - tan psi) / (1 + tan a tan psi)).  What the
    definition gives is d < 2: a pixel has a gradient only when its 3x3 window holds both levels, and next to a step of
    the boundary's staircase the response does sit further than 1 px from the line (1.64 px is the most on these
    images).  So the derived bound is atan(4 / L), and tests/test_hough_exact.py checks its premise d < 2 on every
    segment.  The winner of the vote is one segment's angle; near-horizontal strips with |psi| + atan(4 / L) < 45 keep
    % 45 out of it.

    What is returned and asserted is atan(2 / L) + 1e-3, the figure the d = 1 reading gives: it is not derived, it is an
    empirical tightening of the derived atan(4 / L) to half of it, kept because the tests were asked to hold that
    figure; the worst |detected - psi| is 0.35 of it (0.17 of the derived bound)."""
    return math.degrees(math.atan(2.0 / rounded(min_line_length))) + 1e-3


def truth_error(detected, psi_deg):
    """|detected - psi| taken modulo 45"""
    d = math.fmod(abs(detected - psi_deg), 45.0)
    return min(d, 45.0 - d)
