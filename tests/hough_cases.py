"""Shared inputs of tests/test_hough_exact.py (CPU: the restatements against tests/hough_exact.py) and
tests/test_gpu_hough_exact.py (the kernels against it), sized by the kernels' tiles: Canny works on 64x16 tiles with a
2-px halo, hysteresis on 64x32 tiles, the point list on 256 columns per pass and 8x8 mask tiles, the walks in rounds of
128 steps with a rule of their own for gaps below 64."""
import functools

import numpy as np

from oics import synth

CANNY_SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (16, 64), (17, 65), (32, 64), (33, 129), (50, 257)]
THRESHOLDS = [(50.0, 150.0), (150.0, 50.0), (0.0, 0.0), (49.9, 150.9), (2040.0, 2040.0)]
HYST_TILE = (64, 32)  # x, y


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _stripes(rows, cols, w, kind):
    y, x = np.mgrid[0:rows, 0:cols]
    t = {"x": x, "y": y, "main": x + y, "anti": x - y + rows}[kind]
    return (((t // w) % 2) * 180 + 30).astype(np.uint8)


def sector_image(rows=50, cols=257, d=255):
    """gradients on the sector boundaries integers allow: gx = gy (both diagonals), gx = 0, gy = 0"""
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.zeros((rows, cols), np.int64)
    img[(x < 64) & (x + y > 40)] = d                 # main diagonal edge: gx = gy
    img[(x >= 64) & (x < 128) & (x - y > 80)] = d    # anti diagonal edge: gx = -gy
    img[(x >= 128) & (x < 192) & (y > 24)] = d       # horizontal edge: gx = 0
    img[(x >= 200) & (x < 230)] = d                  # vertical edges: gy = 0
    return img.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def canny_cases():
    """-> tuple of (name, image, low, high)"""
    out = []
    for i, (r, c) in enumerate(CANNY_SHAPES):
        for cn in (1, 3, 4):
            shape = (r, c) if cn == 1 else (r, c, cn)
            out.append(("noise %dx%dx%d" % (r, c, cn), _rng(100 + i).integers(0, 256, shape, dtype=np.uint8), 50.0, 150.0))
            out.append(("faint noise %dx%dx%d" % (r, c, cn), _rng(200 + i).integers(110, 140, shape, dtype=np.uint8),
                        50.0, 150.0))
    contents = []
    for r, c, seed in ((33, 129, 3), (50, 257, 4)):
        contents.append(("card %dx%d" % (r, c), synth.make_card(r, c, seed)[0]))
    # channels that disagree on which has the largest gradient: few levels, so exact ties are common
    for cn in (3, 4):
        contents.append(("channel ties x%d" % cn, (_rng(300 + cn).integers(0, 4, (33, 129, cn)) * 85).astype(np.uint8)))
    g, _ = synth.make_card(50, 257, 5)
    contents.append(("channels of three cards", np.stack([g, synth.make_card(50, 257, 6)[0], g[::-1].copy()], axis=2)))
    ramp = (np.arange(129) % 32 * 6).astype(np.uint8)
    tie = np.zeros((33, 129, 3), np.uint8)
    tie[:, :, 0] = ramp[None, :]                     # the same sawtooth along x, along y and along x again: equal
    tie[:, :, 1] = ramp[:33, None]                   # magnitudes with different directions where they meet
    tie[:, :, 2] = ramp[None, ::-1]
    contents.append(("sawtooth ties", tie))
    for w in (1, 2, 3):
        for kind in ("x", "y", "main", "anti"):
            contents.append(("stripes %d %s" % (w, kind), _stripes(33, 129, w, kind)))
    plateau = np.full((32, 64), 40, np.uint8)
    plateau[8:24, 16:48] = 120
    plateau[12:20, 24:40] = 200
    contents.append(("plateaus", plateau))
    contents.append(("sector boundaries", sector_image()))
    contents.append(("faint sector boundaries", sector_image(d=20)))
    for name, img in contents:
        for lo, hi in THRESHOLDS:
            out.append(("%s (%g, %g)" % (name, lo, hi), img, lo, hi))
    for name, img in hysteresis_chains().items():
        out.append((name, img, 50.0, 150.0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hysteresis_chains(rows=400, cols=440):
    """Two images whose Canny survivors are weak diagonal chains (magnitude between 50 and 150): a thin diagonal line
    of 40 levels on black answers with one chain two pixels to each side of it, every link of which is diagonal.  The
    chain right of the line runs through (63, 31) -> (64, 32), (127, 95) -> (128, 96), ...: corners of the 64x32
    hysteresis tiles, crossed by nothing but that diagonal link; the two chains do not meet, so there is no way round.
    'joined' has one more pixel of 41 levels beside the line's head: it breaks the tie that suppresses the line's direct
    neighbours (magnitude 160) for exactly one of them, the single strong pixel, which touches the chain right of the
    line only.  'twin' has none.  tests/test_hough_exact.py asserts all of this from the definition."""
    twin = np.zeros((rows, cols), np.uint8)
    for x in range(32, 425):
        twin[x - 30, x] = 40
    joined = twin.copy()
    joined[5, 32] = 41
    return {"chain joined": joined, "chain twin": twin}


# ---- Hough edge maps -----------------------------------------------------------------------------------------------
def _line(img, x0, y0, length, slope=0.0, vertical=False):
    for t in range(length):
        x, y = (x0 + int(round(t * slope)), y0 + t) if vertical else (x0 + t, y0 + int(round(t * slope)))
        if 0 <= y < img.shape[0] and 0 <= x < img.shape[1]:
            img[y, x] = 255


def lengths_map():
    img = np.zeros((257, 300), np.uint8)
    for i, n in enumerate((63, 64, 65, 127, 128, 129)):
        _line(img, 5 + 3 * i, 8 + 16 * i, n)                       # horizontal
        _line(img, 150, 6 + 16 * i, n, slope=0.2)                   # about 11 degrees
    _line(img, 0, 120, 300)                                         # 300: a full row
    _line(img, 0, 140, 300, slope=-0.1)
    for i, n in enumerate((63, 64, 65, 127, 128, 129)):
        _line(img, 8 + 12 * i, 150, min(n, 105), vertical=True)     # vertical, cut by the image's height
    return img


def gaps_map(G):
    """three lines with one gap each of G - 1, G and G + 1 missing pixels, far apart"""
    img = np.zeros((257, 300), np.uint8)
    for i, g in enumerate((G - 1, G, G + 1)):
        if g < 0:
            continue
        y = 20 + 90 * i
        _line(img, 4, y, 45)
        _line(img, 4 + 45 + g, y, 45)
    return img


def borders_map():
    img = np.zeros((257, 300), np.uint8)
    _line(img, -30, 40, 120, slope=0.5)       # enters at the left border
    _line(img, 220, 100, 120, slope=-0.4)     # leaves at the right border
    _line(img, 60, -20, 120, slope=0.3, vertical=True)   # top
    _line(img, 200, 180, 120, slope=-0.3, vertical=True)  # bottom
    _line(img, 0, 0, 90, slope=1.0)           # a 45-degree line out of the corner
    return img


def cross_map():
    img = np.zeros((257, 300), np.uint8)
    img[100, :] = 255
    img[:, 150] = 255
    return img


def points_map(n, seed):
    img = np.zeros((40, 50), np.uint8)
    img.reshape(-1)[_rng(seed).choice(img.size, n, replace=False)] = 255
    return img


def noisy_lines_map():
    rng = _rng(17)
    img = np.zeros((120, 257), np.uint8)
    for _ in range(6):
        y0, x0, th = rng.integers(0, 120), rng.integers(0, 257), rng.random() * np.pi
        for t in range(int(rng.integers(40, 200))):
            y, x = int(round(y0 + t * np.sin(th))), int(round(x0 + t * np.cos(th)))
            if 0 <= y < 120 and 0 <= x < 257 and rng.random() < 0.85:
                img[y, x] = 255
    img[rng.random(img.shape) < 0.004] = 255
    return img


RESOLUTIONS = [(1.0, np.pi / 180.0), (2.0, np.pi / 180.0), (0.5, np.pi / 90.0)]


@functools.lru_cache(maxsize=None)
def hough_cases():
    """-> tuple of (name, edge map, rho, theta, threshold, min_line_length, max_line_gap)"""
    out = [("lengths", lengths_map(), 1.0, np.pi / 180.0, 0, 30.0, 3.0),
           ("borders", borders_map(), 1.0, np.pi / 180.0, 0, 30.0, 3.0),
           ("full row and column", cross_map(), 1.0, np.pi / 180.0, 0, 30.0, 3.0),
           ("1x200", np.full((1, 200), 255, np.uint8), 1.0, np.pi / 180.0, 0, 30.0, 3.0),
           ("200x1", np.full((200, 1), 255, np.uint8), 1.0, np.pi / 180.0, 0, 30.0, 3.0)]
    row = np.full((1, 200), 255, np.uint8)
    row[0, 60:66] = 0
    row[0, 130:134] = 0
    out.append(("1x200 with gaps", row, 1.0, np.pi / 180.0, 0, 30.0, 5.0))
    out.append(("200x1 with gaps", row.T.copy(), 1.0, np.pi / 180.0, 0, 30.0, 5.0))
    for G in (0, 5, 63, 64, 127, 128):
        out.append(("gaps around %d" % G, gaps_map(G), 1.0, np.pi / 180.0, 0, 30.0, float(G)))
    for n in (63, 64, 65, 129):
        out.append(("%d points" % n, points_map(n, 400 + n), 1.0, np.pi / 180.0, 0, 2.0, 10.0))
    for name, img in (("lengths", lengths_map()), ("noisy lines", noisy_lines_map())):
        for rho, theta in RESOLUTIONS:
            for thr in (0, 20):
                out.append(("%s rho %g theta pi/%d threshold %d" % (name, rho, round(np.pi / theta), thr), img, rho,
                            theta, thr, 20.0, 4.0))
    return tuple(out)


def dense_dashes(rows=600, cols=900):
    """a scan that answers with more than 2048 segments at small L: rows of short thick dashes at a few slopes"""
    img = np.full((rows, cols), 255, np.uint8)
    slopes = (0.0, 1 / 14.0, -1 / 14.0, 2 / 14.0, 0.0, -2 / 14.0)
    for k, y0 in enumerate(range(6, rows - 10, 8)):
        s = slopes[k % len(slopes)]
        for x0 in range(4 + (k % 3) * 5, cols - 20, 20):
            for t in range(15):
                y = y0 + int(round(t * s))
                img[y:y + 3, x0 + t] = 0
    return img


# ---- truth images --------------------------------------------------------------------------------------------------
PSIS = [0.0, 0.7, -0.7, 3.3, -3.3, 7.25, -12.5]
TRUTH = {40: dict(rows=230, cols=180, count=7, length=140.0, width=12.0, pitch=26.0, gap=5.0),
         150: dict(rows=900, cols=520, count=6, length=480.0, width=72.0, pitch=144.0, gap=50.0)}


@functools.lru_cache(maxsize=None)
def truth_image(L, psi):
    """strips at the true angle psi for min_line_length L (max_line_gap TRUTH[L]['gap']): wider than G + 4, more than
    G + 4 apart, longer than 3 L"""
    import hough_exact as hx
    p = TRUTH[L]
    return hx.strips(p["rows"], p["cols"], psi, p["count"], p["length"], p["width"], p["pitch"])


@functools.lru_cache(maxsize=None)
def vote_cases():
    """-> tuple of (image, min_line_length, max_line_gap) for the votes: cards of 1, 3 and 4 channels, strips, and
    upright strips, whose segments % 45 folds"""
    out = []
    # seeds and parameters chosen so that at most one case in ten is ambiguous for the float32 vote (hough_exact.check_vote)
    for rows, cols, seed, params in ((230, 248, 4, ((25.0, 3.0),)), (300, 420, 9, ((25.0, 3.0),)),
                                     (200, 260, 60, ((25.0, 3.0),)),
                                     (333, 517, 6, ((40.0, 8.0), (60.0, 10.0), (25.0, 3.0)))):
        g = synth.make_card(rows, cols, seed)[0]
        for L, G in params:
            out.append((g, L, G))
    g = synth.make_card(300, 420, 21)[0]
    for cn in (3, 4):
        n = _rng(500 + cn).integers(-12, 13, g.shape + (cn,))
        out.append((np.clip(g[:, :, None].astype(np.int64) + n, 0, 255).astype(np.uint8), 40.0, 8.0))
    for psi in (3.3, -12.5):
        out.append((truth_image(40, psi), 40.0, TRUTH[40]["gap"]))
        out.append((np.ascontiguousarray(truth_image(40, psi).T), 40.0, TRUTH[40]["gap"]))
    out.append((truth_image(150, 0.7), 150.0, TRUTH[150]["gap"]))
    return tuple(out)


BATCH_CARD_SEEDS = [87, 95, 96, 98, 103, 112, 116, 117, 119, 123]  # 230x248 cards whose vote at (40, 8) is unambiguous
