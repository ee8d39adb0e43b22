"""The inputs tests/test_geom_exact.py (the restatements) and tests/test_gpu_geom_exact.py (the kernels) share: both
hold the same cases to the same float64 references (tests/geom_exact.py) and the same bounds."""
import functools
import itertools

import numpy as np

import geom_exact as gx

BORDER = (23, 201, 87, 140)  # test_gpu_rotate_ex.BORDER: its device helpers pass this one
QUARTER_TURNS = (0.0, 90.0, -90.0, 180.0)
# Scales whose destination-to-source map is a multiple of 1 / 32 in every term.  With WARP_INVERSE_MAP the matrix is the
# map: 33/32, 31/32, 17/16, 3/8, 5/2, 4.  Without it the map is the inverse: forward 32/33, 1/2, 2, 4, 1/4.
# A 64 x 16 destination tile's source box is staged in LDS while it fits (16 KB for NEAREST / LINEAR + BORDER_CONSTANT
# on 1 or 3 channels, 32 KB otherwise) and tapped from global memory beyond; staged_share() restates that criterion
# from the geometry, and test_geom_exact.py asserts that maps 2.5 and 4 put tiles on the global side and the others on
# the LDS side.
EXACT_SCALES = {gx.INVERSE_MAP: (33 / 32, 31 / 32, 17 / 16, 3 / 8, 5 / 2, 4.0), 0: (32 / 33, 1 / 2, 2.0, 4.0, 1 / 4)}
EVEN_SHAPES = ((2, 2), (4, 6), (8, 8), (38, 54), (64, 96))
ODD_SHAPES = ((1, 7), (3, 3), (37, 53))  # CONTAIN only: an odd side under DEFAULT leaves the 1 / 32 grid
GENERAL_ANGLES = (7.3, -41.0, 0.05, 33.0)
GENERAL_SCALES = (1.0, 0.37, 2.5)
GENERAL_SHAPES = ((8, 7), (37, 53), (64, 96))
NEAREST_CAP = 0.01  # share of a canvas that may lie within the tie distance of a rounding boundary


def board(rng, rows, cols, cn):
    """test_gpu_rotate_ex._content: noise, the left half a 0 / 255 checkerboard of 2 x 2 squares"""
    a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    yy, xx = np.mgrid[:rows, :cols]
    b = ((yy // 2 + xx // 2) % 2 * 255).astype(np.uint8)
    half = xx < cols // 2
    a[half] = b[half][:, None]
    return a


def smooth(rows, cols, cn=3, seed=0):
    """four sinusoids of wavelength >= 24 px and amplitude 25 around 128, rounded to u8, each channel its own phases"""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[:rows, :cols].astype(np.float64)
    out = np.zeros((rows, cols, cn), np.uint8)
    for c in range(cn):
        v = np.full((rows, cols), 128.0)
        for _ in range(4):
            lam, th, ph = rng.uniform(24, 60), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
            v += 25 * np.sin(2 * np.pi * (xx * np.cos(th) + yy * np.sin(th)) / lam + ph)
        out[:, :, c] = np.rint(v)
    return out


@functools.lru_cache(maxsize=None)
def exact_cases(rows, cols):
    """[(cn, flags, mode, clip, angle, scale)]: every interpolation x border mode (TRANSPARENT included) x {forward,
    WARP_INVERSE_MAP}, the channel count, clip, quarter turn and scale drawn by a fixed generator so that each value
    meets each interpolation and border many times over the shapes"""
    rng = np.random.default_rng(rows * 131 + cols)
    clips = (1,) if (rows % 2 or cols % 2) else (0, 1)
    out = []
    for interp, mode, inv, _ in itertools.product((0, 1, 2, 3, 4), range(6), (0, gx.INVERSE_MAP), range(2)):
        sc = EXACT_SCALES[inv]
        out.append((1 + int(rng.integers(4)), interp | inv, mode, clips[int(rng.integers(len(clips)))],
                    QUARTER_TURNS[int(rng.integers(4))], sc[int(rng.integers(len(sc)))]))
    return out


@functools.lru_cache(maxsize=None)
def general_cases(rows, cols):
    """[(flags, mode, clip, angle, scale)] for LINEAR, CUBIC, LANCZOS4: every angle x scale x clip x interpolation, the
    border mode 0 .. 4 by turns"""
    out, i = [], 0
    for angle, scale, clip, interp in itertools.product(GENERAL_ANGLES, GENERAL_SCALES, (0, 1), (1, 2, 4)):
        out.append((interp, (i + i // 5) % 5, clip, angle, scale))
        i += 1
    return out


def nearest_ambiguous_share(rows, cols, angle, scale, clip):
    M, dr, dc = gx.rotate_geometry(rows, cols, angle, scale, clip)
    x, y = gx.source_coords(M, dr, dc)
    fx, fy = x + 0.5 - np.floor(x + 0.5), y + 0.5 - np.floor(y + 0.5)
    t = gx.NEAREST_TIE
    return float(((fx < t) | (fx > 1 - t) | (fy < t) | (fy > 1 - t)).mean())


@functools.lru_cache(maxsize=None)
def nearest_cases(rows, cols):
    """[(mode, clip, angle, scale)]: the general geometries whose float64 coordinates alone leave at most NEAREST_CAP of
    the canvas within the tie distance of a rounding boundary (test_geom_exact.py asserts the cap, and that most
    geometries pass it), border mode 0 .. 4 by turns"""
    out, i = [], 0
    for angle, scale, clip in itertools.product(GENERAL_ANGLES, GENERAL_SCALES, (0, 1)):
        if nearest_ambiguous_share(rows, cols, angle, scale, clip) <= NEAREST_CAP:
            out.append((i % 5, clip, angle, scale))
            i += 1
    return out


def staged_share(rows, cols, cn, flags, mode, clip, angle, scale):
    """the share of the canvas's 64 x 16 tiles whose source box fits the warp kernels' LDS: the box spans the tile's
    four corner samples plus the taps (K, or 2 + K for the NEAREST / LINEAR BORDER_CONSTANT kernel's slack), rows widened
    to whole dwords"""
    interp = 1 if flags & 7 == 3 else flags & 7
    K = gx.TAPS[interp]
    small = interp <= 1 and mode == gx.CONSTANT and cn in (1, 3)
    lds, extra = (16384, 3 + (interp == 1)) if small else (32768, K)
    M, dr, dc = gx.rotate_geometry(rows, cols, angle, scale, clip, bool(flags & gx.INVERSE_MAP))
    fit = []
    for ty in range(0, dr, 16):
        for tx in range(0, dc, 64):
            xs, ys = np.meshgrid([tx, min(dc, tx + 64) - 1], [ty, min(dr, ty + 16) - 1])
            sx = M[0, 0] * xs + M[0, 1] * ys + M[0, 2]
            sy = M[1, 0] * xs + M[1, 1] * ys + M[1, 2]
            bw = (np.floor(sx.max()) - np.floor(sx.min()) + extra) * cn + 6
            bh = np.floor(sy.max()) - np.floor(sy.min()) + extra
            fit.append(bw * bh <= lds)
    return float(np.mean(fit))


AREA_CASES = (  # rows, cols -> drows, dcols
    (8, 12, 4, 6), (20, 35, 4, 7), (9, 8, 3, 4), (130, 65, 2, 1), (37, 53, 15, 17), (64, 96, 25, 31), (37, 53, 37, 17),
    (38, 54, 19, 54))
ENLARGE_CASES = ((8, 7, 1.5), (8, 7, 2.0), (37, 53, 1.5), (37, 53, 2.0))


def gray_triples():
    """256 x 264 x 3: 65 536 random triples, then the 8 corners of the cube (the three triples with one channel at 255
    and the others 0 among them: what swapped weights move by 47 levels) repeated to fill the image"""
    rng = np.random.default_rng(65536)
    a = rng.integers(0, 256, (256 * 264, 3), dtype=np.uint8)
    corners = np.array(list(itertools.product((0, 255), repeat=3)), np.uint8)
    a[65536:] = np.resize(corners, (256 * 264 - 65536, 3))
    return a.reshape(256, 264, 3)
