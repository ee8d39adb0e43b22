"""The restatements held to float64 first-principles math (tests/geom_exact.py), before the kernels are
(tests/test_gpu_geom_exact.py): warp_ref.rotate_ex, the oracle's resize_area, its enlarging resize and its gray
conversion, on the inputs the GPU tests use (tests/geom_cases.py), every pixel counted.  The kernels are tested byte
for byte against these restatements elsewhere; this file is what ties the restatements to something that was not read
off the same source.  Then sanity cases for the float64 code itself.

Worst |restatement - exact| / bound on these inputs; the kernels give the same figures on an MI355X:
  exact-coordinate warps  NEAREST equal, LINEAR 1.000 (the half-level rounding itself; equal to floor(exact + 0.5)
                          everywhere), CUBIC 0.87, LANCZOS4 0.70
  general warps           LINEAR 0.83, CUBIC 0.56, LANCZOS4 0.36; NEAREST: every pixel equal or one of its tie's two
  area resize 1.000 (a .5 tie), enlarging resize 0.62 (0.78 of the 1.257 levels), gray 0.96"""
import numpy as np
import pytest

import geom_cases as gc
import geom_exact as gx
import warp_ref as wr

RATIOS = {}


def _note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def _hold(got, exact, bound, case, clip=True, key=None):
    """every pixel within the bound, or the case, the count and the worst pixel's got / exact / bound; RATIOS[key] keeps
    the worst error / bound seen (tools print it)"""
    bad, at, ratio = gx.worst(got, exact, bound, clip)
    _note(key, ratio)
    assert bad == 0, "%r: %d pixels over the bound; worst at %r: got %r, exact %.4f, bound %.4f" % ((case, bad) + at)
    return ratio


def exact_map(rows, cols, flags, clip, angle, scale):
    M, dr, dc = gx.rotate_geometry(rows, cols, angle, scale, clip, bool(flags & gx.INVERSE_MAP))
    return gx.snap(M), dr, dc


def check_exact_case(a, got, kept, case):
    """one exact-coordinate case: `got` the canvas, `kept` the pixels BORDER_TRANSPARENT wrote (None: all)"""
    cn, flags, mode, clip, angle, scale = case
    M, dr, dc = exact_map(a.shape[0], a.shape[1], flags, clip, angle, scale)
    assert got.shape == (dr, dc, cn), (case, got.shape, dr, dc)
    interp = flags & 7
    exact = np.clip(gx.warp(a, M, dr, dc, interp, mode, gc.BORDER), 0, 255)
    sel = np.ones((dr, dc), bool) if kept is None else kept
    g, e = got[sel], exact[sel]
    if interp == gx.NEAREST:
        assert (g == e).all(), (a.shape, case, int((g != e).sum()))
        return 0.0
    if gx.TAPS[interp] == 2:
        assert (g == np.floor(e + 0.5)).all(), (a.shape, case, int((g != np.floor(e + 0.5)).sum()))
    return _hold(g, e, gx.exact_warp_bound(interp), (a.shape, case), key=("exact", gx.TAPS[interp]))


def check_general_case(a, got, case):
    flags, mode, clip, angle, scale = case
    M, dr, dc = gx.rotate_geometry(a.shape[0], a.shape[1], angle, scale, clip)
    assert got.shape == (dr, dc, a.shape[2]), (case, got.shape, dr, dc)
    exact = gx.warp(a, M, dr, dc, flags & 7, mode, gc.BORDER)
    return _hold(got, exact, gx.general_warp_bound(flags & 7, a, mode, gc.BORDER), (a.shape, case),
                 key=("general", gx.TAPS[flags & 7]))


def check_nearest_case(a, got, case):
    mode, clip, angle, scale = case
    M, dr, dc = gx.rotate_geometry(a.shape[0], a.shape[1], angle, scale, clip)
    assert got.shape == (dr, dc, a.shape[2]), (case, got.shape, dr, dc)
    ref, alts, amb = gx.nearest_candidates(a, M, dr, dc, mode, gc.BORDER)
    assert amb.mean() <= gc.NEAREST_CAP, (case, amb.mean())
    sure = (got == ref).all(-1)
    either = (got[None] == alts).all(-1).any(0)
    bad = ~np.where(amb, sure | either, sure)
    assert not bad.any(), (a.shape, case, int(bad.sum()), np.argwhere(bad)[:3].tolist())


def _kept(a, flags, mode, clip, angle, scale):
    """which pixels BORDER_TRANSPARENT writes: test_gpu_rotate_ex's business, taken from the restatement"""
    if mode != wr.TRANSPARENT:
        return None
    z = wr.rotate_ex(a, angle, scale, flags, mode, gc.BORDER, clip, init=None)
    o = wr.rotate_ex(a, angle, scale, flags, mode, gc.BORDER, clip, init=np.full(z.shape, 255, np.uint8))
    return (z == o).all(-1)


# ---- the restatement of warpAffine ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", gc.EVEN_SHAPES + gc.ODD_SHAPES)
def test_restated_warp_at_exact_coordinates(rows, cols):
    rng = np.random.default_rng(rows * 7 + cols)
    for case in gc.exact_cases(rows, cols):
        cn, flags, mode, clip, angle, scale = case
        a = gc.board(rng, rows, cols, cn)
        got = wr.rotate_ex(a, angle, scale, flags, mode, gc.BORDER, clip)
        check_exact_case(a, got, _kept(a, flags, mode, clip, angle, scale), case)


@pytest.mark.parametrize("rows,cols", gc.GENERAL_SHAPES)
def test_restated_warp_at_general_angles(rows, cols):
    a = gc.smooth(rows, cols)
    for case in gc.general_cases(rows, cols):
        flags, mode, clip, angle, scale = case
        got = wr.rotate_ex(a, angle, scale, flags, mode, gc.BORDER, clip)
        check_general_case(a, got, case)


@pytest.mark.parametrize("rows,cols", gc.GENERAL_SHAPES)
def test_restated_nearest_at_general_angles_and_the_ambiguity_cap(rows, cols):
    """the cap is a property of the float64 geometry alone; at least half of the 24 geometries meet it at every size"""
    a = gc.smooth(rows, cols)
    cases = gc.nearest_cases(rows, cols)
    assert len(cases) >= 12, len(cases)
    for case in cases:
        mode, clip, angle, scale = case
        assert gc.nearest_ambiguous_share(rows, cols, angle, scale, clip) <= gc.NEAREST_CAP
        check_nearest_case(a, wr.rotate_ex(a, angle, scale, 0, mode, gc.BORDER, clip), case)


def test_exact_scales_lie_on_both_sides_of_the_lds_split():
    """on the 64 x 96 sheet: maps 2.5 and 4 leave tiles whose box does not fit LDS, the maps near 1 and below fit"""
    out = {}
    for cn, flags, mode in ((3, 1, 0), (4, 4, 1), (3, 2, 4), (1, 0, 0)):
        for inv, scales in gc.EXACT_SCALES.items():
            for s in scales:
                m = s if inv else 1 / s
                out.setdefault(round(m, 4), []).append(gc.staged_share(64, 96, cn, flags | inv, mode, 1, 0.0, s))
    assert all(min(out[m]) == 1.0 for m in out if m <= 2.0), out
    assert min(out[2.5]) < 1.0 and min(out[4.0]) < 1.0, out
    assert sum(1 for m in out if m <= 2.0) >= 2


# ---- the oracle's resize and gray -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,drows,dcols", gc.AREA_CASES)
def test_restated_area_resize(oracle, rows, cols, drows, dcols):
    rng = np.random.default_rng(rows + dcols)
    for cn in (1, 3):
        for a in (rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8), gc.board(rng, rows, cols, cn)):
            got = oracle.resize_area(a, drows, dcols)
            _hold(got, gx.area_resize(a, drows, dcols), gx.area_bound(rows, cols, drows, dcols), (rows, cols, drows, dcols, cn),
                  clip=False, key="area")


@pytest.mark.parametrize("rows,cols,scale", gc.ENLARGE_CASES)
def test_restated_enlarging_resize(oracle, rows, cols, scale):
    rng = np.random.default_rng(rows)
    for a in (gc.smooth(rows, cols), gc.board(rng, rows, cols, 3), gc.board(rng, rows, cols, 1)):
        got = oracle.scale_self(a, scale)
        dr, dc = int(rows * scale), int(cols * scale)
        assert got.shape[:2] == (dr, dc)
        _hold(got, gx.linear_resize(a, dr, dc), gx.linear_resize_bound(), (rows, cols, scale), clip=False, key="enlarge")


def test_restated_gray(oracle):
    """COLOR_RGB2GRAY is applied to the bytes as they lie (transfer.rs:287): byte 0 is its R, byte 2 its B, so the
    B, G, R view gx.gray takes is the bytes reversed"""
    a = gc.gray_triples()
    _hold(oracle.rgb2gray(a), gx.gray(a[:, :, ::-1]), gx.gray_bound(), "gray", clip=False, key="gray")


# ---- the float64 code itself ----------------------------------------------------------------------------------------
def test_kernel_norms_and_weights():
    for interp, S, A in ((1, 1.0, 1.0), (2, 1.5, 1.375), (4, 2.0007, 1.7146)):
        s, a = gx.kernel_norms(interp)
        assert abs(s - S) < 2e-3 and abs(a - A) < 2e-3, (interp, s, a)
        w = gx.weights(interp, np.linspace(0, 0.999, 50))
        assert np.abs(w.sum(-1) - 1).max() < 1e-12
    assert np.allclose(gx.weights(2, 0.5), [-0.09375, 0.59375, 0.59375, -0.09375])
    assert np.allclose(gx.weights(4, 0.0), [0, 0, 0, 1, 0, 0, 0, 0])


def test_identity_and_two_half_turns():
    rng = np.random.default_rng(1)
    a = gc.board(rng, 8, 12, 3)
    for interp in (0, 1, 2, 4):
        M, dr, dc = gx.rotate_geometry(8, 12, 0.0, 1.0, 0)
        assert np.abs(gx.warp(a, M, dr, dc, interp, 1, gc.BORDER) - a).max() < 1e-9
        # a half turn about (cols / 2, rows / 2) sends x to cols - x: a permutation of the columns under BORDER_WRAP
        M, dr, dc = exact_map(8, 12, 0, 0, 180.0, 1.0)
        once = gx.warp(a, M, dr, dc, interp, gx.WRAP, gc.BORDER)
        assert np.abs(once - np.roll(a[::-1, ::-1], (1, 1), (0, 1))).max() < 1e-9, interp
        twice = gx.warp(once, M, dr, dc, interp, gx.WRAP, gc.BORDER)
        assert np.abs(twice - a).max() < 1e-9, interp


def test_constant_image_under_every_kernel_and_border():
    a = np.full((5, 6, 2), 77, np.uint8)
    M, dr, dc = gx.rotate_geometry(5, 6, 33.0, 0.7, 1)
    for interp in (0, 1, 2, 4):
        for mode in (1, 2, 3, 4):
            assert np.abs(gx.warp(a, M, dr, dc, interp, mode, gc.BORDER) - 77).max() < 1e-9
        assert np.abs(gx.warp(a, M, dr, dc, interp, 0, (77, 77, 77, 77)) - 77).max() < 1e-9


def test_linear_ramp_is_reproduced_in_the_interior():
    yy, xx = np.mgrid[:40, :50]
    a = (2 * xx + 3 * yy).astype(np.uint8)[:, :, None]  # at most 215
    M, dr, dc = gx.rotate_geometry(40, 50, 7.3, 1.0, 0)
    x, y = gx.source_coords(M, dr, dc)
    inner = (x >= 4) & (x <= 45) & (y >= 4) & (y <= 35)
    assert inner.sum() > 500
    # A kernel reproduces a ramp of slope g up to g m1, m1 = max_t |sum_j (j - t) w_j(t)| its first moment: 0 for the
    # bilinear kernel; (2 A + 1) t (1 - t) (2 t - 1) for Keys' kernel, which only A = -0.5 makes 0 -- at A = -0.75 it peaks
    # at 0.5 / (6 sqrt 3) = 0.0481; the normalised Lanczos-4 kernel has a small one of its own.
    t = np.linspace(0, 1, 2001)
    m1 = {i: np.abs((gx.weights(i, t) * (np.arange(gx.TAPS[i]) - (gx.TAPS[i] // 2 - 1) - t[:, None])).sum(-1)).max() for i in (1, 2, 4)}
    assert m1[1] < 1e-12 and abs(m1[2] - 0.5 / (6 * 3 ** 0.5)) < 1e-6 and m1[4] < 0.02, m1
    for interp in (1, 2, 4):
        v = gx.warp(a, M, dr, dc, interp, 1, gc.BORDER)[:, :, 0]
        assert np.abs(v - (2 * x + 3 * y))[inner].max() <= (2 + 3) * m1[interp] + 1e-9, interp


def test_border_index_by_hand():
    p = np.arange(-5, 9)
    assert gx.border_index(p, 4, gx.REFLECT)[0].tolist() == [3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0]
    assert gx.border_index(p, 4, gx.REFLECT_101)[0].tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert gx.border_index(p, 4, gx.WRAP)[0].tolist() == [3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0]
    assert gx.border_index(p, 4, gx.REPLICATE)[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 2, 3, 3, 3, 3, 3, 3]
    assert gx.border_index(p, 1, gx.REFLECT_101)[0].tolist() == [0] * 14


def test_area_resize_by_one_and_by_hand():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    assert np.abs(gx.area_resize(a, 7, 9) - a).max() < 1e-12
    assert np.abs(gx.area_resize(a, 1, 1)[0, 0] - a.reshape(-1, 3).mean(0)).max() < 1e-9
    row = np.array([[10, 20, 60]], np.uint8)  # 3 -> 2: cells [0, 1.5) and [1.5, 3)
    assert np.allclose(gx.area_resize(row, 1, 2)[0, :, 0], [(10 + 20 * 0.5) / 1.5, (20 * 0.5 + 60) / 1.5])
    assert np.allclose(gx.linear_resize(row, 1, 6)[0, :, 0], [10, 12.5, 17.5, 30, 50, 60])


def test_gray_by_hand():
    assert np.allclose(gx.gray(np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]])), [29.07, 149.685, 76.245])
