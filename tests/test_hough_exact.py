"""The Hough-line restatements held to first principles (tests/hough_exact.py), before the kernels are
(tests/test_gpu_hough_exact.py): oracle.canny, its fast build and oracle_np.canny_np against Canny's definition byte
for byte; oracle.hough_lines_p and oracle_np.hough_lines_p_py against the properties P1-P5 every answer has; the
oracle's votes against hough.rs / omr.rs in float64; its detected angle on strips of a known angle against the bound
of hough_exact.truth_bound.  Then the mutations: each named misreading, applied in Python to a scratch copy of
the restatement or to an answer, must make one of these checks fail.

Figures on these inputs: Canny 0 differing bytes in 161 cases (three restatements); P1-P5 0 violations; votes 1 of 13
cases ambiguous; worst |detected - psi| / bound 0.24 (L = 40) and 0.35 (L = 150), on an MI355X 0.24 and 0.35 too; all
fifteen mutation tests fail their check (the thirteen named misreadings with >= at low and at high apart, plus a wrong
slope for P4); the weakest, >= at low, is caught by one case of 161."""
import math

import numpy as np
import pytest

import hough_cases as hc
import hough_exact as hx
from oracle import oracle_np

PI180 = np.pi / 180.0


# ---- the claim that makes a byte-exact Canny reference possible ----------------------------------------------------
def test_fixed_point_sector_is_the_true_sector():
    """every gradient an 8-bit image can give, 0 <= |gx|, |gy| <= 1020: the fixed-point sector test equals the sector
    of the exact tangents and of atan2, no pair left out"""
    ay, ax = np.mgrid[0:1021, 0:1021]
    fixed = hx.sector_fixed(ax, ay)
    assert int((fixed != hx.sector_exact(ax, ay)).sum()) == 0
    nonzero = (ax + ay) > 0
    assert int(nonzero.sum()) == 1042440
    assert int((fixed != hx.sector_atan2(ax, ay))[nonzero].sum()) == 0
    # the closest any pair comes to a boundary is far above float64's rounding
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ay[nonzero] / ax[nonzero].astype(np.float64)
    assert min(np.abs(t - hx.TAN_22_5).min(), np.abs(t - hx.TAN_67_5).min()) > 1e-7


# ---- Canny ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def canny_exact():
    return [hx.canny(img, lo, hi) for _, img, lo, hi in hc.canny_cases()]


@pytest.mark.parametrize("which", ["oracle", "oracle fast", "oracle_np"])
def test_canny_restatements_equal_the_definition(oracle, canny_exact, which):
    fn = {"oracle": oracle.canny, "oracle fast": lambda i, lo, hi: oracle.canny(i, lo, hi, fast=True),
          "oracle_np": oracle_np.canny_np}[which]
    edge_px = 0
    for (name, img, lo, hi), exact in zip(hc.canny_cases(), canny_exact):
        got = fn(img, lo, hi)
        assert got.shape == exact.shape and (got == exact).all(), "%s: %d bytes differ" % (name, int((got != exact).sum()))
        edge_px += int((exact != 0).sum())
    assert edge_px > 50000  # the cases are not empty pictures


def test_canny_cases_cover_what_they_name():
    cases = hc.canny_cases()
    by = {name: hx.canny(img, lo, hi) for name, img, lo, hi in cases}
    assert not by["card 50x257 (2040, 2040)"].any() and by["card 50x257 (0, 0)"].sum() > by["card 50x257 (50, 150)"].sum()
    assert (by["card 50x257 (50, 150)"] == by["card 50x257 (150, 50)"]).all()
    assert (by["faint noise 33x129x1"] != 0).any() and (by["faint noise 33x129x1"] == 0).any()
    for k in ("stripes 1 x", "stripes 2 y", "stripes 3 main", "stripes 2 anti", "plateaus", "sector boundaries",
              "sawtooth ties", "channel ties x4"):
        assert by[k + " (50, 150)"].any(), k
    shapes = {img.shape[:2] for _, img, _, _ in cases}
    assert set(hc.CANNY_SHAPES) <= shapes
    assert {img.shape[2] for _, img, _, _ in cases if img.ndim == 3} == {3, 4}


def _survivors(img):
    """survivors above 50 (all of them: low = high) and the strong ones (above 150), from the definition"""
    return hx.canny(img, 50.0, 50.0) != 0, hx.canny(img, 150.0, 150.0) != 0


def test_hysteresis_chain_spans_tiles_and_corners():
    """from the definition: the joined chain is kept whole from a single strong pixel, through 7 x 13 hysteresis tiles
    and six tile corners that only a diagonal link crosses; its twin has no strong pixel and is dropped whole"""
    from scipy import ndimage
    chains = hc.hysteresis_chains()
    tx, ty = hc.HYST_TILE
    weak, strong = _survivors(chains["chain joined"])
    kept = hx.canny(chains["chain joined"]) != 0
    assert int(strong.sum()) == 1 and (kept & strong).sum() == 1
    lab, _ = ndimage.label(weak, structure=np.ones((3, 3), int))
    chain = lab == lab[ty - 1, tx - 1]
    assert weak[ty - 1, tx - 1] and (kept == chain).all() and int(chain.sum()) > 380  # whole, and nothing else
    ys, xs = np.nonzero(chain)
    assert xs.max() // tx - xs.min() // tx >= 6 and ys.max() // ty - ys.min() // ty >= 6
    corners = 0
    for k in range(1, 7):
        x, y = tx * k, ty * (2 * k - 1)
        if chain[y - 1, x - 1] and chain[y, x] and not weak[y - 1, x] and not weak[y, x - 1]:
            corners += 1
            cut = chain.copy()
            cut[y, x] = False                         # no way round: without this pixel the chain falls apart
            assert ndimage.label(cut, structure=np.ones((3, 3), int))[1] == 2
    assert corners == 6
    weak2, strong2 = _survivors(chains["chain twin"])
    assert not strong2.any() and int(weak2.sum()) > 700 and not hx.canny(chains["chain twin"]).any()


# ---- HoughLinesP ---------------------------------------------------------------------------------------------------
def test_hough_cases_cover_what_they_name():
    names = [c[0] for c in hc.hough_cases()]
    E = dict((c[0], c[1]) for c in hc.hough_cases())
    assert {E[k].shape for k in ("1x200", "200x1", "lengths")} == {(1, 200), (200, 1), (257, 300)}
    for n in (63, 64, 65, 129):
        assert int((E["%d points" % n] != 0).sum()) == n
    for G in (0, 5, 63, 64, 127, 128):
        row = E["gaps around %d" % G][110] != 0      # the middle line: a gap of exactly G
        on = np.flatnonzero(row)
        assert int(np.diff(on).max()) - 1 == G
    assert {c[4] for c in hc.hough_cases()} == {0, 20} and {(c[2], c[3]) for c in hc.hough_cases()} == set(hc.RESOLUTIONS)
    assert len(names) == len(set(names))


def test_oracle_segments_have_the_properties(oracle):
    total = 0
    for name, E, rho, theta, thr, L, G in hc.hough_cases():
        lines = oracle.hough_lines_p(E, L, G, rho=rho, theta=theta, threshold=thr)
        bad = hx.check_segments(E, lines, rho, theta, L, G)
        assert not bad, (name, len(bad), bad[:3])
        total += len(lines)
    assert total > 400  # 417 segments


def test_numpy_restatement_segments_have_the_properties():
    total = 0
    for name, E, rho, theta, thr, L, G in hc.hough_cases():
        lines = oracle_np.hough_lines_p_py(E, L, G, rho=rho, theta=theta, threshold=thr)
        bad = hx.check_segments(E, lines, rho, theta, L, G)
        assert not bad, (name, len(bad), bad[:3])
        total += len(lines)
    assert total > 400  # every case, 417 segments


def test_oracle_segments_on_canny_output(oracle):
    """the properties on real edge maps: cards through the definition's Canny"""
    for img, L, G in hc.vote_cases()[:4]:
        E = hx.canny(img)
        lines = oracle.hough_lines_p(E, L, G)
        assert len(lines) > 0
        bad = hx.check_segments(E, lines, 1.0, PI180, L, G)
        assert not bad, (img.shape, L, G, len(bad), bad[:3])


# ---- votes ---------------------------------------------------------------------------------------------------------
def test_vote_references_on_hand_cases():
    lines = np.array([[0, 0, 100, 1], [0, 10, 100, 11], [0, 20, 100, 30], [5, 5, 5, 90], [0, 50, 80, -20]], np.int32)
    a = hx.line_angles(lines)
    assert abs(a[0] - math.degrees(math.atan(0.01))) < 1e-12 and a[3] == 0.0 and abs(a[4] + math.degrees(math.atan2(70, 80))) < 1e-12
    assert hx.rust_rem(-50.0, 45.0) == -5.0 and hx.rust_rem(100.0, 45.0) == 10.0
    assert hx.vote_hough_rs(a) == a[0]
    ang, st, cand = hx.vote_omr_rs(a)
    assert ang == a[0] and st == hx.NEED_CHECK and cand.tolist() == [a[0], a[1]]
    assert hx.vote_omr_rs(np.array([1.0, 1.05, 3.0]))[1] == hx.NEED_CHECK
    assert hx.vote_omr_rs(np.array([1.0, 1.05, 1.12]))[1] == hx.BELIEVED
    ok, amb, _ = hx.check_vote(lines, float(np.float32(a[0])))
    assert ok and not amb
    assert not hx.check_vote(lines, float(a[2]))[0]
    # a pair on the window's edge is ambiguous, and either answer passes
    edge = np.array([[0, 0, 1000, 0], [0, 0, 573, 1], [0, 0, 573, 1], [0, 0, 1000, 0]], np.int32)  # 0 and 0.09999
    assert hx.check_vote(np.array([[0, 0, 7, 7]]), 44.999996)[0] and hx.check_vote(np.array([[0, 0, 7, 7]]), 0.0)[0]
    assert hx.check_vote(edge, 0.0)[0]


def _oracle_votes(oracle, cases):
    amb = 0
    for img, L, G in cases:
        lines = oracle.hough_lines_p(oracle.canny(img), L, G)
        assert len(lines) > 0
        ang, n = oracle.get_angle_with_hough(img, L, G)
        assert n == len(lines)
        ok, a1, msg = hx.check_vote(lines, ang)
        assert ok, ("hough.rs", img.shape, L, G, msg)
        ea, es, ec, en = oracle.get_result_from_edges_detection(img, L, G)
        ok, a2, msg = hx.check_omr_vote(lines, ea, es, ec)
        assert ok, ("omr.rs", img.shape, L, G, msg)
        amb += bool(a1 or a2)
    return amb


def test_oracle_votes_equal_the_float64_votes(oracle):
    cases = hc.vote_cases()
    amb = _oracle_votes(oracle, cases)
    print("vote cases %d, ambiguous %d" % (len(cases), amb))
    assert amb * 10 <= len(cases)


# ---- truth images --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [40, 150])
def test_oracle_meets_the_truth_bound(oracle, L):
    p = hc.TRUTH[L]
    worst = 0.0
    for psi in hc.PSIS:
        img = hc.truth_image(L, psi)
        G = p["gap"]
        assert p["width"] > G + 4 and p["pitch"] - p["width"] > G + 4 and p["length"] > 3 * L and p["count"] >= 6
        lines = oracle.hough_lines_p(oracle.canny(img), L, G)
        # the derivation's premise: both endpoints within 2 px, vertically, of one long side's line
        t = math.tan(math.radians(psi))
        cy, cx = (img.shape[0] - 1) / 2.0, (img.shape[1] - 1) / 2.0
        sides = np.array([((k - (p["count"] - 1) / 2.0) * p["pitch"] + s * p["width"] / 2.0) / math.cos(math.radians(psi))
                          for k in range(p["count"]) for s in (-1, 1)])
        for x0, y0, x1, y1 in lines.tolist():
            e0 = (y0 - cy) - (x0 - cx) * t - sides
            e1 = (y1 - cy) - (x1 - cx) * t - sides
            assert (np.maximum(np.abs(e0), np.abs(e1)) < 2.0).any(), (psi, (x0, y0, x1, y1))
        ang, n = oracle.get_angle_with_hough(img, L, G)
        assert n >= p["count"]
        err = hx.truth_error(ang, psi)
        worst = max(worst, err / hx.truth_bound(L))
        assert err <= hx.truth_bound(L), (psi, ang, err, hx.truth_bound(L))
    print("L %d: worst |detected - psi| / bound %.3f" % (L, worst))


# ---- mutations -----------------------------------------------------------------------------------------------------
def canny_scratch(img, low, high, mut=None):
    """A scratch copy of the restatement (fixed-point sector test, component hysteresis) with one misreading switched
    on by `mut`; with none it is the restatement."""
    from scipy import ndimage
    a = np.asarray(img, np.int64)
    if a.ndim == 2:
        a = a[:, :, None]
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="reflect" if mut == "reflect101" and min(a.shape[:2]) > 1 else "edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    if mut == "sobel transposed":
        dx, dy = dy, dx
    lo, hi = int(np.floor(min(low, high))), int(np.floor(max(low, high)))
    if mut == "l2":
        mag_c, lo, hi = dx * dx + dy * dy, lo * lo, hi * hi
    else:
        mag_c = np.abs(dx) + np.abs(dy)
    if mut == "last channel":
        best = mag_c.shape[2] - 1 - np.argmax(mag_c[:, :, ::-1], axis=2)
    else:
        best = np.argmax(mag_c, axis=2)
    ii, jj = np.indices(best.shape)
    gx, gy, c = dx[ii, jj, best], dy[ii, jj, best], mag_c[ii, jj, best]
    m = np.pad(c, 1)
    ax, ay = np.abs(gx), np.abs(gy) << 15
    t22 = ax * 13573
    t67 = t22 + (ax << 16)
    horiz = (c > m[1:-1, :-2]) & (c >= m[1:-1, 2:])
    vert = (c > m[:-2, 1:-1]) & (c >= m[2:, 1:-1])
    same = (c > m[:-2, :-2]) & (c > m[2:, 2:])
    anti = (c > m[:-2, 2:]) & (c > m[2:, :-2])
    if mut == "diagonals swapped":
        same, anti = anti, same
    diag = np.where((gx ^ gy) < 0, anti, same)
    above_lo = c >= lo if mut == ">= low" else c > lo
    keep = above_lo & np.where(ay < t22, horiz, np.where(ay > t67, vert, diag))
    strong = keep & (c >= hi if mut == ">= high" else c > hi)
    structure = ndimage.generate_binary_structure(2, 1) if mut == "4-connected" else np.ones((3, 3), int)
    lab, n = ndimage.label(keep, structure=structure)
    good = np.zeros(n + 1, bool)
    good[np.unique(lab[strong])] = True
    good[0] = False
    return (good[lab] * 255).astype(np.uint8)


CANNY_MUTATIONS = ["diagonals swapped", "sobel transposed", "reflect101", "l2", ">= low", ">= high", "4-connected",
                   "last channel"]


def test_canny_scratch_copy_is_the_restatement():
    for name, img, lo, hi in hc.canny_cases():
        assert (canny_scratch(img, lo, hi) == oracle_np.canny_np(img, lo, hi)).all(), name


@pytest.mark.parametrize("mut", CANNY_MUTATIONS)
def test_canny_mutation_is_caught(canny_exact, mut):
    caught = [name for (name, img, lo, hi), exact in zip(hc.canny_cases(), canny_exact)
              if (canny_scratch(img, lo, hi, mut) != exact).any()]
    print("%s: caught by %d of %d cases" % (mut, len(caught), len(hc.canny_cases())))
    assert caught, mut


def _clean_answer(oracle, case):
    name, E, rho, theta, thr, L, G = hc.hough_cases()[case]
    lines = oracle.hough_lines_p(E, L, G, rho=rho, theta=theta, threshold=thr)
    assert len(lines) >= 2 and not hx.check_segments(E, lines, rho, theta, L, G)
    return E.copy(), lines.copy(), rho, theta, L, G


@pytest.mark.parametrize("mut", ["endpoint off the map", "one short of L", "gap of G + 1", "duplicated endpoint",
                                 "wrong slope"])
def test_segment_mutation_is_caught(oracle, mut):
    E, lines, rho, theta, L, G = _clean_answer(oracle, 2 if mut == "wrong slope" else 0)  # the full row; the lengths
    flat = [i for i, l in enumerate(lines.tolist()) if l[1] == l[3]]
    horizontal = max(flat, key=lambda i: abs(int(lines[i, 2]) - int(lines[i, 0])))
    assert abs(int(lines[horizontal, 2]) - int(lines[horizontal, 0])) >= (250 if mut == "wrong slope" else 60)
    x0, y0, x1, y1 = lines[horizontal].tolist()
    want = {"endpoint off the map": "P1", "one short of L": "P2", "gap of G + 1": "P5", "duplicated endpoint": "P3",
            "wrong slope": "P4"}[mut]
    if mut == "endpoint off the map":
        assert not E[y0 - 1, x0]
        lines[horizontal, 1] = y0 - 1
    elif mut == "one short of L":
        x1 = x0 + (int(L) - 1) * (1 if x1 > x0 else -1)  # the segment cut to L - 1 steps, its new end on the map
        lines[horizontal, 2] = x1
        E[y0, x1] = 255
    elif mut == "gap of G + 1":
        lo = min(x0, x1) + 20
        E[max(y0 - 1, 0):y0 + 2, lo:lo + int(G) + 1] = 0
    elif mut == "duplicated endpoint":
        other = (horizontal + 1) % len(lines)
        lines[other, 2:] = lines[horizontal, :2]
    else:
        lines[horizontal, 3] = y1 + 3                 # 3 px over 250 columns or more: 0 and 1 degree give 0 and 4.4 or more
        E[y1 + 3, x1] = 255
    bad = hx.check_segments(E, lines, rho, theta, L, G)
    assert any(b.startswith(want) for b in bad), (mut, bad[:3])


@pytest.mark.parametrize("mut", ["no % 45", "window 0.2"])
def test_vote_mutation_is_caught(oracle, mut):
    caught = 0
    for img, L, G in hc.vote_cases():
        lines = oracle.hough_lines_p(oracle.canny(img), L, G)
        if mut == "no % 45":
            l = np.asarray(lines, np.float64)
            reported = hx.vote_hough_rs(np.degrees(np.arctan2(l[:, 3] - l[:, 1], l[:, 2] - l[:, 0])))
        else:
            reported = hx.vote_hough_rs(hx.line_angles(lines), width=0.2)
        caught += not hx.check_vote(lines, reported)[0]
    print("%s: caught by %d of %d cases" % (mut, caught, len(hc.vote_cases())))
    assert caught > 0, mut
