"""The Hough-line kernels held to first principles (tests/hough_exact.py) through the existing entry points, on the
inputs of tests/hough_cases.py: hough.canny against Canny's definition byte for byte; hough.hough_lines_p against the
properties P1-P5 on the device's own Canny output and on crafted edge maps; get_angle_with_hough,
get_result_from_edges_detection and their batch forms against hough.rs / omr.rs in float64 on the device's own
segments; the detected angle of strips at a known angle against the bound of hough_exact.truth_bound.  tests/test_hough_exact.py holds the
restatements to the same checks on the CPU, and keeps the mutations that show the checks bite."""
import numpy as np
import pytest

import hough_cases as hc
import hough_exact as hx
from oics import hough, omr

pytestmark = pytest.mark.gpu

PI180 = np.pi / 180.0


def test_canny_equals_the_definition():
    edge_px = 0
    for name, img, lo, hi in hc.canny_cases():
        exact = hx.canny(img, lo, hi)
        got = hough.canny(img, lo, hi)
        assert got.shape == exact.shape and (got == exact).all(), "%s: %d bytes differ" % (name, int((got != exact).sum()))
        edge_px += int((exact != 0).sum())
    print("Canny: %d cases, 0 differing bytes, %d edge pixels" % (len(hc.canny_cases()), edge_px))
    assert edge_px > 50000


def test_hysteresis_crosses_tile_corners():
    """the weak chain that only diagonal links carry across hysteresis tile corners is kept whole from its single
    strong pixel; its twin without one is dropped (the structure itself is asserted in tests/test_hough_exact.py)"""
    chains = hc.hysteresis_chains()
    exact = hx.canny(chains["chain joined"])
    got = hough.canny(chains["chain joined"])
    assert int((exact != 0).sum()) > 380 and (got == exact).all(), int((got != exact).sum())
    assert not hough.canny(chains["chain twin"]).any()


def test_segments_have_the_properties_on_crafted_maps():
    total = 0
    for name, E, rho, theta, thr, L, G in hc.hough_cases():
        lines = hough.hough_lines_p(E, rho, theta, thr, L, G)
        bad = hx.check_segments(E, lines, rho, theta, L, G)
        assert not bad, (name, len(bad), bad[:3])
        total += len(lines)
    print("P1-P5: %d segments of %d crafted maps, 0 violations" % (total, len(hc.hough_cases())))
    assert total > 400  # 417 segments


def test_segments_have_the_properties_on_device_canny():
    total = 0
    for img, L, G in hc.vote_cases():
        E = hough.canny(img)
        lines = hough.hough_lines_p(E, 1.0, PI180, 0, L, G)
        assert len(lines) > 0
        bad = hx.check_segments(E, lines, 1.0, PI180, L, G)
        assert not bad, (img.shape, L, G, len(bad), bad[:3])
        total += len(lines)
    print("P1-P5: %d segments of %d device edge maps, 0 violations" % (total, len(hc.vote_cases())))


def _device_lines(img, L, G):
    return hough.hough_lines_p(hough.canny(img), 1.0, PI180, 0, L, G)


@pytest.fixture(scope="module")
def vote_lines():
    return [_device_lines(img, L, G) for img, L, G in hc.vote_cases()]


def test_votes_equal_the_float64_votes(vote_lines):
    amb = 0
    for (img, L, G), lines in zip(hc.vote_cases(), vote_lines):
        ok, a1, msg = hx.check_vote(lines, hough.get_angle_with_hough(img, L, G))
        assert ok, ("hough.rs", img.shape, L, G, msg)
        r = omr.get_result_from_edges_detection(img, L, G)
        ok, a2, msg = hx.check_omr_vote(lines, r.angle, int(r.status), r.candidates)
        assert ok, ("omr.rs", img.shape, L, G, msg)
        amb += bool(a1 or a2)
    print("votes: %d cases, %d ambiguous" % (len(vote_lines), amb))
    assert amb * 10 <= len(vote_lines)


def test_batch_votes_of_mixed_shapes(vote_lines):
    """get_angles_with_hough groups same-shape images: per (L, G) the cases of every shape in one call"""
    amb = n = 0
    for key in sorted({(L, G) for _, L, G in hc.vote_cases()}):
        idx = [i for i, c in enumerate(hc.vote_cases()) if (c[1], c[2]) == key]
        angles, rc = hough.get_angles_with_hough([hc.vote_cases()[i][0] for i in idx], key[0], key[1])
        for k, i in enumerate(idx):
            assert rc[k] == 0
            ok, a, msg = hx.check_vote(vote_lines[i], float(angles[k]))
            assert ok, (key, hc.vote_cases()[i][0].shape, msg)
            amb += bool(a)
            n += 1
    assert amb * 10 <= n


def test_device_batch_votes():
    """hough_angles_batch_device and edges_detection_batch_device on device-resident same-shape scans: cards"""
    import torch
    from oics import synth
    rows, cols, L, G = 230, 248, 40.0, 8.0
    cases = [(synth.make_card(rows, cols, seed)[0], L, G) for seed in hc.BATCH_CARD_SEEDS]
    vote_lines = [_device_lines(*c) for c in cases]
    idx = list(range(len(cases)))
    d = torch.from_numpy(np.stack([cases[i][0] for i in idx])).to("cuda:0")
    angles, rc, nl = hough.hough_angles_batch_device(d.data_ptr(), len(idx), rows * cols, rows, cols, 1, cols, L, G)
    ang2, st2, nl2 = omr.edges_detection_batch_device(d.data_ptr(), len(idx), rows * cols, rows, cols, 1, cols, L, G)
    amb = 0
    for k, i in enumerate(idx):
        assert rc[k] == 0 and nl[k] == len(vote_lines[i]) and nl2[k] == len(vote_lines[i])
        ok, a1, msg = hx.check_vote(vote_lines[i], float(angles[k]))
        assert ok, ("hough batch", k, msg)
        ok, a2, msg = hx.check_vote(vote_lines[i], float(ang2[k]))
        assert ok, ("omr batch", k, msg)
        want = hx.certain_omr_vote(vote_lines[i])
        if want is not None:
            assert abs(float(ang2[k]) - want[0]) <= hx.EPS and int(st2[k]) == want[1], (k, ang2[k], st2[k], want[:2])
        amb += bool(a1 or a2)
    assert amb * 10 <= len(idx)


def test_large_segment_set_votes_on_the_device():
    """more than 2048 segments: the count of angle_votes_batch_kernel against the float64 vote"""
    img = hc.dense_dashes()
    L, G = 5.0, 1.0
    E = hough.canny(img)
    assert (E == hx.canny(img)).all()
    lines = hough.hough_lines_p(E, 1.0, PI180, 0, L, G)
    assert len(lines) > 2048, len(lines)
    bad = hx.check_segments(E, lines, 1.0, PI180, L, G)
    assert not bad, (len(bad), bad[:3])
    ok, amb, msg = hx.check_vote(lines, hough.get_angle_with_hough(img, L, G))
    assert ok, msg
    r = omr.get_result_from_edges_detection(img, L, G)
    ok, amb2, msg = hx.check_omr_vote(lines, r.angle, int(r.status), r.candidates)
    assert ok, msg
    assert not (amb or amb2)  # the one case of this test: the float64 winner is certain, so the check is the full one
    angles, rc = hough.get_angles_with_hough([img, img[:300].copy()], L, G)
    ok, amb3, msg = hx.check_vote(lines, float(angles[0]))
    assert rc[0] == 0 and ok and not amb3, msg
    print("large set: %d segments, not ambiguous" % len(lines))


@pytest.mark.parametrize("L", [40, 150])
def test_truth_bound(L):
    """strips at a known angle through get_angle_with_hough and through the batch form"""
    G = hc.TRUTH[L]["gap"]
    imgs = [hc.truth_image(L, psi) for psi in hc.PSIS]
    batch, rc = hough.get_angles_with_hough(imgs, float(L), G)
    worst = 0.0
    for psi, img, b, r in zip(hc.PSIS, imgs, batch, rc):
        ang = hough.get_angle_with_hough(img, float(L), G)
        assert r == 0
        for a in (ang, float(b)):
            err = hx.truth_error(a, psi)
            worst = max(worst, err / hx.truth_bound(L))
            assert err <= hx.truth_bound(L), (psi, a, err, hx.truth_bound(L))
    print("L %d: worst |detected - psi| / bound %.3f" % (L, worst))
