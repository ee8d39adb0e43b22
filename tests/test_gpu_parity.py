"""Parity of the HIP path (through the C ABI) against the CPU oracle and the golden vectors.
Bit-exact bar: integer projections, f64 std-dev bit patterns, arg-max index, NEAREST pixels;
INTER_LINEAR pixels within 1 grey level (tolerance written where it applies)."""
import glob
import os

import numpy as np
import pytest

import oics
from oics import projection, synth, transfer
from oics.types import RotateClipStrategy

pytestmark = pytest.mark.gpu

GENERIC, LDS, RUNS = 1, 2, 3


def load(path):
    d = np.load(path)
    rows, cols = [int(v) for v in d["shape"]]
    black = np.unpackbits(d["black_bits"], axis=1, bitorder="little")[:, :cols].astype(bool)
    return d, np.where(black, 0, 255).astype(np.uint8)


def assert_sweep_equal(got, exp, what=""):
    vp, hp, vs, hs = got[:4]
    evp, ehp, evs, ehs = exp[:4]
    assert (vp == evp).all(), "vproj differs " + what
    assert (hp == ehp).all(), "hproj differs " + what
    assert (vs.view(np.uint64) == evs.view(np.uint64)).all(), "v_sd bits differ " + what
    assert (hs.view(np.uint64) == ehs.view(np.uint64)).all(), "h_sd bits differ " + what


def test_device_present():
    assert oics.lib().omr_device_count() >= 1


@pytest.mark.parametrize("kernel", [GENERIC, LDS, RUNS])
def test_golden_vectors(golden_dir, kernel):
    files = sorted(f for f in glob.glob(os.path.join(golden_dir, "*.npz")) if "frontend" not in f and "hough" not in f and "fft_" not in f)
    assert len(files) >= 9
    for f in files:
        d, b = load(f)
        plan = projection.SweepPlan(b.shape[0], b.shape[1], int(d["max_angle"]), float(d["step"]),
                                    float(d["matrix_scale"]))
        try:
            plan.set_kernel(kernel)
        except oics.OmrError:
            assert kernel in (LDS, RUNS)
            plan.close()
            continue
        vp, hp, vs, hs, best = plan.run(b)
        plan.close()
        assert (vp == d["vproj"]).all() and (hp == d["hproj"]).all(), f
        assert (vs.view(np.uint64) == d["v_sd_bits"]).all() and (hs.view(np.uint64) == d["h_sd_bits"]).all(), f
        assert best == int(d["argmax"]) and best in d["accept"].tolist(), f
        assert projection.argmax_projection(vs, hs) == int(d["argmax"])
        N = int(float(d["max_angle"]) / float(d["step"]))
        r = oics.omr.select_projection_result(vs, hs, N, float(d["step"]))
        assert r.angle == float(d["path2_angle"]) and int(r.status) == int(d["path2_status"])


def test_fixed_point_tables_match_oracle(oracle):
    # OpenCV hal::warpAffine tables at the headline size and at odd sizes
    for (rows, cols, ma, st, sc) in ((3508, 2480, 10, 0.05, 1.0), (230, 248, 45, 0.2, 0.2), (97, 131, 45, 1.0, 1.7)):
        plan = projection.SweepPlan(rows, cols, ma, st, sc)
        Ms = oracle.rotation_matrices(rows, cols, ma, st, sc)
        for a in sorted(set([0, 1, plan.A // 3, plan.A // 2, plan.A - 1])):
            ad, bd, X0, Y0 = plan.tables(a)
            ead, ebd, eX0, eY0 = oracle.warp_tables(oracle.invert_affine(Ms[a]), cols, rows)
            assert (ad == ead).all() and (bd == ebd).all() and (X0 == eX0).all() and (Y0 == eY0).all(), (rows, a)
        plan.close()


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (33, 31), (64, 64), (65, 129), (100, 257), (300, 200)])
def test_shapes_and_both_kernels(oracle, shape):
    rows, cols = shape
    rng = np.random.Generator(np.random.PCG64(rows * 1000 + cols))
    b = np.where(rng.random((rows, cols)) < 0.3, 0, 255).astype(np.uint8)
    exp = oracle.sweep(b, 45, 1.5)
    for kernel in (GENERIC, LDS, RUNS):
        plan = projection.SweepPlan(rows, cols, 45, 1.5)
        try:
            plan.set_kernel(kernel)
        except oics.OmrError:
            assert kernel == RUNS
            plan.close()
            continue
        got = plan.run(b)
        plan.close()
        assert_sweep_equal(got, exp, "%s kernel %d" % (shape, kernel))
        assert got[4] in oracle.argmax_path1(exp[2], exp[3])[1].tolist()


def test_all_black_all_white_and_ties(oracle):
    for fill in (0, 255):
        b = np.full((50, 60), fill, np.uint8)
        exp = oracle.sweep(b, 5, 0.5)
        plan = projection.SweepPlan(50, 60, 5, 0.5)
        got = plan.run(b)
        plan.close()
        assert_sweep_equal(got, exp)
        lowest, accept = oracle.argmax_path1(exp[2], exp[3])
        assert got[4] == lowest and got[4] in accept.tolist()
    # blank page: every score is 0 -> len/2 (projection.rs:183-186)
    assert got[4] == 10


def test_non_binary_values_and_row_pitch(oracle):
    rng = np.random.Generator(np.random.PCG64(3))
    g = rng.integers(0, 256, (90, 150), dtype=np.uint8)
    g[rng.random(g.shape) < 0.2] = 0
    # black iff == 0 (transfer.rs:322), grey values are "white"
    exp = oracle.sweep(g, 10, 1.0)
    wide = np.zeros((90, 192), np.uint8)
    wide[:, :150] = g
    view = wide[:, :150]  # row pitch 192 > cols
    _, im = transfer.as_image(g)
    Ms = projection.sweep_matrices(90, 150, 10, 1.0)
    got = projection.projection_sweep(g, Ms)
    assert_sweep_equal(got, exp)
    # fused threshold: black iff <= 127 equals threshold(127,255,BINARY) then == 0
    bin_ = oracle.threshold_binary(g)
    exp_t = oracle.sweep(bin_, 10, 1.0)
    plan = projection.SweepPlan(90, 150, 10, 1.0)
    got_t = plan.run(g, black_max=127)
    plan.close()
    assert_sweep_equal(got_t, exp_t)
    del view, im


def test_arbitrary_matrices(oracle):
    # the kernel must honour any 2x3 matrix (omr.rs:159-163 passes scale != 1): scale, shear,
    # translation, reflections, big magnification (window does not fit -> generic kernel)
    rng = np.random.Generator(np.random.PCG64(11))
    b = np.where(rng.random((120, 140)) < 0.25, 0, 255).astype(np.uint8)
    Ms = []
    for _ in range(24):
        ang = rng.uniform(-180, 180)
        sc = float(rng.choice([0.2, 0.5, 1.0, 1.0, 1.3, 5.0]))
        M = oracle.get_rotation_matrix_2d(rng.uniform(0, 140), rng.uniform(0, 120), ang, sc)
        M[1] += rng.uniform(-0.2, 0.2)  # shear
        M[2] += rng.uniform(-30, 30)
        M[5] += rng.uniform(-30, 30)
        Ms.append(M)
    Ms.append(np.array([1, 0, 0, 0, 1, 0], np.float64))
    Ms.append(np.array([-1, 0, 139, 0, 1, 0], np.float64))  # mirror
    Ms.append(np.array([0.01, 0, 0, 0, 0.01, 0], np.float64))  # 100x magnification of the inverse map
    Ms = np.array(Ms)
    exp = oracle.sweep_matrices(b, Ms)
    got = projection.projection_sweep(b, Ms)
    assert_sweep_equal(got, exp)
    for kernel in (GENERIC,):
        plan = projection.SweepPlan(120, 140, matrices=Ms)
        plan.set_kernel(kernel)
        assert_sweep_equal(plan.run(b), exp)
        plan.close()


def test_singular_and_out_of_range_matrices():
    b = np.zeros((20, 20), np.uint8)
    # singular: OpenCV inverts with D = 0 -> all-zero linear part: every pixel samples (b1, b2) -> fine
    Ms = np.array([[0, 0, 3, 0, 0, 4]], np.float64)
    vp, hp, vs, hs = projection.projection_sweep(b, Ms)
    assert vp.shape == (1, 20)
    with pytest.raises(oics.OmrError):
        projection.projection_sweep(b, np.array([[1e-9, 0, 0, 0, 1e-9, 0]]))  # leaves the int32 range
    with pytest.raises(oics.OmrError):
        projection.projection_sweep(b, np.array([[np.nan, 0, 0, 0, 1, 0]]))


def test_helpers_match_oracle(oracle, golden_dir):
    d = np.load(os.path.join(golden_dir, "frontend.npz"))
    rgb = d["rgb"]
    gray = transfer.transfer_rgb_image_to_gray_image(rgb).get_mat()
    assert (gray == d["gray"]).all()
    assert (transfer.transfer_gray_image_to_thresh_binary(gray).get_mat() == oracle.threshold_binary(gray)).all()
    b = oracle.threshold_binary(gray)
    b[::3, ::2] = 0
    assert (transfer.get_vertical_projection(b) == oracle.vertical_projection(b)).all()
    assert (transfer.get_horizontal_projection(b) == oracle.horizontal_projection(b)).all()
    h, v = oics.omr.get_mat_projection_data(b)
    eh, ev = oracle.mat_projection_data(b)
    assert (h == eh).all() and (v == ev).all()
    assert transfer.get_projection_standard_deviations(b) == oracle.projection_standard_deviations(b)
    white = (255.0, 255.0, 255.0, 0.0)
    # NEAREST: exact copy of source pixels
    for clip in (RotateClipStrategy.DEFAULT, RotateClipStrategy.CONTAIN):
        for ang in (-12.6, 0.0, 33.3):
            for img in (rgb, gray):
                got = transfer.rotate_mat(img, ang, 1.0, transfer.INTER_NEAREST, 0, white, clip).get_mat()
                exp = oracle.rotate_mat(img, ang, 1.0, interp=0, clip=int(clip))
                assert got.shape == exp.shape and (got == exp).all()
    assert (transfer.rotate_mat(rgb, -12.6, 1.0, 0, 0, white, RotateClipStrategy.CONTAIN).get_mat() == d["warp_nn"]).all()
    # INTER_LINEAR: north_star tolerance = 1 grey level (the integer arithmetic is restated, so 0 is expected)
    for clip in (RotateClipStrategy.DEFAULT, RotateClipStrategy.CONTAIN):
        for ang in (7.3, -41.0):
            got = transfer.rotate_mat(rgb, ang, 1.0, transfer.INTER_LINEAR, 0, white, clip).get_mat()
            exp = oracle.rotate_mat(rgb, ang, 1.0, interp=1, clip=int(clip))
            assert got.shape == exp.shape
            assert np.abs(got.astype(int) - exp.astype(int)).max() <= 1


def test_drivers_match_oracle(oracle):
    # projection.rs:17-194 with scale_self 0.2 (integer INTER_AREA factor, as every caller uses)
    g, theta = synth.make_card(1150, 1240, 21)
    rgb = np.repeat(g[:, :, None], 3, axis=2).copy()
    rgb[:, :, 0] = np.minimum(255, rgb[:, :, 0].astype(int) + 9).astype(np.uint8)  # not grey-valued: weights matter
    ang = projection.get_angle_with_projections(rgb, 45, 0.2, 0.2, 1)
    eang, eidx = oracle.get_angle_with_projections(rgb, 45, 0.2, 0.2)
    assert ang == eang
    assert abs(ang - theta) < 0.5  # lib.rs:103-113
    # fractional INTER_AREA factor (dataset's 1237x1300 sheets: quirk-free general area path)
    g2, theta2 = synth.make_card(650, 619, 22)
    rgb2 = np.repeat(g2[:, :, None], 3, axis=2)
    assert projection.get_angle_with_projections(rgb2, 10, 0.5, 0.37, 1) == oracle.get_angle_with_projections(rgb2, 10, 0.5, 0.37)[0]
    # resize_scale 1.0: no resize at all
    assert projection.get_angle_with_projections(rgb2, 10, 0.5, 1.0, 4) == oracle.get_angle_with_projections(rgb2, 10, 0.5, 1.0)[0]
    # find_target_angle on a binarised sheet (app test.rs:83-178)
    b = oracle.threshold_binary(g2)
    _, _, vs, hs = oracle.sweep(b, 10, 0.5, want_proj=False)
    assert projection.find_target_angle(10, 0.5, b, 1) == (oracle.argmax_path1(vs, hs)[0] - 20) * 0.5
    # omr.rs:52-229 with the app's defaults (248 x 230 working size, quirk B4) and with no resize
    for (mw, mh) in ((248, 230), (0, 0), (300, 100)):
        r = oics.omr.get_result_from_projection(rgb, 45, 0.2, mw, mh)
        ea, es, ec = oracle.get_result_from_projection(rgb, 45, 0.2, mw, mh)
        assert (r.angle, int(r.status), r.candidates.tolist()) == (ea, es, ec.tolist()), (mw, mh)


def test_headline_size_against_oracle(oracle):
    # C2: 2480 x 3508, +-10 deg @ 0.05 deg (400 candidates); oracle on all host cores
    b, theta = synth.make_binary_card(3508, 2480, 2)
    plan = projection.SweepPlan(3508, 2480, 10, 0.05)
    results = {}
    for kernel in (LDS, GENERIC, RUNS):
        plan.set_kernel(kernel)
        results[kernel] = plan.run(b)
    plan.close()
    got = results[RUNS]
    assert_sweep_equal(results[GENERIC], got, "generic vs runs")
    assert_sweep_equal(results[LDS], got, "lds vs runs")
    # size-independent properties
    total = (b == 0).sum()
    assert (got[0].sum(axis=1) == got[1].sum(axis=1)).all()  # both projections count the same pixels
    # (NOT an invariant, so not asserted: "a rotation never adds black pixels".  Nearest-neighbour sampling repeats a
    # source column every 1 / (1 - cos t) pixels and a source row every 1 / |sin t|, so a candidate's count can exceed the
    # scan's by a fraction of a per cent; what must hold is the equality of the two projections' totals above, the exact
    # sums at angle 0 below, and bit-equality with the oracle.)
    assert (np.abs(got[0].sum(axis=1).astype(np.int64) - int(total)) <= 0.08 * int(total)).all()  # within the canvas loss at 10 degrees
    assert (got[0][200] == (b == 0).sum(axis=0)).all() and (got[1][200] == (b == 0).sum(axis=1)).all()  # angle 0
    exp = oracle.sweep(b, 10, 0.05, threads=os.cpu_count() or 4, fast=True)
    assert_sweep_equal(got, exp, "headline size")
    lowest, accept = oracle.argmax_path1(exp[2], exp[3])
    assert got[4] == lowest
    assert abs((got[4] - 200) * 0.05 - theta) < 0.5


def test_device_resident_batch_matches_single_runs(oracle):
    import torch
    rows, cols, n = 230, 248, 7
    cards = [synth.make_card(rows, cols, 40 + i)[0] for i in range(n)]
    dev = torch.device("cuda:0")
    scans = torch.from_numpy(np.stack(cards)).to(dev)
    best = torch.full((n,), -1, dtype=torch.int32, device=dev)
    vs = torch.zeros((n, 400), dtype=torch.float64, device=dev)
    hs = torch.zeros((n, 400), dtype=torch.float64, device=dev)
    batch = projection.Batch(rows, cols, 10, 0.05, device=0, n_streams=3)
    torch.cuda.synchronize()
    batch.run_device(scans.data_ptr(), rows * cols, cols, n, 127, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
    batch.sync()
    for i in range(n):
        e = oracle.sweep(oracle.threshold_binary(cards[i]), 10, 0.05, want_proj=False)
        assert (vs[i].cpu().numpy().view(np.uint64) == e[2].view(np.uint64)).all()
        assert (hs[i].cpu().numpy().view(np.uint64) == e[3].view(np.uint64)).all()
        assert int(best[i]) == oracle.argmax_path1(e[2], e[3])[0]
    batch.close()
    # host-buffer batch over the visible devices (omr_sweep_batch)
    bins = [oracle.threshold_binary(c) for c in cards]
    bidx, bang, _, _ = projection.sweep_batch(bins, 10, 0.05)
    assert bidx.tolist() == best.cpu().tolist()
    assert bang.tolist() == [(int(k) - 200) * 0.05 for k in bidx]


def test_plan_is_reusable_and_thread_safe(oracle):
    import threading
    b1, _ = synth.make_binary_card(200, 180, 61)
    b2, _ = synth.make_binary_card(200, 180, 62)
    e1, e2 = oracle.sweep(b1, 10, 0.5), oracle.sweep(b2, 10, 0.5)
    plan = projection.SweepPlan(200, 180, 10, 0.5)
    errs = []

    def work(b, e):
        try:
            for _ in range(5):
                assert_sweep_equal(plan.run(b), e)
                # the driver path shares cached plans between threads as the Tauri pool would
                assert projection.find_target_angle(10, 0.5, b, 1) == (oracle.argmax_path1(e[2], e[3])[0] - 20) * 0.5
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)

    ts = [threading.Thread(target=work, args=(b1, e1)), threading.Thread(target=work, args=(b2, e2))]
    [t.start() for t in ts]
    [t.join() for t in ts]
    plan.close()
    assert not errs, errs


def test_device_argmax_tie_policy(oracle):
    import torch
    rng = np.random.Generator(np.random.PCG64(17))
    dev = torch.device("cuda:0")
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    for trial in range(200):
        n = int(rng.integers(1, 700))
        levels = int(rng.integers(1, 5))  # few distinct values -> many exact ties
        v = rng.integers(0, levels, n).astype(np.float64) * 1.5
        h = rng.integers(0, levels, n).astype(np.float64) * 0.5
        dv, dh = torch.from_numpy(v).to(dev), torch.from_numpy(h).to(dev)
        oics._lib.check(oics.lib().omr_argmax_projection_device(dv.data_ptr(), dh.data_ptr(), n, out.data_ptr(), None))
        torch.cuda.synchronize()
        lowest, accept = oracle.argmax_path1(v, h)
        assert int(out.item()) == lowest, (trial, n)


def test_c2_as_baseline_words_it_401_inclusive_candidates(oracle):
    """BASELINE.json config 2 says "401 candidate angles" (-10 .. +10 inclusive); the reference's range is half-open
    (projection.rs:36-38: 400).  The inclusive set goes through omr_sweep_plan_create (arbitrary matrices): all 401 are
    run-merged and equal the oracle bit for bit; the first 400 are the half-open sweep's matrices (round-3 verdict
    item 7 / weak 9)."""
    b, theta = synth.make_binary_card(3508, 2480, 5)
    M400 = oracle.rotation_matrices(3508, 2480, 10, 0.05)
    last = oracle.get_rotation_matrix_2d(float(np.float32(2480) / np.float32(2.0)), float(np.float32(3508) / np.float32(2.0)), 10.0, 1.0)
    Ms = np.concatenate([M400, np.asarray(last, np.float64).reshape(1, 6)])
    assert Ms.shape == (401, 6)
    plan = projection.SweepPlan(3508, 2480, matrices=Ms)
    assert plan.info() == (401, 0)
    got = plan.run(b)
    plan.close()
    exp = oracle.sweep_matrices(b, Ms, threads=os.cpu_count() or 4, fast=True)
    assert_sweep_equal(got, exp, "401 inclusive candidates")
    assert got[4] == oracle.argmax_path1(exp[2], exp[3])[0]
    assert abs((got[4] - 200) * 0.05 - theta) < 0.5


def test_run_merging_kernel_covers_the_headline_sweep():
    # every candidate of +-10 deg @ 0.05 deg on an A4 scan must qualify for the run-merging kernel
    plan = projection.SweepPlan(3508, 2480, 10, 0.05)
    assert plan.info() == (400, 0)
    plan.close()
    # the app's default +-45 deg sweep is split: small angles run-merged, steep ones gathered
    plan = projection.SweepPlan(1150, 1240, 45, 0.2)
    n_runs, n_gather = plan.info()
    assert n_runs > 80 and n_gather > 80 and n_runs + n_gather == 450
    plan.close()


@pytest.mark.parametrize("shape,max_angle,step", [((700, 500), 20, 0.5), ((513, 1031), 12, 0.25), ((40, 2000), 8, 1.0),
                                                  ((2000, 37), 8, 1.0), ((257, 255), 45, 0.9),
                                                  # > 7 bands of 512 rows: the column counters flush more than once
                                                  ((4300, 300), 6, 1.5), ((7700, 70), 3, 1.0),
                                                  # > 256 columns x many word groups, last group partial
                                                  ((90, 5000), 4, 2.0)])
def test_run_merging_kernel_odd_shapes(oracle, shape, max_angle, step):
    rows, cols = shape
    rng = np.random.Generator(np.random.PCG64(rows + 7 * cols))
    # blocky random content: long runs plus isolated pixels
    b = np.where(rng.random((rows // 4 + 1, cols // 4 + 1)) < 0.3, 0, 255).astype(np.uint8)
    b = np.kron(b, np.ones((4, 4), np.uint8))[:rows, :cols].copy()
    b[rng.random(b.shape) < 0.02] = 0
    exp = oracle.sweep(b, max_angle, step)
    plan = projection.SweepPlan(rows, cols, max_angle, step)
    plan.set_kernel(RUNS)
    assert plan.info()[0] > 0
    got = plan.run(b)
    plan.close()
    assert_sweep_equal(got, exp, str(shape))


def test_pack_paths_agree(oracle):
    # wide (16-byte aligned rows) and byte-wise bit-pack must give the same sweep: odd widths, row
    # pitches that are / are not multiples of 16, both thresholds
    import torch
    rng = np.random.Generator(np.random.PCG64(23))
    dev = torch.device("cuda:0")
    for (rows, cols, pitch) in ((70, 160, 160), (70, 150, 160), (33, 47, 64), (33, 47, 47), (64, 2480, 2480)):
        g = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        g[rng.random(g.shape) < 0.3] = 0
        buf = torch.zeros((rows, pitch), dtype=torch.uint8, device=dev)
        buf[:, :cols] = torch.from_numpy(g).to(dev)
        for black_max, ref in ((127, oracle.threshold_binary(g)), (0, np.where(g == 0, 0, 255).astype(np.uint8))):
            exp = oracle.sweep(ref, 5, 1.0, want_proj=True)
            plan = projection.SweepPlan(rows, cols, 5, 1.0)
            vs = torch.zeros(plan.A, dtype=torch.float64, device=dev)
            hs = torch.zeros(plan.A, dtype=torch.float64, device=dev)
            vp = torch.zeros((plan.A, cols), dtype=torch.int32, device=dev)
            hp = torch.zeros((plan.A, rows), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            plan.run_device(buf.data_ptr(), pitch, black_max, None, vp.data_ptr(), hp.data_ptr(), vs.data_ptr(),
                            hs.data_ptr(), None)
            torch.cuda.synchronize()
            plan.close()
            assert (vp.cpu().numpy().astype(np.uint32) == exp[0]).all(), (rows, cols, pitch, black_max)
            assert (hp.cpu().numpy().astype(np.uint32) == exp[1]).all(), (rows, cols, pitch, black_max)
            assert (vs.cpu().numpy().view(np.uint64) == exp[2].view(np.uint64)).all()
            assert (hs.cpu().numpy().view(np.uint64) == exp[3].view(np.uint64)).all()


def test_device_resident_stages_match_oracle(oracle):
    """Front end (omr.rs:87-139) and final warp (transfer.rs:487-519) on device buffers, tuned
    1-channel / 4-px-per-lane kernels and their generic fallbacks."""
    import ctypes as C
    import torch
    from oics._lib import check, lib, u8p
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(31))
    L = lib()
    for (rows, cols) in ((1150, 1240), (115, 125), (64, 64), (37, 41)):
        rgb = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        d_rgb = torch.from_numpy(rgb).to(dev)
        d_gray = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
        check(L.omr_rgb_to_gray_device(d_rgb.data_ptr(), cols * 3, rows, cols, 3, d_gray.data_ptr(), cols, None))
        gray = oracle.rgb2gray(rgb)
        assert (d_gray.cpu().numpy() == gray).all(), (rows, cols)
        d_er = torch.empty_like(d_gray)
        check(L.omr_erode3_device(d_gray.data_ptr(), cols, rows, cols, d_er.data_ptr(), cols, None))
        er = oracle.erode_cross3(gray, 3)
        assert (d_er.cpu().numpy() == er).all(), (rows, cols)
        d_th = torch.empty_like(d_gray)
        check(L.omr_threshold_binary_device(d_gray.data_ptr(), cols, rows, cols, d_th.data_ptr(), cols, None))
        assert (d_th.cpu().numpy() == oracle.threshold_binary(gray)).all()
        for k in (2, 5):
            if rows % k or cols % k:  # fractional factors: resizeArea_'s tap tables (used to be -213)
                d_frac = torch.empty((rows // k + 1, cols // k), dtype=torch.uint8, device=dev)
                check(L.omr_resize_area_device(d_er.data_ptr(), cols, rows, cols, 1, d_frac.data_ptr(), cols // k,
                                               rows // k + 1, cols // k, None))
                assert (d_frac.cpu().numpy() == oracle.resize_area(er, rows // k + 1, cols // k)).all(), (rows, cols, k)
                continue
            d_small = torch.empty((rows // k, cols // k), dtype=torch.uint8, device=dev)
            check(L.omr_resize_area_device(d_er.data_ptr(), cols, rows, cols, 1, d_small.data_ptr(), cols // k,
                                           rows // k, cols // k, None))
            assert (d_small.cpu().numpy() == oracle.resize_area(er, rows // k, cols // k)).all(), (rows, cols, k)
        white = np.array([255, 255, 255, 0], np.uint8)
        for clip in (0, 1):
            for interp in (0, 1):
                for ang in (-7.35, 3.1, 44.0):
                    dr, dc = C.c_int32(), C.c_int32()
                    check(L.omr_rotate_size(rows, cols, ang, clip, C.byref(dr), C.byref(dc)))
                    for (img, d_img, cn) in ((gray, d_gray, 1), (rgb, d_rgb, 3)):
                        shape = (dr.value, dc.value) if cn == 1 else (dr.value, dc.value, 3)
                        d_out = torch.empty(shape, dtype=torch.uint8, device=dev)
                        check(L.omr_rotate_device(d_img.data_ptr(), cols * cn, rows, cols, cn, ang, 1.0, interp,
                                                  white.ctypes.data_as(u8p), clip, d_out.data_ptr(), dc.value * cn,
                                                  dr.value, dc.value, None))
                        torch.cuda.synchronize()
                        exp = oracle.rotate_mat(img, ang, 1.0, interp=interp, clip=clip)
                        got = d_out.cpu().numpy()
                        assert got.shape == exp.shape
                        if interp == 0:
                            assert (got == exp).all(), (rows, cols, clip, ang, cn)
                        else:  # north_star tolerance for the bilinear warp: 1 grey level
                            assert np.abs(got.astype(int) - exp.astype(int)).max() <= 1, (rows, cols, clip, ang, cn)


def test_batch_launch_groups_do_not_change_results(oracle):
    """omr_batch_set_group: several scans per kernel launch (blockIdx.z) -- same bits as one per launch."""
    import torch
    rows, cols, n = 301, 437, 7
    cards = [synth.make_card(rows, cols, 70 + i)[0] for i in range(n)]
    d = torch.from_numpy(np.stack(cards)).to("cuda:0")
    N, A = projection.candidate_count(10, 0.25)
    res = {}
    for group in (1, 3, 4):
        best = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        vs = torch.zeros((n, A), dtype=torch.float64, device="cuda:0")
        hs = torch.zeros((n, A), dtype=torch.float64, device="cuda:0")
        b = projection.Batch(rows, cols, 10, 0.25, device=0, n_streams=1)
        b.set_group(group)
        for _ in range(2):  # twice: scratch sets are reused
            b.run_device(d.data_ptr(), rows * cols, cols, n, 127, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
        b.sync()
        res[group] = (best.cpu().numpy().copy(), vs.cpu().numpy().copy(), hs.cpu().numpy().copy())
        b.close()
    for group in (3, 4):
        assert (res[group][0] == res[1][0]).all()
        assert (res[group][1].view(np.uint64) == res[1][1].view(np.uint64)).all()
        assert (res[group][2].view(np.uint64) == res[1][2].view(np.uint64)).all()
    for i in (0, n - 1):
        bimg = oracle.threshold_binary(cards[i])
        _, _, evs, ehs = oracle.sweep(bimg, 10, 0.25)
        assert (res[4][1][i].view(np.uint64) == evs.view(np.uint64)).all()
        assert (res[4][2][i].view(np.uint64) == ehs.view(np.uint64)).all()


@pytest.mark.parametrize("rows,cols,ma,st,sc", [(253, 129, 15, 0.2, 0.2), (394, 882, 15, 0.25, 0.2), (610, 685, 15, 1.0, 0.2)])
def test_gather_tiles_of_odd_height(oracle, rows, cols, ma, st, sc):
    """Strongly magnified inverse maps (omr.rs:162's scale 0.2 at 15 degrees) get LDS tiles of 6, 3, 2 or 1
    rows: a group of four rows may then straddle the 64-row block of the row counters (found by
    tests/fuzz/fuzz_sweep.py; the gather kernel used to mis-park those counts)."""
    rng = np.random.Generator(np.random.PCG64(rows + cols))
    b = np.where(rng.random((rows, cols)) < 0.3, 0, 255).astype(np.uint8)
    exp = oracle.sweep(b, ma, st, sc)
    for kernel in (0, GENERIC, LDS):
        plan = projection.SweepPlan(rows, cols, ma, st, sc)
        plan.set_kernel(kernel)
        got = plan.run(b)
        plan.close()
        assert_sweep_equal(got, exp, "kernel %d" % kernel)


def test_strided_and_unaligned_views(oracle):
    """cv::Mat ROIs reach the ABI with step_bytes > cols * channels and odd base addresses: the entry
    points must honour the stride (2-D copies, the scalar bit-pack) exactly like packed inputs."""
    import ctypes as C
    from oics import hough
    from oics._lib import OmrImage, OmrImageOwned, check, f64p, lib, u8p, u32p
    rng = np.random.Generator(np.random.PCG64(99))
    big = np.where(rng.random((300, 517)) < 0.25, 0, 255).astype(np.uint8)
    view = big[7:7 + 240, 13:13 + 401]                      # step 517, base address odd
    assert not view.flags["C_CONTIGUOUS"]
    packed = np.ascontiguousarray(view)
    im = OmrImage(view.ctypes.data, view.shape[0], view.shape[1], 1, view.strides[0])
    Ms = oracle.rotation_matrices(240, 401, 5, 0.5)
    A = Ms.shape[0]
    vp, hp = np.zeros((A, 401), np.uint32), np.zeros((A, 240), np.uint32)
    vs, hs = np.zeros(A), np.zeros(A)
    check(lib().omr_projection_sweep(C.byref(im), Ms.ctypes.data_as(f64p), A, vp.ctypes.data_as(u32p),
                                     hp.ctypes.data_as(u32p), vs.ctypes.data_as(f64p), hs.ctypes.data_as(f64p)))
    assert_sweep_equal((vp, hp, vs, hs), oracle.sweep(packed, 5, 0.5), "strided view")
    # Canny and rotate on a strided 3-channel ROI
    col = rng.integers(0, 256, (200, 333, 3), dtype=np.uint8)
    v3 = col[5:150, 9:290]
    p3 = np.ascontiguousarray(v3)
    im3 = OmrImage(v3.ctypes.data, v3.shape[0], v3.shape[1], 3, v3.strides[0])
    out = OmrImageOwned()
    check(lib().omr_canny(C.byref(im3), 50.0, 150.0, C.byref(out)))
    assert (hough._take(out) == oracle.canny(p3)).all()
    out = OmrImageOwned()
    border = np.array([255, 255, 255, 0], np.uint8)
    check(lib().omr_rotate(C.byref(im3), 7.5, 1.0, 0, border.ctypes.data_as(u8p), 1, C.byref(out)))
    assert (hough._take(out) == oracle.rotate_mat(p3, 7.5, 1.0, 0, (255, 255, 255, 0), 1)).all()


def test_per_call_drivers_under_threads(oracle):
    """Worker threads of the host application call the per-file drivers concurrently; their device
    buffers come from the shared block cache (engine.cpp) -- results must not depend on the interleaving."""
    import threading
    from oics import omr
    cards = []
    for k in range(4):
        g, _ = synth.make_card(400 + 37 * k, 520 - 29 * k, 80 + k)
        cards.append(np.stack([g, np.roll(g, 1, 0), g], axis=2))
    exp = [oracle.get_result_from_projection(c, 45, 0.2, 248, 230) for c in cards]
    rot = [oracle.rotate_mat(c, 3.0 + k, 1.0, 0, (255, 255, 255, 0), 1) for k, c in enumerate(cards)]
    errs = []

    def work(k):
        try:
            for _ in range(15):
                r = omr.get_result_from_projection(cards[k], 45, 0.2, 248, 230)
                assert r.angle == exp[k][0] and int(r.status) == exp[k][1] and r.candidates.tolist() == exp[k][2].tolist()
                got = transfer.rotate_mat(cards[k], 3.0 + k, 1.0, 0, 0, (255, 255, 255, 0), RotateClipStrategy.CONTAIN).get_mat()
                assert (got == rot[k]).all()
        except Exception as e:  # noqa: BLE001
            errs.append((k, repr(e)[:200]))

    ts = [threading.Thread(target=work, args=(k % 4,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def test_degenerate_inputs(oracle):
    """Blank, solid, one-pixel-wide and tiny scans; null / empty images are refused with the
    OpenCV-style codes instead of crashing."""
    import ctypes as C
    from oics import omr
    from oics._lib import OmrImage, lib
    for rows, cols in ((1, 1), (1, 200), (200, 1), (2, 3), (33, 64)):
        for fill in (255, 0):
            b = np.full((rows, cols), fill, np.uint8)
            plan = projection.SweepPlan(rows, cols, 5, 0.5)
            got = plan.run(b)
            plan.close()
            assert_sweep_equal(got, oracle.sweep(b, 5, 0.5), "%dx%d fill %d" % (rows, cols, fill))
            assert got[4] == oracle.argmax_path1(got[2], got[3])[0]
    # path 2 on a blank sheet: the reference would index an empty candidate list (omr.rs:211) -> NotAResult
    blank = np.full((300, 400, 3), 255, np.uint8)
    r = omr.get_result_from_projection(blank, 45, 0.2, 248, 230)
    ea, es, ec = oracle.get_result_from_projection(blank, 45, 0.2, 248, 230)
    assert int(r.status) == es == 2 and r.angle == ea
    # refused inputs
    vs, hs = np.zeros(4), np.zeros(4)
    M = oracle.rotation_matrices(8, 8, 1, 0.5)
    A = M.shape[0]
    data = np.zeros((8, 8), np.uint8)
    f64p = C.POINTER(C.c_double)
    for im, code in ((OmrImage(None, 8, 8, 1, 8), -5), (OmrImage(data.ctypes.data, 0, 8, 1, 8), -215),
                     (OmrImage(data.ctypes.data, 8, 8, 1, 4), -5), (OmrImage(data.ctypes.data, 8, 8, 3, 24), -215)):
        rc = lib().omr_projection_sweep(C.byref(im), M.ctypes.data_as(f64p), A, None, None, vs.ctypes.data_as(f64p),
                                        hs.ctypes.data_as(f64p))
        assert rc == code, (rc, code, lib().omr_last_error())


def test_resizers_match_oracle(oracle):
    """TransformableMatrix::scale_self / shrink_to / resize_self (transfer.rs:66-145) in every branch of
    OpenCV's resize dispatch: INTER_LINEAR enlargement, INTER_AREA integer / fractional shrink, INTER_AREA's
    bilinear emulation when an axis enlarges, identity -- exact."""
    rng = np.random.Generator(np.random.PCG64(77))
    for shape in ((37, 53), (64, 48, 3), (1, 9), (9, 1), (120, 200, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        for scale in (1.5, 2.0, 3.7, 1.0, 0.5, 0.2, 0.37):
            r, c = img.shape[:2]
            if int(r * scale) < 1 or int(c * scale) < 1:
                continue
            got = transfer.TransformableMatrix(img).scale_self(scale).get_mat()
            exp = oracle.scale_self(img, scale)
            assert got.shape == exp.shape and (got == exp).all(), (shape, scale)
        for (mw, mh) in ((20, 20), (0, 5), (1000, 1000), (30, 0)):
            r, c = img.shape[:2]
            t = min(1.0 if mw <= 0 else mw / c, 1.0 if mh <= 0 else mh / r)
            if t < 1.0 and (int(r * t) < 1 or int(c * t) < 1):  # empty target: OpenCV's resize raises, so do we
                with pytest.raises(oics.OmrError):
                    transfer.TransformableMatrix(img).shrink_to(mw, mh)
                continue
            got = transfer.TransformableMatrix(img).shrink_to(mw, mh).get_mat()
            exp = oracle.shrink_to(img, mw, mh)
            assert got.shape == exp.shape and (got == exp).all(), (shape, mw, mh)
        for (w, h) in ((80, 90), (11, 7), (shape[1], shape[0]), (shape[1] * 2, max(1, shape[0] // 2)), (5, 300)):
            got = transfer.TransformableMatrix(img).resize_self(w, h).get_mat()
            exp = oracle.resize_area(img, h, w)
            assert got.shape == exp.shape and (got == exp).all(), (shape, w, h)


def test_small_inputs_are_enlarged_like_the_reference(oracle):
    """Round-1 verdict, missing item 4: a 200x150 photo with the app's 248x230 defaults makes path 2 UP-scale
    (omr.rs:60-82 has no clamp; resize INTER_AREA then runs OpenCV's bilinear emulation) -- used to be -213."""
    from oics import omr
    for seed, (rows, cols) in ((5, (150, 200)), (6, (97, 131)), (7, (229, 247))):
        g, th = synth.make_card(rows, cols, seed, skew=3.2)
        bgr = np.stack([g, g, g], axis=2)
        r = omr.get_result_from_projection(bgr, 45, 0.2, 248, 230)
        ea, es, ec = oracle.get_result_from_projection(bgr, 45, 0.2, 248, 230)
        assert np.float64(r.angle).view(np.uint64) == np.float64(ea).view(np.uint64) and int(r.status) == es
        assert r.candidates.size == ec.size and (r.candidates.view(np.uint64) == ec.view(np.uint64)).all()
        ang, chk, rot = omr.correct_default(bgr, 45, 0.2, 248, 230, 30.0, 10.0)
        if es == 0:
            e_ang, e_chk = ea, False
        else:
            ha, _, _, nl = oracle.get_result_from_edges_detection(bgr, 30.0, 10.0)
            e_ang, e_chk = oracle.correct_default_decision(ea, es, ec, ha)
        assert np.float64(ang).view(np.uint64) == np.float64(e_ang).view(np.uint64) and chk == e_chk
    # path 1 with resize_scale > 1: scale_self enlarges with INTER_LINEAR (projection.rs:24-27, transfer.rs:82-86)
    g, th = synth.make_card(120, 160, 8, skew=-4.0)
    bgr = np.stack([g, g, g], axis=2)
    for scale in (1.5, 2.0, 1.01):
        got = projection.get_angle_with_projections(bgr, 10, 0.5, scale, 1)
        exp, _ = oracle.get_angle_with_projections(bgr, 10, 0.5, scale)
        assert got == exp, scale


def test_resize_area_device_all_branches(oracle):
    import torch
    from oics._lib import check, lib
    rng = np.random.Generator(np.random.PCG64(78))
    img = rng.integers(0, 256, (90, 130), dtype=np.uint8)
    d = torch.from_numpy(img).to("cuda:0")
    for (dr, dc) in ((18, 26), (45, 65), (33, 47), (90, 130), (180, 260), (200, 100), (91, 131)):
        out = torch.zeros((dr, dc), dtype=torch.uint8, device="cuda:0")
        check(lib().omr_resize_area_device(d.data_ptr(), 130, 90, 130, 1, out.data_ptr(), dc, dr, dc, None))
        torch.cuda.synchronize()
        exp = oracle.resize_area(img, dr, dc)
        assert (out.cpu().numpy() == exp).all(), (dr, dc)
    # colour, integer factors that differ per axis (ky = 3, kx = 4), a row pitch that is no multiple of 4
    img3 = rng.integers(0, 256, (12, 20, 3), dtype=np.uint8)
    buf = np.full((12, 61), 7, np.uint8)
    buf[:, :60] = img3.reshape(12, 60)
    d3 = torch.from_numpy(buf).to("cuda:0")
    out3 = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda:0")
    check(lib().omr_resize_area_device(d3.data_ptr(), 61, 12, 20, 3, out3.data_ptr(), 15, 4, 5, None))
    torch.cuda.synchronize()
    assert (out3.cpu().numpy() == oracle.resize_area(img3, 4, 5)).all()


def test_fused_erode_fast_path_edges(oracle):
    """erode3x_cross_x4_kernel (4 px per lane, packed 16-bit minima): widths that end inside a dword, padded
    row pitch, heights that end inside a strip / tile, tiny images, all-black and checkerboard content."""
    import torch
    from oics._lib import check, lib
    rng = np.random.Generator(np.random.PCG64(123))
    for (rows, cols, pitch) in ((70, 259, 260), (64, 256, 256), (1, 4, 4), (5, 3, 4), (129, 1030, 1032), (200, 77, 80)):
        for kind in ("rand", "sparse", "check"):
            if kind == "rand":
                img = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
            elif kind == "sparse":
                img = np.where(rng.random((rows, cols)) < 0.02, 0, 255).astype(np.uint8)
            else:
                img = (((np.arange(rows)[:, None] // 3 + np.arange(cols)[None, :] // 5) & 1) * 200 + 20).astype(np.uint8)
            buf = np.full((rows, pitch), 7, np.uint8)
            buf[:, :cols] = img
            d = torch.from_numpy(buf).to("cuda:0")
            out = torch.full((rows, pitch), 9, dtype=torch.uint8, device="cuda:0")
            check(lib().omr_erode3_device(d.data_ptr(), pitch, rows, cols, out.data_ptr(), pitch, None))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (got[:, :cols] == oracle.erode_cross3(img, 3)).all(), (rows, cols, kind)
            assert (got[:, cols:] == 9).all()  # padding bytes of the destination stay untouched


def test_large_results_through_the_staging_buffer(oracle):
    """Image-sized results leave the device through a per-thread pinned staging buffer (engine.cpp staged_d2h):
    packed and strided destinations, sizes around the 256 KB switch and above one staging piece."""
    import ctypes as C
    from oics._lib import check, lib, u8p
    from oics.transfer import as_image
    rng = np.random.Generator(np.random.PCG64(321))
    for (rows, cols, pitch) in ((600, 700, 700), (600, 700, 768), (300, 800, 801), (20, 30, 64), (9000, 8000, 8000)):
        g = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        a, im = as_image(g)
        out = np.full((rows, pitch), 7, np.uint8)
        check(lib().omr_threshold_binary(C.byref(im), out.ctypes.data_as(u8p), pitch))
        assert (out[:, :cols] == np.where(g > 127, 255, 0)).all(), (rows, cols, pitch)
        assert (out[:, cols:] == 7).all()
