"""tests/fft_ref.py proved without a GPU: a float32 stand-in transform (scipy.fft on complex64) laid out as the hook
omr_fft_spectrum_raw lays its arrays out passes every check tests/test_gpu_fft_spectrum.py makes of the kernels -- held
to itself it sits far inside the limits -- and the same spectrum with one small error injected misses the check that is
there for it.  The layouts go there and back, the impulses' closed form is the float64 DFT, the pictures' float64
restatement reproduces oracle_fft.get_fft_image, and every case's input keeps its pictures off the rounding boundaries."""
import numpy as np
import pytest

import fft_ref as R
from oracle import oracle_fft as offt

SHAPES = [(8, 64), (64, 8), (9, 100), (100, 9), (75, 100), (7, 877), (33, 40)]


def _case(kind, rows, cols):
    g, closed, (rp, mag, ext) = R.choose_input(kind, rows, cols)
    return g, closed, rp, mag, ext


def _limits(g, closed, rp, mag, factor=8):
    er, ef = R.measure(g, closed, rp, mag)
    return R.bounds(er, factor), R.bounds(ef, factor)


def _within(err, lim):
    return all(e <= b for e, b in zip(err, lim))


@pytest.mark.parametrize("rows,cols", [(1, 8), (8, 1), (2, 2), (5, 7), (6, 7), (7, 6), (8, 8), (75, 100), (33, 64)])
def test_layouts_go_there_and_back(rows, cols):
    rng = np.random.Generator(np.random.PCG64(rows * 100 + cols))
    g = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    F = np.abs(R.ref_full(g))
    hook = R.full_to_hook(F)
    assert hook.shape == (cols // 2 + 1, rows)
    # the mirror rebuilds the columns the passes never compute, odd and even sizes alike
    assert np.allclose(R.hook_to_full(hook, cols), F, rtol=0, atol=1e-15)
    assert np.allclose(R.full_to_hook_mirrored(F), hook, rtol=0, atol=1e-15)
    # the shift rule is oracle_fft's (an odd last row / column stays put) and undoes itself
    pic = R.hook_to_picture(hook, cols)
    assert (pic == offt.fft_shift(R.hook_to_full(hook, cols))).all()
    assert (R.picture_to_hook(pic) == hook).all()
    if rows % 2 and cols % 2 and rows > 1 and cols > 1:
        full = R.hook_to_full(hook, cols)
        assert (pic[-1, :] == full[-1, :]).all() and (pic[:, -1] == full[:, -1]).all()
    assert pic[rows // 2, cols // 2] == F[0, 0] or rows == 1 or cols == 1
    rp = R.ref_rows(g)
    assert (R.hook_to_rows(R.rows_to_hook(rp)) == rp).all() and R.rows_to_hook(rp).shape == (cols // 2 + 1, rows)


@pytest.mark.parametrize("rows,cols", [(5, 7), (8, 100), (75, 100), (877, 8)])
def test_impulses_closed_form_is_the_dft(rows, cols):
    for variant in (0, 3):
        g, p0, p1 = R.impulses(rows, cols, variant)
        assert p0 != p1 and int(g.sum()) == 510
        closed = R.impulses_closed_form(rows, cols, p0, p1)
        assert np.abs(closed - R.ref_full(g)).max() <= 1e-15


@pytest.mark.parametrize("kind", R.INPUTS)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_standin_passes_every_check(kind, rows, cols):
    g, closed, rp, mag, (mn, mx) = _case(kind, rows, cols)
    # (a), (b): finite errors of float32 size against the float64 definition
    er, ef = R.measure(g, closed, rp, mag)
    assert max(er + ef) < 1e-4 and all(np.isfinite(er + ef)), (er, ef)
    # (c)
    assert mn == mag.min() and mx == mag.max()
    # (d): the stand-in's float32 pictures against the float64 restatement on the same |F| and extrema
    pic = R.hook_to_picture(mag, cols)
    m8, l8, pm, pl = R.pictures64(pic, mn, mx)
    a8, b8 = R.pictures32(pic, mn, mx)
    for got, exp, pre in ((a8, m8, pm), (b8, l8, pl)):
        share, bad = R.picture_check(got, exp, pre)
        assert share <= R.ZONE_MAX_SHARE and bad == 0, (share, bad)


def test_every_case_has_an_input_off_the_rounding_boundaries():
    """the GPU test's precondition for (d), judged here on the stand-in for every shape and input it runs"""
    cases = [(s, k) for s in R.shapes_all_inputs() for k in R.INPUTS] + [(s, "noise") for s in R.shapes_noise_only()]
    assert len(cases) > 300
    for (rows, cols), kind in cases:
        g, closed, (rp, mag, (mn, mx)) = R.choose_input(kind, rows, cols)
        assert g.shape == (rows, cols) and g.dtype == np.uint8
        _, _, pm, pl = R.pictures64(R.hook_to_picture(mag, cols), mn, mx)
        assert R.boundary_zone(pm).mean() <= R.ZONE_MAX_SHARE and R.boundary_zone(pl).mean() <= R.ZONE_MAX_SHARE


def test_paths_and_factors():
    want = {8: "pow2", 8192: "pow2", 16384: "pow2-inplace", 4096: "mixed", 1240: "mixed", 2480: "mixed", 4960: "mixed",
            3: "chirp-lds", 2047: "chirp-lds", 2049: "chirp-lds", 4097: "chirp-inplace", 5001: "chirp-inplace",
            3508: "sub4-1792", 4000: "sub4-2048", 7016: "sub8-1792", 8160: "sub8-2048", 9000: "chirp-global-32768",
            16400: "chirp-global-65536", 1: "pow2"}
    for n, name in want.items():
        path, factor = R.axis_path(n)
        assert path == name and factor == (16 if ("chirp" in name or "sub" in name) else 8), (n, path, factor)
    assert {R.axis_path(n)[0] for n in R.LENGTHS} == set(want.values())  # the GPU test's lengths reach every path
    assert R.bounds((0.0, 1e-6, 3e-7), 8) == (8 * 2e-7, 8e-6, 8 * 3e-7)


# ------------------------------------------------------------------------------------------------ injected errors
@pytest.fixture(scope="module")
def noise():
    rows, cols = 64, 100
    g, closed, rp, mag, ext = _case("noise", rows, cols)
    lim_r, lim_f = _limits(g, closed, rp, mag)  # the stand-in held to the kernels' tightest factor of its own error
    assert _within(R.measure(g, closed, rp, mag)[0], lim_r) and _within(R.measure(g, closed, rp, mag)[1], lim_f)
    return g, closed, rp, mag, ext, lim_r, lim_f


def test_one_bin_scaled_is_caught(noise):
    g, closed, rp, mag, _, lim_r, lim_f = noise
    c, k = np.unravel_index(int(np.argmax(mag.reshape(-1)[1:])) + 1, mag.shape)  # (a bin of the size of the rms or above)
    bad = mag.copy()
    bad[c, k] *= np.float32(1.0 + 1e-4)
    _, ef = R.measure(g, closed, rp, bad)
    assert ef[1] > lim_f[1], (ef, lim_f)
    bad = rp.copy()
    c, k = np.unravel_index(int(np.argmax(np.abs(rp).reshape(-1)[1:])) + 1, rp.shape)
    bad[c, k] *= np.float32(1.0 + 1e-4)
    er, _ = R.measure(g, closed, bad, mag)
    assert er[1] > lim_r[1], (er, lim_r)


def test_one_rotated_row_pass_line_is_caught_by_the_complex_measure_only(noise):
    g, closed, rp, mag, _, lim_r, lim_f = noise
    bad = rp.copy()
    bad[17] = (bad[17].astype(np.complex128) * np.exp(1j * 1e-4)).astype(np.complex64)
    er, _ = R.measure(g, closed, bad, mag)
    assert er[1] > lim_r[1], (er, lim_r)
    # its magnitudes are untouched: this is what the complex comparison of the row pass is for
    ref = R.rows_to_hook(R.ref_rows(g))
    assert R.magnitude_errors(np.abs(bad), ref)[1] <= 2 * R.magnitude_errors(np.abs(rp), ref)[1]


def test_two_swapped_neighbours_are_caught(noise):
    g, closed, rp, mag, _, lim_r, lim_f = noise
    bad = mag.copy()
    bad[20, 30], bad[20, 31] = mag[20, 31], mag[20, 30]
    _, ef = R.measure(g, closed, rp, bad)
    assert ef[0] > lim_f[0] and ef[1] > lim_f[1], (ef, lim_f)
    bad = rp.copy()
    bad[20, 30], bad[20, 31] = rp[20, 31], rp[20, 30]
    er, _ = R.measure(g, closed, bad, mag)
    assert er[0] > lim_r[0] and er[1] > lim_r[1], (er, lim_r)


def test_the_mirror_without_its_modulus_is_caught(noise):
    g, closed, rp, mag, (mn, mx), lim_r, lim_f = noise
    rows, cols = g.shape
    full = R.hook_to_full(mag, cols)
    # columns: C - c instead of (C - c) % C sends column 0 to the next row's first bin
    assert _within(R.measure(g, closed, rp, R.full_to_hook_mirrored(full))[1], lim_f)
    _, ef = R.measure(g, closed, rp, R.full_to_hook_mirrored(full, wrong_mirror=True))
    assert ef[1] > lim_f[1] and ef[2] > lim_f[2], (ef, lim_f)
    # rows: R - k instead of (R - k) % R moves row 0 of the mirrored half; the pictures' comparison sees it
    pic = R.hook_to_picture(mag, cols)
    m8, l8, pm, pl = R.pictures64(pic, mn, mx)
    a8, b8 = R.pictures32(R.hook_to_picture(mag, cols, wrong_mirror=True), mn, mx)
    assert R.picture_check(b8, l8, pl)[1] > 0


def test_a_twiddle_sized_error_in_one_stage_is_caught(noise):
    g, closed, rp, mag, _, lim_r, lim_f = noise
    bad = mag.copy()
    bad.reshape(-1)[4::8] *= np.float32(1.0 + 3e-5)
    _, ef = R.measure(g, closed, rp, bad)
    assert ef[0] > lim_f[0], (ef, lim_f)
    bad = rp.copy()
    bad.reshape(-1)[4::8] *= np.float32(1.0 + 3e-5)
    er, _ = R.measure(g, closed, bad, mag)
    assert er[0] > lim_r[0], (er, lim_r)


def test_wrong_scale_and_wrong_extrema_are_caught(noise):
    g, closed, rp, mag, (mn, mx), lim_r, lim_f = noise
    _, ef = R.measure(g, closed, rp, mag * np.float32(4096.0 / 4095.0))  # a wrong 1 / M
    assert ef[0] > lim_f[0] and ef[2] > lim_f[2]
    pic = R.hook_to_picture(mag, g.shape[1])
    _, l8, _, pl = R.pictures64(pic, mn, mx)
    _, b8 = R.pictures32(pic, np.float32(mn) * np.float32(2.0) + np.float32(1e-4), mx)
    assert R.picture_check(b8, l8, pl)[1] > 0


# ------------------------------------------------------------------------------------------------------ the pictures
@pytest.mark.parametrize("rows,cols,seed", [(64, 64, 1), (75, 100, 3), (65, 81, 7), (230, 248, 4)])
def test_pictures_restatement_reproduces_the_oracle(rows, cols, seed):
    from oics import synth
    g, _ = synth.make_card(rows, cols, seed)
    re, im = offt.spectrum(g)  # float64 DFT rounded to float32, shifted
    mag = np.sqrt(re * re + im * im).astype(np.float32)
    em, elg = offt.get_fft_image(g)
    m8, l8, pm, pl = R.pictures64(mag, mag.min(), mag.max())
    for got, exp, pre in ((em, m8, pm), (elg, l8, pl)):
        share, bad = R.picture_check(got, exp, pre)
        assert share <= R.ZONE_MAX_SHARE and bad == 0, (share, bad)
    # and from the hook's layout: the mirror and the shift put every bin where the oracle has it
    hook = R.picture_to_hook(mag)
    assert np.allclose(R.hook_to_picture(hook, cols), mag, rtol=1e-6, atol=1e-12)


def test_boundary_zone():
    pre = np.array([0.2, 0.495, 0.5, 0.509, 0.52, 100.5, 254.505, 254.6, 255.5, 300.0, -3.0, 65025.0])
    assert R.boundary_zone(pre).tolist() == [False, True, True, True, False, True, True, False, False, False, False, False]
    assert R.to_u8(np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.4, 1e6])).tolist() == [0, 2, 2, 254, 255, 0, 255]
