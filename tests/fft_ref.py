"""Float64 references, layouts and error measures for the FFT path's float arrays (fft.spectrum_raw, the hook
omr_fft_spectrum_raw) -- numpy only, no GPU.  tests/test_fft_ref.py proves this file on a float32 stand-in transform
(scipy.fft on complex64), tests/test_gpu_fft_spectrum.py holds the kernels to it.

The reference is the definition (oracle/oracle_fft.py's line): F = np.fft.fft2(x.astype(float64)) / (R C) with
x = float32(g) * float32(1 / 255); for the row pass np.fft.fft(x64, axis=1)[:, :C // 2 + 1].

Layouts, an [R, C] scan, H = C // 2 + 1:
  full     [R, C]   F[k, c], unshifted, DC at [0, 0]
  hook     [H, R]   column index major, what the two passes leave: row pass [c, r] = row r's bin c (complex, unscaled),
                    column pass [c, k] = |F[k, c]|
  picture  [R, C]   full after the mirror (columns c > C // 2 are |F[(R - k) % R, C - c]|) and fft_shift (fft.rs:67-86:
                    the quadrants of [0 : 2 (R // 2), 0 : 2 (C // 2)] swap, an odd last row or column stays put)
"""
import numpy as np

f32 = np.float32
FLOOR = 2e-7           # a stand-in's error counts as at least this much (about 3 float32 roundings)
ZONE = 0.01            # grey levels around a rounding boundary in which a picture byte is not compared
ZONE_MAX_SHARE = 0.05  # of a picture's pixels
MARGIN = 0.002         # grey levels by which the stand-in's pictures may differ from the kernel's before rounding


# ---------------------------------------------------------------------------------------------- inputs and references
def image_f32(g):
    """convert_to(CV_32F, 1 / 255): the alpha cast to float, as the row pass does it"""
    return (np.asarray(g, np.uint8).astype(f32) * f32(1.0 / 255.0)).astype(f32)


def ref_rows(g):
    """the row pass in float64, full layout [R, H]"""
    x = image_f32(g).astype(np.float64)
    return np.fft.fft(x, axis=1)[:, :x.shape[1] // 2 + 1]


def ref_full(g):
    """the 2-D DFT with DFT_SCALE in float64, full layout [R, C]"""
    x = image_f32(g).astype(np.float64)
    return np.fft.fft2(x) / float(x.shape[0] * x.shape[1])


def impulses(rows, cols, variant=0):
    """two pixels of 255 on black, at distinct places off the axes where the shape allows -> (g, (r0, c0), (r1, c1));
    variant moves the second one"""
    p0 = (rows // 3, cols // 5)
    flat = (((2 * rows) // 3) * cols + (3 * cols) // 4 + variant) % (rows * cols)
    if flat == p0[0] * cols + p0[1]:
        flat = (flat + 1) % (rows * cols)
    p1 = (flat // cols, flat % cols)
    g = np.zeros((rows, cols), np.uint8)
    g[p0] = g[p1] = 255
    return g, p0, p1


def impulses_closed_form(rows, cols, p0, p1):
    """F of impulses(): (v / R C) (e^{-2 pi i (k r0 / R + c c0 / C)} + the same for p1), v = float32(255) * float32(1 / 255);
    the phases are reduced as integers before they reach a cosine"""
    v = float(f32(255.0) * f32(1.0 / 255.0))
    k = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]

    def wave(p):
        num = (k * p[0] * cols + c * p[1] * rows) % (rows * cols)  # (k r / R + c c0 / C) mod 1, times R C
        return np.exp(-2j * np.pi * num.astype(np.float64) / float(rows * cols))
    return (v / float(rows * cols)) * (wave(p0) + wave(p1))


# ----------------------------------------------------------------------------------------------------------- layouts
def rows_to_hook(rowspec):
    """[R, H] -> [H, R]"""
    return np.ascontiguousarray(np.asarray(rowspec).T)


def hook_to_rows(hook):
    return np.ascontiguousarray(np.asarray(hook).T)


def full_to_hook(full):
    """[R, C] (any dtype) -> the half the passes compute, [H, R]"""
    full = np.asarray(full)
    return np.ascontiguousarray(full[:, :full.shape[1] // 2 + 1].T)


def full_to_hook_mirrored(full_mag, wrong_mirror=False):
    """the same half of |F|, taken from the OTHER side of the Hermitian mirror: [c, k] = |F[(R - k) % R, (C - c) % C]| --
    equal to full_to_hook for the spectrum of a real image.  wrong_mirror: the column taken as C - c instead of
    (C - c) % C, read from the flat row-major array as a kernel would (column C of a row is column 0 of the next row)."""
    full_mag = np.asarray(full_mag)
    rows, cols = full_mag.shape
    flat = np.concatenate([full_mag.reshape(-1), full_mag.reshape(-1)[:1]])
    k = np.arange(rows)
    out = np.empty((cols // 2 + 1, rows), full_mag.dtype)
    for c in range(cols // 2 + 1):
        mc = (cols - c) if wrong_mirror else (cols - c) % cols
        out[c] = flat[((rows - k) % rows) * cols + mc]
    return out


def hook_to_full(hook, cols, wrong_mirror=False):
    """|F| [H, R] -> [R, C]: the columns beyond C // 2 from the conjugate-symmetric points, |F[k, c]| = |F[(R - k) % R,
    (C - c) % C]|.  wrong_mirror: the row index taken as R - k instead of (R - k) % R, read from the flat array as a
    kernel would (row R of a column is row 0 of the next one) -- the error tests/test_fft_ref.py injects."""
    hook = np.asarray(hook)
    half, rows = hook.shape
    assert half == cols // 2 + 1
    out = np.empty((rows, cols), hook.dtype)
    out[:, :half] = hook.T
    k = np.arange(rows)
    flat = np.concatenate([hook.reshape(-1), hook.reshape(-1)[:rows]])
    for c in range(half, cols):
        mk = (rows - k) if wrong_mirror else (rows - k) % rows
        out[:, c] = flat[(cols - c) * rows + mk]
    return out


def fft_shift(a):
    """fft.rs:67-86"""
    a = np.array(a)
    rows, cols = a.shape
    cx, cy = cols // 2, rows // 2
    out = a.copy()
    out[0:cy, 0:cx] = a[cy:2 * cy, cx:2 * cx]
    out[cy:2 * cy, cx:2 * cx] = a[0:cy, 0:cx]
    out[0:cy, cx:2 * cx] = a[cy:2 * cy, 0:cx]
    out[cy:2 * cy, 0:cx] = a[0:cy, cx:2 * cx]
    return out


def fft_unshift(a):
    """fft_shift is its own inverse on the even part (the quadrants swap back)"""
    return fft_shift(a)


def hook_to_picture(hook, cols, wrong_mirror=False):
    """|F| [H, R] -> [R, C] in the pictures' pixel order"""
    return fft_shift(hook_to_full(hook, cols, wrong_mirror))


def picture_to_hook(pic):
    return full_to_hook(fft_unshift(pic))


# ---------------------------------------------------------------------------------------------------- error measures
def _no_dc(a):
    return np.asarray(a).reshape(-1)[1:]  # DC is element [0, 0] of the full and of the hook layout alike


def magnitude_errors(got_mag, ref, scale=None):
    """| |G| - |F| | over every bin but DC, normalised by the rms of |F| over those bins (scale: by that instead -- the
    constant image, whose other bins are all leakage, is measured against DC) -> (rel_rms, rel_max, dc): dc is the DC bin's
    error relative to itself.  got_mag and ref in one layout; ref complex or real."""
    g = np.abs(np.asarray(got_mag, np.float64))
    f = np.abs(np.asarray(ref))
    assert g.shape == f.shape
    d = np.abs(_no_dc(g) - _no_dc(f))
    if scale is None:
        scale = float(np.sqrt(np.mean(_no_dc(f) ** 2))) if d.size else 1.0
    f0, g0 = float(f.reshape(-1)[0]), float(g.reshape(-1)[0])
    dc = abs(g0 - f0) / f0 if f0 else abs(g0)
    if not d.size:
        return 0.0, 0.0, dc
    return float(np.sqrt(np.mean(d ** 2))) / scale, float(d.max()) / scale, dc


def complex_errors(got, ref, scale=None):
    """the same of |G - F|, complex (the row pass); dc = |G0 - F0| / |F0|"""
    g = np.asarray(got, np.complex128)
    f = np.asarray(ref, np.complex128)
    assert g.shape == f.shape
    d = np.abs(_no_dc(g) - _no_dc(f))
    if scale is None:
        scale = float(np.sqrt(np.mean(np.abs(_no_dc(f)) ** 2))) if d.size else 1.0
    f0, g0 = f.reshape(-1)[0], g.reshape(-1)[0]
    dc = abs(g0 - f0) / abs(f0) if f0 else abs(g0)
    if not d.size:
        return 0.0, 0.0, dc
    return float(np.sqrt(np.mean(d ** 2))) / scale, float(d.max()) / scale, dc


def bounds(standin_errors, factor):
    """the kernel's limit for each measure: `factor` times the stand-in's error on the same case, the stand-in's error
    counted as at least FLOOR (a stand-in that happens to be exact, as on a constant image, must not turn the limit into
    rounding noise: 2e-7 is three float32 roundings, the low end of what the stand-in shows on noise)"""
    return tuple(factor * max(float(e), FLOOR) for e in standin_errors)


# ------------------------------------------------------------------------------------------------------ the pictures
def pictures64(mag_picture, mn, mx):
    """launch_spec_pictures's expressions (fft.rs:90-122, :134-138) in float64 on |F| laid out as a picture, from given
    extrema: correction, * 255, the 8-bit conversion (* 255, round half to even, saturate); log(. + 1 / 255),
    correction with the images of the extrema, the 8-bit conversion.
    -> (magnitude u8, log u8, magnitude before rounding, log before rounding)"""
    mg = np.asarray(mag_picture, np.float64)
    mn, mx = float(mn), float(mx)

    def m3(v):
        return ((v - mn) * (1.0 / (mx - mn))) * 255.0

    def lg(v):
        return np.log(v + 1.0 / 255.0)
    m = m3(mg)
    pm = m * 255.0
    lmn, lmx = float(lg(m3(mn))), float(lg(m3(mx)))
    pl = ((lg(m) - lmn) * (1.0 / (lmx - lmn))) * 255.0
    return to_u8(pm), to_u8(pl), pm, pl


def to_u8(pre):
    return np.clip(np.rint(pre), 0, 255).astype(np.uint8)


def boundary_zone(pre, zone=ZONE):
    """pixels whose value before rounding lies within `zone` of a boundary between two bytes (k + 1 / 2, k = 0 .. 254)"""
    pre = np.asarray(pre, np.float64)
    frac = np.abs(pre - np.floor(pre) - 0.5)
    return (frac < zone) & (pre > 0.5 - zone) & (pre < 254.5 + zone)


def picture_check(got_u8, exp_u8, pre):
    """-> (share of pixels in the boundary zone, mismatches outside it)"""
    zone = boundary_zone(pre)
    bad = (np.asarray(got_u8) != np.asarray(exp_u8)) & ~zone
    return float(zone.mean()), int(bad.sum())


def pictures32(mag_picture, mn, mx):
    """the same expressions evaluated as the kernel evaluates them, in float32 with the double alpha / beta cast to float
    (the stand-in's pictures) -> (magnitude u8, log u8)"""
    with np.errstate(invalid="ignore", divide="ignore"):  # (a log of a negative value: wrong extrema, injected by the tests)
        return _pictures32(mag_picture, mn, mx)


def _pictures32(mag_picture, mn, mx):
    mg = np.asarray(mag_picture, f32)
    mn, mx = float(f32(mn)), float(f32(mx))
    beta, alpha = f32(-mn), f32(1.0 / (mx - mn))
    k255, inv255 = f32(255.0), f32(1.0 / 255.0)

    def m3(v):
        return ((v + beta) * alpha) * k255

    def lg(v):
        return np.log((v + inv255).astype(f32)).astype(f32)
    m = m3(mg)
    lmn, lmx = float(lg(m3(np.array([mn], f32)))[0]), float(lg(m3(np.array([mx], f32)))[0])
    beta2, alpha2 = f32(-lmn), f32(1.0 / (lmx - lmn))
    pl = ((lg(m) + beta2) * alpha2) * k255
    return to_u8((m * k255).astype(np.float64)), to_u8(pl.astype(np.float64))


# ------------------------------------------------------------------------------------------------------- the cases
MIXED = (1240, 2480, 4960, 4096)  # fft_mixed_radices: lengths with a mixed-radix kernel (4096 = 16 * 16 * 16)


def axis_path(n):
    """which factorisation AxisTables::build (oics_fft.cpp) gives a line of n points -> (name, factor): the factor by
    which the kernel's error may exceed the stand-in's, 8 for the direct transforms, 16 for the chirp transforms (three
    transforms of M >= 2 n points and two pointwise products where the stand-in runs one transform)"""
    if n in MIXED:
        return "mixed", 8
    if n & (n - 1) == 0:
        return ("pow2-inplace" if n > 8192 else "pow2"), 8
    if 2048 < n <= 4096 and n % 4 == 0:
        return "sub4-%d" % (1792 if 2 * (n // 4) - 1 <= 1792 else 2048), 16
    if 4096 < n <= 8192 and n % 8 == 0:
        return "sub8-%d" % (1792 if 2 * (n // 8) - 1 <= 1792 else 2048), 16
    m = 1
    while m < 2 * n - 1:
        m *= 2
    if m > 16384:
        return "chirp-global-%d" % m, 16
    return ("chirp-inplace" if m > 8192 else "chirp-lds"), 16


# every length once as columns (row pass, real pairs) and once as rows (column pass); the other axis 5 or 8
LENGTHS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,  # powers of two: log2 m mod 3 = 0, 1, 2 on both
                                                                         # sides of the radix-16 tail rule; 4096 mixed
           3, 7, 100, 877, 2047, 2049, 4097, 5001,                        # Bluestein in LDS, m = 8 .. 8192 and 16384 in place
           1240, 2480, 4960,                                              # mixed radix
           3508, 4000, 7016, 8160,                                        # sub-lines: SUB 4 / 8 with M 1792 / 2048
           9000, 16400)                                                   # the chirp through global memory, M 32768 / 65536
INPUTS = ("noise", "impulses", "constant", "card")


def shapes_all_inputs():
    out = []
    for i, n in enumerate(LENGTHS):
        o = 5 if i % 2 and n >= 8 else 8  # (a picture of 15 pixels has no room for one pixel near a rounding boundary)
        out += [(o, n), (n, 13 - o if n >= 8 else 8)]  # (an odd and an even other axis per length)
    # pairing edges of the row pass: 1, 2, 3 rows; an even and an odd count at a mixed-radix and at a chirp length; an odd
    # cols (the half spectrum's last column is not its own mirror) next to an even one
    out += [(1, 64), (2, 64), (3, 64), (1, 100), (2, 100), (3, 100), (6, 1240), (7, 1240), (6, 877), (7, 877), (9, 63), (9, 65), (9, 101)]
    # both passes non-trivial at once
    out += [(75, 100), (877, 1240), (333, 512)]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def shapes_noise_only():
    """every axis length from the smallest the entry points accept (1) to 33, as n x 8 and 8 x n"""
    out = []
    for n in range(1, 34):
        out += [(n, 8), (8, n)]
    return sorted(set(out))


def make_input(kind, rows, cols, variant=0):
    """-> (g uint8 [rows, cols], closed-form F or None); variant: another draw of the same kind"""
    if kind == "noise":  # uniform bytes: a flat spectrum, every bin counts
        rng = np.random.Generator(np.random.PCG64(rows * 40503 + cols + 7919 * variant))
        return rng.integers(0, 256, (rows, cols), dtype=np.uint8), None
    if kind == "impulses":
        g, p0, p1 = impulses(rows, cols, variant)
        return g, impulses_closed_form(rows, cols, p0, p1)
    if kind == "constant":
        return np.full((rows, cols), 255, np.uint8), None
    if kind == "card":
        from oics import synth
        return synth.make_card(rows, cols, rows + cols + 1000 * variant)[0], None
    raise ValueError(kind)


def choose_input(kind, rows, cols):
    """The first variant of the input whose pictures can be compared byte for byte: at most 4 % (of the 5 % allowed) of
    either picture's pixels within ZONE + MARGIN of a rounding boundary, judged on the float32 stand-in's |F|.  The
    kernel's |F| differs from it by 1e-6 of a bin, 1e-4 grey level, so a picture that passes here passes the test's own
    assertion on the kernel's |F|; a picture of a dozen pixels must have no pixel there.
    -> (g, closed form or None, standin(g))"""
    for variant in range(64):
        g, closed = make_input(kind, rows, cols, variant)
        s = standin(g)
        mn, mx = float(s[2][0]), float(s[2][1])
        if mn == mx:
            continue  # (one bin: no picture)
        # several bins tied at a minimum that is not zero differ by rounding noise alone, which the log picture's steep
        # foot turns into tenths of a grey level: their bytes depend on the transform's last bit, so they count as lying
        # in the zone (two are always there: the smallest bin of column 0 and its Hermitian twin)
        pic = hook_to_picture(s[1], cols)
        tied = (pic - mn <= 1e-5 * mn) & (mn > 1e-6 * mx)
        if tied.sum() <= 2:
            tied[:] = False
        _, _, pm, pl = pictures64(pic, mn, mx)
        if max(boundary_zone(pm, ZONE + MARGIN).mean(), (boundary_zone(pl, ZONE + MARGIN) | tied).mean()) <= 0.8 * ZONE_MAX_SHARE:
            return g, closed, s
        if kind == "constant":
            break
    raise AssertionError("no %s input of %d x %d keeps its pictures off the rounding boundaries" % (kind, rows, cols))


def standin(g):
    """the float32 stand-in transform (scipy's pocketfft on complex64) in the hook's layouts and with its extrema:
    -> (row_pass complex64 [H, R], magnitude float32 [H, R], (min, max) float32)"""
    import scipy.fft
    x = image_f32(g)
    rows, cols = x.shape
    rp = scipy.fft.fft(x.astype(np.complex64), axis=1)[:, :cols // 2 + 1]
    assert rp.dtype == np.complex64
    F = scipy.fft.fft2(x.astype(np.complex64))
    assert F.dtype == np.complex64
    F = F * f32(1.0 / (float(rows) * float(cols)))
    mag = full_to_hook(np.sqrt(F.real * F.real + F.imag * F.imag).astype(f32))
    return rows_to_hook(rp), mag, (mag.min(), mag.max())


def measure(g, closed, row_pass, magnitude):
    """the measures of section (a) and (b) for arrays in the hook's layouts -> ((rms, max, dc) of the row pass, of |F|)"""
    rows, cols = g.shape
    ref_r = rows_to_hook(ref_rows(g))
    ref_f = full_to_hook(closed if closed is not None else ref_full(g))
    scale_r = scale_f = None
    if (np.asarray(g) == g.flat[0]).all():  # a constant image: every bin but DC is leakage, measured against DC
        scale_r, scale_f = abs(ref_r[0, 0]), abs(ref_f[0, 0])
    return complex_errors(row_pass, ref_r, scale_r), magnitude_errors(magnitude, ref_f, scale_f)
