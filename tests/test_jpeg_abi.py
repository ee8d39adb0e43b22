"""CPU-side checks of the JPEG encoder's boundary (omr_jpeg_*, omr_correct_default_batch_jpeg, omr_bytes_free): declared
in the header, the ctypes table and ffi.rs alike and exported; the host-only entry points against tests/jpeg_ref.py; every
argument error before any device work; the Python and Rust front doors."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import jpeg_ref  # noqa: E402
import oics  # noqa: E402
from oics import _lib, jpeg, omr  # noqa: E402

NEW = {
    "omr_jpeg_quant_tables": ("int", ["int32_t", "uint16_t *", "uint16_t *"]),
    "omr_jpeg_bound": ("int", ["int32_t", "int32_t", "int32_t", "int64_t *"]),
    "omr_jpeg_encode_batch_device": ("int", ["const uint8_t *", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t",
                                             "const int32_t *", "int32_t", "int32_t", "uint8_t *", "int64_t", "int64_t *"]),
    "omr_jpeg_encode": ("int", ["const omr_image *", "int32_t", "uint8_t *", "int64_t", "int64_t *"]),
    "omr_correct_default_batch_jpeg": ("int", ["const omr_image *", "int32_t", "uint16_t", "double", "int32_t", "int32_t",
                                               "double", "double", "int32_t", "double *", "int32_t *", "int32_t *",
                                               "uint8_t * *", "int64_t *"]),
    "omr_bytes_free": ("void", ["uint8_t *"]),
}
# what ffi.rs must say, argument for argument (written out here, not derived with the generator's own mapping)
RUST = {
    "omr_jpeg_quant_tables": (["i32", "*mut u16", "*mut u16"], "c_int"),
    "omr_jpeg_bound": (["i32", "i32", "i32", "*mut i64"], "c_int"),
    "omr_jpeg_encode_batch_device": (["*const u8", "i64", "i64", "i32", "i32", "i32", "*const i32", "i32", "i32", "*mut u8", "i64",
                                      "*mut i64"], "c_int"),
    "omr_jpeg_encode": (["*const OmrImage", "i32", "*mut u8", "i64", "*mut i64"], "c_int"),
    "omr_correct_default_batch_jpeg": (["*const OmrImage", "i32", "u16", "f64", "i32", "i32", "f64", "f64", "i32", "*mut f64",
                                        "*mut i32", "*mut i32", "*mut *mut u8", "*mut i64"], "c_int"),
    "omr_bytes_free": (["*mut u8"], None),
}
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint16_t": C.c_uint16, "double": C.c_double}
SHAPES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 16), (16, 17), (37, 53), (64, 48)]
PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)
NO_GPU = oics.lib().omr_device_count() < 1


def _err():
    return oics.lib().omr_last_error().decode()


def test_symbols_agree_everywhere():
    import gen_shim_ffi as g
    decls = {name: (ret, [t for t, _ in params]) for name, ret, params in g.parse_header()}
    L = C.CDLL(_lib.LIB_PATH)
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for name, (ret, args) in NEW.items():
        assert decls[name] == (ret, args), (name, decls.get(name))
        assert hasattr(L, name)
        res, at = _lib.SYMBOLS[name]
        assert (res is None) == (ret == "void") and len(at) == len(args), name
        for c, t in zip(args, at):
            if "*" in c:
                assert t is C.c_void_p or hasattr(t, "contents") or hasattr(t, "_type_"), (name, c, t)
            else:
                assert t is CTYPES[c], (name, c, t)
        m = re.search(r"pub fn %s\(([^)]*)\)( -> (\w+))?;" % name, ffi)
        assert m, name
        rust_args = [a.split(":", 1)[1].strip() for a in m.group(1).split(",") if a.strip()]
        assert (rust_args, m.group(3)) == RUST[name], (name, rust_args, m.group(3))


def test_quant_tables_equal_the_restatement():
    for q in range(-3, 105):
        luma, chroma = jpeg.quant_tables(q)
        rl, rc = jpeg_ref.quant_tables(q)
        assert (luma == rl).all() and (chroma == rc).all(), q
    assert oics.lib().omr_jpeg_quant_tables(50, None, None) == -5


def test_bound_holds_and_is_monotone():
    for rows, cols in SHAPES:
        for cn in (1, 3):
            shape = (rows, cols) if cn == 1 else (rows, cols, 3)
            rng = np.random.Generator(np.random.PCG64(rows + 31 * cols))
            noise = rng.integers(0, 256, shape, dtype=np.uint8)
            c = ((np.add.outer(np.arange(rows), np.arange(cols)) & 1) * 255).astype(np.uint8)
            checker = c if cn == 1 else np.repeat(c[..., None], 3, 2)
            b = jpeg.bound(rows, cols, cn)
            for img in (noise, checker):
                assert len(jpeg_ref.encode(img, 100)) <= b, (rows, cols, cn)
    for cn in (1, 3):
        last = 0
        for r in range(1, 70):
            b = jpeg.bound(r, 33, cn)
            assert b >= last and jpeg.bound(33, r, cn) >= jpeg.bound(33, max(r - 1, 1), cn)
            last = b
    # the derivation: header + 2 x ceil(blocks x 1660 / 8) + EOI
    assert jpeg.bound(16, 16, 3) == 623 + 2 * ((6 * 1660 + 7) // 8) + 2
    assert jpeg.bound(8, 9, 1) == 623 + 2 * ((2 * 1660 + 7) // 8) + 2
    out = C.c_int64(-1)
    L = oics.lib()
    assert L.omr_jpeg_bound(8, 8, 3, None) == -5
    assert L.omr_jpeg_bound(0, 8, 3, C.byref(out)) == -215 and L.omr_jpeg_bound(8, 65536, 1, C.byref(out)) == -215
    assert L.omr_jpeg_bound(8, 8, 2, C.byref(out)) == -215 and L.omr_jpeg_bound(8, 8, 4, C.byref(out)) == -213
    assert out.value == -1


def _batch(d_imgs=0x1000, stride=None, step=None, rows=16, cols=24, cn=3, sizes=None, n=2, q=90, d_out=0x2000,
           out_stride=None, out_len=True):
    step = cols * cn if step is None else step
    stride = rows * step if stride is None else stride
    out_stride = 1 << 40 if out_stride is None else out_stride
    lens = np.full(max(n, 1), -7, np.int64)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
    rc = oics.lib().omr_jpeg_encode_batch_device(d_imgs, stride, step, rows, cols, cn,
                                                 None if sz is None else sz.ctypes.data_as(_lib.i32p), n, q, d_out, out_stride,
                                                 lens.ctypes.data_as(C.POINTER(C.c_int64)) if out_len else None)
    return rc, lens


def test_batch_argument_errors_come_before_any_device_work():
    """the pointers are not device memory: a call that touched them would crash, with or without a GPU"""
    cases = [
        (dict(d_imgs=None), -5, "null"), (dict(d_out=None), -5, "null"), (dict(out_len=False), -5, "null"),
        (dict(n=-1), -5, "negative n"),
        (dict(cn=2), -215, "1 or 3 channels"), (dict(cn=4), -213, "not implemented"),
        (dict(rows=0), -215, "empty"), (dict(cols=70000), -215, "65535"),
        (dict(step=24 * 3 - 1), -5, "step_bytes"), (dict(stride=16 * 72 - 1), -5, "img_stride_bytes"),
        (dict(sizes=[[16, 24], [17, 24]]), -5, "sizes[1]"), (dict(sizes=[[16, 25], [1, 1]]), -5, "sizes[0]"),
        (dict(sizes=[[16, 24], [-1, 3]]), -5, "sizes[1]"), (dict(sizes=[[0, 5], [1, 1]]), -5, "sizes[0]"),
        (dict(out_stride=jpeg.bound(16, 24, 3) - 1), -5, "omr_jpeg_bound"),
    ]
    for kw, code, text in cases:
        rc, lens = _batch(**kw)
        assert rc == code and text in _err(), (kw, rc, _err())
        assert (lens == -7).all(), kw
    rc, lens = _batch(n=0)
    assert rc == 0 and (lens == -7).all()


def test_bad_sizes_have_the_wording_all_four_encoders_share():
    """the same four bad `sizes` stand in test_jpeg_abi, test_png_encode_abi, test_tiff_encode_abi and test_tiff8_encode_abi:
    every encoder's batch entry point answers them with these words, to the letter"""
    for sizes, text in [([[16, 24], [17, 24]], "sizes[1] = 17 x 24 does not fit the 16 x 24 slot"),
                        ([[16, 25], [1, 1]], "sizes[0] = 16 x 25 does not fit the 16 x 24 slot"),
                        ([[16, 24], [-1, 3]], "sizes[1] = -1 x 3 does not fit the 16 x 24 slot"),
                        ([[0, 5], [1, 1]], "sizes[0] = 0 x 5 does not fit the 16 x 24 slot")]:
        rc, lens = _batch(sizes=sizes)
        assert rc == -5 and _err() == text and (lens == -7).all(), (sizes, rc, _err())


def test_the_2_pow_32_bit_decision():
    """Bit offsets inside an image are 32-bit on the device, so a slot whose scan could exceed 2^32 bits is refused with
    -215 before any device work.  From omr_jpeg_bound's arithmetic: blocks x 1660 bits; 3 channels, 16 x 16 MCUs of 6."""
    def worst_bits(rows, cols, cn):
        return (jpeg.bound(rows, cols, cn) - 623 - 2) // 2 * 8   # ceil to bytes: within 7 bits of blocks x 1660

    ok = (10496, 10496)      # 656 x 656 MCUs: 4 285 747 200 bits, below 2^32 = 4 294 967 296
    big = (10512, 10512)     # 657 x 657 MCUs: 4 298 823 240 bits
    assert worst_bits(*ok, 3) < 2 ** 32 - 64 < 2 ** 32 < worst_bits(*big, 3)
    huge = 1 << 40
    rc, lens = _batch(rows=big[0], cols=big[1], n=1, out_stride=huge, sizes=[[8, 8]])
    assert rc == -215 and "2^32" in _err() and (lens == -7).all()
    assert jpeg.bound(*big, 3) > 0  # the bound itself is 64-bit and stays defined
    rc, _ = _batch(rows=ok[0], cols=ok[1], n=0, out_stride=huge)
    assert rc == 0
    if NO_GPU:
        rc, _ = _batch(rows=ok[0], cols=ok[1], n=1, out_stride=huge, sizes=[[8, 8]])
        assert rc == -217
    # the composite: a 9000 x 9000 colour sheet has a canvas slot of about 12 730 x 12 732 (796 x 796 MCUs, 6.3e9 bits);
    # refused before the sheet (not real memory here) is read or a device is asked for, and nothing is returned
    sheet = (_lib.OmrImage * 1)(_lib.OmrImage(0x1000, 9000, 9000, 3, 27000))
    ang, chk, src = np.full(1, -7.0), np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    ptrs = (_lib.u8p * 1)()
    lens1 = np.full(1, -7, np.int64)
    rc = oics.lib().omr_correct_default_batch_jpeg(sheet, 1, *PARAMS, 100, ang.ctypes.data_as(_lib.f64p),
                                                   chk.ctypes.data_as(_lib.i32p), src.ctypes.data_as(_lib.i32p), ptrs,
                                                   lens1.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == -215 and "2^32" in _err() and not ptrs[0] and lens1[0] == 0 and ang[0] == -7.0 and src[0] == -7
    r, c = omr.correct_batch_canvas(9000, 9000)
    assert worst_bits(r, c, 3) > 2 ** 32
    r, c = omr.correct_batch_canvas(7000, 7000)   # 9 900 x 9 900: 619 x 619 MCUs, 3.8e9 bits -- accepted
    assert worst_bits(r, c, 3) < 2 ** 32 - 64
    if NO_GPU:
        sheet = (_lib.OmrImage * 1)(_lib.OmrImage(0x1000, 7000, 7000, 3, 21000))
        rc = oics.lib().omr_correct_default_batch_jpeg(sheet, 1, *PARAMS, 100, ang.ctypes.data_as(_lib.f64p),
                                                       chk.ctypes.data_as(_lib.i32p), src.ctypes.data_as(_lib.i32p), ptrs,
                                                       lens1.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == -217
    img = _lib.OmrImage(0x1000, 20000, 20000, 1, 20000)  # gray: 6 250 000 blocks
    n = C.c_int64(-7)
    assert oics.lib().omr_jpeg_encode(C.byref(img), 90, None, 0, C.byref(n)) == -215 and "2^32" in _err() and n.value == -7


def test_host_form_argument_errors():
    L = oics.lib()
    a = np.zeros((8, 8, 3), np.uint8)
    _, im = oics.transfer.as_image(a)
    n = C.c_int64(-7)
    buf = np.full(64, 0xA5, np.uint8)
    assert L.omr_jpeg_encode(None, 90, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == -5
    assert L.omr_jpeg_encode(C.byref(im), 90, buf.ctypes.data_as(_lib.u8p), 64, None) == -5
    assert L.omr_jpeg_encode(C.byref(im), 90, None, 64, C.byref(n)) == -5
    bad = _lib.OmrImage(a.ctypes.data, 8, 8, 3, 23)
    assert L.omr_jpeg_encode(C.byref(bad), 90, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == -5 and "step_bytes" in _err()
    for cn, code in ((2, -215), (4, -213)):
        bad = _lib.OmrImage(a.ctypes.data, 8, 8, cn, 8 * cn)
        assert L.omr_jpeg_encode(C.byref(bad), 90, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == code
    assert n.value == -7 and (buf == 0xA5).all()
    rc = L.omr_jpeg_encode(C.byref(im), 90, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n))
    if NO_GPU:  # (with a GPU: -4 and the length, tests/test_gpu_jpeg.py::test_cap_too_small)
        assert rc == -217 and n.value == -7
    assert (buf == 0xA5).all()


def test_composite_argument_errors_and_no_gpu():
    L = oics.lib()
    a = np.zeros((16, 16, 3), np.uint8)
    _, im = oics.transfer.as_image(a)
    arr = (_lib.OmrImage * 1)(im)
    ang, chk, rc1 = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32)
    ptrs = (_lib.u8p * 1)()
    lens = np.full(1, -7, np.int64)
    args = (ang.ctypes.data_as(_lib.f64p), chk.ctypes.data_as(_lib.i32p), rc1.ctypes.data_as(_lib.i32p))
    lp = lens.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.omr_correct_default_batch_jpeg(arr, 1, *PARAMS, 100, *args, None, lp) == -5
    assert L.omr_correct_default_batch_jpeg(arr, 1, *PARAMS, 100, *args, ptrs, None) == -5
    assert L.omr_correct_default_batch_jpeg(None, 1, *PARAMS, 100, *args, ptrs, lp) == -5
    assert L.omr_correct_default_batch_jpeg(arr, 0, *PARAMS, 100, *args, ptrs, lp) == -5
    assert lens[0] == -7
    bad = (_lib.OmrImage * 1)(_lib.OmrImage(a.ctypes.data, 16, 16, 4, 64))
    assert L.omr_correct_default_batch_jpeg(bad, 1, *PARAMS, 100, *args, ptrs, lp) == -213
    if NO_GPU:
        assert L.omr_correct_default_batch_jpeg(arr, 1, *PARAMS, 100, *args, ptrs, lp) == -217
        assert not ptrs[0] and lens[0] == 0
        with pytest.raises(oics.OmrError) as e:
            omr.correct_default_batch_jpeg([a], *PARAMS)
        assert e.value.code == -217
        with pytest.raises(oics.OmrError) as e:
            oics.transfer.TransformableMatrix(a).encode_jpeg()
        assert e.value.code == -217
        with pytest.raises(oics.OmrError) as e:
            jpeg.encode_batch_device(0x1000, 768, 48, 16, 16, 3, None, 1, 100, 0x2000, jpeg.bound(16, 16, 3))
        assert e.value.code == -217
    L.omr_bytes_free(None)  # free(NULL)


def test_front_doors():
    assert callable(oics.transfer.TransformableMatrix.encode_jpeg) and callable(jpeg.encode_batch_device)
    assert callable(omr.correct_default_batch_jpeg)
    src = os.path.join(ROOT, "shim", "oics", "src")
    transfer = open(os.path.join(src, "transfer.rs")).read()
    omr_rs = open(os.path.join(src, "omr.rs")).read()
    enc = transfer.split("pub fn encode_jpeg(")[1].split("\n}\n")[0]
    assert "ffi::omr_jpeg_encode(" in enc and "imgcodecs" not in enc
    assert re.search(r"pub fn encode_jpeg\(\s*m: &TransformableMatrix,\s*quality: i32\s*\)\s*->\s*Result<Vec<u8>", transfer)
    many = omr_rs.split("pub fn correct_defaults(")[1].split("\n}\n")[0]
    assert "ffi::omr_correct_default_batch_jpeg(" in many and "ffi::omr_bytes_free(" in many and "std::fs::write(" in many
    assert "imgcodecs::imread(" in many and "imgcodecs::imwrite" not in many
    assert re.search(r"inputs: &\[&str\],\s*outputs: &\[&str\]", omr_rs) and "Result<Vec<(f64, bool)>" in omr_rs
    # the existing per-call functions still write through OpenCV
    im_write = transfer.split("pub fn im_write(")[1].split("\n    }\n")[0]
    assert "imgcodecs::imwrite(" in im_write and "ffi::omr_jpeg" not in im_write
    one = omr_rs.split("pub fn correct_default(")[1].split("\n}\n")[0]
    assert "ffi::omr_jpeg" not in one and "omr_correct_default_batch_jpeg" not in one
    assert "imwrite" in one or "im_write" in one
