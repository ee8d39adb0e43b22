"""CPU-side checks of the PNG encoder's boundary (omr_png_bound, omr_png_encode*, omr_correct_default_batch_png,
omr_correct_default_batch_streams_png): declared in the header, the ctypes table and ffi.rs alike and exported; the bound
against its documented formula; every argument error before any device work; the CRC-32 combine arithmetic the device
uses (csrc/crc32_combine.hpp, compiled into a host program) against zlib; the Python and Rust front doors."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import png_enc_ref as ref  # noqa: E402
import oics  # noqa: E402
from oics import _lib, omr, png  # noqa: E402

BATCH = ("int", ["const uint8_t *", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "const int32_t *", "int32_t", "int32_t",
                 "uint8_t *", "int64_t", "int64_t *"])
NEW = {
    "omr_png_bound": ("int", ["int32_t", "int32_t", "int32_t", "int64_t *"]),
    "omr_png_encode_batch_device": BATCH,
    "omr_png_encode": ("int", ["const omr_image *", "int32_t", "uint8_t *", "int64_t", "int64_t *"]),
    "omr_png_encode_stats": ("int", ["int32_t", "int32_t *", "double *"]),
    "omr_correct_default_batch_png": ("int", ["const omr_image *", "int32_t", "uint16_t", "double", "int32_t", "int32_t",
                                              "double", "double", "int32_t", "double *", "int32_t *", "int32_t *",
                                              "uint8_t * *", "int64_t *"]),
    "omr_correct_default_batch_streams_png": ("int", ["const uint8_t * const *", "const int64_t *", "int32_t", "uint16_t",
                                                      "double", "int32_t", "int32_t", "double", "double", "int32_t",
                                                      "double *", "int32_t *", "int32_t *", "uint8_t * *", "int64_t *"]),
}
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint16_t": C.c_uint16, "double": C.c_double}
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
        assert res is C.c_int and len(at) == len(args), name
        for c, t in zip(args, at):
            if "*" in c:
                assert t is C.c_void_p or hasattr(t, "contents") or hasattr(t, "_type_"), (name, c, t)
            else:
                assert t is CTYPES[c], (name, c, t)
        assert re.search(r"pub fn %s\(" % name, ffi), name
    # the PNG entry points mirror their JPEG twins argument for argument
    for a, b in (("omr_png_bound", "omr_jpeg_bound"), ("omr_png_encode_batch_device", "omr_jpeg_encode_batch_device"),
                 ("omr_png_encode", "omr_jpeg_encode"), ("omr_correct_default_batch_png", "omr_correct_default_batch_jpeg"),
                 ("omr_correct_default_batch_streams_png", "omr_correct_default_batch_streams")):
        assert decls[a] == decls[b], (a, b)
        assert _lib.SYMBOLS[a] == _lib.SYMBOLS[b], (a, b)


def test_bound_against_its_formula_and_the_limits():
    def formula(rows, cols, cn):
        raw = rows * (1 + cols * cn)
        return 43 + raw + 5 * ((raw + 16383) // 16384) + 20

    for rows, cols in [(1, 1), (1, 300), (300, 1), (15, 17), (150, 270), (1 << 20, 1), (1, 1 << 20), (1 << 15, 1 << 15),
                       (1 << 20, 1 << 10)]:
        for cn in (1, 3, 4):
            if formula(rows, cols, cn) - 43 - 20 + 6 > 2 ** 31 - 1:
                continue
            assert png.bound(rows, cols, cn) == formula(rows, cols, cn) == ref.bound(rows, cols, cn), (rows, cols, cn)
    assert png.bound(1 << 15, 1 << 15, 1) == formula(1 << 15, 1 << 15, 1)   # 2^30 pixels, gray: the largest taken
    out = C.c_int64(-1)
    L = oics.lib()
    assert L.omr_png_bound(8, 8, 3, None) == -5
    for rows, cols, cn, text in [(0, 8, 3, "empty"), (8, 0, 1, "empty"), (8, 8, 2, "channels"), (8, 8, 5, "channels"),
                                 ((1 << 20) + 1, 1, 1, "imread"), (1, (1 << 20) + 1, 1, "imread"),
                                 ((1 << 15) + 1, 1 << 15, 1, "imread"), (1 << 15, 1 << 15, 3, "IDAT"),
                                 (1 << 15, 1 << 15, 4, "IDAT"), (1 << 15, 1 << 14, 4, "IDAT")]:
        assert L.omr_png_bound(rows, cols, cn, C.byref(out)) == -215 and text in _err(), (rows, cols, cn, _err())
    assert out.value == -1
    # the 2^31 decision from the formula: 2 + raw + 5 x blocks + 4 must stay below 2^31
    def idat(rows, cols, cn):
        raw = rows * (1 + cols * cn)
        return 2 + raw + 5 * ((raw + 16383) // 16384) + 4

    rows = 1 << 15
    cols = max(c for c in range(21000, 22000) if idat(rows, c, 3) <= 2 ** 31 - 1)   # the last width taken at 3 channels
    assert idat(rows, cols + 1, 3) > 2 ** 31 - 1 and png.bound(rows, cols, 3) == formula(rows, cols, 3)
    assert L.omr_png_bound(rows, cols + 1, 3, C.byref(out)) == -215 and "IDAT" in _err()


def _batch(d_imgs=0x1000, stride=None, step=None, rows=16, cols=24, cn=3, sizes=None, n=2, q=1, d_out=0x2000,
           out_stride=None, out_len=True):
    step = cols * cn if step is None else step
    stride = rows * step if stride is None else stride
    out_stride = 1 << 40 if out_stride is None else out_stride
    lens = np.full(max(n, 1), -7, np.int64)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
    rc = oics.lib().omr_png_encode_batch_device(d_imgs, stride, step, rows, cols, cn,
                                                None if sz is None else sz.ctypes.data_as(_lib.i32p), n, q, d_out, out_stride,
                                                lens.ctypes.data_as(C.POINTER(C.c_int64)) if out_len else None)
    return rc, lens


def test_batch_argument_errors_come_before_any_device_work():
    """the pointers are not device memory: a call that touched them would crash, with or without a GPU"""
    cases = [
        (dict(d_imgs=None), -5, "null"), (dict(d_out=None), -5, "null"), (dict(out_len=False), -5, "null"),
        (dict(n=-1), -5, "negative n"),
        (dict(cn=2), -215, "1, 3 or 4 channels"), (dict(rows=0), -215, "empty"), (dict(cols=(1 << 20) + 1), -215, "imread"),
        (dict(rows=1 << 15, cols=1 << 15), -215, "IDAT"),
        (dict(step=24 * 3 - 1), -5, "step_bytes"), (dict(stride=16 * 72 - 1), -5, "img_stride_bytes"),
        (dict(sizes=[[16, 24], [17, 24]]), -5, "sizes[1]"), (dict(sizes=[[16, 25], [1, 1]]), -5, "sizes[0]"),
        (dict(sizes=[[16, 24], [-1, 3]]), -5, "sizes[1]"), (dict(sizes=[[0, 5], [1, 1]]), -5, "sizes[0]"),
        (dict(out_stride=png.bound(16, 24, 3) - 1), -5, "omr_png_bound"),
        (dict(cn=4, out_stride=png.bound(16, 24, 4) - 1), -5, "omr_png_bound"),
    ]
    for q in (-5, 0, 1, 9, 1000):   # the clamp: no level is an error
        for kw, code, text in cases:
            rc, lens = _batch(q=q, **kw)
            assert rc == code and text in _err(), (kw, rc, _err())
            assert (lens == -7).all(), kw
        rc, lens = _batch(n=0, q=q)
        assert rc == 0 and (lens == -7).all()
        if NO_GPU:
            assert _batch(q=q, out_stride=png.bound(16, 24, 3))[0] == -217


def test_bad_sizes_have_the_wording_all_four_encoders_share():
    """the same four bad `sizes` stand in test_jpeg_abi, test_png_encode_abi, test_tiff_encode_abi and test_tiff8_encode_abi:
    every encoder's batch entry point answers them with these words, to the letter"""
    for sizes, text in [([[16, 24], [17, 24]], "sizes[1] = 17 x 24 does not fit the 16 x 24 slot"),
                        ([[16, 25], [1, 1]], "sizes[0] = 16 x 25 does not fit the 16 x 24 slot"),
                        ([[16, 24], [-1, 3]], "sizes[1] = -1 x 3 does not fit the 16 x 24 slot"),
                        ([[0, 5], [1, 1]], "sizes[0] = 0 x 5 does not fit the 16 x 24 slot")]:
        rc, lens = _batch(sizes=sizes)
        assert rc == -5 and _err() == text and (lens == -7).all(), (sizes, rc, _err())


def test_host_form_argument_errors():
    L = oics.lib()
    a = np.zeros((8, 8, 3), np.uint8)
    _, im = oics.transfer.as_image(a)
    n = C.c_int64(-7)
    buf = np.full(64, 0xA5, np.uint8)
    assert L.omr_png_encode(None, 1, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == -5
    assert L.omr_png_encode(C.byref(im), 1, buf.ctypes.data_as(_lib.u8p), 64, None) == -5
    assert L.omr_png_encode(C.byref(im), 1, None, 64, C.byref(n)) == -5
    assert L.omr_png_encode(C.byref(im), 1, buf.ctypes.data_as(_lib.u8p), -1, C.byref(n)) == -5
    bad = _lib.OmrImage(a.ctypes.data, 8, 8, 3, 23)
    assert L.omr_png_encode(C.byref(bad), 1, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == -5 and "step_bytes" in _err()
    bad = _lib.OmrImage(a.ctypes.data, 8, 8, 2, 16)
    assert L.omr_png_encode(C.byref(bad), 1, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == -215
    big = _lib.OmrImage(0x1000, 1 << 15, 1 << 15, 3, 3 << 15)
    assert L.omr_png_encode(C.byref(big), 1, None, 0, C.byref(n)) == -215 and "IDAT" in _err()
    assert n.value == -7 and (buf == 0xA5).all()
    if NO_GPU:  # (with a GPU: -4 and the length, tests/test_gpu_png_encode.py)
        assert L.omr_png_encode(C.byref(im), 1, buf.ctypes.data_as(_lib.u8p), 64, C.byref(n)) == -217 and n.value == -7
        with pytest.raises(oics.OmrError) as e:
            oics.transfer.TransformableMatrix(a).encode_png()
        assert e.value.code == -217
    assert (buf == 0xA5).all()


def test_flow_argument_errors_and_no_gpu():
    L = oics.lib()
    a = np.zeros((16, 16, 3), np.uint8)
    _, im = oics.transfer.as_image(a)
    arr = (_lib.OmrImage * 1)(im)
    ang, chk, rc1 = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32)
    ptrs = (_lib.u8p * 1)()
    lens = np.full(1, -7, np.int64)
    args = (ang.ctypes.data_as(_lib.f64p), chk.ctypes.data_as(_lib.i32p), rc1.ctypes.data_as(_lib.i32p))
    lp = lens.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.omr_correct_default_batch_png(arr, 1, *PARAMS, 1, *args, None, lp) == -5
    assert L.omr_correct_default_batch_png(arr, 1, *PARAMS, 1, *args, ptrs, None) == -5
    assert L.omr_correct_default_batch_png(None, 1, *PARAMS, 1, *args, ptrs, lp) == -5
    assert L.omr_correct_default_batch_png(arr, 0, *PARAMS, 1, *args, ptrs, lp) == -5
    assert lens[0] == -7
    bad = (_lib.OmrImage * 1)(_lib.OmrImage(a.ctypes.data, 16, 16, 4, 64))
    assert L.omr_correct_default_batch_png(bad, 1, *PARAMS, 1, *args, ptrs, lp) == -213
    # a colour sheet whose canvas slot the encoder refuses: before the sheet (not real memory) is read
    sheet = (_lib.OmrImage * 1)(_lib.OmrImage(0x1000, 20000, 20000, 3, 60000))
    ang[0] = -7.0
    assert L.omr_correct_default_batch_png(sheet, 1, *PARAMS, 1, *args, ptrs, lp) == -215 and "IDAT" in _err()
    assert not ptrs[0] and lens[0] == 0 and ang[0] == -7.0
    s = np.frombuffer(b"not an image at all", np.uint8)
    sp = (C.c_void_p * 1)(s.ctypes.data)
    sl = np.array([s.size], np.int64)
    slp = sl.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.omr_correct_default_batch_streams_png(None, slp, 1, *PARAMS, 1, *args, ptrs, lp) == -5
    assert L.omr_correct_default_batch_streams_png(sp, slp, 0, *PARAMS, 1, *args, ptrs, lp) == -5
    assert L.omr_correct_default_batch_streams_png(sp, slp, 1, *PARAMS, 1, *args, None, lp) == -5
    # every stream refused: the codes are in scan_rc and there is no device work, with or without a GPU
    assert L.omr_correct_default_batch_streams_png(sp, slp, 1, *PARAMS, 1, *args, ptrs, lp) == 0
    assert rc1[0] != 0 and not ptrs[0] and lens[0] == 0
    if NO_GPU:
        assert L.omr_correct_default_batch_png(arr, 1, *PARAMS, 1, *args, ptrs, lp) == -217
        with pytest.raises(oics.OmrError) as e:
            omr.correct_default_batch_png([a], *PARAMS)
        assert e.value.code == -217
    L.omr_bytes_free(None)


def test_stats_are_zero_until_an_encode_ran_with_the_collection_on():
    groups, ms = png.encode_stats(True)
    assert groups == 0 and ms == [0.0] * len(png.STAGES_ENC) and len(png.STAGES_ENC) == 6
    png.encode_stats(False)
    assert oics.lib().omr_png_encode_stats(0, None, None) == 0


CRC_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "crc32_combine.hpp"
using namespace omr;
// stdin: the message; argv: the sizes of its pieces.  Prints the CRC-32 put together from the pieces' raw registers.
int main(int argc, char **argv)
{
    std::vector<unsigned char> m;
    for (int c; (c = getchar()) != EOF;) m.push_back((unsigned char)c);
    size_t at = 0;
    uint32_t acc = 0;
    for (int k = 1; k < argc; k++) {
        const size_t n = (size_t)atoll(argv[k]);
        uint32_t c = 0;
        for (size_t i = 0; i < n; i++) c = crc_byte(c, m[at + i]);
        at += n;
        acc ^= crc_shift(c, m.size() - at);
    }
    if (at != m.size()) return 2;
    printf("%08x %08x %08x\n", ~(crc_shift(0xffffffffu, m.size()) ^ acc), crc_x8n(1), crc_mulmod(0x80000000u, 0x12345678u));
    return 0;
}
"""


def test_crc_combine_header_against_zlib():
    # a host compiler is part of the build: g++, else the one hipcc drives (host only: -x c++)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = ["g++"] if shutil.which("g++") else [hipcc, "-x", "c++"]
    assert shutil.which(cxx[0]), "no host compiler: neither g++ nor hipcc"
    rng = np.random.Generator(np.random.PCG64(11))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "m.cpp"), "w").write(CRC_MAIN)
        exe = os.path.join(td, "m")
        subprocess.check_call(cxx + ["-std=c++17", "-O1", "-fsanitize=address,undefined", "-I",
                               os.path.join(ROOT, "omr-img-corrector_amd", "csrc"), "-o", exe, os.path.join(td, "m.cpp")])
        for cuts in ([0], [1], [5], [1, 1], [3, 0, 4], [16384, 16389, 7], [100, 4, 65536, 1, 33], [70000] * 3):
            msg = rng.integers(0, 256, sum(cuts), dtype=np.uint8).tobytes()
            out = subprocess.run([exe] + [str(c) for c in cuts], input=msg, stdout=subprocess.PIPE, check=True).stdout.split()
            assert int(out[0], 16) == zlib.crc32(msg) & 0xffffffff, cuts
            assert int(out[1], 16) == 0x00800000 and int(out[2], 16) == 0x12345678   # x^8, and x^0 is the unit


def test_front_doors():
    assert callable(oics.transfer.TransformableMatrix.encode_png) and callable(png.encode_batch_device)
    assert callable(png.bound) and callable(png.encode) and callable(png.encode_stats)
    assert callable(omr.correct_default_batch_png) and callable(omr.correct_default_batch_streams_png)
    src = os.path.join(ROOT, "shim", "oics", "src")
    transfer = open(os.path.join(src, "transfer.rs")).read()
    omr_rs = open(os.path.join(src, "omr.rs")).read()
    enc = transfer.split("pub fn encode_png(")[1].split("\n}\n")[0]
    assert "ffi::omr_png_encode(" in enc and "imgcodecs" not in enc
    many = omr_rs.split("pub fn correct_defaults_png(")[1].split("\n}\n")[0]
    assert "ffi::omr_correct_default_batch_png(" in many and "write_streams(" in many and "imgcodecs::imwrite" not in many
    files = omr_rs.split("pub fn correct_default_files_png(")[1].split("\n}\n")[0]
    assert "ffi::omr_correct_default_batch_streams_png(" in files and "write_streams(" in files and "std::fs::read(" in files
    tail = omr_rs.split("fn write_streams(")[1].split("\n}\n")[0]   # the two functions' shared tail: write, and always free
    assert "ffi::omr_bytes_free(" in tail and "std::fs::write(" in tail
