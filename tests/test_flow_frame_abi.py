"""What a refused call of the batch deskew flows leaves in the caller's arrays, entry point by entry point, without a GPU.

Every entry point that ends in the shared bucket-and-chunk frame (csrc/flow_frame.hpp) gets one
call-level refusal -- a null streams[1], or a host image without data -- with every output array pre-filled with
sentinels; the table records the code and what comes back.  The projection and detector forms write nothing unless the
whole call succeeds.  The correct forms clear their outputs once every image has been checked, so an image that fails
its check leaves them alone and a canvas their encoder cannot take leaves `out` / `out_len` cleared; the correct streams
forms write scan_rc, zero angles, need_check and cleared outputs during the header pass.  The frame's own bookkeeping is
run under the sanitizers by a stand-alone program (tests/flow_frame_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oics import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = _lib.lib()
N = 3
F64, I32, I64, PTR = 7.5, 77, 99, 0x1234
BORDER = (C.c_uint8 * 4)(255, 255, 255, 0)
PROJ = (10, 0.5, 0.5, 1, BORDER)                    # max_angle, step, resize_scale, interp, border_value
HOUGH = (40.0, 5.0, 1, 0, BORDER, 1)                # line length and gap; flags, border_mode, border_value, clip
FFT = (30.0, 90.0) + HOUGH
CORRECT = (45, 0.2, 248, 230, 150.0, 50.0)

# symbol -> (input kind, the arguments between the inputs and the outputs, outputs that keep their sentinels: all)
ENTRIES = {
    "omr_get_angles_with_projections_batch": ("host", PROJ[:3]),
    "omr_deskew_with_projections_batch": ("host", PROJ),
    "omr_deskew_with_projections_batch_streams": ("streams3", PROJ + (90,)),
    "omr_deskew_with_projections_batch_streams_png": ("streams3", PROJ + (1,)),
    "omr_deskew_with_projections_batch_streams_tiff": ("streams3", PROJ + (127, 0, 0)),
    "omr_deskew_with_projections_batch_streams_tiff8": ("streams3", PROJ + (5, 1, 0, 0)),
    "omr_deskew_with_hough_batch": ("host", HOUGH),
    "omr_deskew_with_fft_batch": ("host", FFT),
    "omr_deskew_with_hough_batch_streams": ("streams3", HOUGH + (0, 90)),
    "omr_deskew_with_fft_batch_streams": ("streams3", FFT + (1, 1)),
    "omr_deskew_with_hough_batch_streams_tiff": ("streams3", HOUGH + (127, 0, 0)),
    "omr_deskew_with_fft_batch_streams_tiff": ("streams3", FFT + (127, 0, 0)),
    "omr_deskew_with_hough_batch_streams_tiff8": ("streams3", HOUGH + (5, 1, 0, 0)),
    "omr_deskew_with_fft_batch_streams_tiff8": ("streams3", FFT + (5, 1, 0, 0)),
    "omr_correct_default_batch": ("host", CORRECT),
    "omr_correct_default_batch_jpeg": ("host", CORRECT + (90,)),
    "omr_correct_default_batch_png": ("host", CORRECT + (1,)),
    "omr_correct_default_batch_streams": ("streams", CORRECT + (90,)),
    "omr_correct_default_batch_streams_png": ("streams", CORRECT + (1,)),
}
_KEEP = []


def _host_images(rows=40, cols=30, hole=None):
    img = np.zeros((40, 30, 3), np.uint8)
    _KEEP.append(img)
    ims = [_lib.OmrImage(None if i == hole else img.ctypes.data, rows, cols, 3, cols * 3) for i in range(N)]
    return [(_lib.OmrImage * N)(*ims), N]


def _streams(kind, contents):
    bufs = [np.frombuffer(s, np.uint8) if s is not None else None for s in contents]
    _KEEP.append(bufs)
    sp = (C.c_void_p * N)(*[None if b is None else b.ctypes.data for b in bufs])
    sl = (C.c_int64 * N)(*[0 if b is None else b.size for b in bufs])
    return [sp, sl, N] + ([3] if kind == "streams3" else [])


def _outputs(symbol, first):
    """sentinel-filled outputs for the argument types from position `first` on, and a reader for each"""
    args, read = [], []
    for t in _lib.SYMBOLS[symbol][1][first:]:
        if t is _lib.f64p:
            a = np.full(N, F64, np.float64)
            args.append(a.ctypes.data_as(t)), read.append(lambda a=a: a.tolist())
        elif t is _lib.i32p:
            a = np.full(N, I32, np.int32)
            args.append(a.ctypes.data_as(t)), read.append(lambda a=a: a.tolist())
        elif t is C.POINTER(C.c_int64) or t == C.POINTER(C.c_int64):
            a = np.full(N, I64, np.int64)
            args.append(a.ctypes.data_as(t)), read.append(lambda a=a: a.tolist())
        elif t == C.POINTER(_lib.u8p):
            a = (C.c_void_p * N)(*[PTR] * N)
            args.append(C.cast(a, t)), read.append(lambda a=a: [v or 0 for v in a])
        else:
            assert t == C.POINTER(_lib.OmrImageOwned), (symbol, t)
            a = (_lib.OmrImageOwned * N)()
            C.memset(a, 0x5A, C.sizeof(a))
            args.append(a), read.append(lambda a=a: bytes(a))
        _KEEP.append(a)
    return args, read


def _call(symbol, inputs):
    kind, mid = ENTRIES[symbol]
    outs, read = _outputs(symbol, len(inputs) + len(mid))
    before = [r() for r in read]
    rc = getattr(L, symbol)(*inputs, *mid, *outs)
    return rc, before, [r() for r in read]


@pytest.mark.parametrize("symbol", sorted(ENTRIES))
def test_a_refused_input_leaves_every_array_as_it_was(symbol):
    """a host image without data / a null streams[1]: -5 from every entry point, nothing written -- the correct forms
    included, whose clearing comes after the images' checks"""
    kind = ENTRIES[symbol][0]
    inputs = _host_images(hole=1) if kind == "host" else _streams(kind, [b"\xff\xd8", None, b"\xff\xd8"])
    rc, before, after = _call(symbol, inputs)
    assert rc == -5 and len(L.omr_last_error()) > 0
    assert after == before


@pytest.mark.parametrize("symbol", ["omr_correct_default_batch_jpeg", "omr_correct_default_batch_png"])
def test_correct_forms_clear_their_streams_before_the_encoders_canvas_check(symbol):
    """30000 x 30000 sheets: a canvas slot the encoder's 32-bit offsets cannot take refuses the call (-215) before any device
    work; `out` / `out_len` were cleared by then, the angles, need_check and scan_rc not yet written"""
    rc, before, after = _call(symbol, _host_images(rows=30000, cols=30000))
    assert rc == -215
    assert after[:3] == before[:3]
    assert after[3] == [0] * N and after[4] == [0] * N


@pytest.mark.parametrize("symbol", ["omr_correct_default_batch_streams", "omr_correct_default_batch_streams_png"])
def test_correct_streams_forms_write_during_the_header_pass(symbol):
    """three streams no decoder takes: the call succeeds without device work, every sheet with its parse code, angle 0.0,
    need_check 0 and no output"""
    rc, _, after = _call(symbol, _streams("streams", [b"\xff\xd8\xff", b"II*\x00\x08\x00\x00\x00", b"\x89PNG\r\n\x1a\n"]))
    assert rc == 0
    ang, chk, codes, out, out_len = after
    assert ang == [0.0] * N and chk == [0] * N and out == [0] * N and out_len == [0] * N
    assert all(c in (-5, -213, -215) for c in codes), codes


@pytest.mark.parametrize("symbol", [s for s in sorted(ENTRIES) if ENTRIES[s][0] == "streams3"])
def test_streams_forms_with_a_bad_channel_count_write_nothing(symbol):
    kind, mid = ENTRIES[symbol]
    inputs = _streams(kind, [b"\xff\xd8"] * N)
    inputs[3] = 2
    rc, before, after = _call(symbol, inputs)
    assert rc == -5 and after == before


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return c
    pytest.fail("no host C++ compiler: neither $CXX, g++ nor ROCm's clang++")


def test_the_frames_bookkeeping_under_the_sanitizers(tmp_path):
    """tests/flow_frame_main.cpp: the chunk bounds, the slot stride and the write-back of a streams call's accepted sheets on
    plain host data, with the address and undefined-behaviour sanitizers where a one-line program shows that the compiler has
    their runtimes (the test prints which build ran)"""
    exe = str(tmp_path / "flow_frame_main")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "omr-img-corrector_amd", "csrc"),
           "-o", exe, os.path.join(HERE, "flow_frame_main.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = str(tmp_path / "probe")
    with open(probe + ".cpp", "w") as f:
        f.write("int main() { return 0; }\n")
    have = subprocess.run([cmd[0]] + san + ["-o", probe, probe + ".cpp"], capture_output=True).returncode == 0 and \
        subprocess.run([probe], capture_output=True).returncode == 0
    print("flow_frame_main: built %s" % ("with -fsanitize=address,undefined" if have else "WITHOUT sanitizers (no runtimes for %s)" % cmd[0]))
    subprocess.check_call(cmd + (san if have else []))  # with the runtimes present, a failure of the sanitizer build is a failure
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.strip() == "ok"
