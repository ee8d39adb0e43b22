"""The detectors' pure host rules (csrc/hough_select.hpp: line_angles, select_omr_rs, select_fft_rs) alone, on the CPU:
compiled into a host program (tests/hough_select_main.cpp) twice -- plainly, and with the address and undefined-behaviour
sanitizers where a one-line program shows that the compiler has their runtimes (the test prints which builds ran; both must
answer alike) -- and compared with the float64 statements of tests/hough_exact.py and with fft.rs's quirk-B10 rule."""
import math
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import hough_exact as hx  # noqa: E402

CSRC = os.path.join(ROOT, "omr-img-corrector_amd", "csrc")


def _many(n):
    """n segments from the origin whose directions sweep a quarter turn: clusters, ties and lone angles among them"""
    return [(0, 0, 1 + (k * 7) % 61, (k * 13) % 53) for k in range(n)]


LISTS = {
    "empty": [],
    "one": [(3, 4, 40, 9)],
    "tie of 2": [(0, 0, 50, 3), (0, 0, 50, 20)],
    "tie of 3": [(0, 0, 50, 20), (0, 0, 50, 3), (0, 5, 50, 16), (1, 1, 51, 4), (2, 0, 52, 3)],  # lone, three alike, lone
    "vertical": [(5, 0, 5, 10), (7, 30, 7, 2), (0, 0, 9, 0), (9, 4, 0, 4)],   # atan2 = +-90, 0, 180 -> fmodf
    "raw +-45": [(0, 0, 20, 20), (0, 20, 20, 0), (30, 30, 2, 2), (0, 0, 20, 1), (0, 0, 60, 59)],
    "2049": _many(2049),
}


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return c
    pytest.fail("no host C++ compiler: neither $CXX, g++ nor ROCm's clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """-> run(text): the program's output lines, the same from every build"""
    d = str(tmp_path_factory.mktemp("hough_select"))
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC]
    src = os.path.join(HERE, "hough_select_main.cpp")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = os.path.join(d, "probe")
    with open(probe + ".cpp", "w") as f:
        f.write("int main() { return 0; }\n")
    have = subprocess.run([cmd[0]] + san + ["-o", probe, probe + ".cpp"], capture_output=True).returncode == 0 and \
        subprocess.run([probe], capture_output=True).returncode == 0
    print("hough_select_main: built plainly%s" % (" and with -fsanitize=address,undefined" if have else
                                                  ", WITHOUT sanitizers (no runtimes for %s)" % cmd[0]))
    exes = [os.path.join(d, "plain")] + ([os.path.join(d, "sanitized")] if have else [])
    subprocess.check_call(cmd + ["-o", exes[0], src])
    if have:  # with the runtimes present, a failure of the sanitizer build is a failure
        subprocess.check_call(cmd + san + ["-o", exes[1], src])

    def run(text):
        outs = []
        for exe in exes:  # run directly: the sanitized program needs no preload
            p = subprocess.run([exe], input=text, capture_output=True, text=True)
            assert p.returncode == 0, (exe, p.returncode, p.stderr[-2000:])
            outs.append(p.stdout.splitlines())
        assert all(o == outs[0] for o in outs)
        return outs[0]
    return run


def _f32(h):
    return struct.unpack("<f", struct.pack("<I", int(h, 16)))[0]


def _f64(h):
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def _angles(program, lines):
    """the program's line_angles, widened to float64 as omr.rs widens them"""
    text = "%d 0 0\n%s\n%s\n" % (len(lines), " ".join("%d %d %d %d" % s for s in lines), " ".join("0" for _ in lines))
    out = program(text)
    assert len(out) == 4 and out[0].split()[0] == "A"
    return np.array([_f32(h) for h in out[0].split()[1:]], np.float64)


def _fft_rs(lines):
    """fft.rs:197-247 with quirk B10: line i's inner loop compares its own raw and folded angle n - 1 times"""
    n, best, votes_max = len(lines), 0.0, 0
    for x1, y1, x2, y2 in lines:
        raw = (math.atan2(float(y2) - float(y1), float(x2) - float(x1)) * 180.0) / math.pi
        angle = raw + 90.0 if raw < -45.0 else raw - 90.0 if raw > 45.0 else raw
        votes = n - 1 if abs(raw - angle) < 0.1 else 0
        if votes > votes_max:
            votes_max, best = votes, angle
    return best


@pytest.mark.parametrize("name", list(LISTS))
def test_line_angles_are_the_float64_angles(program, name):
    """every f32 angle within hough_exact.EPS of its segment's float64 angle -- of either fold where the raw angle is a
    nonzero multiple of 45, as float32 rounding decides the side there (hough_exact._admissible)"""
    lines = LISTS[name]
    got = _angles(program, lines)
    assert len(got) == len(lines)
    if not lines:
        return
    vals, own, two = hx._admissible(lines)
    assert name != "raw +-45" or two[:3].all() and not two[3:].any()
    for i, g in enumerate(got.tolist()):
        assert np.abs(vals[own == i] - g).min() <= hx.EPS, (name, i, lines[i], g, vals[own == i])
    if name == "vertical":  # exact in either precision: 90 % 45, -90 % 45 (the dividend's sign), 0, 180 % 45
        assert got.tolist() == [0.0, 0.0, 0.0, 0.0] and [math.copysign(1, g) for g in got.tolist()] == [1, -1, 1, 1]


@pytest.mark.parametrize("name", list(LISTS))
def test_select_omr_rs_is_the_float64_vote(program, name):
    """given omr.rs's counts -- float64 windows on the widened f32 angles, hough_exact.window_counts -- the angle, the
    status and the candidates are hough_exact.vote_omr_rs's bit for bit, with a cand_cap below and above the tie count:
    cand_len counts every candidate, only the first cand_cap are written"""
    lines = LISTS[name]
    a = _angles(program, lines)
    if lines:
        want_angle, want_status, want_cand = hx.vote_omr_rs(a)
        counts = hx.window_counts(a, a, 0.1)
    else:  # the reference panics on angles[0]: the header's statement for no segment
        want_angle, want_status, want_cand, counts = 0.0, hx.NOT_A_RESULT, np.zeros(0), []
    ties = len(want_cand)
    assert {"empty": 0, "one": 1, "tie of 2": 2, "tie of 3": 3}.get(name, ties) == ties
    caps = (max(ties - 1, 0), ties + 2)
    text = "%d %d %d\n%s\n%s\n" % (len(lines), caps[0], caps[1], " ".join("%d %d %d %d" % s for s in lines),
                                 " ".join(str(int(c)) for c in counts))
    out = program(text)
    for cap, row in zip(caps, out[1:3]):
        f = row.split()
        assert f[0] == "S" and int(f[1]) == cap
        assert struct.pack("<d", _f64(f[2])) == struct.pack("<d", want_angle), (name, cap)
        assert (int(f[3]), int(f[4])) == (want_status, ties), (name, cap)
        assert [_f64(h) for h in f[5:]] == want_cand[:cap].tolist(), (name, cap)


@pytest.mark.parametrize("name", list(LISTS))
def test_select_fft_rs_is_the_quirk_b10_rule(program, name):
    lines = LISTS[name]
    text = "%d 0 0\n%s\n%s\n" % (len(lines), " ".join("%d %d %d %d" % s for s in lines), " ".join("0" for _ in lines))
    got = _f64(program(text)[3].split()[1])
    assert struct.pack("<d", got) == struct.pack("<d", _fft_rs(lines)), (name, got)


def test_the_lists_hold_what_they_are_named_for(program):
    a = _angles(program, LISTS["2049"])
    assert len(a) == 2049 > 2048 and len(np.unique(a)) > 100
    assert abs(_fft_rs(LISTS["raw +-45"])) == 45.0 and _fft_rs(LISTS["vertical"]) == 0.0 and _fft_rs(LISTS["one"]) == 0.0
