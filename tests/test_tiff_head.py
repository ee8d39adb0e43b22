"""The one TIFF head writer (csrc/tiff_head.hpp) alone, on the CPU: compiled into a host program (tests/tiff_head_main.cpp,
with the address and undefined-behaviour sanitizers where a one-line program shows that the compiler has their runtimes;
the test prints which build ran) and compared, byte for byte and position for position, with the heads the two
restatements build: tiff_enc_ref.assemble for the Group 4 writer's descriptions, tiff8_enc_ref.head for the 8-bit writer's."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tiff8_enc_ref as ref8  # noqa: E402
import tiff_enc_ref as ref  # noqa: E402

CSRC = os.path.join(ROOT, "omr-img-corrector_amd", "csrc")
SHAPES = [(1, 1), (16, 24), (17, 3)]
RPS = [0, 1, 5]  # one strip, a strip a row, several strips (a short last one for 16 and 17 rows)
DPI = [0, 300]


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return c
    pytest.fail("no host C++ compiler: neither $CXX, g++ nor ROCm's clang++")


@pytest.fixture(scope="module")
def writer(tmp_path_factory):
    """-> run(lines): the program's answers, one (head_len, off_pos, cnt_pos, data_at, head) per description"""
    exe = str(tmp_path_factory.mktemp("tiff_head") / "tiff_head")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(HERE, "tiff_head_main.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = os.path.join(os.path.dirname(exe), "probe")
    with open(probe + ".cpp", "w") as f:
        f.write("int main() { return 0; }\n")
    have = subprocess.run([cmd[0]] + san + ["-o", probe, probe + ".cpp"], capture_output=True).returncode == 0 and \
        subprocess.run([probe], capture_output=True).returncode == 0
    print("tiff_head_main: built %s" % ("with -fsanitize=address,undefined" if have else "WITHOUT sanitizers (no runtimes for %s)" % cmd[0]))
    subprocess.check_call(cmd + (san if have else []))  # with the runtimes present, a failure of the sanitizer build is a failure

    def run(lines):
        p = subprocess.run([exe], input="".join(" ".join(str(int(v)) for v in ln) + "\n" for ln in lines), capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        out = [ln.split() for ln in p.stdout.splitlines()]
        assert len(out) == len(lines)
        return [(int(a), int(b), int(c), int(d), bytes.fromhex(h)) for a, b, c, d, h in out]
    return run


def test_group4_heads_are_the_restatements(writer):
    cases = [(r, c, k, dpi) for r, c in SHAPES for k in RPS for dpi in DPI]
    desc, files = [], []
    for rows, cols, k, dpi in cases:
        rps = rows if k <= 0 else min(k, rows)
        strips = [bytes([j + 1]) * (j + 3) for j in range((rows + rps - 1) // rps)]  # lengths 3, 4, ..: odd and even
        desc.append((rows, cols, rps, len(strips), 1, 1, 4, 0, 1, 1, dpi))
        files.append((ref.assemble(rows, cols, rps, strips, dpi), strips))
    assert {len(s) for _, s in files} >= {1, 4, 17}
    for case, (f, strips), (head_len, off_pos, cnt_pos, data_at, head) in zip(cases, files, writer(desc)):
        ns = len(strips)
        want = bytearray(f[:head_len])
        if ns == 1:  # the two values stand inside their entries: the device writes them, the head leaves zeros
            want[off_pos:off_pos + 4] = want[cnt_pos:cnt_pos + 4] = bytes(4)
        else:
            assert (off_pos, cnt_pos) == (head_len, head_len + 4 * ns), case
        assert head == bytes(want), case
        assert data_at == head_len + (8 * ns if ns > 1 else 0), case
        assert struct.unpack_from("<%dI" % ns, f, off_pos)[0] == data_at and f[data_at:data_at + 3] == strips[0], case
        assert list(struct.unpack_from("<%dI" % ns, f, cnt_pos)) == [len(s) for s in strips], case


def test_8bit_heads_are_the_restatements(writer):
    cases = [(r, c, k, dpi, cn, comp, pred) for r, c in SHAPES for k in RPS for dpi in DPI for cn in (1, 3)
             for comp, pred in ((1, 1), (5, 1), (5, 2))]
    desc = []
    for rows, cols, k, dpi, cn, comp, pred in cases:
        rps = ref8.rows_of_strip(rows, cols, cn, k)
        desc.append((rows, cols, rps, (rows + rps - 1) // rps, 8, cn, comp, 2 if cn == 3 else 1, pred, 0, dpi))
    assert len(cases) + 18 + 4 < 200
    for case, d, (head_len, off_pos, cnt_pos, data_at, head) in zip(cases, desc, writer(desc)):
        rows, cols, k, dpi, cn, comp, pred = case
        h, want_off, want_cnt, want_data = ref8.head(rows, cols, cn, comp, pred, d[2], d[3], dpi)
        assert head == bytes(h) and head_len == len(h), case
        assert (off_pos, cnt_pos, data_at) == (want_off, want_cnt, want_data), case


def test_the_lengths_the_encoders_hold_their_buffer_to(writer):
    """tiff_head_len of the longest description either encoder gives (what TENC_HEAD_MAX and TENC8_HEAD_MAX are, and what the
    bounds count for the head) and of the shortest"""
    got = writer([(16, 24, 5, 4, 1, 1, 4, 0, 1, 1, 300), (16, 24, 5, 4, 8, 3, 5, 2, 2, 0, 300), (1, 1, 1, 1, 1, 1, 4, 0, 1, 1, 0),
                  (1, 1, 1, 1, 8, 1, 1, 1, 1, 0, 0)])
    assert [g[0] for g in got] == [8 + 2 + 12 * 13 + 4 + 16, 8 + 2 + 12 * 14 + 4 + 16 + 8, 8 + 2 + 12 * 10 + 4, 8 + 2 + 12 * 9 + 4]
