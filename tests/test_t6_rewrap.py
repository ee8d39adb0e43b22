"""t6_rewrap.py, the instrument of test_gpu_tiff_foreign.py, validated before the kernels are held to it.  No GPU.

Its "libtiff" policy equals libtiff's encoder byte for byte on every G4 picture of tiff_cases; every dialect stream is read
by Pillow (libtiff's decoder) as the picture it was made from, and by the restatement tiff_ref.decode; every pin is
Refused or Damaged there.  The conditions under which a policy proves nothing are asserted: h-only streams hold only
horizontal codes, the random ones reach all nine modes, "split" did write runs of three and more make-up codes and mixed
extended with ordinary ones, and the widest h-only strip does outrun the kernel's input window.

Dropped from the comparison with Pillow, by name (t6_rewrap.NO_ARBITER): a file of several strips of Compression 4 or
32773 without StripByteCounts.  libtiff estimates the counts for one strip only; Pillow raises OSError("decoder error -2")
behind libtiff's 'MissingRequired: TIFF directory is missing required "StripByteCounts" field'."""
import os
import re

import numpy as np
import pytest

import t6_rewrap as T
import tiff_cases
import tiff_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_MODES = {"H", "P", "V0", "V+1", "V-1", "V+2", "V-2", "V+3", "V-3"}


def _constant(name):
    text = open(os.path.join(ROOT, "omr-img-corrector_amd", "csrc", "tiff_dec.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def _modes(stream):
    """the modes of every code of a G4 stream, and of its first strip's first row alone"""
    h = tiff_ref.parse(stream)
    lsb = h["fill_order"] == 2
    m = []
    for k, (off, n) in enumerate(h["strips"]):
        tiff_ref.t6_decode(stream[off:off + n], min(h["rps"], h["rows"] - k * h["rps"]), h["cols"], lsb, modes=m)
    return m


def test_the_libtiff_policy_writes_what_libtiff_writes():
    n = 0
    for kind in tiff_cases.CONTENTS:
        for rows in tiff_cases.ROWS:
            for cols in tiff_cases.WIDTHS:
                a = tiff_cases.content(kind, rows, cols, seed=rows * 1000 + cols)
                for rps in sorted({1, min(8, rows), rows}):
                    s = tiff_ref.pillow_tiff(a, "group4", rps)
                    bits = a if tiff_ref.parse(s)["photometric"] == 0 else 1 - a  # the polarity Pillow stores
                    for k, strip in enumerate(tiff_ref.strips_of(s)):
                        assert T.t6_encode(bits[k * rps:(k + 1) * rps], "libtiff", "fewest", "eofb") == strip, (kind, rows, cols, rps, k)
                        n += 1
    assert n == 8 * 9 * (1 + (2 + 1) + (37 + 5 + 1))
    for (name, a), (_, s) in zip(T.long_pictures(), tiff_cases.long_run_cases()):
        bits = a if tiff_ref.parse(s)["photometric"] == 0 else 1 - a
        assert [T.t6_encode(bits)] == tiff_ref.strips_of(s), name


def _check(cases):
    for name, s, want in cases:
        got = tiff_ref.decode(s)
        assert got.shape == want.shape and (got == want).all(), (name, "the restatement")
        if name in T.NO_ARBITER:
            with pytest.raises(OSError, match="decoder error -2"):
                tiff_ref.pillow_read(s)
            continue
        got = tiff_ref.pillow_read(s)
        assert got.shape == want.shape and (got == want).all(), (name, "Pillow")


def test_t6_dialects_are_read_by_pillow_and_the_restatement():
    cases = T.t6_dialects()
    assert len(cases) == 8 * 9 * 4 * 2
    for ending in T.ENDINGS:
        assert sum("-%s-" % ending in n for n, _, _ in cases) >= 100, ending
    _check(cases)


def _libtiff_modes(s, want):
    """the modes of the "libtiff" stream of the same picture in the same strips; with the fewest make-up codes the modes
    decide the code stream, so two streams differ exactly where these lists do"""
    h = tiff_ref.parse(s)
    bits = ((want == 0) if h["photometric"] == 0 else (want != 0)).astype(np.uint8)
    lib = tiff_ref.assemble(h["rows"], h["cols"], T.t6_strips(bits, h["rps"], "libtiff", "fewest", "eofb", 0), 4, rps=h["rps"])
    return _modes(lib)


def test_h_only_streams_hold_horizontal_codes_only_and_differ_from_libtiff():
    n, same = 0, []
    for name, s, want in T.t6_dialects() + T.split_dialects()[0] + T.widest_rows():
        if "-h-only" not in name:
            continue
        m = _modes(s)
        assert set(m) == {"H"}, name
        lib = _libtiff_modes(s, want)
        if name.startswith("split-"):  # the same modes with other make-up codes: test_split_runs_are_split counts those
            continue
        # under the white line above a strip T.6 itself may need horizontal pairs alone (a black row is one pair): for such
        # a one-row picture no other stream exists
        assert m != lib or (set(lib) == {"H"} and want.shape[0] == 1), name
        same += [name] * (m == lib)
        n += 1
    assert n == 288 + 2 and 8 * len(same) <= n, same


def test_random_streams_reach_every_mode_and_differ_from_libtiff():
    seen, differ, several = set(), 0, 0
    for name, s, want in T.t6_dialects():
        if "-random-" not in name:
            continue
        m = _modes(s)
        seen |= set(m)
        if want.shape[0] >= 2:
            several += 1
            differ += m != _libtiff_modes(s, want)
    assert seen == ALL_MODES, seen
    assert several == 8 * 9 * 3 and 2 * differ >= several, (differ, several)


def test_split_runs_are_split():
    cases, stats = T.split_dialects()
    assert stats["three"] >= 20 and stats["mixed"] >= 1, stats
    _check(cases)
    # 128 as 64 + 64, and what the restatement makes of a hand-split run
    rng = np.random.RandomState(0)
    white = T.by_run()[0]
    assert T.run_codes(128, 0, "split", rng) == white[64] * 2 + white[0]
    assert T.run_codes(130, 0, "fewest") == white[128] + white[2]


def test_the_widest_h_only_strip_outruns_the_window():
    cases = T.widest_rows()
    _check(cases)
    win, cols, pad = _constant("TDEC_WIN_BYTES"), _constant("TDEC_T6_MAX_COLS"), _constant("TDEC_T6_PAD")
    assert (win, cols, pad) == (8192, T.WIDEST, 8)
    by_name = {n: (s, w) for n, s, w in cases}
    s, want = by_name["widest-black-first-equal-h-only"]
    assert len(T.changes(want[0] == 0)) == cols  # a change at every column: the line buffer's last entry is written
    row0 = T.t6_encode((want[:1] == 0).astype(np.uint8), "h-only", "fewest", "none")
    assert len(row0) > win and len(tiff_ref.strips_of(s)[0]) > 2 * win, len(row0)
    s2, want2 = by_name["widest-white-first-inverse-h-only"]
    assert len(T.changes(want2[1] == 0)) == cols and len(T.changes(want2[0] == 0)) == cols - 1
    assert tiff_ref.parse(s)["cols"] == tiff_ref.T6_MAX_COLS
    with pytest.raises(tiff_ref.Refused) as e:
        tiff_ref.parse(tiff_ref.assemble(2, cols + 1, [b"\0"], 4))
    assert e.value.code == -213


def test_packbits_dialects_are_read_by_pillow_and_the_restatement():
    cases = T.packbits_dialects()
    assert len(cases) == 8 * 9 * 6 * 4
    _check(cases)
    raw = bytes(range(7)) + bytes(300) + b"\1\2\2\3"
    lit = T.packbits_encode(raw, "literal1")
    assert len(lit) == 2 * len(raw) and set(lit[::2]) == {0}
    mx = T.packbits_encode(raw, "max")
    assert bytes([257 - 128, 0]) in mx and len(mx) < 30
    rows = T.packbits_encode(bytes(300), "max", 0, 100)
    assert rows == bytes([257 - 100, 0]) * 3 and T.packbits_encode(bytes(300), "crossing", 0, 100) == bytes([129, 0, 129, 0, 257 - 44, 0])
    no = T.packbits_encode(raw, "noop", 3)
    assert no.endswith(b"\x80") and no.count(b"\x80") >= 2 and no.replace(b"\x80", b"") == mx
    for enc in (lit, mx, no):
        assert tiff_ref.packbits_decode(enc, len(raw)) == raw


def test_ifd_dialects_are_read_by_pillow_and_the_restatement():
    cases = T.ifd_dialects()
    assert len(T.NO_ARBITER) == 8 and all("no-counts" in n for n in T.NO_ARBITER)
    _check(cases)
    # the first page of a chained file comes back, its second one is another picture
    chained = [s for n, s, _ in cases if "-chained-p" in n][0]
    assert chained.count(T.pack_rows(tiff_cases.content("checker", 5, 40))) == 1


def test_assembler_keeps_what_existing_callers_get():
    """the default layout: strips from byte 8, the IFD behind them at an even offset, sorted entries, values behind it"""
    import struct
    s = tiff_ref.assemble(3, 9, [b"abcd", b"ef"], 1, rps=2)
    assert s[:4] == b"II*\0" and s[8:14] == b"abcdef" and struct.unpack("<I", s[4:8])[0] == 14
    tags = [struct.unpack("<H", s[16 + 12 * k:18 + 12 * k])[0] for k in range(struct.unpack("<H", s[14:16])[0])]
    assert tags == sorted(tags) == [256, 257, 258, 259, 262, 266, 273, 277, 278, 279]
    assert tiff_ref.parse(s)["strips"] == [(8, 4), (12, 2)]


def test_missing_strip_byte_counts_are_derived():
    s = tiff_ref.assemble(3, 9, [b"abcd", b"de"], 1, rps=2, drop=(279,), reverse=True, gap=2)
    h = tiff_ref.parse(s)
    assert h["strips"] == [(12, len(s) - 12), (8, 4)] and s[8:12] == b"de\xa5\xa5"  # to the next offset above its own, or to the stream's end
    with pytest.raises(tiff_ref.Refused):
        tiff_ref.parse(tiff_ref.assemble(3, 9, [b"abcd", b"de"], 1, rps=2, drop=(273,)))
    with pytest.raises(tiff_ref.Refused):  # a present tag is taken at its word
        tiff_ref.parse(tiff_ref.assemble(3, 9, [b"abcd", b"de"], 1, rps=2, extra=[(279, 4, [4])]))


def test_pins_are_refused_or_damaged_in_the_restatement():
    pins = T.pins()
    assert [c for _, _, c in pins] == [-215, -215, -213, -213, -5, -215, -215]
    for name, s, code in pins:
        if code == -215:
            with pytest.raises(tiff_ref.Damaged):
                tiff_ref.decode(s)
        else:
            with pytest.raises(tiff_ref.Refused) as e:
                tiff_ref.decode(s)
            assert e.value.code == code, name
    # the two chosen differences from libtiff: Pillow reads both
    a = np.zeros((1, 200), np.uint8)
    a[0, 130:135] = 1
    assert (tiff_ref.pillow_read(pins[0][1]) == T.want_of(a, 0)).all()
    assert (tiff_ref.pillow_read(pins[1][1]) == 255).all()  # libtiff clips the run
