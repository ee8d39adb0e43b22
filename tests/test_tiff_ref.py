"""tiff_ref.py (the restatement of the bilevel TIFF decoder) against Pillow's libtiff, and the T.4 run-length code tables the
library holds (omr_tiff_code_tables) proven entry by entry against what libtiff's encoder writes.  No GPU."""
import io

import numpy as np
import pytest
from PIL import Image

import tiff_cases
import tiff_ref
from oics import tiff


def _bitstring(data):
    return "".join("{:08b}".format(b) for b in data)


def _expected_run(table, n):
    """the codes of one run as an encoder writes them: 2560s, one make-up code, one terminating code"""
    by_run = {r: (c, b) for (c, b), r in table.items()}
    out = ""
    while n >= 2624:
        c, b = by_run[2560]
        out += "{:0{}b}".format(c, b)
        n -= 2560
    if n >= 64:
        c, b = by_run[n & ~63]
        out += "{:0{}b}".format(c, b)
        n &= 63
    c, b = by_run[n]
    return out + "{:0{}b}".format(c, b)


def _g4_single_strip(bits):
    """-> (the T.6 strip Pillow writes for the picture, 1 where its runs are "black": a set bit of the decoded row)"""
    img = Image.fromarray(np.where(bits != 0, 0, 255).astype(np.uint8)).convert("1")
    bio = io.BytesIO()
    img.save(bio, format="TIFF", compression="group4")
    s = bio.getvalue()
    h = tiff_ref.parse(s)
    assert h["compression"] == 4 and len(h["strips"]) == 1 and h["fill_order"] == 1
    (off, n), = h["strips"]
    return s[off:off + n], h["photometric"]


def test_tables_are_complete_and_prefix_free():
    for k in (0, 1):
        t = tiff.code_tables(k)
        assert len(t) == 104
        assert [r for r, _, _ in t] == list(range(64)) + list(range(64, 1729, 64)) + list(range(1792, 2561, 64))
        words = ["{:0{}b}".format(c, b) for _, c, b in t]
        assert all(c < (1 << b) and 2 <= b <= 13 for _, c, b in t)
        for i, a in enumerate(words):
            for j, b in enumerate(words):
                assert i == j or not b.startswith(a), (k, a, b)
    # the extended make-up codes are the same for both colours
    assert tiff.code_tables(0)[91:] == tiff.code_tables(1)[91:]


def _row_with(white, black):
    """a one-row picture whose first line is coded in horizontal mode as a white run, then a black run"""
    cols = white + black + 10
    row = np.zeros((1, cols), np.uint8)
    row[0, white:white + black] = 1
    return row


RUNS = list(range(64)) + list(range(64, 1729, 64)) + list(range(1792, 2561, 64)) + [5000]


@pytest.mark.parametrize("colour", [0, 1])
def test_every_code_is_what_libtiff_writes(colour):
    """For every run length 0..63, every make-up code and one run above 2560: Pillow encodes a crafted row, and the strip
    begins with the horizontal-mode prefix, the white run's codes and the black run's codes by our tables."""
    white, black = tiff_ref.tables()
    # which polarity Pillow stores: the strip's "black" runs are the picture's black pixels when Photometric is 0
    _, photo = _g4_single_strip(_row_with(5, 5))
    for n in RUNS:
        if colour == 1 and n == 0:
            continue  # a black run of 0 is written only behind a make-up code: 64 covers the terminating code 0
        w, b = (n, 7) if colour == 0 else (5, n)
        row = _row_with(w, b)
        strip, _ = _g4_single_strip(row if photo == 0 else 1 - row)
        got = _bitstring(strip)
        want = "001" + _expected_run(white, w) + _expected_run(black, b)
        assert got.startswith(want), (colour, n, got[:len(want) + 8], want)
        # and the restatement reads the strip back
        assert (tiff_ref.t6_decode(strip, 1, row.shape[1]) == row).all()


def test_restatement_equals_pillow_on_every_small_case():
    modes = set()
    for name, s in tiff_cases.small_cases():
        want = tiff_ref.pillow_read(s)
        got = tiff_ref.decode(s)
        assert got.shape == want.shape and (got == want).all(), name
    # the contents do force every mode
    for kind in ("checker", "stair", "stair4", "blobs", "text", "white"):
        a = tiff_cases.content(kind, 37, 100, seed=37100)
        s = tiff_ref.pillow_tiff(a)
        h = tiff_ref.parse(s)
        m = []
        for k, (off, n) in enumerate(h["strips"]):
            tiff_ref.t6_decode(s[off:off + n], min(h["rps"], 37 - k * h["rps"]), 100, modes=m)
        modes |= set(m)
    assert modes >= {"H", "P", "V0", "V+1", "V-1", "V+2", "V-2", "V+3", "V-3"}, modes


def test_long_runs_use_the_2560_code():
    white, _ = tiff_ref.tables()
    code2560 = "{:0{}b}".format(*[cb for cb, r in white.items() if r == 2560][0])
    for name, s in tiff_cases.long_run_cases():
        want = tiff_ref.pillow_read(s)
        assert (tiff_ref.decode(s) == want).all(), name
        h = tiff_ref.parse(s)
        off, n = h["strips"][0]
        m = []
        tiff_ref.t6_decode(s[off:off + n], min(h["rps"], h["rows"]), h["cols"], modes=m)
        if name != "wide-white":
            assert m[0] == "H", (name, m)
            bits = _bitstring(s[off:off + n])  # the long run comes first, or behind a white run of 0 (8 bits)
            assert bits[3:15] == code2560 or bits[11:23] == code2560, (name, bits[:40])


def test_assembler_round_trip():
    a = tiff_cases.content("text", 20, 100, seed=5)
    base = tiff_ref.pillow_tiff(a, "group4", 8)
    for order in "<>":
        for fill in (1, 2):
            for ot, ct in ((3, 3), (4, 4), (3, 4)):
                s = tiff_ref.rewrap(base, fill_order=fill, order=order, offsets_type=ot, counts_type=ct)
                assert (tiff_ref.pillow_read(s) == tiff_ref.pillow_read(base)).all()
                assert (tiff_ref.decode(s) == tiff_ref.pillow_read(base)).all()


def test_damage_is_reported():
    a = tiff_cases.content("text", 37, 257, seed=9)
    s = tiff_ref.pillow_tiff(a)
    (strip,) = tiff_ref.strips_of(s)
    with pytest.raises(tiff_ref.Damaged):
        tiff_ref.t6_decode(strip[:len(strip) // 2], 37, 257)
    pb = tiff_ref.strips_of(tiff_ref.pillow_tiff(a, "packbits"))
    with pytest.raises(tiff_ref.Damaged):
        tiff_ref.packbits_decode(pb[0] + b"\x7f" + bytes(128), 37 * 33 + 5)
