"""tiff8_rewrap.py, the instrument of test_gpu_tiff8_foreign.py, validated before the kernels are held to it.  No GPU.

Every dialect stream is read by Pillow (libtiff's decoder) as the picture it was made from, and by the restatement
tiff8_ref.decode; every pin raises there with its code.  The conditions under which a dialect proves nothing are asserted:
the literal streams hold literals of 9 bits alone, a capped code is no longer than its cap, "short" is another code stream
than the longest-match coder's, the period streams name entries made within the last 64 codes and exactly 63, 64 and 65
codes earlier, the cut strips hold a code that straddles the rows' end, and the long constant page reaches the entry
lengths a real page does.

Dropped from the comparison with Pillow, by name (tiff8_rewrap.NO_ARBITER): the files of several LZW or PackBits strips
without StripByteCounts.  Pillow raises OSError("decoder error -2") behind libtiff's 'MissingRequired: TIFF directory is
missing required "StripByteCounts" field'."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import t6_rewrap  # noqa: E402
import tiff8_ref as R  # noqa: E402
import tiff8_rewrap as T  # noqa: E402
import tiff_ref  # noqa: E402


def _check(cases):
    for case in cases:
        name, s, want = case[:3]
        got = R.decode(s)
        assert got.shape == want.shape and (got == want).all(), (name, "the restatement")
        if name in T.NO_ARBITER:
            with pytest.raises(OSError, match="decoder error -2"):
                R.pillow_read(s)
            continue
        got = R.pillow_read(s)
        assert got.shape == want.shape and (got == want).all(), (name, "Pillow")


def _strip_codes(s):
    """[(the codes of a strip up to the one that fills its rows, the bytes of its rows)]"""
    h = R.parse(s)
    out = []
    for k, (off, ln) in enumerate(h["strips"]):
        total = min(h["rps"], h["rows"] - k * h["rps"]) * h["cols"] * h["spp"]
        out.append((T.read_codes(s[off:off + ln], total), total))
    return out


@pytest.mark.parametrize("spp", [1, 3])
def test_policy_dialects_are_read_by_pillow_and_the_restatement(spp):
    cases = T.policy_dialects(spp)
    assert len(cases) == 5 * (1 + 2 + 3) * len(T.POLICIES) == 450
    for ending, least in (("eoi", 90), ("none", 90), ("junk", 90), ("rows+", 90), ("overrun", 20)):  # 42 of the 90 have a policy that matches at all
        assert sum("-%s-" % ending in n for n, _, _ in cases) >= least, ending
    for policy in T.POLICIES:  # every policy with and without EOI
        mine = [n for n, _, _ in cases if n.startswith("lzw-%s-" % policy)]
        assert any("-eoi-" in n for n in mine) and any("-none-" in n or "-junk-" in n for n in mine), policy
    _check(cases)


def test_literal_streams_hold_literals_of_9_bits_and_nothing_else():
    n = 0
    for spp in (1, 3):
        for name, s, _ in T.policy_dialects(spp):
            if not name.startswith("lzw-literal-"):
                continue
            every = int(name.split("-")[2])
            for codes, total in _strip_codes(s):
                w = T.walk(codes)
                assert all(c < 256 and R.width(i) == 9 for _, i, c, _, _, _ in w), name
                assert max(i for _, i, _, _, _, _ in w) == min(every, total) - 1, name
                # the Clear behind `every` literals: 9 bits, but for 254, where its index is the first of 10 bits
                assert all(c == T.CLEAR for c in codes[every + 1::every + 1]) and R.width(every) == (10 if every == 254 else 9)
                n += 1
    assert n > 1000


def test_a_capped_code_is_no_longer_than_its_cap():
    longest = {}
    for spp in (1, 3):
        for name, s, _ in T.policy_dialects(spp):
            if name.startswith("lzw-cap-"):
                cap = int(name.split("-")[2])
                for codes, _ in _strip_codes(s):
                    ln = max(w[4] for w in T.walk(codes))
                    assert ln <= cap, name
                    longest[cap] = max(longest.get(cap, 0), ln)
    assert longest == {2: 2, 3: 3, 8: 8}


def test_short_is_another_code_stream_than_the_longest_match_coders():
    """for every content but noise, at least half of the codes "short" writes stand where the longest-match coder has
    none, or have another length there"""
    for kind in T.KINDS:
        differ = total = 0
        for spp in (1, 3):
            a = R.content(kind, 33, 257, spp, seed=33257)
            raw = a.tobytes()
            greedy = set(T._recode(raw, "cadence-0")[1])
            short = T._recode(raw, "short", 5)[1]
            differ += sum(sp not in greedy for sp in short)
            total += len(short)
        if kind != "noise":
            assert 2 * differ >= total, (kind, differ, total)
    # it names earlier entries of equal bytes and writes short codes in front of the entry that would have covered them
    codes = T.lzw_recode(bytes(300), "short", 1)
    w = T.walk(codes)
    assert any(a[4] < b[4] and a[2] < b[2] for a, b in zip(w, w[1:])) and R.lzw_decode(R.pack_codes(codes), 300) == bytes(300)


def test_period_streams_name_entries_made_in_the_same_round_and_across_its_boundary():
    cases = T.period_dialects()
    assert len(cases) == 2 * len(T.PERIODS)
    _check(cases)
    for name, s, _ in cases:
        p = int(name.split("-")[1])
        back = set()
        for codes, _ in _strip_codes(s):
            back |= {w[5] for w in T.walk(codes) if w[5] is not None}
        assert min(back) < 64, name
        if p in (63, 64, 65):
            assert {63, 64, 65} <= back, (name, sorted(back))


def test_cut_strips_hold_a_code_across_the_rows_end():
    cases = T.cut_dialects()
    lzw = [c for c in cases if c[0].startswith("cut-lzw-")]
    assert len(lzw) >= 60 and len(cases) - len(lzw) == 12
    assert sum(n.endswith("-rps5") for n, _, _ in lzw) >= 16  # five strips each, a good strip behind every cut one but the last
    for ending in ("rows+", "overrun"):
        for policy in ("cadence-300", "cap-8", "short", "cadence-1800"):
            assert sum("-%s-%s-" % (policy, ending) in n for n, _, _ in lzw) >= 4, (policy, ending)
    _check(cases)
    for name, s, _ in lzw:
        h = R.parse(s)
        for k, (off, ln) in enumerate(h["strips"]):
            total = min(h["rps"], h["rows"] - k * h["rps"]) * h["cols"] * h["spp"]
            codes = T.read_codes(s[off:off + ln], total)
            last = T.walk(codes)[-1]
            assert last[3] < total < last[3] + last[4], (name, k)  # cut, not dropped whole
            if "-overrun-" in name:  # nothing stands behind that code
                assert len(R.pack_codes(codes)) == ln, (name, k)
            else:
                assert ln > len(R.pack_codes(codes)) + 2, (name, k)
    # the files of the two other compressions carry RowsPerStrip rows in the last strip
    for name, s, _ in cases:
        if name.startswith("cut-lzw-"):
            continue
        h = R.parse(s)
        rb, tag = h["cols"] * h["spp"], int(name.rsplit("rps", 1)[1])
        off, ln = h["strips"][-1]
        data = s[off:off + ln]
        assert tag > h["rows"] - (len(h["strips"]) - 1) * h["rps"]
        assert len(data if h["compression"] == 1 else tiff_ref.packbits_decode(data, tag * rb)) == tag * rb, name


def test_the_long_constant_page_reaches_the_longest_entries():
    cases = T.long_constant()
    assert [c[0] for c in cases] == ["long-constant-libtiff", "long-constant-late", "long-constant-rows+"]
    assert [c[3] for c in cases] == [3836, 3839, 3839] and min(c[3] for c in cases) >= 3800
    _check(cases)
    for name, s, want, _ in cases:
        (codes, total) = _strip_codes(s)[-1]
        w = T.walk(codes)
        assert max(x[4] for x in w) >= (3000 if name.endswith("rows+") else 3800)
        assert (max(x[2] for x in w) == 4095) == name.endswith("late"), name  # entry 4095 made and used
        if name.endswith("rows+"):
            assert total == T.LONG_CUT * T.LONG_COLS and w[-1][3] < total < w[-1][3] + w[-1][4] and w[-1][4] >= 3000
    # the closed form is what the longest-match coder writes
    assert T.constant_codes(200, 5000, 300)[0] == T.lzw_recode(bytes([200]) * 5000, "cadence-300")
    assert T.constant_codes(7, 70 * 257)[0] == R.lzw_codes(bytes([7]) * (70 * 257))


def test_wide_rows_packbits_and_ifd_dialects_are_read_by_pillow_and_the_restatement():
    wide = T.wide_dialects()
    assert sorted({c[2].shape[1] for c in wide}) == [1023, 1024, 1025, 2048, 2049] and len(wide) == 10
    assert all(R.parse(s)["predictor"] == 2 for _, s, _ in wide) and sum(R.parse(s)["photometric"] == 0 for _, s, _ in wide) == 1
    _check(wide)
    pb = T.packbits_dialects()
    assert len(pb) == 2 * 2 * 3 * 4
    _check(pb)
    # a crossing run does straddle a row of 77 and of 3 x 53 bytes
    for cols, spp in ((77, 1), (53, 3)):
        a = R.content("constant", 19, cols, spp)
        assert t6_rewrap.packbits_encode(a.tobytes(), "crossing", 0, cols * spp)[:2] == bytes([129, 200])
    ifd = T.ifd_dialects()
    assert len(T.NO_ARBITER) == 9 and all("no-counts" in n and "raw" not in n for n in T.NO_ARBITER)
    for form in ("ifd-first", "odd", "shuffled", "reverse-gaps", "gaps", "shared", "counts-over", "big-endian", "short-arrays", "bits-long",
                 "chained", "no-278", "no-counts"):
        assert {"ifd-%s-%s" % (p, form) for p in ("lzw2-rgb", "lzw-gray", "packbits-gray", "raw-rgb")} <= {n for n, _, _ in ifd}, form
    assert sum(n.endswith("-no-277") for n, _, _ in ifd) == 2
    _check(ifd)
    for name, s, _ in ifd:  # the odd forms put every strip at an odd offset
        if name.endswith("-odd"):
            assert all(off & 1 for off, _ in R.parse(s)["strips"]), name


def test_pins_raise_in_the_restatement_with_their_codes():
    pins = T.pins()
    assert [c for _, _, c in pins] == [-213] * 6 + [-215] * 2
    for name, s, code in pins:
        if code == -215:
            assert R.parse(s)["compression"] == 5
            with pytest.raises(R.Damaged):
                R.decode(s)
            with pytest.raises(OSError):
                R.pillow_read(s)
        else:
            with pytest.raises(R.Refused) as e:
                R.parse(s)
            assert e.value.code == code, name
    by = {n: s for n, s, _ in pins}
    # the chosen differences from libtiff: it reads a file without PhotometricInterpretation as MinIsWhite (Pillow: mode L,
    # the stored bytes inverted), PlanarConfiguration 2 as three planes, and FillOrder 2 at 8 bits with every byte bit-reversed
    g = R.content("text", 6, 40, 1, seed=4)
    assert (R.pillow_read(by["no PhotometricInterpretation at 8 bits"]) == 255 - g).all()
    assert R.pillow_read(by["PlanarConfiguration 2 with three samples"]).shape == (6, 40, 3)
    assert (R.pillow_read(by["FillOrder 2 at 8 bits"]) == np.frombuffer(g.tobytes().translate(tiff_ref._REV), np.uint8).reshape(6, 40)).all()
    # the 9-bit literals: the strip is sound but for its widths
    hi = by["literals at 9 bits past index 253"]
    off, ln = R.parse(hi)["strips"][0]
    bits = "".join("{:08b}".format(b) for b in hi[off:off + ln])
    nine = [int(bits[k:k + 9], 2) for k in range(0, 9 * 258, 9)]
    assert nine[0] == 256 and all(c < 256 for c in nine[1:256]) and nine[256] == 256
