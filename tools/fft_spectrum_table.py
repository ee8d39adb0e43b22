"""Makes profiles/r29_fft_spectrum.md from the figures tests/test_gpu_fft_spectrum.py prints (pytest -s): one FFTSPEC line
per case.  Usage: python tools/fft_spectrum_table.py <pytest log> > profiles/r29_fft_spectrum.md"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fft_ref as R  # noqa: E402


def ratio(kernel, standin):
    """the worst of rms, maximum and DC, each against the stand-in's error counted as at least the floor"""
    return max(k / max(s, R.FLOOR) for k, s in zip(kernel, standin))


def fmt(e):
    return "%.1e / %.1e / %.1e" % tuple(e)


def line(c, which):
    s, k, f = (c["standin_row"], c["kernel_row"], c["row_factor"]) if which == "row" else (c["standin_mag"], c["kernel_mag"], c["mag_factor"])
    return "| %s | %s | %.2f | %d | %.3f / %.3f | %d / %d |" % (fmt(s), fmt(k), ratio(k, s), f, c["zone"][0], c["zone"][1],
                                                               c["mismatch"][0], c["mismatch"][1])


def main():
    cases = [json.loads(m.group(1)) for m in re.finditer(r"FFTSPEC (\{.*\})", open(sys.argv[1]).read())]
    by_shape = {}
    for c in cases:
        by_shape.setdefault((c["rows"], c["cols"]), {})[c["kind"]] = c
    head = "| stand-in rms / max / DC | kernel rms / max / DC | worst ratio | factor | zone share mag / log | mismatches mag / log |"
    rule = "|---|---|---|---|---|---|"
    out = ["# The FFT kernels' float spectrum against a float64 DFT (`tests/test_gpu_fft_spectrum.py`, MI355X)", "",
           "Errors over every bin but DC, normalised by the rms of the float64 reference over those bins (the constant image:",
           "by DC); DC relative to itself.  Stand-in: `scipy.fft` on complex64, same input, same measures.  Ratio: kernel /",
           "max(stand-in, 2e-7), the worst of the three; it must stay under the factor (8 direct, 16 chirp; for the magnitudes the",
           "larger of the two axes').  Row pass: the complex half spectrum; column pass: the magnitudes of the 2-D transform",
           "(the other axis is 5 or 8 points, a power of two or a small Bluestein line).  Zone: share of a picture's pixels",
           "within 0.01 grey level of a rounding boundary in the float64 restatement (limit 0.05); mismatches: bytes that",
           "differ outside it.  %d cases." % len(cases), "",
           "## Every factorisation as row pass and as column pass", "",
           "| path | n | pass | shape | input " + head, "|---|---|---|---|---" + rule]
    worst = {}
    lengths = set(R.LENGTHS)
    for (rows, cols), kinds in by_shape.items():
        for which, n, o in (("row", cols, rows), ("column", rows, cols)):
            if n in lengths and o in (5, 8) and (rows, cols) in R.shapes_all_inputs()[:2 * len(R.LENGTHS)]:
                for kind in R.INPUTS:
                    c = kinds[kind]
                    path = c["row_path"] if which == "row" else c["col_path"]
                    out.append("| %s | %d | %s | %d × %d | %s %s" % (path, n, which, rows, cols, kind, line(c, "row" if which == "row" else "mag")))
                    s, k = (c["standin_row"], c["kernel_row"]) if which == "row" else (c["standin_mag"], c["kernel_mag"])
                    key = (path, which, c["row_factor"] if which == "row" else c["mag_factor"])
                    worst[key] = max(worst.get(key, 0.0), ratio(k, s))
    out += ["", "## Worst ratio per path and pass", "", "| path | pass | worst ratio | factor |", "|---|---|---|---|"]
    for (path, which, factor), r in sorted(worst.items()):  # (a direct column pass behind a 5-point chirp row pass: 16)
        out.append("| %s | %s | %.2f | %d |" % (path, which, r, factor))
    out += ["", "## Pairing edges and both passes at once", "", "| shape | input | measure " + head, "|---|---|---" + rule]
    for shape in R.shapes_all_inputs()[2 * len(R.LENGTHS):]:
        for kind in R.INPUTS:
            c = by_shape[shape][kind]
            out.append("| %d × %d | %s | row pass %s" % (shape + (kind, line(c, "row"))))
            out.append("| %d × %d | %s | magnitudes %s" % (shape + (kind, line(c, "mag"))))
    small = [by_shape[s]["noise"] for s in R.shapes_noise_only() if s in by_shape]
    out += ["", "## Every axis length 1 … 33 on noise (n × 8 and 8 × n, %d cases)" % len(small), "",
            "worst ratio, row pass: %.2f; magnitudes: %.2f; largest zone share: %.3f; mismatches: %d." % (
                max(ratio(c["kernel_row"], c["standin_row"]) for c in small),
                max(ratio(c["kernel_mag"], c["standin_mag"]) for c in small),
                max(max(c["zone"]) for c in small), sum(sum(c["mismatch"]) for c in small)), "",
            "All %d cases: extrema bit-identical in %d, worst ratio to its factor %.2f, largest zone share %.3f, mismatches %d." % (
                len(cases), sum(c["extrema"] for c in cases),
                max(max(ratio(c["kernel_row"], c["standin_row"]) / c["row_factor"], ratio(c["kernel_mag"], c["standin_mag"]) / c["mag_factor"]) for c in cases),
                max(max(c["zone"]) for c in cases), sum(sum(c["mismatch"]) for c in cases)), ""]
    print("\n".join(out))


if __name__ == "__main__":
    main()
