"""slane_wave_map (csrc/slane.hpp): which (strip place, scan group) each of the 16 waves of a scan-lane workgroup with null
strip places takes.  Compiled on its own (no GPU, no HIP), for every composition of a workgroup (4 strips x 4 scan groups,
8 x 2, 16 x 1), every number of places that hold a strip and of scan groups that hold scans:
  * the map is a permutation of the workgroup's (place, scan group) pairs -- every task is run once;
  * waves w, w + 4, w + 8, w + 12 share a SIMD: no SIMD holds more than ceil(nulls / 4) null waves (stacked on one SIMD they
    left it idle while the other three set the workgroup's duration);
  * the waves of a strip share a SIMD as far as they fit: a strip is never spread over more SIMDs than a strip that was cut
    once needs, and at the bench's case (4 x 4, three strips) three SIMDs hold three waves of ONE strip each."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = os.path.join(ROOT, "omr-img-corrector_amd", "csrc", "slane.hpp")

MAIN = r"""#include <stdint.h>
#include <stdio.h>
#include <string.h>
%s
int main() {
    for (int lg = 0; lg < 3; lg++)
        for (int rp = 1; rp <= 16 >> lg; rp++)
            for (int rs = 1; rs <= 1 << lg; rs++) {
                const int places = 16 >> lg, sgw = 1 << lg, nulls = 16 - rp * rs;
                uint8_t m[16];
                slane_wave_map(4 - lg, rp, rs, m);
                int seen[16][4], null_on[4] = {0, 0, 0, 0}, simds_of[16];
                memset(seen, 0, sizeof seen), memset(simds_of, 0, sizeof simds_of);
                for (int w = 0; w < 16; w++) {
                    const int p = m[w] & 15, s = m[w] >> 4;
                    if (p >= places || s >= sgw || seen[p][s]++) return printf("not a permutation: lg %%d rp %%d rs %%d\n", lg, rp, rs), 1;
                    if (p >= rp || s >= rs) null_on[w & 3]++;
                    else simds_of[p] |= 1 << (w & 3);
                }
                for (int k = 0; k < 4; k++)
                    if (null_on[k] > (nulls + 3) / 4) return printf("%%d null waves on SIMD %%d: lg %%d rp %%d rs %%d\n", null_on[k], k, lg, rp, rs), 2;
                const int per = (rp * rs + 3) / 4;  // real waves a SIMD can take
                for (int p = 0; p < rp; p++)
                    if (__builtin_popcount(simds_of[p]) > (rs + per - 1) / per + 1)
                        return printf("strip %%d on %%d SIMDs: lg %%d rp %%d rs %%d\n", p, __builtin_popcount(simds_of[p]), lg, rp, rs), 3;
            }
    uint8_t m[16];
    slane_wave_map(2, 3, 4, m);  // 4 x 4, the last strip group of 39 strips
    for (int k = 0; k < 3; k++)
        if ((m[k] & 15) != k || (m[k + 4] & 15) != k || (m[k + 8] & 15) != k || (m[k + 12] & 15) != 3)
            return printf("SIMD %%d does not hold three waves of strip %%d and one null wave\n", k, k), 4;
    puts("ok");
    return 0;
}
"""


def test_null_places_are_spread_and_strips_stay_together(tmp_path):
    m = re.search(r"inline void slane_wave_map\(.*?\n\}\n", open(HPP).read(), re.S)
    assert m, "slane_wave_map not found in slane.hpp"
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    src, exe = str(tmp_path / "w.cpp"), str(tmp_path / "w")
    open(src, "w").write(MAIN % m.group(0))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
