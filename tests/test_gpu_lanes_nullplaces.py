"""Null places of the scan-lane sweep's workgroups (slane.hip: slane_kernel, slane.hpp:
slane_wave_map, tools/gen_slane_asm.py: null_body).  A workgroup is 4 strips x 4 scan groups, 8 x 2 or 16 x 1; places
beyond the last strip, and scan groups that hold no scans in THIS launch, run a body of duties only, and a workgroup with
null strip places deals its waves to the SIMDs through a table.  Bar: bit-exact against the CPU oracle -- integer
projections of probed (scan, candidate) pairs, f64 std-dev bit patterns and the arg-max of EVERY scan -- at widths that
leave 0, 3, 2 and 1 null places in a workgroup of four strips (NS = 4, 5, 6, 7; one of them with the moved grid), for
every composition of a workgroup, and across launches of different sizes on one context, where the scan groups a smaller
launch does not use still hold the bit images of a larger one: they must not be swept (their row counts stay zero).
Rows: more than two 64-row blocks and a partial one, so the null waves meet the others three times or more."""
import numpy as np
import pytest
import torch

from oics import projection

pytestmark = pytest.mark.gpu

MAX_ANGLE, STEP = 2, 0.5
# cols -> rows; destination words 8, 10, 12, 14 and (287 = 31 modulo 32: the grid is moved 16 columns) 10
SHAPES = {256: 150, 289: 139, 353: 171, 417: 198, 287: 160}


def make_scans(rows, cols, n, seed):
    """n different binary scans: random dots of every density, some with rules, a white and a black one"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        img = np.where(rng.random((rows, cols)) < rng.uniform(0.02, 0.7), 0, 255).astype(np.uint8)
        if i % 3 == 1:
            img[rng.integers(0, rows, 5), :] = 0
            img[:, rng.integers(0, cols, 4)] = 0
        if i % 29 == 7:
            img[:] = 255 if i % 2 else 0
        out.append(img)
    return out


_pools = {}


def pool(oracle, cols, n):
    """the first n scans of the width's pool and their oracle scores (computed once per width, never changed)"""
    rows = SHAPES[cols]
    have = _pools.setdefault(cols, ([], []))
    if len(have[0]) < n:
        scans = make_scans(rows, cols, n, 13 * rows + cols)  # (a longer pool starts with the same scans: one seeded stream)
        for img in scans[len(have[0]):]:
            evs, ehs = oracle.sweep(img, MAX_ANGLE, STEP, want_proj=False)[2:]
            have[0].append(img)
            have[1].append((evs, ehs, oracle.argmax_path1(evs, ehs)[0]))
    return have[0][:n], have[1][:n]


class Lanes:
    """One scan-lane context and its device buffers"""

    def __init__(self, rows, cols, lanes):
        self.rows, self.cols, self.lanes = rows, cols, lanes
        self.A = projection.candidate_count(MAX_ANGLE, STEP)[1]
        self.dev = torch.device("cuda:0")
        self.b = projection.Batch(rows, cols, MAX_ANGLE, STEP, n_streams=1)
        self.b.set_lanes(lanes)

    def run(self, scans):
        n = len(scans)
        buf = torch.from_numpy(np.stack(scans)).to(self.dev)
        best = torch.zeros(n, dtype=torch.int32, device=self.dev)
        vs = torch.zeros((n, self.A), dtype=torch.float64, device=self.dev)
        hs = torch.zeros((n, self.A), dtype=torch.float64, device=self.dev)
        self.b.run_device(buf.data_ptr(), self.rows * self.cols, self.cols, n, 127, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
        self.b.sync()
        return best.cpu().numpy(), vs.cpu().numpy(), hs.cpu().numpy()

    def close(self):
        self.b.close()


def same_bits(x, y):
    return bool((np.ascontiguousarray(x).view(np.uint64) == np.ascontiguousarray(y).view(np.uint64)).all())


def check_scores(got, want, what):
    best, vs, hs = got
    for i, (evs, ehs, ebest) in enumerate(want):
        assert same_bits(vs[i], evs), "v_sd bits, %s scan %d" % (what, i)
        assert same_bits(hs[i], ehs), "h_sd bits, %s scan %d" % (what, i)
        assert best[i] == ebest, "arg-max, %s scan %d" % (what, i)


def rows_are_zero_beyond(L, n, scratch_set, what):
    """the row counts of the scan groups that hold no scans, first and last lane of each: nothing was added"""
    for g in range((n + 63) // 64, L.lanes // 64):
        for i in (64 * g, 64 * g + 63):
            for a in (0, L.A // 2, L.A - 1):
                hp = L.b.lanes_projections(i, a, L.rows, L.cols, scratch_set=scratch_set)[1]
                assert not hp.any(), "%s: row counts in scan group %d (lane %d, candidate %d) of a launch of %d scans" % (what, g, i % 64, a, n)


# scans, lanes of the context: 16 strips x 1 scan group (NS = 5: 11 null places), 8 x 2, 4 x 4 with one scan group of the
# quad empty (it exists in the scratch: a null task of this launch), 4 x 4 with every scan group in use
@pytest.mark.parametrize("n,lanes", [(1, 128), (70, 128), (130, 256), (256, 256)])
@pytest.mark.parametrize("cols", sorted(SHAPES))
def test_every_composition_at_every_count_of_null_strips(oracle, cols, n, lanes):
    rows = SHAPES[cols]
    scans, want = pool(oracle, cols, n)
    L = Lanes(rows, cols, lanes)
    L.b.lanes_keep(True)
    got = L.run(scans)
    probes = sorted({0, n - 1, n // 2, 64 * ((n - 1) // 64)})  # first and last lane, the middle, first lane of the last group
    proj = {(i, a): L.b.lanes_projections(i, a, rows, cols) for i in probes for a in range(L.A)}
    rows_are_zero_beyond(L, n, 0, "%d columns" % cols)
    L.close()
    check_scores(got, want, "%d columns, %d scans," % (cols, n))
    for i in probes:
        evp, ehp = oracle.sweep(scans[i], MAX_ANGLE, STEP)[:2]
        for a in range(L.A):
            assert (proj[(i, a)][0] == evp[a]).all(), "column counts, scan %d candidate %d" % (i, a)
            assert (proj[(i, a)][1] == ehp[a]).all(), "row counts, scan %d candidate %d" % (i, a)


# Launches of different sizes on one context of 512 lanes.  Its two scratch sets alternate, so with one launch more in
# front the smaller launches fall on the other set; either way a launch of 320 scans finds, in scan groups 5-7 of its set,
# the bit images a launch of 512 scans left there.  The 512-scan launches take their scans from the pool's first half, the
# smaller ones from its second half: what lies in the unused groups is never what the launch was given.
SEQUENCE = ((512, 0), (320, 512), (512, 0), (64, 768), (320, 512))  # scans, first scan of the pool


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("lead", [0, 1])
def test_scan_groups_without_scans_are_not_swept(oracle, lead, keep):
    cols = 289
    rows = SHAPES[cols]
    scans, want = pool(oracle, cols, 832)
    rng = np.random.Generator(np.random.PCG64(5 + lead))
    L = Lanes(rows, cols, 512)
    L.b.lanes_keep(keep)
    for call, (n, first) in enumerate(((512, 0),) * lead + SEQUENCE):
        pick = first + rng.permutation(512 if n == 512 else n)[:n]
        got = L.run([scans[k] for k in pick])
        check_scores(got, [want[k] for k in pick], "call %d (%d scans)," % (call, n))
        if keep:
            i = n - 1  # the last scan's row counts are there ...
            hp = L.b.lanes_projections(i, L.A - 1, rows, cols, scratch_set=call % 2)[1]
            assert (hp == oracle.sweep(scans[pick[i]], MAX_ANGLE, STEP)[1][L.A - 1]).all(), "row counts, call %d scan %d" % (call, i)
            rows_are_zero_beyond(L, n, call % 2, "call %d" % call)  # ... and none beyond the groups in use
    L.close()
