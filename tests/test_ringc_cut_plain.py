"""A filter bank on a tripolar plan (gcmf_apply_bank on TRIPOLAR_POP_WITH_LAND) runs the plain strips below the tripole seam and k_fold_band on
the seam's rows: ringc_march has no per-entry polynomial form of the zipped strips.  The planner is told through RingcCutIn::stacked, and
must honour it at the seam as it does everywhere else: tests/ringc_cut/plain_cut.cpp (g++ against csrc/gcmf_ringc_cut.hpp alone -- no HIP, no
library, no GPU) asks for every launch a bank can make on the shapes of tests/test_gpu_filter_bank_pop.py and at BASELINE size -- batches
1 .. 64, 5 .. 8 levels, the band beside and after the launch, the zipped forms switched on -- and the answer must be k_ringc on the rows
below the band with one grid row per entry.  The same inputs without `stacked` do take the zipped fold strips where the grid qualifies:
that is what an ordinary gcmf_apply keeps running."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")
SHAPES = [(96, 160), (96, 168), (200, 520), (2400, 3600)]


def _cuts(tmp_path):
    exe = str(tmp_path / "plain_cut")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "ringc_cut", "plain_cut.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, cut = line.split(" -> ")
        rows, nx, batch, S, beside, stacked = (int(x) for x in key.split())
        form, *fields = cut.split()
        out[(rows, nx, batch, S, beside, stacked)] = dict(form=form, **{k: int(v) for k, v in (f.split("=") for f in fields)})
    return out


def test_a_bank_on_the_seams_plan_runs_the_plain_strips(tmp_path):
    cuts = _cuts(tmp_path)
    assert len(cuts) == len(SHAPES) * 64 * 4 * 2 * 2
    wrong = []
    for (rows, nx) in SHAPES:
        for batch in range(1, 65):
            for S in range(5, 9):
                for beside in (0, 1):
                    c = cuts[(rows, nx, batch, S, beside, 1)]
                    if not (c["form"] == "k_ringc" and c["xe"] == 0 and c["rows"] == rows - S and c["grid_y"] == batch and c["npack"] == 0
                            and c["fold_rows"] == 0):
                        wrong.append(((rows, nx, batch, S, beside), c))
    assert not wrong, wrong[:10]
    # ... and an ordinary launch of the same shape keeps the zipped fold strips (nx >= 256, a band that does not run beside)
    for (rows, nx) in [(200, 520), (2400, 3600)]:
        for S in range(5, 9):
            c = cuts[(rows, nx, 1, S, 0, 0)]
            assert c["form"] == "k_ringcz+fold" and c["rows"] == rows and c["fold_rows"] >= S, (rows, nx, S, c)
    for S in range(5, 9):      # (nx < 256: the band either way)
        assert cuts[(96, 160, 1, S, 0, 0)]["rows"] == 96 - S
