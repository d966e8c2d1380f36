"""The tight cut of the wet-row table (round 8) is decided by one host-only function, wet_cut_tight() in csrc/gcmf_wet_cut.hpp.
tests/wet_cut/print_wet_cut.cpp is compiled with g++ against that header alone -- no HIP, no library, no GPU -- and must give every mask
the cut that the numpy restatement of the rules gives (tests/wet_tight_model.py), and pairs that own every exchanging cell exactly once."""
import os
import subprocess

import numpy as np
import pytest

from gcm_filters_amd import testing as T
from tests import wet_tight_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")
BIG, SMALL = (192, 432), (97, 236)


def band(shape):
    ny, nx = shape
    wet = np.ones(shape)
    wet[ny // 2 - 36 : ny // 2 + 36, :] = 0
    wet[ny // 2, 150:152] = 1
    return wet


def masks():
    out = []
    for shape in (BIG, SMALL):
        out.append(("fixture", T.land_mask(shape)))
        for name in ("lakes", "all_land", "on_the_cuts", "one_land_cell", "speckle"):
            out.append((name, T.coastline(name, shape, seed=7)))
    out.append(("band", band(BIG)))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wet_cut") / "print_wet_cut")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "wet_cut", "print_wet_cut.cpp"), "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def _ask(exe, opened, S, list_units):
    ny, nx = opened.shape
    text = f"{ny} {nx} {S} 0 {ny} {int(list_units)}\n" + "\n".join("".join("1" if v else "0" for v in row) for row in opened) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    head = dict(kv.split("=") for kv in lines[0].split())
    units = [tuple(int(v) for v in line.split()) for line in lines[1:]]
    return {k: int(v) for k, v in head.items()}, units


def test_the_planner_header_is_host_only():
    with open(os.path.join(CSRC, "gcmf_wet_cut.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<algorithm>", "<cstdint>", "<vector>", '"gcmf_ringc_cut.hpp"'], includes


@pytest.mark.parametrize("S", [9, 8, 5])
def test_planner_gives_the_models_cut_and_owns_every_exchanging_cell_once(exe, S):
    for name, wet in masks():
        opened = M.exchanging(wet)
        ny, nx = opened.shape
        head, units = _ask(exe, opened, S, True)
        want = M.model(wet, S)
        got = (head["units"], head["H"], head["nstrips"], head["xoff"], head["march"])
        assert head["ok"] == 1 and got == want, (name, wet.shape, S, got, want)
        assert len(units) == head["units"] <= 512
        WI = M.window_width(S)
        Mg = (128 - WI) // 2
        owned = np.zeros(opened.shape, int)
        tallest = 0
        for x0, lo, mid, hi in units:
            assert 0 <= lo and lo + 2 <= mid and mid + 2 <= hi <= ny, (name, x0, lo, mid, hi)
            tallest = max(tallest, mid - lo, hi - mid)
            first = x0 + Mg
            assert (first - head["xoff"]) % WI == 0 and first % 2 == 0
            cols = np.arange(first, min(first + WI, head["xoff"] + nx)) % nx
            owned[lo:hi, cols] += 1
        assert tallest == head["H"]
        assert owned.max(initial=0) <= 1, name
        assert (owned[opened] == 1).all(), name
        assert owned.sum() <= head["owned"] * WI
        assert [u[2] for u in units] == sorted(u[2] for u in units)


def test_a_row_range_and_a_mask_the_table_refuses(exe):
    wet = T.land_mask(BIG)
    opened = M.exchanging(wet)
    ny, nx = opened.shape
    text = f"{ny} {nx} 9 40 100 1\n" + "\n".join("".join("1" if v else "0" for v in row) for row in opened) + "\n"
    text += "3 8 9 0 3 0\n" + "11111111\n" * 3          # (fewer than four rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("ok=1 ")
    units = [tuple(int(v) for v in line.split()) for line in lines[1:-1]]
    assert units and all(40 <= lo and hi <= 100 for _, lo, _, hi in units)
    assert lines[-1].startswith("ok=0 ")


def test_baseline_size_fixture_mask(exe):
    """2400 x 3600 at nine levels: 510 pairs, the tallest strip 60 rows marching 72, the window grid shifted by 36 columns (the table of
    round 7: 507 pairs, 67 rows marching 80; the tight rules with the grid pinned at column 0: 76)."""
    wet = T.land_mask((2400, 3600))
    head, _ = _ask(exe, M.exchanging(wet), 9, False)
    assert (head["units"], head["H"], head["xoff"], head["march"]) == (510, 60, 36, 72), head
    assert M.model(wet, 9)[:2] + M.model(wet, 9)[3:] == (510, 60, 36, 72)
    assert M.model(wet, 9, xoffs=[0])[4] == 76
