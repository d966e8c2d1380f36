"""Whether a nine-level table launch of k_ringcz streams its state planes (round 10, option "stream_state" 1) is host arithmetic:
``stream_state_ok(owned cells)`` of csrc/gcmf_wet_cut.hpp -- owned cells x 65 bytes against ONE named budget, the 256 MiB of the memory-side
cache -- on the count ``table_owned_cells`` takes from the table's pairs.  tests/stream_state/print_stream.cpp is compiled with g++ against
that header alone -- no HIP, no library, no GPU -- and asked about config 3's table, a grid whose whole working set is cache-resident, and
both sides of the budget's edge."""
import os
import subprocess

import numpy as np
import pytest

from gcm_filters_amd import testing as T
from tests import wet_tight_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")
BUDGET, CELL = 256 * 2**20, 65


def _compile(tmp, src, name):
    path = str(tmp / name)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", *src), "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stream_state")
    return _compile(tmp, ("stream_state", "print_stream.cpp"), "print_stream"), _compile(tmp, ("wet_cut", "print_wet_cut.cpp"), "print_wet_cut")


def _answers(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]


def _rows(opened):
    return "\n".join("".join("1" if v else "0" for v in row) for row in opened) + "\n"


def _table(exes, shape):
    """(the predicate's answer for the tight nine-level table of the fixture mask, the cells its pairs own counted in numpy)"""
    opened = M.exchanging(T.land_mask(shape))
    ny, nx = opened.shape
    (ans,) = _answers(exes[0], f"m {ny} {nx} 9\n" + _rows(opened))
    r = subprocess.run([exes[1]], input=f"{ny} {nx} 9 0 {ny} 1\n" + _rows(opened), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    head = dict(kv.split("=") for kv in lines[0].split())
    WI = M.window_width(9)
    owned = np.zeros(shape, int)
    for line in lines[1:]:
        x0, lo, mid, hi = (int(v) for v in line.split())
        first = x0 + (128 - WI) // 2
        owned[lo:hi, np.arange(first, min(first + WI, int(head["xoff"]) + nx)) % nx] += 1
    assert owned.max() == 1
    return ans, int(owned.sum())


def test_one_named_budget(exes):
    (ans,) = _answers(exes[0], "c 1\n")
    assert (ans["budget"], ans["cell_bytes"]) == (BUDGET, CELL)
    with open(os.path.join(CSRC, "gcmf_wet_cut.hpp")) as f:
        text = f.read()
    assert text.count("256ll << 20") == 1 and "constexpr long long STREAM_CACHE_BYTES = 256ll << 20;" in text


def test_config_3_streams(exes):
    """2400 x 3600, the fixture mask: 510 pairs own 6.5 M cells, 421 MB a launch."""
    ans, cells = _table(exes, (2400, 3600))
    assert ans["cells"] == cells and 6_400_000 < cells < 6_600_000, (ans, cells)
    assert cells * CELL > BUDGET and ans["stream"] == 1


def test_a_cache_resident_grid_keeps_the_default_policy(exes):
    """1080 x 1440: the whole grid is 1.56 M cells, 101 MB a launch -- the state IS re-read from the cache."""
    ans, cells = _table(exes, (1080, 1440))
    assert ans["cells"] == cells and 0 < cells <= 1080 * 1440, (ans, cells)
    assert cells * CELL < BUDGET and ans["stream"] == 0


def test_the_edge_of_the_budget(exes):
    edge = BUDGET // CELL          # the most cells whose 65 bytes each still fit
    assert edge * CELL <= BUDGET < (edge + 1) * CELL
    counts = [-5, 0, 1, edge - 1, edge, edge + 1, edge + 2, 2400 * 3600, 2**40, 2**62]
    got = _answers(exes[0], "".join(f"c {n}\n" for n in counts))
    assert [a["cells"] for a in got] == counts
    assert [a["stream"] for a in got] == [1 if n * CELL > BUDGET else 0 for n in counts] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]


def test_the_launcher_asks_the_predicate():
    with open(os.path.join(CSRC, "gcmf_ringc_impl.hpp")) as f:
        text = f.read()
    assert "pl->stream_state >= 2 || (pl->stream_state == 1 && stream_state_ok(tab->cells))" in text
    with open(os.path.join(CSRC, "gcmf_ringc_zip.hip")) as f:
        assert f.read().count("nt.cells = table_owned_cells(") == 2      # (the tight table and round 7's)
