"""A table march of k_ringcz (round 9) addresses a plane with one 32-bit byte offset per lane and row; the launcher takes a table only where
table_rows_fit32() of csrc/gcmf_wet_cut.hpp says that every byte of a plane, and one row beyond the last, lies below 2^32 -- and, the march
knowing no closed end, where the grid wraps in y (table_rows_ok).  The predicates are host arithmetic on numbers: tests/table_rows/print_fit32.cpp is compiled with g++ against that header alone -- no HIP, no library, no
GPU, nothing allocated -- and asked about shapes on both sides of the boundary."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("table_rows") / "print_fit32")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "table_rows", "print_fit32.cpp"), "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def _ask(exe, shapes):
    text = "".join(f"{r} {n} {c}\n" for r, n, c in shapes)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(shapes)
    for fit, ok_wrap, ok_closed in rows:      # (table_rows_ok: the same answer on a grid that wraps in y, never on one with closed ends)
        assert ok_wrap == fit and ok_closed == 0
    return [row[0] for row in rows]


def test_the_boundary_on_both_sides(exe):
    """rows nx cell < 2^32 exactly: the last shape below, the first at and the first above, for planes of one row, of square-ish shapes
    and of f32 cells; the model is Python's integers."""
    shapes = [
        (1, 2**29 - 1, 8), (1, 2**29, 8), (1, 2**29 + 1, 8),          # one row: 2^32 - 8, 2^32, 2^32 + 8 bytes
        (2**29 - 1, 1, 8), (2**29, 1, 8),
        (16384, 32768, 8), (16383, 32768, 8), (16384, 32766, 8),     # 2^32 exactly, one row less, two columns less
        (23170, 23170, 8), (23171, 23170, 8),                        # 4 294 791 200 fits; one row more: 4 294 976 560 > 2^32 - 1
        (32768, 32768, 4), (32767, 32768, 4),                        # f32 cells
        (65536, 65536, 1), (65535, 65536, 1), (65536, 65535, 1),
        (2**31, 2**31, 8), (2**40, 2**40, 8), (1, 2**62, 8),         # products beyond 64 bits must not wrap into "fits"
    ]
    want = [1 if r * n * c < 2**32 else 0 for r, n, c in shapes]
    assert 0 in want and 1 in want and want[:3] == [1, 0, 0] and want[5:8] == [0, 1, 1] and want[8:10] == [1, 0]
    assert _ask(exe, shapes) == want


def test_shapes_that_are_no_plane_are_refused(exe):
    assert _ask(exe, [(0, 3600, 8), (2400, 0, 8), (2400, 3600, 0), (-1, 3600, 8), (2400, -3600, 8)]) == [0, 0, 0, 0, 0]


def test_the_grids_of_the_benchmark_fit(exe):
    """config 3 (2400 x 3600 f64: 69 MB a plane), the mid-size grids and a 1/12-degree global grid (4320 x 8640: 299 MB)."""
    assert _ask(exe, [(2400, 3600, 8), (1080, 1440, 8), (97, 236, 8), (192, 432, 8), (4320, 8640, 8)]) == [1, 1, 1, 1, 1]


def test_the_launcher_asks_the_predicate():
    """launch_ringc_zip_sf takes no table for a plane the offsets cannot span."""
    with open(os.path.join(CSRC, "gcmf_ringc_impl.hpp")) as f:
        text = f.read()
    assert "table_rows_ok(pl->g.rows, pl->g.nx, (long long)sizeof(T), pl->g.south_wrap && pl->g.north_wrap)" in text
