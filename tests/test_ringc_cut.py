"""How a backward scalar launch is cut (kernel form, strip height, strips, pairs, fold strips, packed runs, grid) is decided by one host-only
function, ringc_cut() in csrc/gcmf_ringc_cut.hpp.  tests/ringc_cut/print_cut.cpp is compiled with g++ against that header alone -- no HIP,
no library, no GPU -- and must give every launch of tests/golden/ringc_cuts.txt the cut recorded there: the cuts the launchers and
policies made before the decision moved into the planner (a row on each side of every choice it makes)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")
TABLE = os.path.join(REPO, "tests", "golden", "ringc_cuts.txt")


def _rows():
    with open(TABLE) as f:
        return [line.rstrip("\n") for line in f if line.strip() and not line.startswith("#")]


def _build(tmp_path):
    exe = str(tmp_path / "print_cut")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "ringc_cut", "print_cut.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_planner_header_is_host_only():
    with open(os.path.join(CSRC, "gcmf_ringc_cut.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<algorithm>"], includes


def test_planner_reproduces_the_recorded_cuts(tmp_path):
    rows = _rows()
    assert len(rows) >= 200
    forms = {r.split(" -> ")[1].split()[0] for r in rows}
    assert forms == {"none", "k_ringc", "k_ringcs", "k_ringcz", "k_ringcz+fold", "k_ringcp"}, forms
    inputs = "".join(r.split(" -> ")[0] + "\n" for r in rows)
    r = subprocess.run([_build(tmp_path)], input=inputs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(rows)
    wrong = [f"recorded {a!r}\n planner {b!r}" for a, b in zip(rows, got) if a != b]
    assert not wrong, "\n".join(wrong[:10])
