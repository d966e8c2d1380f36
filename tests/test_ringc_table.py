"""Which launches of the backward strip kernels exist is stated once, ringc_offered() in csrc/gcmf_ringc_cut.hpp; where each launcher
instantiation is compiled is the table of csrc/gcmf_ringc_table.hpp, which the units gcmf_ringc_*.hip define from and the dispatcher
(gcmf_ringc_dispatch.hip) declares from.  Two checks, no GPU:

  * the predicate, printed by tests/ringc_cut/print_offered.cpp (g++ against the header alone), is the list written out below -- taken from
    the switch statements the units held before the table (each row names the unit that instantiates it);
  * in the objects a build leaves in csrc/: every launcher instantiation the dispatcher's object refers to is defined in exactly one unit,
    none is defined twice (explicit instantiations are weak symbols: the linker would not say), none is defined and never referred to, the
    dispatcher defines none -- and what it refers to is exactly what the predicate offers."""
import glob
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")

D5_8, D5_9 = [5, 6, 7, 8], [5, 6, 7, 8, 9]
# (form, state) -> depths as a first launch, depths as a later launch; what is not listed is not offered
OFFERED = {
    ("reg", "f64"): (D5_8, D5_8),            # gcmf_ringc_reg.hip
    ("reg", "f32"): ([5, 6, 7], D5_8),       # gcmf_ringc_reg_f32.hip: eight levels never as a first launch
    ("maskz", "f64"): (D5_8, D5_8),          # gcmf_ringc_maskz.hip
    ("maskz", "f32"): ([5, 6, 7], D5_8),     # gcmf_ringc_maskz_f32.hip
    ("flux", "f64"): (D5_9, D5_9),           # gcmf_ringc_flux.hip, nine: gcmf_ringc_flux9.hip
    ("flux", "f32"): ([5, 6, 7], D5_8),      # gcmf_ringc_flux_f32.hip
    ("slab", "f64"): (D5_8, D5_8),           # gcmf_ringc_flux_slab.hip (5, 6), gcmf_ringc_flux_slab_b.hip (7, 8)
    ("slab", "f32"): ([5, 6, 7], D5_8),      # gcmf_ringc_flux_slab_f32.hip (5, 6), gcmf_ringc_flux_slab_f32b.hip (7, 8 later)
    ("zip", "f64"): (D5_9, D5_9),            # gcmf_ringc_zip.hip (9), _b (8), _c (7), _d (5, 6)
    ("levels", "f64"): (D5_9, D5_9),         # gcmf_ringc_levels.hip (9, 8), _b (7, 6, 5)
    ("bank", "f64"): (D5_9, D5_9),           # gcmf_ringc_bank.hip (9), _b (8, 5), _c (7, 6)
    ("bank_gaps", "f64"): (D5_9, D5_9),      # gcmf_ringc_bank_gaps.hip (9), _b (8, 5), _c (7, 6)
}
FORMS = ["reg", "maskz", "flux", "slab", "zip", "levels", "bank", "bank_gaps"]


def offered(form, state, S, when):
    first, later = OFFERED.get((form, state), ([], []))
    return S in (first if when == "first" else later)


@pytest.fixture(scope="module")
def predicate(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ringc_table") / "print_offered")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "ringc_cut", "print_offered.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_the_predicate_is_the_list(predicate):
    want = [f"{form} {state} {S} {when} {int(offered(form, state, S, when))}"
            for form in FORMS for state in ("f64", "f32") for S in range(4, 11) for when in ("first", "later")]
    got = [l for l in predicate if not l.startswith("any ")]
    assert len(want) == 8 * 2 * 7 * 2
    wrong = [f"list {a!r}, predicate {b!r}" for a, b in zip(want, got) if a != b]
    assert len(got) == len(want) and not wrong, "\n".join(wrong[:10])


def test_what_the_policies_ask(predicate):
    """clenshaw_depth_refused and clenshaw_cut: 5..9 levels exist; f64 state runs them all as first and later launches; f32 state 5..7 as a
    first launch, 5..8 later."""
    got = [l for l in predicate if l.startswith("any ")]
    want = [f"any {S} exists={int(5 <= S <= 9)} f64={int(5 <= S <= 9)}{int(5 <= S <= 9)} f32={int(5 <= S <= 7)}{int(5 <= S <= 8)}" for S in range(4, 11)]
    assert got == want


# ---- the objects ----------------------------------------------------------------------------------------------------------------
KIND = {"reg": 0, "maskz": 5, "flux": 2, "slab": 2, "levels": 2, "bank": 2, "bank_gaps": 2}
XE_PF_LV = {"reg": "false, false, false", "maskz": "false, false, false", "flux": "false, false, false", "slab": "true, false, false",
            "levels": "false, false, true", "bank": "false, true, true", "bank_gaps": "false, true, false"}
LAUNCHER = re.compile(r"^\s*([0-9a-f]*)\s+([A-Za-z])\s+int (gcmf::launch_ringc_(?:zip_)?sf<[^>]*>)\(")


def _symbols(obj):
    """{launcher instantiation: symbol type} of an object."""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-C", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        m = LAUNCHER.match(line)
        if m:
            assert m.group(3) not in out, (obj, m.group(3))
            out[m.group(3)] = m.group(2)
    return out


@pytest.fixture(scope="module")
def objects():
    dispatcher = os.path.join(CSRC, "gcmf_ringc_dispatch.o")
    units = sorted(p[:-4] + ".o" for p in glob.glob(os.path.join(CSRC, "gcmf_ringc_*.hip")) if not p.endswith("gcmf_ringc_dispatch.hip"))
    assert len(units) == 24     # (23 units of strip kernels and gcmf_ringc_one)
    if not all(os.path.exists(p) for p in units + [dispatcher]):
        pytest.skip("no objects in csrc/ (the library was not built in this tree)")
    return _symbols(dispatcher), {os.path.basename(p): _symbols(p) for p in units}


def test_every_reference_has_one_definition(objects):
    disp, units = objects
    wanted = {n for n, t in disp.items() if t == "U"}
    assert wanted and wanted == set(disp), "the dispatcher's object defines launcher instantiations: " + str(sorted(set(disp) - wanted)[:5])
    where = {}
    for unit, syms in units.items():
        for n, t in syms.items():
            assert t in "WwTt", (unit, n, t)      # (a unit refers to no launcher of another unit)
            where.setdefault(n, []).append(unit)
    twice = {n: u for n, u in where.items() if len(u) > 1}
    assert not twice, twice
    assert not sorted(wanted - set(where)), "referred to and defined nowhere"
    assert not sorted(set(where) - wanted), "defined and never referred to"


def test_the_dispatcher_refers_to_what_the_predicate_offers(objects):
    disp, _ = objects
    want = set()
    for (form, state), (first, later) in OFFERED.items():
        T = "double" if state == "f64" else "float"
        for when, depths in (("true", first), ("false", later)):
            for S in depths:
                want.add(f"gcmf::launch_ringc_zip_sf<{T}, {S}, {when}>" if form == "zip" else
                         f"gcmf::launch_ringc_sf<{T}, {KIND[form]}, {S}, {when}, {XE_PF_LV[form]}>")
    assert len(want) == 102
    assert set(disp) == want, (sorted(set(disp) - want)[:5], sorted(want - set(disp))[:5])


def test_the_dispatcher_holds_no_kernel(objects):
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, os.path.join(CSRC, "gcmf_ringc_dispatch.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "k_ringc" not in r.stdout
