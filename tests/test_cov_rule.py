"""The two cell rules of gcmf_apply_cov (gcm_filters_amd/csrc/gcmf_cov.hpp), compiled into a plain C++ program (tests/cov/) with
-ffp-contract=off and compared with numpy BIT FOR BIT: the pre rule (common gaps, one product) and the post rule (a - b * c in two
roundings).  No GPU, nothing loaded into Python; the program is built a second time with the address and undefined-behaviour
sanitizers and run alone.

numpy's float64 product and difference are each rounded once, which is the rule; NaNs are compared as NaNs (their payload is not part
of the contract, except that without common gaps f and g pass through with every bit)."""
import os
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest
from numpy.random import PCG64, Generator

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cov", "cov_main.cpp")
INC = os.path.join(REPO, "gcm_filters_amd", "csrc")
TINY = np.finfo(np.float64).tiny


def plane(rng, n, kind):
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    if kind == "offset":                      # large offsets: the cancellation tau is made of
        x = x + rng.choice([50.0, -30.0, 1.0e6, -1.0e9], n)
    if kind == "special":
        k = rng.integers(0, 12, n)
        x[k == 0] = np.nan
        x[k == 1] = np.inf
        x[k == 2] = -np.inf
        x[k == 3] = 0.0
        x[k == 4] = -0.0
        x[k == 5] = TINY * rng.random(n)[k == 5]              # denormals
        x[k == 6] = -TINY / 8
        x[k == 7] = np.finfo(np.float64).max * rng.random(n)[k == 7]      # products that overflow
        x[:6] = [np.nan, np.inf, -np.inf, 0.0, -0.0, TINY / 4][:n]      # (one of each whatever the draw)
    return x


def cases():
    out = []
    for n in (1, 2, 7, 64, 501):
        for kind in ("plain", "offset", "special"):
            for common in (0, 1):
                for var in (0, 1):
                    rng = Generator(PCG64(17 * len(out) + 3))
                    f, g = plane(rng, n, kind), plane(rng, n, kind)
                    if kind == "special" and n >= 7:
                        g = np.roll(g, 3)      # NaN against finite, inf against 0, NaN against NaN ...
                        f[6], g[6] = np.nan, np.nan
                    a, b, c = plane(rng, n, kind), plane(rng, n, kind), plane(rng, n, kind)
                    if kind == "offset":       # a close to b * c, as F(fg) is to F(f) F(g)
                        a = (b * b if var else b * c) + rng.standard_normal(n)
                    out.append((n, common, var, f, g, a, b, c))
    return out


CASES = cases()


def build(tmp, flags, name):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/cov/cov_main.cpp")
    exe = os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", INC, SRC, "-o", exe], check=True)
    return exe


def run(exe, tmp):
    src, dst = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(CASES)))
        for n, common, var, f, g, a, b, c in CASES:
            fh.write(struct.pack("<iii", n, common, var))
            for x in ((f, a, b) if var else (f, g, a, b, c)):
                fh.write(np.ascontiguousarray(x, dtype="<f8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), r.stdout
    got, blob, off = [], open(dst, "rb").read(), 0
    for n, common, var, *_ in CASES:
        planes = []
        for _ in range(3 if var else 4):
            planes.append(np.frombuffer(blob, "<f8", n, off))
            off += 8 * n
        got.append(planes)
    assert off == len(blob)
    return got


def same_bits(x, y, nan_payload=False):
    """Every bit equal; NaNs equal as NaNs unless their payload counts, too."""
    bx, by = np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)
    if nan_payload:
        return np.array_equal(bx, by)
    nx, ny = np.isnan(x), np.isnan(y)
    return np.array_equal(nx, ny) and np.array_equal(bx[~nx], by[~ny])


def compare(got):
    seen = {"united": 0, "nan-out": 0, "signed-zero": 0, "denormal": 0, "not-fused": 0}
    for (n, common, var, f, g, a, b, c), planes in zip(CASES, got):
        what = (n, common, var)
        g, c = (f, b) if var else (g, c)
        fo, go, fg, out = (planes[0], planes[0], planes[1], planes[2]) if var else planes
        with np.errstate(all="ignore"):
            ok = ~np.isnan(f) & ~np.isnan(g)
            wf, wg = (np.where(ok, f, np.nan), np.where(ok, g, np.nan)) if common else (f, g)
            wfg = wf * wg
            want = a - b * c
        assert same_bits(fo, wf, nan_payload=not common), what
        assert same_bits(go, wg, nan_payload=not common), what
        assert same_bits(fg, wfg), what
        assert same_bits(out, want), what
        assert np.array_equal(np.isnan(out), np.isnan(a) | np.isnan(b) | np.isnan(c) | np.isnan(want)), what
        seen["united"] += int(common and (np.isnan(fo) & ~np.isnan(f)).sum())
        seen["nan-out"] += int(np.isnan(out).sum())
        seen["signed-zero"] += int((np.signbit(fg) & (fg == 0)).sum())
        seen["denormal"] += int(((np.abs(fg) < TINY) & (fg != 0)).sum())
        for q in range(min(n, 16)):      # the fused result, rounded once from the exact one: the cases tell the two apart
            if np.isfinite([a[q], b[q], c[q]]).all() and np.isfinite(want[q]):
                fused = float(Fraction(float(a[q])) - Fraction(float(b[q])) * Fraction(float(c[q])))
                seen["not-fused"] += int(fused != out[q])
    assert all(seen.values()), seen


def test_rules_match_numpy_bit_for_bit(tmp_path):
    compare(run(build(str(tmp_path), [], "cov_main"), str(tmp_path)))


def test_rules_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program and cases, built with -fsanitize=address,undefined (the runtimes linked into the program itself) and run on its
    own."""
    exe = build(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                                "-static-libubsan"], "cov_main_san")
    compare(run(exe, str(tmp_path)))
