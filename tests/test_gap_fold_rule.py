"""The fold rule of GCMF_FACES_FROM_NAN (gcm_filters_amd/csrc/gcmf_gap_fold.hpp), compiled into a plain C++ program (tests/gap_fold/)
and compared BIT FOR BIT -- signs of zero included -- with the plan-time formulas (the reference's masks, kappas and metric ratios in
east- / north-face form, as k_pre_irregular and k_pre_mom5 fold them) applied to wet_mask * [field is not NaN], and with
k_pre_isolated's land-byte rule on those planes.  No GPU, nothing loaded into Python; the program is built a second time with the
address and undefined-behaviour sanitizers and run alone."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from numpy.random import PCG64, Generator

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "gap_fold", "gap_fold_main.cpp")
INC = os.path.join(REPO, "gcm_filters_amd", "csrc")
KINDS = ("IRREGULAR_WITH_LAND", "MOM5U", "MOM5T")
SHAPES = ((7, 9), (12, 16))

E = lambda a: np.roll(a, -1, axis=-1)     # the value at (j, i + 1)
W = lambda a: np.roll(a, 1, axis=-1)
N = lambda a: np.roll(a, -1, axis=-2)     # the value at (j + 1, i)
S = lambda a: np.roll(a, 1, axis=-2)


def coefficients(kind, m, g):
    """cE, cN of a plan with wet mask m (periodic in x and y)."""
    with np.errstate(all="ignore"):
        if kind == "IRREGULAR_WITH_LAND":
            # west / south face of (j, i): ratio * (m * m_west * kappa_w); the east face of (j, i) is the west face of (j, i + 1)
            cE = E(g["dyw"] / g["dxw"] * (m * W(m) * g["kappa_w"]))
            cN = N(g["dxs"] / g["dys"] * (m * S(m) * g["kappa_s"]))
            return cE, cN
        mask_a, mask_b = m * E(m), m * N(m)      # (the reference masks the axis -2 difference with m * E(m): reproduced as written)
        if kind == "MOM5U":
            cN = 2.0 / (N(g["dxt"]) + N(E(g["dxt"]))) * mask_a * (0.5 * (g["dyu"] + N(g["dyu"])))
            cE = 2.0 / (E(g["dyt"]) + N(E(g["dyt"]))) * mask_b * (0.5 * (g["dxu"] + E(g["dxu"])))
        else:
            cN = 2.0 / (g["dxu"] + W(g["dxu"])) * mask_a * (0.5 * (g["dyt"] + N(g["dyt"])))
            cE = 2.0 / (g["dyu"] + S(g["dyu"])) * mask_b * (0.5 * (g["dxt"] + E(g["dxt"])))
        return cE, cN


def land_bytes(cE, cN):
    return ((cE != 0) | (W(cE) != 0) | (cN != 0) | (S(cN) != 0)).astype(np.uint8)


def grid(kind, shape, seed, negative_ratio=False, kappa_zeros=False):
    rng = Generator(PCG64(seed))
    names = ("dxw", "dyw", "dxs", "dys", "kappa_w", "kappa_s") if kind == "IRREGULAR_WITH_LAND" else ("dxt", "dyt", "dxu", "dyu")
    g = {k: 0.5 + rng.random(shape) for k in names}
    if kind == "IRREGULAR_WITH_LAND":
        g["kappa_w"], g["kappa_s"] = rng.random(shape), rng.random(shape)
        if kappa_zeros:
            g["kappa_w"][rng.random(shape) < 0.3] = 0.0
            g["kappa_s"][rng.random(shape) < 0.3] = 0.0
            g["kappa_s"][1, 2] = -0.0
    if negative_ratio:      # a metric with the other sign: closed faces become -0.0
        for k in (("dxw", "dys") if kind == "IRREGULAR_WITH_LAND" else ("dyu", "dxt")):
            g[k] = np.where(rng.random(shape) < 0.4, -g[k], g[k])
    m = (rng.random(shape) < 0.8).astype(np.float64)
    m[shape[0] // 2, 1:4] = 0.0
    return m, g


def cases():
    out = []
    for kind in KINDS:
        for shape in SHAPES:
            ny, nx = shape
            for name in ("edges", "next-to-land", "kappa-zeros", "negative-ratio", "enclosed", "no-gaps", "all-gaps", "random"):
                seed = 17 * len(out) + 3
                m, g = grid(kind, shape, seed, negative_ratio=name in ("negative-ratio", "random"), kappa_zeros=name in ("kappa-zeros", "random"))
                rng = Generator(PCG64(seed + 1))
                f = rng.standard_normal(shape)
                if name == "edges":             # gaps on all four edges and in the corners: the wrap applies
                    m[:] = 1.0
                    f[0, [0, 3, nx - 1]] = np.nan
                    f[ny - 1, [0, 4, nx - 1]] = np.nan
                    f[2:5, 0] = np.nan
                    f[3, nx - 1] = np.nan
                elif name == "next-to-land":
                    land = np.argwhere(m == 0)
                    for j, i in land[:6]:
                        f[j, (i + 1) % nx] = np.nan
                        f[(j - 1) % ny, i] = np.nan
                    f[land[0][0], land[0][1]] = np.nan      # a gap ON land too
                elif name == "enclosed":        # a wet cell whose four neighbours are gaps, in the interior and in a corner
                    m[:] = 1.0
                    for j, i in ((3, 4), (0, 0)):
                        for dj, di in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                            f[(j + dj) % ny, (i + di) % nx] = np.nan
                elif name == "all-gaps":
                    f[:] = np.nan
                elif name != "no-gaps":
                    f[rng.random(shape) < 0.25] = np.nan
                if name == "random":
                    f[1, 1], f[2, 3] = np.inf, -np.inf      # data, not gaps
                out.append((kind, shape, name, m, g, f))
    return out


CASES = cases()


def build(tmp, flags, name):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/gap_fold/gap_fold_main.cpp")
    exe = os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe], check=True)
    return exe


def run(exe, tmp):
    src, dst = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(CASES)))
        for kind, (ny, nx), _, m, g, f in CASES:
            cE, cN = coefficients(kind, m, g)
            fh.write(struct.pack("<iii", ny, nx, 0 if kind == "IRREGULAR_WITH_LAND" else 1))
            for a in (f, cE, cN):
                fh.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), r.stdout
    got, blob, off = [], open(dst, "rb").read(), 0
    for _, (ny, nx), *_ in CASES:
        n = ny * nx
        cEb = np.frombuffer(blob, "<f8", n, off).reshape(ny, nx)
        cNb = np.frombuffer(blob, "<f8", n, off + 8 * n).reshape(ny, nx)
        land = np.frombuffer(blob, np.uint8, n, off + 16 * n).reshape(ny, nx)
        off += 17 * n
        got.append((cEb, cNb, land))
    assert off == len(blob)
    return got


def compare(got):
    seen_negative_zero = seen_closed_in = False
    for (kind, shape, name, m, g, f), (cEb, cNb, land) in zip(CASES, got):
        n = (~np.isnan(f)).astype(np.float64)
        wantE, wantN = coefficients(kind, m * n, g)
        what = (kind, shape, name)
        assert np.array_equal(cEb.view(np.uint64), wantE.view(np.uint64)), what       # bit for bit: the sign of a closed face too
        assert np.array_equal(cNb.view(np.uint64), wantN.view(np.uint64)), what
        assert np.array_equal(land, land_bytes(wantE, wantN)), what
        seen_negative_zero |= bool(np.any((wantE == 0) & np.signbit(wantE)) or np.any((wantN == 0) & np.signbit(wantN)))
        if name == "enclosed":
            assert land[3, 4] == 0 and land[0, 0] == 0 and m[3, 4] == 1 and not np.isnan(f[3, 4])
            seen_closed_in = True
        if name == "all-gaps":
            assert not land.any() and not wantE.any() and not wantN.any()
        if name == "no-gaps":
            plainE, plainN = coefficients(kind, m, g)
            assert np.array_equal(cEb.view(np.uint64), plainE.view(np.uint64)) and np.array_equal(cNb.view(np.uint64), plainN.view(np.uint64))
    assert seen_negative_zero and seen_closed_in


def test_rule_matches_the_plan_formulas_bit_for_bit(tmp_path):
    compare(run(build(str(tmp_path), [], "gap_fold_main"), str(tmp_path)))


def test_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program and cases, built with -fsanitize=address,undefined (the runtimes linked into the program itself) and run on its
    own."""
    exe = build(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"], "gap_fold_main_san")
    compare(run(exe, str(tmp_path)))
