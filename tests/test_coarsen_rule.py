"""The block-mean rule of gcmf_apply_coarsen (gcm_filters_amd/csrc/gcmf_coarsen.hpp), compiled into a plain C++ program
(tests/coarsen/) and compared with numpy: which cells count, the NaN and wsum == 0 patterns exactly, the values to the rounding of
fy * fx products and additions.  No GPU, nothing loaded into Python; the program is built a second time with the address and
undefined-behaviour sanitizers and run alone.

Bounds (per coarse cell, u = 2^-53): products are rounded once and summed recursively on both sides, then divided once, so
|got - want| <= 4 fy fx u sum(w |F|) / sum(w) whatever the order of the sums, and wsum agrees to 2 fy fx u relative.  Where a counted F
is +-inf only the non-finite pattern is compared."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from numpy.random import PCG64, Generator

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "coarsen", "coarsen_main.cpp")
INC = os.path.join(REPO, "gcm_filters_amd", "csrc")
U = 2.0 ** -53
GEOMETRIES = (((7, 9), (7, 3)), ((7, 9), (1, 9)), ((12, 16), (3, 4)), ((12, 16), (2, 16)), ((12, 16), (12, 16)), ((12, 16), (1, 1)))


def cases():
    out = []
    for shape, (fy, fx) in GEOMETRIES:
        ny, nx = shape
        for name in ("plain", "odd-weights", "non-finite", "all-skipped-block", "no-weights"):
            rng = Generator(PCG64(31 * len(out) + 5))
            f = rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)
            w = 0.1 + rng.random(shape) * 10.0 ** rng.integers(-2, 3, shape)
            if name in ("odd-weights", "non-finite", "all-skipped-block"):
                kinds = rng.integers(0, 8, shape)
                w[kinds == 0] = 0.0
                w[kinds == 1] = -0.0
                w[kinds == 2] = -rng.random(shape)[kinds == 2] - 0.5
                w[kinds == 3] = np.nan
                w[0, 0], w[0, 1], w[1, 0], w[1, 1] = 0.0, -0.0, -2.0, np.nan      # (one of each whatever the draw)
            if name == "non-finite":
                f[rng.random(shape) < 0.2] = np.nan
                f[rng.random(shape) < 0.1] = np.inf         # ... in counted and in skipped cells alike
                f[rng.random(shape) < 0.1] = -np.inf
                f[ny - 1, nx - 1], w[ny - 1, nx - 1] = np.inf, 1.5     # counted
                f[ny - 1, 0], w[ny - 1, 0] = -np.inf, 0.0              # skipped: must not turn its block into NaN
                f[0, nx - 1], w[0, nx - 1] = np.inf, np.nan            # skipped
            if name == "all-skipped-block" and (fy, fx) != shape:
                f[:fy, :fx] = np.where(rng.random((fy, fx)) < 0.5, np.nan, f[:fy, :fx])
                w[:fy, :fx] = np.where(np.isnan(f[:fy, :fx]), w[:fy, :fx], 0.0)
            if name == "all-skipped-block" and (fy, fx) == shape:
                f[:] = np.nan
            out.append((shape, (fy, fx), name, f, None if name == "no-weights" else w))
    return out


CASES = cases()


def want_of(f, w, fy, fx):
    """(coarse, wsum, sum(w |F|) / sum(w), the blocks in which a counted F is not finite) by the rule, in numpy."""
    ny, nx = f.shape
    w = np.ones(f.shape) if w is None else w
    with np.errstate(invalid="ignore"):
        counts = (w > 0) & ~np.isnan(f)
    blocks = lambda a: a.reshape(ny // fy, fy, nx // fx, fx)
    with np.errstate(all="ignore"):
        wc = np.where(counts, w, 0.0)
        fc = np.where(counts, f, 0.0)
        wsum = blocks(wc).sum(axis=(1, 3))
        num = blocks(wc * fc).sum(axis=(1, 3))
        mag = blocks(wc * np.abs(fc)).sum(axis=(1, 3))
        coarse = np.where(wsum > 0, num / np.where(wsum > 0, wsum, 1.0), np.nan)
        scale = np.where(wsum > 0, mag / np.where(wsum > 0, wsum, 1.0), 0.0)
    wild = blocks(counts & ~np.isfinite(f)).any(axis=(1, 3))
    return coarse, wsum, scale, wild


def build(tmp, flags, name):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/coarsen/coarsen_main.cpp")
    exe = os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe], check=True)
    return exe


def run(exe, tmp):
    src, dst = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(CASES)))
        for (ny, nx), (fy, fx), _, f, w in CASES:
            fh.write(struct.pack("<iiiii", ny, nx, fy, fx, 0 if w is None else 1))
            fh.write(np.ascontiguousarray(f, dtype="<f8").tobytes())
            if w is not None:
                fh.write(np.ascontiguousarray(w, dtype="<f8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), r.stdout
    got, blob, off = [], open(dst, "rb").read(), 0
    for (ny, nx), (fy, fx), *_ in CASES:
        cy, cx = ny // fy, nx // fx
        coarse = np.frombuffer(blob, "<f8", cy * cx, off).reshape(cy, cx)
        wsum = np.frombuffer(blob, "<f8", cy * cx, off + 8 * cy * cx).reshape(cy, cx)
        off += 16 * cy * cx
        got.append((coarse, wsum))
    assert off == len(blob)
    return got


def compare(got):
    seen = {"nan-block": 0, "wild": 0, "skipped-inf": 0}
    for (shape, (fy, fx), name, f, w), (coarse, wsum) in zip(CASES, got):
        what = (shape, (fy, fx), name)
        want, want_w, scale, wild = want_of(f, w, fy, fx)
        assert np.array_equal(wsum == 0, want_w == 0), what
        assert np.array_equal(np.isnan(coarse) & ~wild, np.isnan(want) & ~wild), what
        assert np.array_equal(np.isnan(coarse), wsum == 0) or wild.any(), what
        calm = ~wild & ~np.isnan(want)
        err = np.abs(coarse[calm] - want[calm])
        assert np.all(err <= 4 * fy * fx * U * scale[calm]), (what, float(err.max()))
        assert np.all(np.abs(wsum - want_w) <= 2 * fy * fx * U * np.abs(want_w)), what
        with np.errstate(invalid="ignore"):
            same = (np.isnan(coarse[wild]) & np.isnan(want[wild])) | (coarse[wild] == want[wild])
        assert np.all(same) and not np.isfinite(coarse[wild]).any(), what      # +inf, -inf or (inf - inf) NaN, as numpy has it
        seen["nan-block"] += int(np.isnan(want[~wild]).sum())
        seen["wild"] += int(wild.sum())
        if name == "non-finite":
            skipped = ~((np.ones(f.shape) if w is None else w) > 0) & np.isinf(f)
            seen["skipped-inf"] += int(skipped.sum())
    assert all(seen.values()), seen


def test_rule_matches_numpy(tmp_path):
    compare(run(build(str(tmp_path), [], "coarsen_main"), str(tmp_path)))


def test_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program and cases, built with -fsanitize=address,undefined (the runtimes linked into the program itself) and run on its
    own."""
    exe = build(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                                "-static-libubsan"], "coarsen_main_san")
    compare(run(exe, str(tmp_path)))
