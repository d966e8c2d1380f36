"""Every kernel in csrc/ is reached by a case of the dispatch-edge sweep (tests/test_gpu_dispatch_edges.py), or is listed here with the
reason it is not and the test that covers it.  A new kernel without an edge case fails this (CPU) test."""
import glob
import os
import re

from test_gpu_dispatch_edges import CASES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcm_filters_amd", "csrc")

# kernel -> why the sweep does not name it, and where it is covered
ALLOWLIST = {
    # plan-time precompute: run by every plan creation; covered by tests/test_gpu_parity.py::test_kernel_vs_reference_zarr
    "k_pre_mask": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    "k_pre_isolated": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr; cells cut off from the sea (lakes, a checkerboard, "
                      "kappa zeros, land on the tripole seam): tests/test_gpu_coastlines.py",
    "k_count_land": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    "k_pre_irregular": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    "k_pre_pop": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    "k_pre_mom5": "plan precompute; tests/test_gpu_parity.py::test_bit_exact_recurrence",
    "k_pre_cgrid": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    "k_pre_bgrid1": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    "k_pre_bgrid2": "plan precompute; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    # helpers that run beside the recurrence kernels; Plan.last_kernel() names only the recurrence kernel
    "k_prepare": "area-weighted prepare step, not named by last_kernel; tests/test_gpu_parity.py::test_kernel_vs_reference_zarr",
    "k_fold_band": "tripole seam band beside / after the blocked launch, not named by last_kernel; "
                   "tests/test_gpu_zip.py::test_the_seam_band_after_or_beside_the_launch; with land on the seam: "
                   "tests/test_gpu_coastlines.py (tripolar-band-*)",
    "k_land_fix": "land fix-up after the backward evaluation, not named by last_kernel; tests/test_gpu_parity.py::test_land_kept_out_of_the_state; "
                  "words of mixed land and water, finite and NaN values on land: tests/test_gpu_coastlines.py",
    "k_zero_land": "zeroes land in the state, not named by last_kernel; tests/test_gpu_parity.py::test_land_kept_out_of_the_state; "
                   "words of mixed land and water: tests/test_gpu_coastlines.py",
    # multi-rank halo exchange
    "k_pack_rows": "halo exchange packing; tests/test_gpu_exchange.py::test_raw_exchange_fills_ghost_rows_direct_and_packed",
    "k_p2p_post": "peer-to-peer halo exchange; tests/test_gpu_distributed.py::test_slabs_on_one_gpu_match_single_domain",
    "k_p2p_collect": "peer-to-peer halo exchange; tests/test_gpu_distributed.py::test_slabs_on_one_gpu_match_single_domain",
    "k_p2p_guard": "peer-to-peer failure guard; tests/test_gpu_distributed.py::test_p2p_rank_that_skips_a_post_fails_every_rank_loudly",
}


def csrc_kernels():
    """Names of every __global__ kernel and every kernel a note_kernel call records."""
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        with open(path) as f:
            src = f.read()
        names.update(re.findall(r'note_kernel\(pl, std::string\("gcmf::(k_[a-z_0-9]+)<', src))
        names.update(re.findall(r"__global__[^\n]*?\bvoid\s+(k_[a-z_0-9]+)\s*\(", src))
    return names


def reached(cases=CASES):
    return {k for c in cases for k in c.kernels()}


def test_sources_parse():
    names = csrc_kernels()
    for k in ("k_ring", "k_ringc", "k_ringcs", "k_ringcz", "k_ringcp", "k_cgrid_ring", "k_scalar_step", "k_cgrid_step", "k_pre_mask"):
        assert k in names, k
    assert len(names) >= 35, sorted(names)


def test_every_kernel_is_reached_or_allowlisted():
    names = csrc_kernels()
    missing = sorted(names - reached() - set(ALLOWLIST))
    assert not missing, f"kernels with no case in tests/test_gpu_dispatch_edges.py and no ALLOWLIST entry: {missing}"


def test_allowlist_is_not_stale():
    names, hit = csrc_kernels(), reached()
    assert not sorted(set(ALLOWLIST) - names), "ALLOWLIST names kernels that no longer exist"
    assert not sorted(set(ALLOWLIST) & hit), "ALLOWLIST names kernels the sweep reaches"
    assert not sorted(hit - names), f"cases claim kernels csrc/ does not have: {sorted(hit - names)}"

