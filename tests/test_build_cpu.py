"""The register allocator's verdict on the 256x256 GEMM kernels, recorded by the build (lib/kernel_resources.json).

hipcc 7.2 flips between two allocations of vlm_gemm_big_kernel on edits that do not change a single value (the staging
offsets written directly instead of "swizzled, then un-swizzled"): in the bad one 40 accumulator registers live in VGPRs
and are shuffled through a[52:55] inside the K loop -- 1 832 instead of 1 488 cycles per 32-deep step, -11 % on the
forward / dgrad GEMMs, with every numerics test still green.  This test is the tripwire."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RES = os.path.join(HERE, "..", "vl-merging_amd", "lib", "kernel_resources.json")


CSRC = os.path.join(HERE, "..", "vl-merging_amd", "csrc")


def _stale():
    """No record, or a kernel source / header newer than the record (an edit that was never rebuilt)."""
    if not os.path.exists(RES):
        return True
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    return max(os.path.getmtime(f) for f in srcs) > os.path.getmtime(RES)


@pytest.fixture(scope="module")
def resources():
    """lib/kernel_resources.json is a BUILD product (git-ignored): rebuilt here whenever it is missing or older than a
    source, so the tripwire can never pass on stale numbers."""
    if _stale():
        import importlib.util
        spec = importlib.util.spec_from_file_location("graft_entry", os.path.join(HERE, "..", "__graft_entry__.py"))
        ge = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ge)
        ge.build()
    assert os.path.exists(RES), "the build did not record kernel resources"
    with open(RES) as f:
        return json.load(f)


def test_big_gemm_accumulators_stay_in_agprs(resources):
    big = {k: v for k, v in resources.items() if "vlm_gemm_big_kernel" in k}
    assert len(big) == 11, sorted(big)  # six plain + the five GROUPED variants a block uses (round 5: + residual without aux)
    for name, r in big.items():
        assert r["AGPRs"] == 256, (name, r)            # the 4 x 64 accumulator registers of a 128x128 wave tile
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["Occupancy"] == 1 and r["LDS Size"] <= 160 * 1024, (name, r)
        residual = "ILb1ELb1E" in name                 # <OUT_F32, RES, AUX>: the residual variants hold 36-register input sets
        assert r["VGPRs"] <= (248 if residual else 232), (name, r)


def test_gemm_kernel_variants(resources):
    small = [k for k in resources if "vlm_gemm_kernel" in k]
    assert len(small) == 10, sorted(small)  # 8 (TA, TB, OUT_F32) keys + the two split-K launches; staging follows from them


def test_wgrad_kernel_resources(resources):
    both = [(k, v) for k, v in resources.items() if "vlm_gemm_bigT_kernel" in k]
    assert len(both) == 2, sorted(k for k, _ in both)  # plain + GROUPED
    for name, r in both:
        assert r["AGPRs"] == 256 and r["Occupancy"] == 1, (name, r)
        assert r["VGPRs Spill"] <= 32, (name, r)       # the tail's epilogue setup spills a few; the K loop does not


def test_attention_kernels_keep_their_occupancy(resources):
    occ = {k: v["Occupancy"] for k, v in resources.items() if "attn_" in k and "kernel" in k}
    assert occ, "no attention kernels recorded"
    for name, o in occ.items():
        if "attn_bwd_dkvb_kernelILi4E" in name:
            continue  # the four-wave form of the fused dK/dV + bias-gradient kernel (480^2 panels): one wave per SIMD by design
        if "attn_fwd_kernel" in name or "attn_bwd_dq" in name or "attn_bwd_dkv" in name or "attn_bwd_dbias" in name:
            assert o >= 2, (name, o)


def test_hand_placed_forward_fits_two_waves_per_simd(resources):
    """attn_fwd2_kernel's stream names its registers (v32..v191, a0..a63): 192 + 64 = the 256 a wave may have at two waves
    per SIMD.  One register more and the second workgroup of a CU -- the one that covers a workgroup's prologue -- is gone."""
    r = [v for k, v in resources.items() if "attn_fwd2_kernel" in k]
    assert len(r) == 1
    r = r[0]
    assert r["Occupancy"] == 2 and r["VGPRs"] <= 192 and r["AGPRs"] == 64, r
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0 and 2 * r["LDS Size"] <= 160 * 1024, r


def test_generated_stream_is_current():
    """csrc/attention_fwd2_body.inc is what csrc/gen/attn_fwd2_gen.py writes."""
    import subprocess
    import sys
    gen = os.path.join(CSRC, "gen", "attn_fwd2_gen.py")
    assert subprocess.call([sys.executable, gen, "--check"]) == 0, "run python vl-merging_amd/csrc/gen/attn_fwd2_gen.py"


def test_hand_placed_dq_fits_two_waves_per_simd(resources):
    """attn_bwd_dq2_kernel: v32..v201 + 32 accumulator registers, two workgroups of 34 KiB per CU."""
    r = [v for k, v in resources.items() if "attn_bwd_dq2_kernel" in k]
    assert len(r) == 1
    r = r[0]
    assert r["Occupancy"] == 2 and r["VGPRs"] + r["AGPRs"] <= 256 and r["AGPRs"] == 32, r
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0 and 2 * r["LDS Size"] <= 160 * 1024, r


def test_generated_dq_stream_is_current():
    import subprocess
    import sys
    gen = os.path.join(CSRC, "gen", "attn_dq2_gen.py")
    assert subprocess.call([sys.executable, gen, "--check"]) == 0, "run python vl-merging_amd/csrc/gen/attn_dq2_gen.py"


def _row_kernels(resources, prefix):
    """Itanium names: ln_bwd_kernel<MAXU, DY_BF16, SCALE> = _Z13ln_bwd_kernelILi<MAXU>ELb<0|1>ELi<SCALE>EE..."""
    return {k: v for k, v in resources.items() if k.startswith(prefix)}


def test_row_kernels_keep_the_occupancy_their_grid_counts_on(resources):
    """vlm_layernorm_bwd launches one round of resident workgroups: ln_bwd_per_cu (rowops.hip) per CU, which is also the
    kernel's __launch_bounds__.  The allocator may meet that bound by spilling; these are the verdicts the grid and the
    measured times rest on (bounds: the values the separate tails compiled to)."""
    ln = _row_kernels(resources, "_Z13ln_bwd_kernelIL")
    assert len(ln) == 18, sorted(ln)  # MAXU 1 / 3 / 4 x dy f32 / bf16 x plain / fused / fused with a folded LayerScale
    for name, r in ln.items():
        maxu, scale = int(name.split("ILi")[1][0]), int(name.split("ELi")[1][0])
        if maxu == 3 and scale == 0:
            assert r["Occupancy"] == 4 and r["VGPRs"] <= 128 and r["ScratchSize"] <= 20, (name, r)
        elif maxu == 3:
            assert r["Occupancy"] >= 3 and r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
            assert 3 * r["LDS Size"] <= 160 * 1024, (name, r)
        elif maxu == 4:
            assert r["Occupancy"] == 2 and r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    sc = _row_kernels(resources, "_Z16scale_bwd_kernelILi3E")
    assert len(sc) == 2, sorted(sc)
    for name, r in sc.items():
        assert r["Occupancy"] >= 6 and r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)


def test_f64_block_entry_points_and_switch_are_retired(resources):
    """The library no longer exports the per-block steps of the float64 factorisation (the drivers own them), f64ops.hip
    reads no environment variable (the columns per right-looking update are the constant 256), and each float64 operation
    has its table kernel only.  `resources` brings the build up to date first."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(HERE, "..", "vl-merging_amd", "lib", "libvlm_hip.so"))
    for gone in ("vlm_potrf_block_f64", "vlm_trsm_block_f64"):
        assert not hasattr(lib, gone), gone
    assert hasattr(lib, "vlm_cholesky_f64_batched")  # (the probe does find what is there)
    with open(os.path.join(CSRC, "f64ops.hip")) as f:
        text = f.read()
    assert "getenv" not in text and "environ" not in text and "stdlib.h" not in text
    assert not [k for k in resources if "gemm_f64_kernel" in k or "potrf_block_kernel" in k or "trsm_block_kernel" in k]
    assert len([k for k in resources if "gemm_f64_batched_kernel" in k]) == 2  # A as float64 / float32
    assert len([k for k in resources if "potrf_block_batched_kernel" in k or "trsm_block_batched_kernel" in k]) == 2


def test_one_fold_kernel(resources):
    assert [k for k in resources if "colreduce_batch_kernel" in k]
    assert not [k for k in resources if "colreduce_kernel" in k]


def test_merge_family_keeps_the_occupancy_its_grids_count_on(resources):
    """The chunk walkers of merge.hip, ties.hip, dare.hip, pairstats.hip, band.hip and della.hip are one template
    (csrc/chunk_walk.h) around each method's rule, the radix select of ties.hip (one rank) and band.hip (two ranks) is one
    pair of kernel templates (csrc/ties_select.h), and the reducers of stock.hip, sphere.hip and sce.hip are one run
    (csrc/chunk_records.h); the grids are sized from resident workgroups (one wave per SIMD each).
    TIES_HIST_BLOCKS_PER_CU = 4 counts on exactly four histogram workgroups per CU (registers allow four, and four times 32 KiB of
    LDS fit), with one rank and with two; TIES_APPLY_BLOCKS_PER_CU = DARE_APPLY_BLOCKS_PER_CU = 12 is four rounds of three, for
    vlm_band_apply_kernel too; vlm_merge_run's 96 per CU strides the table with at least five resident; DELLA_BLOCKS_PER_CU = 12
    counts on two (66 KiB of LDS each).  None of them may spill: the kernels are HBM-bound streams."""
    def only(name):
        r = [v for k, v in resources.items() if name in k]
        assert len(r) == 1, (name, sorted(k for k in resources if name in k))
        return r[0]

    hists = []
    for sel in ("ties_sel", "band_sel"):  # one rank, two ranks
        hist = {k: v for k, v in resources.items() if "vlm_select_hist_kernel" in k and sel in k}
        assert len(hist) == 3, (sel, sorted(hist))  # PASS 0 / 1 / 2
        for name, r in hist.items():
            assert r["Occupancy"] == 4 and r["LDS Size"] == 32768, (name, r)
        hists += hist.values()
    apply_ties, apply_dare, plain = only("vlm_ties_apply_kernel"), only("vlm_dare_apply_kernel"), only("vlm_merge_kernel")
    apply_band, apply_della = only("vlm_band_apply_kernel"), only("vlm_della_apply_kernel")
    assert apply_ties["Occupancy"] >= 3 and apply_dare["Occupancy"] >= 3 and apply_band["Occupancy"] >= 3, (apply_ties, apply_dare,
                                                                                                          apply_band)
    assert plain["Occupancy"] >= 5, plain
    assert apply_della["Occupancy"] == 2, apply_della
    for r in hists + [apply_ties, apply_dare, apply_band, apply_della, plain]:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
