"""The spherical merge (SLERP / Karcher mean), host side (no GPU): the restatement of the rule (sphere_restatement.py) against the
closed form and against the properties a spherical mean has, the ABI additions, the host surface, merge_ckpt.py's command line,
the build's record of the four kernels, and the host checks of the upload under a sanitizer.  The reference has no such merge:
nothing here is pinned to it."""
import ctypes
import importlib
import json
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sphere_restatement as R
from pairstats_restatement import bits
from test_ties_cpu import header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F, D = np.float32, np.float64


def randn(n, S, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(F) for _ in range(S)]


def combo(xs, coef):
    return sum(c * x.astype(D) for c, x in zip(coef, xs))


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("t", [0.0, 0.3, 0.5, 1.0])
@pytest.mark.parametrize("n", [2, 64, 1000])
def test_two_sources_are_closed_form_slerp_with_the_norm_interpolated(t, n):
    x0, x1 = randn(n, 2, seed=n)
    x1 = (F(2.5) * x1).astype(F)  # different norms: the norm is interpolated, not the vectors
    out, res = R.sphere(None, [x0, x1], [1 - t, t])
    assert res["status"] == R.OK
    got = combo([x0, x1], res["coef64"])
    want = R.slerp(x0.astype(D), x1.astype(D), t)
    scale = np.max(np.abs(want))
    assert np.max(np.abs(got - want)) <= 1e-12 * scale, (t, n)
    # the fp32 output is that combination up to the rounding of the coefficients and of step 4's three operations per source
    assert np.max(np.abs(out.astype(D) - want)) <= 8 * 2.0 ** -24 * max(np.max(np.abs(x0)), np.max(np.abs(x1)))
    if t in (0.0, 1.0):
        assert [round(c, 12) for c in res["coef64"]] == [1.0 - t, t]


def test_equal_sources_give_that_source_back():
    (x,) = randn(300, 1, seed=1)
    for S, w in ((2, [0.3, 0.7]), (3, [0.2, 0.5, 0.3]), (4, [1, 1, 1, 1])):
        out, res = R.sphere(None, [x.copy() for _ in range(S)], w)
        assert res["status"] == R.OK and abs(sum(res["coef64"]) - 1.0) <= 1e-15 and res["resid"] <= 1e-15
        assert np.max(np.abs(out.astype(D) - x.astype(D))) <= 4 * 2.0 ** -24 * np.max(np.abs(x))
    c = randn(300, 1, seed=2)[0]
    out, res = R.sphere(c, [x, x.copy()], [0.5, 0.5], lam=1.0)
    assert np.max(np.abs(out.astype(D) - x.astype(D))) <= 8 * 2.0 ** -24 * max(np.max(np.abs(x)), np.max(np.abs(c)))


def test_one_source_has_coefficient_one_exactly():
    for n in (1, 3, 4097):
        (x,) = randn(n, 1, seed=n)
        out, res = R.sphere(None, [x], [0.37])
        assert res["coef64"] == [1.0] and res["coef32"] == [1.0] and res["status"] == R.OK and res["resid"] == 0.0
        assert res["rho"] == math.sqrt(res["sq"][0]) and out.tobytes() == (np.zeros(n, F) + F(1) * x).tobytes()
    c = randn(5, 1, seed=9)[0]
    (x,) = randn(5, 1, seed=10)
    out, res = R.sphere(c, [x], [2.0], lam=0.5)
    assert res["coef32"] == [1.0] and out.tobytes() == (c + F(0.5) * (np.zeros(5, F) + (x - c))).astype(F).tobytes()


@pytest.mark.parametrize("S,n", [(2, 64), (3, 64), (4, 200), (3, 4096), (4, 1000)])
def test_the_norm_of_the_result_is_rho(S, n):
    xs = randn(n, S, seed=S * n)
    xs = [(F(1 + m) * x).astype(F) for m, x in enumerate(xs)]
    w = [1.0 + 0.5 * m for m in range(S)]
    _, res = R.sphere(None, xs, w)
    assert res["status"] == R.OK and res["resid"] < 1e-12
    got = combo(xs, res["coef64"])
    assert abs(math.sqrt(float(got @ got)) / res["rho"] - 1.0) <= 1e-12
    ws = sum(w)
    assert abs(res["rho"] - sum(wm / ws * math.sqrt(float(x.astype(D) @ x.astype(D))) for wm, x in zip(w, xs))) <= 1e-12 * res["rho"]
    # per row: every row's own rho
    L = n // 4 if n % 4 == 0 else n
    _, rows = R.sphere(None, xs, w, row_len=L)
    for r, row in enumerate(rows):
        got = combo([x[r * L:(r + 1) * L] for x in xs], row["coef64"])
        assert abs(math.sqrt(float(got @ got)) / row["rho"] - 1.0) <= 1e-12


def test_permuting_sources_and_weights_permutes_the_coefficients():
    xs = randn(512, 4, seed=5)
    g = randn(512, 1, seed=6)[0]
    xs = [(x + F(0.8) * g).astype(F) for x in xs]  # a shared component: well posed
    w = [0.1, 0.2, 0.3, 0.4]
    _, res = R.sphere(None, xs, w)
    big = max(abs(c) for c in res["coef64"])
    for perm in ([1, 0, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):
        _, other = R.sphere(None, [xs[p] for p in perm], [w[p] for p in perm])
        assert other["status"] == R.OK
        assert max(abs(other["coef64"][k] - res["coef64"][p]) for k, p in enumerate(perm)) <= 1e-12 * big, perm


def test_zero_and_linear_are_reached():
    z = np.zeros(8, F)
    x = np.arange(1, 9, dtype=F)
    out, res = R.sphere(None, [z, z.copy()], [0.5, 0.5])
    assert (res["status"], res["coef64"], res["rho"], res["resid"]) == (R.ZERO, [0.0, 0.0], 0.0, 0.0) and not out.any()
    out, res = R.sphere(None, [x, z], [0.0, 1.0])  # the one non-zero source has no weight
    assert res["status"] == R.ZERO
    out, res = R.sphere(None, [x, -x], [0.5, 0.5])  # an exactly opposite pair, equal weights: plain interpolation
    assert (res["status"], res["coef64"], res["coef32"]) == (R.LINEAR, [0.5, 0.5], [0.5, 0.5]) and not out.any()
    out, res = R.sphere(None, [x, -x], [0.7, 0.3])  # unequal weights: the heavier side, at the mean norm
    assert res["status"] == R.OK and abs(res["coef64"][0] - res["coef64"][1] - 1.0) <= 1e-12
    out, res = R.sphere(None, [x, z, (F(2) * x).astype(F)], [0.25, 0.5, 0.25])  # a zero source drops out with its weight
    assert res["status"] == R.OK and res["coef64"][1] == 0.0 and abs(res["coef64"][0] + 2 * res["coef64"][2] - 1.5) <= 1e-12
    c = np.ones(8, F)
    _, rows = R.sphere(c, [np.concatenate([c[:4], c[:4] + x[:4]]), np.concatenate([c[:4], c[:4] - x[:4]])], [0.5, 0.5], row_len=4)
    assert [r["status"] for r in rows] == [R.ZERO, R.LINEAR] and R.counters(rows) == (1, 1, 0.0)


def test_row_sums_follow_the_pinned_lane_order():
    """65 elements: lane 0 adds elements 0 and 64, then the fold by halves -- against the same tree written out by hand."""
    rng = np.random.default_rng(3)
    t = rng.standard_normal((1, 2 * 65))
    got = R.row_sums(t, 65)
    for r in range(2):
        lanes = [float(t[0, r * 65 + l]) for l in range(64)]
        lanes[0] = (0.0 + lanes[0]) + float(t[0, r * 65 + 64])
        for half in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l + half] for l in range(half)]
        assert bits(float(got[0, r])) == bits(lanes[0])
    assert bits(float(R.row_sums(np.array([[-0.0]]), 1)[0, 0])) == bits(0.0)  # from +0.0: never -0.0


def test_twenty_four_iterations_have_converged_on_well_posed_inputs():
    for seed, S in enumerate((2, 3, 4, 3, 4)):
        xs = randn(256, S, seed=50 + seed)
        g = randn(256, 1, seed=70 + seed)[0]
        xs = [(x + F(0.5) * g).astype(F) for x in xs]
        _, res = R.sphere(None, xs, [1.0 + m for m in range(S)])
        assert res["status"] == R.OK and res["resid"] <= 1e-13 and all(math.isfinite(c) for c in res["coef64"])


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_sphere_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_sphere_plan_bytes", "vlm_sphere_plan_upload", "vlm_sphere_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert L.SIGNATURES["vlm_sphere_plan_bytes"] == L.SIGNATURES["vlm_stock_plan_bytes"]
    assert L.SIGNATURES["vlm_sphere_run"] == L.SIGNATURES["vlm_stock_run"]
    assert L.SIGNATURES["vlm_sphere_plan_upload"][1][1:] == L.SIGNATURES["vlm_stock_plan_upload"][1][1:]
    assert lib.vlm_abi_version() == 11  # entry points are added, nothing moves
    raw = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()  # the rule and the difference from mergekit's slerp are stated
    for word in ("nuslerp", "does NOT renormalise", "#define VLM_SPHERE_ITERS 24", "ITERS = 24, EDGE = 2^-20, QMIN = 2^-40"):
        assert word in raw, word


def test_sphere_struct_layouts_are_the_compilers(pkg, tmp_path):
    """sizeof and the offsets of the ctypes structures against what the host compiler makes of include/vlm_hip.h."""
    L = importlib.import_module("vl_merging_amd._lib")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    types = {"vlm_sphere_job_t": L.SphereJob, "vlm_sphere_header_t": L.SphereHeader, "vlm_sphere_result_t": L.SphereResult}
    consts = {"VLM_SPHERE_OK": L.SPHERE_OK, "VLM_SPHERE_LINEAR": L.SPHERE_LINEAR, "VLM_SPHERE_ZERO": L.SPHERE_ZERO,
              "VLM_SPHERE_ITERS": L.SPHERE_ITERS}
    lines = ['printf("%s %%d\\n", %s);' % (c, c) for c in consts]
    for cname, ty in types.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in ty._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vlm_hip.h"\nint main() {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = str(tmp_path / "layout")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    got = dict(ln.split() for ln in r.stdout.splitlines())
    want = {c: str(v) for c, v in consts.items()}
    for cname, ty in types.items():
        want[cname] = str(ctypes.sizeof(ty))
        for field, _ in ty._fields_:
            want[cname + "." + field] = str(getattr(ty, field).offset)
    assert got == want
    assert (ctypes.sizeof(L.SphereJob), ctypes.sizeof(L.SphereHeader), ctypes.sizeof(L.SphereResult)) == (112, 72, 176)
    assert L.SphereResult.coef64.offset == 8 * L.STOCK_SUMS  # a result begins as a record does
    assert (ctypes.sizeof(L.StockJob), ctypes.sizeof(L.StockResult), ctypes.sizeof(L.DellaJob)) == (64, 152, 104)  # untouched
    assert R.ITERS == L.SPHERE_ITERS and R.MAX_SRC == L.MERGE_MAX_SRC


def fake_job(L, **fields):
    job = L.SphereJob()
    job.dst, job.base, job.n_src, job.n_elem, job.lam, job.row_len = 0x1000, 0x2000, 2, 16, 1.0, 0
    job.src[0], job.src[1] = 0x3000, 0x4000
    job.w[0], job.w[1] = 0.5, 0.5
    for k, v in fields.items():
        setattr(job, k, v)
    return job


def test_sphere_host_side_argument_checks(pkg):
    """vlm_sphere_plan_upload rejects bad jobs before it touches the device: every pointer here is fake."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_sphere_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_sphere_plan_bytes(1, 4096), lib.vlm_sphere_plan_bytes(100, 1 << 24)
    assert 0 < small < big and big >= 100 * (112 + 176) + (8 + 80) * (1 << 12) + 8 * (1 << 13)  # jobs, results; chunks, records; tiles
    ws = ctypes.c_void_p(0x10000)

    def upload(j, n=1, w=ws, nbytes=64):
        return lib.vlm_sphere_plan_upload((L.SphereJob * 1)(j), n, w, nbytes, None)

    def with_w(*w, **fields):
        j = fake_job(L, **fields)
        for k, v in enumerate(w):
            j.w[k] = v
        return j

    assert upload(fake_job(L)) == -3                              # VLM_ERR_WORKSPACE: every argument check passed
    assert upload(fake_job(L), w=ctypes.c_void_p(0)) == -1        # no workspace
    assert upload(fake_job(L), w=ctypes.c_void_p(0x10008)) == -1  # misaligned workspace
    assert upload(fake_job(L), n=0) == -1                         # no jobs
    for field, value in (("n_src", 0), ("n_src", 5), ("n_src", -1), ("n_elem", 0), ("dst", 0), ("dst", 0x1004), ("base", 0x2008),
                         ("dst", 0x2000), ("dst", 0x3000), ("dst", 0x4000), ("dst", 0x2010), ("dst", 0x1FF0), ("dst", 0x3FF0),
                         ("row_len", 3), ("row_len", 5), ("row_len", 32), ("row_len", 4097), ("row_len", 1 << 31),  # a bad row_len
                         ("coef_out", 0x5004),                    # misaligned
                         ("coef_out", 0x1000), ("coef_out", 0x2030), ("coef_out", 0x3000), ("coef_out", 0x403C),  # meets a tensor
                         ("coef_out", 0x1030)):                   # inside dst
        assert upload(fake_job(L, **{field: value})) == -1, (field, value)
    for w in ((-0.5, 1.0), (0.0, 0.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0, -1e-300), (1.0, float("-inf"))):
        assert upload(with_w(*w)) == -1, w                        # a negative or non-finite weight; weights that are all zero
    assert upload(with_w(0.0, 0.0, 1.0, n_src=2)) == -1           # the weight of a source the job does not have does not count
    assert upload(fake_job(L, base=0, lam=0.5)) == -1             # lam != 1 without a base
    assert upload(fake_job(L, base=0, lam=float("nan"))) == -1
    assert upload(fake_job(L, n_elem=1 << 34, dst=1 << 60)) == -4  # VLM_ERR_UNSUPPORTED: the length limit of the family
    for idx, src in ((1, 0), (1, 0x4004), (0, 0x3008), (0, 0x1010)):
        bad = fake_job(L)
        bad.src[idx] = src
        assert upload(bad) == -1, (idx, src)
    # the controls that pass every check: no base, a base with another lam, rows, a zero weight, one source, a coef_out that
    # meets nothing (a row job's is rows x 16 bytes long: four rows end where dst begins)
    for ok in (fake_job(L, base=0), fake_job(L, lam=0.25), fake_job(L, row_len=4), fake_job(L, row_len=16), fake_job(L, row_len=1),
               with_w(0.0, 2.0), with_w(1e300, 1e300), fake_job(L, n_src=1), fake_job(L, coef_out=0x5000), fake_job(L, coef_out=0x0FF0),
               fake_job(L, row_len=4, coef_out=0x0FC0), fake_job(L, base=0, row_len=8, coef_out=0x2000)):
        assert upload(ok) == -3, bytes(ok)
    assert upload(fake_job(L, row_len=4, coef_out=0x0FD0)) == -1  # four rows of coefficients: the last reaches into dst
    assert lib.vlm_sphere_run(ctypes.c_void_p(0), None) == -1


# ------------------------------------------------------------------------------------------------------- the host surface
def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.SpherePlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, loss_names={}, merge_ratio=0.5)
    with pytest.raises(L.VlmError):
        merge.sphere_merge({}, cfg, device="cpu")
    with pytest.raises(ValueError):
        merge.sphere_merge({}, cfg, on="tangent")
    with pytest.raises(ValueError):
        merge.sphere_merge({}, cfg, on="weights", lam=0.5)
    assert merge.SpherePlan.PASSES == 2 and merge.SpherePlan.HAS_DST
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.sphere_merge) and vm.ViLTransformerSS.sphere_merge.__defaults__ == ("weights", False, None)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


def test_sphere_merge_on_weights_never_touches_the_central_checkpoint(pkg, monkeypatch):
    """on="weights" reads no central checkpoint: not the argument, not config["central_weight"].  A plan class that records its jobs
    stands in for the device."""
    merge = importlib.import_module("vl_merging_amd.merge")

    class Boom(dict):
        def __getitem__(self, k):
            raise AssertionError("the central checkpoint was read: %r" % (k,))

        def __contains__(self, k):
            raise AssertionError("the central checkpoint was searched: %r" % (k,))

    calls = []

    class FakePlan:
        def __init__(self, device):
            self.device, self.jobs = device, []

        def add(self, *a, **kw):
            self.jobs.append((a, kw))
            calls.append((type(self).__name__, a, kw))
            return "merged"

        def run(self):
            pass

        def report(self):
            return []

    monkeypatch.setattr(merge, "SpherePlan", type("FakeSphere", (FakePlan,), {}))
    monkeypatch.setattr(merge, "MergePlan", type("FakeMerge", (FakePlan,), {}))
    monkeypatch.setattr(merge, "_central", lambda *a: (_ for _ in ()).throw(AssertionError("_central was called")))
    from test_oracle_merge import merge_cfg, tiny_state
    sd = tiny_state("all_moe")
    cfg = dict(merge_cfg(merge_ratio=0.3), central_weight="/nonexistent/ufo.ckpt")
    out = merge.sphere_merge(sd, cfg, central_weight=Boom(), on="weights", device="cuda")
    sphere = [c for c in calls if c[0] == "FakeSphere"]
    assert len(sphere) == 12 * 13 and all(c[1][1] is None and c[2]["lam"] == 1.0 for c in sphere)  # no base, no lam
    ratios = merge.interpolation_ratios(["v", "l"], 0.3)
    assert sphere[0][1][2] == [ratios["v"], ratios["l"]] and len(sphere[-1][1][2]) == 3  # merge_weights' weights
    assert sum(isinstance(v, str) and v == "merged" for v in out.values()) == 12 * 13
    with pytest.raises(AssertionError):  # the control: on="delta" does read it
        merge.sphere_merge(sd, cfg, central_weight=Boom(), on="delta", device="cuda")


def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_merge_ckpt_parses_slerp_before_any_device(pkg):
    mc = tool()
    assert "slerp" in mc.METHODS and "karcher" in mc.METHODS
    io = ["--ckpt", "a.ckpt", "--out", "b.ckpt"]
    args, cfg = mc.parse_args(["--method", "slerp"] + io + ["--report", "r.json", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.sphere_on, args.sphere_rows, args.report) == ("slerp", "weights", False, "r.json")
    args, cfg = mc.parse_args(["--method", "karcher"] + io + ["--sphere-on", "delta", "--sphere-rows", "--central", "c.ckpt",
                                                             "--lambda", "0.4", "--ratio", "0.25"])
    assert (args.method, args.sphere_on, args.sphere_rows, args.central) == ("karcher", "delta", True, "c.ckpt")
    assert cfg["sum_lambda"] == 0.4 and cfg["merge_ratio"] == 0.25  # as for taskvec and interp
    with pytest.raises(SystemExit):
        mc.parse_args(["--method", "slerp"] + io + ["--sphere-on", "tangent"])
    args, _ = mc.parse_args(["--method", "stock"] + io)  # the other methods parse as before
    assert (args.sphere_on, args.sphere_rows) == ("weights", False)
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "slerp" in r.stdout and "karcher" in r.stdout and "sphere_merge" in r.stdout and "--sphere-rows" in r.stdout


# ------------------------------------------------------------------------------------------------------ the build record
def test_sphere_kernels_keep_the_occupancy_their_grids_count_on():
    """None of the four may spill or use scratch.  The reducer and the apply pass are Model Stock's kernels over another job type:
    the same occupancy (three and at least four workgroups per CU).  The row kernel's grid counts on two resident workgroups per
    CU: 68 KiB of LDS each and at most 256 registers."""
    import test_build_cpu as tb
    if tb._stale():
        import __graft_entry__ as ge
        ge.build()
    with open(tb.RES) as f:
        resources = json.load(f)
    found = {}
    for name in ("vlm_sphere_reduce_kernel", "vlm_sphere_fold_kernel", "vlm_sphere_apply_kernel", "vlm_sphere_rows_kernel"):
        hit = [v for k, v in resources.items() if name in k]
        assert len(hit) == 1, sorted(k for k in resources if "sphere" in k)
        found[name] = hit[0]
        assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0, (name, hit[0])
    assert found["vlm_sphere_reduce_kernel"]["Occupancy"] >= 3, found["vlm_sphere_reduce_kernel"]
    assert found["vlm_sphere_apply_kernel"]["Occupancy"] >= 4, found["vlm_sphere_apply_kernel"]
    assert found["vlm_sphere_reduce_kernel"]["LDS Size"] == 2 * 4 * 10 * 8  # two buffers of four waves' ten sums
    rows = found["vlm_sphere_rows_kernel"]
    assert rows["Occupancy"] >= 2 and rows["LDS Size"] == (4 * 4096 + 256 * 4) * 4 and 2 * rows["LDS Size"] <= 160 * 1024, rows
    for name in ("vlm_stock_reduce_kernel", "vlm_stock_fold_kernel", "vlm_stock_apply_kernel"):  # still one each
        assert len([k for k in resources if name in k]) == 1, name


# -------------------------------------------------------------------------------------------------------- the sanitizer
def test_sphere_upload_checks_under_the_sanitizers(tmp_path):
    """helpers/sphere_plan_check.cpp: the checks and the two table fills of vlm_sphere_plan_upload have no HIP in them
    (chunk_plan.h and della_tiles.h compile without it); the program restates them over the same headers, walks plans of mixed
    tensor and row jobs and is built with -fsanitize=address,undefined."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "tests", "helpers", "sphere_plan_check.cpp")
    exe = str(tmp_path / "sphere_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "sphere_plan_check: ok" in r.stdout
