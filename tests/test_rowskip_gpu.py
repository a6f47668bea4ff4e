"""Row skipping (vlm_gemm_bf16_live, ops.gemm(..., row_live=...)): a 256-row tile of the 256x256 GEMM kernel whose rows are all
dead (row_live == 0) skips its K loop and writes epilogue(0); every other tile computes what the call without the vector computes.

Everything here is a byte comparison between two launches of the same kernel on the same inputs, so there is no tolerance: a live
tile runs the unchanged code path, and a dead tile runs the epilogue's own arithmetic on +0 accumulators, which is what the full
computation leaves when the tile's rows of A are zero (a sum of +-0 products in round-to-nearest is +0).  The shapes are small, so
the tests force the 256x256 kernel (vlm_gemm_set_big_tile_mode(2)) and check that a dead tile really was skipped: with random A its
rows differ from the full computation's."""
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
KEEP = 1.0 / 0.9  # what DropPath leaves on a kept row; only zero is tested, any other value must count as live


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("vl_merging_amd.ops")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("vl_merging_amd._lib")


@pytest.fixture
def big_tiles(L):
    """The 256x256 kernel whenever it is legal (by default launches this small go to the 128x128 kernel, which ignores the vector)."""
    assert L.get_lib().vlm_gemm_set_big_tile_mode(2) == 0
    yield
    L.get_lib().vlm_gemm_set_big_tile_mode(-1)


def same_bytes(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == BF16 else torch.int32))


class _Fold:
    """Stands in for ops.FoldBatch: hands ops.gemm one region for the per-tile column sums and folds nothing."""

    def __init__(self, region):
        self.region, self.jobs = region, []

    def next_region(self):
        return self.region

    def add(self, *a):
        pass


VARIANTS = ("plain", "residual", "gelu_deriv", "mul_aux")
SENTINEL = 7.0


def make_inputs(M, N, K, seed):
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)  # noqa: E731
    return dict(A=rnd(M, K).to(BF16), W=(rnd(N, K) / math.sqrt(K)).to(BF16), bias=0.5 * rnd(N), residual=rnd(M, N),
                row_scale=0.5 + torch.rand(M, device="cuda", generator=gen), aux_in=rnd(M, N).to(BF16))


def run_variant(ops, L, variant, inp, A, live):
    """One call; -> the tensors it writes, all pre-filled with a sentinel.  ws: per-half column sums [M // 128][2][N]."""
    M, N = A.shape[0], inp["W"].shape[0]
    res = {}
    if variant == "plain":
        res["out"] = torch.full((M, N), SENTINEL, device="cuda", dtype=BF16)
        ops.gemm(A, inp["W"], res["out"], bias=inp["bias"], row_live=live)
    elif variant == "residual":
        res["out"] = torch.full((M, N), SENTINEL, device="cuda", dtype=F32)
        ops.gemm(A, inp["W"], res["out"], bias=inp["bias"], row_scale=inp["row_scale"], residual=inp["residual"], row_live=live)
    elif variant == "gelu_deriv":
        res["out"] = torch.full((M, N), SENTINEL, device="cuda", dtype=BF16)
        res["aux"] = torch.full((M, N), SENTINEL, device="cuda", dtype=BF16)
        ops.gemm(A, inp["W"], res["out"], bias=inp["bias"], act=L.ACT_GELU_DERIV, aux=res["aux"], row_live=live)
    else:
        res["out"] = torch.full((M, N), SENTINEL, device="cuda", dtype=BF16)
        res["col_sum"] = torch.zeros(N, device="cuda")
        res["ws"] = torch.full((M // 128, 2, N), SENTINEL, device="cuda")
        ops.gemm(A, inp["W"], res["out"], act=L.ACT_MUL_AUX, aux=inp["aux_in"], col_sum=res["col_sum"],
                 col_sum_fold=_Fold(res["ws"].view(-1)), row_live=live)
    return res


def live_vectors(M):
    """name -> (vector, tiles that are wholly dead).  M = 1048: four whole tiles and a ragged one of 24 rows."""
    assert M == 1048
    def vec(*dead):
        v = torch.full((M,), KEEP, device="cuda")
        for lo, hi in dead:
            v[lo:hi] = 0.0
        return v
    return {"all_live": (vec(), ()),
            "tile1_dead": (vec((256, 512)), (1,)),
            "tile2_dead_but_last_row": (vec((512, 767)), ()),
            "ragged_dead": (vec((1024, 1048)), (4,)),
            "all_dead": (vec((0, 1048)), (0, 1, 2, 3, 4))}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("K", [128, 768])
def test_gemm_tile_rule(ops, L, big_tiles, K, N, variant):
    M = 1048
    inp = make_inputs(M, N, K, seed=K * 7 + N)
    A = inp["A"]
    full = run_variant(ops, L, variant, inp, A, None)
    for name, (live, dead) in live_vectors(M).items():
        got = run_variant(ops, L, variant, inp, A, live)
        want_dead = None
        if dead:
            Az = A.clone()
            for t in dead:
                Az[256 * t:256 * (t + 1)] = 0
            want_dead = run_variant(ops, L, variant, inp, Az, None)
        torch.cuda.synchronize()
        for t in range(5):
            rows = slice(256 * t, min(256 * (t + 1), M))
            want = want_dead if t in dead else full
            for key in ("out", "aux"):
                if key in got:
                    assert same_bytes(got[key][rows], want[key][rows]), (name, key, "tile", t)
            if "ws" in got and t < 4:  # the two complete 128-row halves of a whole tile
                assert same_bytes(got["ws"][2 * t:2 * t + 2], want["ws"][2 * t:2 * t + 2]), (name, "col_sum_ws", "tile", t)
            if t in dead:  # the tile was skipped, not computed: with random A the full computation gives other values
                assert not same_bytes(got["out"][rows], full["out"][rows]), (name, "tile %d was not skipped" % t)
        if "col_sum" in got:  # only the ragged tile adds to col_sum directly
            assert same_bytes(got["col_sum"], (want_dead if 4 in dead else full)["col_sum"]), (name, "col_sum")


# the layout of test 3 and of the flagship: B samples of T text rows, then B samples of I image rows
B_, T_, I_ = 3, 40, 577
M_ = B_ * (T_ + I_)


def sample_rows(s):
    return [(s * T_, (s + 1) * T_), (B_ * T_ + s * I_, B_ * T_ + (s + 1) * I_)]


def dead_tiles(live):
    """Tiles of 256 rows whose rows inside [0, M) are all zero in `live`."""
    v = live.detach().cpu()
    return [t for t in range((v.numel() + 255) // 256) if not bool((v[256 * t:256 * (t + 1)] != 0).any())]


@pytest.mark.parametrize("name,K,N", [("fc2_dgrad", 256, 1024), ("fc1_dgrad", 1024, 256), ("proj_dgrad", 256, 256),
                                      ("qkv_dgrad", 768, 256)])
def test_gemm_backward_identity(ops, L, big_tiles, name, K, N):
    """The four dgrad GEMMs of a D = 256, F = 1024 block over 3 samples at the 384^2 geometry, sample 1 dropped: its rows of A are
    exact zeros, as the backward pass leaves them, so the outputs with and without the vector are equal (==: a zero's sign may
    differ where the epilogue multiplies by a negative saved factor)."""
    inp = make_inputs(M_, N, K, seed=K + N)
    A = inp["A"].clone()
    live = torch.full((M_,), KEEP, device="cuda")
    for lo, hi in sample_rows(1):
        A[lo:hi] = 0
        live[lo:hi] = 0.0
    assert dead_tiles(live) == [3]  # image rows 697 .. 1273 contain the tile 768 .. 1023
    variant = "mul_aux" if name == "fc2_dgrad" else "plain"
    if variant == "plain":
        inp["bias"] = None
    full = run_variant(ops, L, variant, inp, A, None)
    got = run_variant(ops, L, variant, inp, A, live)
    torch.cuda.synchronize()
    for key in got:
        assert torch.equal(got[key], full[key]), key
    assert bool((got["out"][768:1024] == 0).all())


@pytest.mark.parametrize("off", [1, 2, 3])
def test_gemm_vector_at_any_float_address(ops, L, big_tiles, off):
    """The engine's vectors are rows of one [sites, rows] table, so a site's vector starts 4, 8 or 12 bytes past a 16-byte
    boundary whenever `rows` is no multiple of 4 (the flagship's 13 574 rows: every second site).  Such a view must skip like an
    aligned one: tile 1 and the ragged tile dead, checked as in test_gemm_tile_rule."""
    M, N, K = 1048, 256, 128
    inp = make_inputs(M, N, K, seed=off)
    A = inp["A"]
    live = torch.full((M + 4,), KEEP, device="cuda")[off:off + M]
    assert live.data_ptr() % 16 == 4 * off
    live[256:512] = 0.0
    live[1024:] = 0.0
    Az = A.clone()
    Az[256:512] = 0
    Az[1024:] = 0
    for variant in ("plain", "mul_aux"):
        full, zero = run_variant(ops, L, variant, inp, A, None), run_variant(ops, L, variant, inp, Az, None)
        got = run_variant(ops, L, variant, inp, A, live)
        torch.cuda.synchronize()
        for t in range(5):
            rows = slice(256 * t, min(256 * (t + 1), M))
            want = zero if t in (1, 4) else full
            assert same_bytes(got["out"][rows], want["out"][rows]), (variant, "tile", t)
            if "ws" in got and t < 4:
                assert same_bytes(got["ws"][2 * t:2 * t + 2], want["ws"][2 * t:2 * t + 2]), (variant, "col_sum_ws", t)
            if t in (1, 4):
                assert not same_bytes(got["out"][rows], full["out"][rows]), (variant, "tile %d was not skipped" % t)
        if "col_sum" in got:
            assert same_bytes(got["col_sum"], zero["col_sum"])


# ---- one block, forward and backward, with and without the skip in one process ------------------------------------------------
def _spy_gemm(real, calls, a, b, out, *args, row_live=None, **kw):
    """ops.gemm as the engine calls it, plus a record of every call that carries a vector.  For a call that can show it (qkv and
    fc1 forward: no row scale that zeroes the dead rows anyway, no column sums, dead rows of A not zero) the same call is made again WITHOUT the vector into copies of its outputs: `skipped` says that
    the rows of the vector's first dead tile differ, that is, that the kernel took the vector as it came and skipped the tile."""
    r = real(a, b, out, *args, row_live=row_live, **kw)
    if row_live is not None:
        dead, skipped = dead_tiles(row_live), None
        rows = slice(256 * dead[0], 256 * (dead[0] + 1)) if dead else None
        if dead and kw.get("col_sum") is None and kw.get("row_scale") is None and bool((a[rows] != 0).any()):
            kw2 = dict(kw)
            if kw2.get("aux") is not None:
                kw2["aux"] = kw2["aux"].clone()
            out2 = out.clone()
            real(a, b, out2, *args, row_live=None, **kw2)
            skipped = not same_bytes(out2[rows], out[rows])
        calls.append(("gemm", row_live.data_ptr(), skipped))
    return r


def _block_run(pkg, skip):
    """Forward + backward of ONE ufo block at D = 256, 4 heads, F = 1024 over 3 samples of 40 text + 577 image tokens (1 851 rows)
    with seeded inputs; the injected draws drop sample 1 at the block's first DropPath site and sample 2 at its second."""
    engine = importlib.import_module("vl_merging_amd.engine")
    ops = importlib.import_module("vl_merging_amd.ops")
    cfgmod = importlib.import_module("vl_merging_amd.vilt.config")
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    vt = importlib.import_module("vl_merging_amd.vilt.modules.vision_transformer")
    D, H = 256, 4
    torch.manual_seed(11)
    vt._VIT_ARCH["vit_w256_patch16_384"] = dict(img_size=384, patch_size=16, embed_dim=D, depth=12, num_heads=H)
    prev = engine._ROWSKIP["enabled"]
    try:
        cfg = cfgmod.make_config("ufo", vit="vit_w256_patch16_384", hidden_size=D, num_heads=H, vocab_size=1024,
                                 max_text_len=T_, patch_size=16, vlffn_start_layer_index=10, image_size=384, max_vl_text_len=T_,
                                 tasks=["vl"], loss_names=cfgmod._loss_names({"itm": 1}), drop_rate=0.2)
        model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg)).cuda().train()
        with torch.no_grad():  # the shipped init leaves biases at zero and gammas equal: make every gradient path non-trivial
            gen = torch.Generator(device="cuda"); gen.manual_seed(5)
            for n, p in model.named_parameters():
                if n.startswith("transformer.blocks.6.") or n == "relative_position_bias_table":
                    p.add_(0.02 * torch.randn(p.shape, device="cuda", generator=gen))
        model.setup_engine()
        engine._ROWSKIP["enabled"] = skip
        blk = model.transformer.blocks[6]
        assert 0 < blk.drop_path_prob < 0.5
        keep0 = torch.ones(B_, T_, device="cuda", dtype=torch.uint8)
        pc = model._pass_ctx(ops.Seq(B_, T_, I_), H, model.get_rel_pos_bias(model.vl_text_imag_relative_position_index, T_),
                             keep0=keep0)

        def draws(pc_, S, streams):  # kept where u < keep
            u = torch.zeros(streams, S, B_)
            u[:, 0, 1] = 0.99
            u[:, 1, 2] = 0.99
            return u

        pc.uniform_source = draws
        pc.plan_drop_path([blk.drop_path_prob, blk.drop_path_prob])
        gen = torch.Generator(device="cuda"); gen.manual_seed(17)
        x = torch.randn(M_, D, device="cuda", generator=gen).requires_grad_(True)
        g = torch.randn(M_, D, device="cuda", generator=gen)
        model.zero_grad()
        calls = []  # every vector that reaches a kernel: (entry, address, skipped) -- skipped: see _spy_gemm
        real_gemm, real_attn = ops.gemm, ops.attention_bwd
        ops.gemm = lambda *a, **k: _spy_gemm(real_gemm, calls, *a, **k)
        ops.attention_bwd = lambda *a, **k: (calls.append(("attention_bwd", k["row_live"].data_ptr(), None))
                                             if k.get("row_live") is not None else None, real_attn(*a, **k))[1]
        try:
            y = blk.run(x, pc, 2)
            fold = engine._folded(blk.plan(2, pc.seq).ranges)
            y.backward(g)
        finally:
            ops.gemm, ops.attention_bwd = real_gemm, real_attn
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
                 if (n.startswith("transformer.blocks.6.") or n == "relative_position_bias_table") and p.grad is not None}
        weights = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith("transformer.blocks.6.")}
        return dict(y=y.detach().clone(), dx=x.grad.detach().clone(), grads=grads, w=weights, fold=fold,
                    factors=pc._dp_all.detach().clone(), calls=calls, sites=[pc._dp_all[i].data_ptr() for i in range(2)])
    finally:
        engine._ROWSKIP["enabled"] = prev
        del vt._VIT_ARCH["vit_w256_patch16_384"]


WEIGHTS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")


def test_block_forward_backward_with_and_without_skip(pkg, big_tiles):
    """x2 byte-identical, dx equal; weight gradients, column-sum gradients and the bias table within the bounds of
    tests/test_wgrad_batch_gpu.py (their atomics are not bit-reproducible between two runs of one tree): wgrad rtol 1e-3 and atol
    2e-3 sqrt(rows), column sums 1e-4 of the tensor's largest element, and for a folded gamma the wgrad bound carried through
    dgamma[n] = sum_k W[n,k] raw_w[n,k] + b[n] raw_b[n]."""
    on, off = _block_run(pkg, True), _block_run(pkg, False)
    # the draws and the layout: sample 1 dead at site 1 (tile 768 .. 1023), sample 2 at site 2 (tiles from 1280 to the end)
    assert torch.equal(on["factors"], off["factors"]) and on["factors"].shape == (2, M_)
    for site, s in ((0, 1), (1, 2)):
        f = on["factors"][site]
        dead = f == 0
        want = torch.zeros(M_, dtype=torch.bool, device="cuda")
        for lo, hi in sample_rows(s):
            want[lo:hi] = True
        assert torch.equal(dead, want), "site %d" % site
    assert dead_tiles(on["factors"][0]) == [3] and dead_tiles(on["factors"][1]) == [5, 6, 7]
    # ... and both sites' vectors reached the kernels as they are, and the kernel skipped by them: four GEMMs per site (two forward,
    # two dgrad) and the attention backward at site 1 got the site's own row of the table -- the second row starts 7 404 bytes
    # after the first, 12 bytes past a 16-byte boundary -- and the site's first forward GEMM (qkv, fc1) left other bytes in a dead
    # tile than the full computation does.  (The residual GEMMs and the dgrads cannot show it: a zero row scale, zero rows of A.
    # They receive the same address.)
    assert not off["calls"] and on["sites"][1] - on["sites"][0] == 4 * M_ and (on["sites"][1] - on["sites"][0]) % 16 == 12
    for site in (0, 1):
        mine = [c for c in on["calls"] if c[1] == on["sites"][site]]
        assert [c[0] for c in mine].count("gemm") == 4 and [c[0] for c in mine].count("attention_bwd") == (1 if site == 0 else 0), mine
        assert [c[2] for c in mine if c[0] == "gemm"].count(True) == 1 and not [c for c in mine if c[2] is False], mine
    assert len(on["calls"]) == 9
    assert same_bytes(on["y"], off["y"]), "x2 differs"
    assert torch.equal(on["dx"], off["dx"]), "dx differs"
    fold, w = on["fold"], on["w"]
    assert sorted(on["grads"]) == sorted(off["grads"]) and len(on["grads"]) == 16, sorted(on["grads"])
    atol = 2e-3 * math.sqrt(M_)
    pre = "transformer.blocks.6."
    seen = 0
    for n in sorted(on["grads"]):
        a, b = on["grads"][n], off["grads"][n]
        assert float(b.abs().max()) > 0, n + ": zero gradient, the case checks nothing"
        short = n[len(pre):] if n.startswith(pre) else n
        err = (a - b).abs()
        if short in WEIGHTS:
            seen += 1
            gamma = {"attn.proj.weight": w[pre + "gamma_1"], "mlp.fc2.weight": w[pre + "gamma_2"]}.get(short) if fold else None
            scale = gamma.abs()[:, None] if gamma is not None else 1.0
            bound = scale * atol + 1e-3 * b.abs()
        else:
            bound = torch.full_like(b, 1e-4 * float(b.abs().max()))
            if fold and short in ("gamma_1", "gamma_2"):
                lin = "attn.proj" if short == "gamma_1" else "mlp.fc2"
                W, gm = w[pre + lin + ".weight"], w[pre + short]
                raw = off["grads"][pre + lin + ".weight"] / gm[:, None]
                bound = bound + (W.abs() * (atol + 1e-3 * raw.abs())).sum(1)
        print("%-40s max err %.4g of max %.4g" % (short, float(err.max()), float(b.abs().max())))
        assert not bool((err > bound).any()), "%s: max err %.4g of max %.4g" % (n, float(err.max()), float(b.abs().max()))
    assert seen == 4


# ---- attention backward: a dead (sample, segment) is not recomputed --------------------------------------------------------------
def _attn_case(B, n0, n1, H, seed):
    """The inputs of tests/test_attention_gpu.py's cases: random qkv, a random index with the reference's constant text <-> image
    blocks, a two-layer table, a ragged text keep mask."""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    D, rows = H * 64, B * (n0 + n1)
    qkv = (torch.randn(rows, 3 * D, device="cuda", generator=g) * 1.5).to(BF16)
    pos1 = (n0 + 7) // 8 * 8
    NP = pos1 + n1
    R = 300
    idx = torch.randint(0, R, (NP, (NP + 3) // 4 * 4), device="cuda", generator=g).to(torch.int16)
    idx[:n0, pos1:] = R - 2
    idx[pos1:, :n0] = R - 1
    idx_t = torch.zeros(NP, (NP + 3) // 4 * 4, device="cuda", dtype=torch.int16)
    idx_t[:, :NP] = idx[:NP, :NP].t() * 4
    table = torch.randn(R, 2 * H, device="cuda", generator=g)
    lens = torch.randint(max(1, n0 // 4), n0 + 1, (B,), device="cuda", generator=g)
    keep0 = (torch.arange(n0, device="cuda")[None] < lens[:, None]).to(torch.uint8).contiguous()
    dout = torch.randn(rows, D, device="cuda", generator=g).to(BF16)
    return dict(qkv=qkv, idx=idx * 4, idx_t=idx_t, bias_t=table.t().contiguous(), keep0=keep0, dout=dout, D=D, rows=rows)


@pytest.mark.parametrize("sep", [False, True])
def test_attention_bwd_dead_sample(ops, L, sep):
    """B = 3, H = 2, segments of 8 and 65 positions, sample 1 dead: both segments in JOINT mode (one draw per sample), the image
    segment alone in SEPARATE mode (a draw per segment); dO is zero on the dead rows, as the proj dgrad leaves it.  The dqkv rows
    of the dead (sample, segment) are zero, every other row has the bytes of the call without the vector, and the table gradient
    agrees within the attention test's bound (2e-2 of its largest element + 2e-2 relative; its float atomics arrive in any
    order).  The column sums meet that test's bound for them as well."""
    B, n0, n1, H = 3, 8, 65, 2
    c = _attn_case(B, n0, n1, H, seed=40 + sep)
    seq = ops.Seq(B, n0, n1)
    rows, D, layer = c["rows"], c["D"], 1
    assert seq.rows == rows
    dead = torch.zeros(rows, dtype=torch.bool, device="cuda")
    dead[B * n0 + 1 * n1:B * n0 + 2 * n1] = True
    if not sep:
        dead[1 * n0:2 * n0] = True
    live = torch.full((rows,), KEEP, device="cuda")
    live[dead] = 0.0
    dout = c["dout"].clone()
    dout[dead] = 0
    kw = dict(bias_t=c["bias_t"], head_row0=layer * H, rel_index=c["idx"], rel_index_t=c["idx_t"], keep0=c["keep0"],
              mode=L.ATTN_SEPARATE if sep else L.ATTN_JOINT)
    out = torch.empty(rows, D, device="cuda", dtype=BF16)
    lse = torch.empty(H, rows, device="cuda")
    ops.attention_fwd(c["qkv"], out, lse, seq, H, **kw)
    res = []
    for vec in (None, live):
        dqkv = torch.full((rows, 3 * D), SENTINEL, device="cuda", dtype=BF16)
        dbias_t = torch.zeros_like(c["bias_t"])
        csq = [torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")]
        csv = [torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")]
        ops.attention_bwd(c["qkv"], out, dout, lse, dqkv, seq, H, dbias_t=dbias_t, dq_colsum=csq, dv_colsum=csv, row_live=vec, **kw)
        torch.cuda.synchronize()
        res.append((dqkv, dbias_t, csq + csv))
    (full, tab_full, cs_full), (got, tab_got, cs_got) = res
    assert float(full.float().abs().max()) > 0 and float(tab_full.abs().max()) > 0
    assert bool((got[dead] == 0).all()), "dead rows are not zero"
    assert bool((full[dead] == 0).all())  # (what the promise about dO means for the full computation)
    assert same_bytes(got[~dead], full[~dead]), "live rows differ"
    b = tab_full[layer * H:(layer + 1) * H]
    err = (tab_got[layer * H:(layer + 1) * H] - b).abs()
    print("dbias max err %.4g of max %.4g" % (float(err.max()), float(b.abs().max())))
    assert bool((err <= 2e-2 * float(b.abs().max()) + 2e-2 * b.abs()).all())
    assert float(tab_got[:H].abs().max()) == 0.0  # the other layer's rows untouched
    for a, w in zip(cs_got, cs_full):
        assert float((a - w).abs().max()) <= 2e-2 * float(w.abs().max()) + 0.05
