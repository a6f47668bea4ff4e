"""Kept rows: the attention kernels with a per-segment query prefix (vlm_attn_desc_t.q_keep0 / q_keep1), a block evaluation that
works on the kept rows behind the attention (engine.run_block(keep=...)), and the passes that ask for them (infer(reads="text"),
infer_unimodal_pair(reads="cls")).

Every case compares two runs of this tree on the same inputs: with the limit, and without it on a gradient that is zero outside
the kept rows.  Where both runs execute the same instructions on the same operands the comparison is a byte comparison; the
tolerances elsewhere are the ones the existing tests state for the same quantities and are quoted where they are used."""
import importlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
KEEP = 1.0 / 0.9


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("vl_merging_amd.ops")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("vl_merging_amd._lib")


@pytest.fixture(scope="module")
def engine(pkg):
    return importlib.import_module("vl_merging_amd.engine")


def same_bytes(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == BF16 else torch.int32))


# ---- attention -------------------------------------------------------------------------------------------------------------------
def attn_case(B, n0, n1, H, seed, mask):
    """The inputs of tests/test_attention_gpu.py's cases (as tests/test_rowskip_gpu.py builds them): random qkv, a random index with
    the reference's constant text <-> image blocks, a two-layer table, a ragged text key-padding mask or none."""
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
    keep0 = (torch.arange(n0, device="cuda")[None] < lens[:, None]).to(torch.uint8).contiguous() if mask else None
    dout = torch.randn(rows, D, device="cuda", generator=g).to(BF16)
    return dict(qkv=qkv, idx=idx * 4, idx_t=idx_t, bias_t=table.t().contiguous(), keep0=keep0, dout=dout, D=D, rows=rows, pos1=pos1)


def kept_mask(B, n0, n1, q):
    """bool [rows]: the rows of the per-segment query prefixes q = (k0, k1)."""
    m = torch.zeros(B * (n0 + n1), dtype=torch.bool, device="cuda")
    m[:B * n0].view(B, n0)[:, :min(q[0], n0)] = True
    if n1:
        m[B * n0:].view(B, n1)[:, :min(q[1], n1)] = True
    return m


def launched_mask(B, n0, n1, pos1, q, sep):
    """bool [rows]: the rows of the 128-position query tiles that hold a kept position (what the forward may write)."""
    m = torch.zeros(B * (n0 + n1), dtype=torch.bool, device="cuda")
    kept = [p for p in range(min(q[0], n0))] + [pos1 + i for i in range(min(q[1], n1))]
    for p in range(pos1 + n1):
        if p >= n0 and p < pos1:
            continue
        org = (pos1 if p >= pos1 else 0) if sep else 0
        same_part = [k for k in kept if (not sep) or ((k >= pos1) == (p >= pos1))]
        if any((k - org) // 128 == (p - org) // 128 for k in same_part):
            if p < n0:
                m[:B * n0].view(B, n0)[:, p] = True
            else:
                m[B * n0:].view(B, n1)[:, p - pos1] = True
    return m


def run_attention(ops, L, c, seq, H, sep, q, live=None, with_dbias=True, poison=True):
    """Forward + backward of one attention call; q = None: no limit, dO zero outside `zero_outside`.  With a limit every buffer the
    kernels may not read outside the prefixes holds NaN there (out and lse: whatever the limited forward did not write; dO: the
    rows outside the prefixes), and dqkv starts as NaN, so a row that was not written or an operand that was read shows."""
    rows, D, layer = c["rows"], c["D"], 1
    kw = dict(bias_t=c["bias_t"], head_row0=layer * H, rel_index=c["idx"], rel_index_t=c["idx_t"], keep0=c["keep0"],
              mode=L.ATTN_SEPARATE if sep else L.ATTN_JOINT)
    out = torch.full((rows, D), float("nan"), device="cuda", dtype=BF16)
    lse = torch.full((H, rows), float("nan"), device="cuda")
    ops.attention_fwd(c["qkv"], out, lse, seq, H, q_keep=q, **kw)
    dout = c["dout_kept"].clone()
    if q is not None and poison:
        dout[~c["kept"]] = float("nan")
    dqkv = torch.full((rows, 3 * D), float("nan"), device="cuda", dtype=BF16)
    dbias_t = torch.zeros_like(c["bias_t"]) if with_dbias else None
    csq = [torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")]
    csv = [torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")]
    ops.attention_bwd(c["qkv"], out, dout, lse, dqkv, seq, H, dbias_t=dbias_t, dq_colsum=csq, dv_colsum=csv, row_live=live,
                      q_keep=q, **kw)
    torch.cuda.synchronize()
    return dict(out=out, lse=lse, dqkv=dqkv, dbias=dbias_t, cs=csq + csv)


def compare_attention(full, got, c, H, q, launched, same_dkv):
    """The checks of the issue: kept rows of out / lse and dQ byte-identical, dQ zero everywhere else and every row written; dK, dV,
    the column sums and the table gradient within the bounds tests/test_attention_gpu.py states for them (dK / dV: 3e-2 of the
    tensor's largest element + 3e-2 relative; column sums: 2e-2 of the largest + 0.05; table: 2e-2 + 2e-2, its float atomics arrive
    in any order), dK / dV byte-identical where `same_dkv`."""
    D, kept, layer = c["D"], c["kept"], 1
    assert float(full["dqkv"].float().abs().max()) > 0 and not bool(torch.isnan(full["dqkv"].float()).any())
    assert same_bytes(got["out"][kept], full["out"][kept]), "kept rows of out differ"
    assert same_bytes(got["lse"][:, kept], full["lse"][:, kept]), "kept rows of lse differ"
    if launched is not None:  # the other tiles were not launched: their rows still hold what they held
        assert bool(torch.isnan(got["out"][~launched].float()).all()) and bool(torch.isnan(got["lse"][:, ~launched]).all())
    assert not bool(torch.isnan(got["dqkv"].float()).any()), "a row of dqkv was not written, or an operand outside the prefix was read"
    assert same_bytes(got["dqkv"][kept][:, :D], full["dqkv"][kept][:, :D]), "dQ of kept rows differs"
    assert float(full["dqkv"][kept][:, :D].float().abs().max()) > 0
    assert bool((got["dqkv"][~kept][:, :D] == 0).all()), "dQ outside the prefix is not zero"
    assert bool((full["dqkv"][~kept][:, :D] == 0).all())  # (what the promise about dO means for the full computation)
    for name, sl in (("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        a, b = got["dqkv"][:, sl].float(), full["dqkv"][:, sl].float()
        assert float(b.abs().max()) > 0
        err = (a - b).abs()
        print("%s max err %.4g of max %.4g" % (name, float(err.max()), float(b.abs().max())))
        assert bool((err <= 3e-2 * float(b.abs().max()) + 3e-2 * b.abs()).all()), name
        if same_dkv:
            assert same_bytes(got["dqkv"][:, sl], full["dqkv"][:, sl]), name + " is not byte-identical"
    for a, w in zip(got["cs"], full["cs"]):
        assert float((a - w).abs().max()) <= 2e-2 * float(w.abs().max()) + 0.05
    assert float(sum(float(w.abs().max()) for w in full["cs"])) > 0
    if full["dbias"] is not None:
        b = full["dbias"][layer * H:(layer + 1) * H]
        err = (got["dbias"][layer * H:(layer + 1) * H] - b).abs()
        print("dbias max err %.4g of max %.4g" % (float(err.max()), float(b.abs().max())))
        assert float(b.abs().max()) > 0 and bool((err <= 2e-2 * float(b.abs().max()) + 2e-2 * b.abs()).all())
        assert float(got["dbias"][:H].abs().max()) == 0.0  # the other layer's rows untouched


def one_block_per_part(n0, n1, pos1, q, sep):
    """Does every part stream at most ONE 32-query block under the limit?  Then a key's dK / dV accumulators receive the same
    products in the same order as in the unlimited call, where the other blocks add exact zeros (dO = 0 there): byte-identical.
    With two kept blocks the order of the two depends on which wave takes the sample (the skew), and fp32 sums do not commute
    across four accumulation steps."""
    def blocks(ps):
        return len({p // 32 for p in ps})
    text, image = list(range(min(q[0], n0))), [pos1 + i for i in range(min(q[1], n1))]
    if sep:
        return blocks(text) <= 1 and blocks([p - pos1 for p in image]) <= 1
    return blocks(text + image) <= 1


# n0 = 40; n1 = 145: four full 32-position blocks and a ragged one, pos1 = 40; B = 9: one more than the eight waves
GEOM = dict(B=9, n0=40, n1=145, H=2)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("q", [(40, 0), (1, 1), (1, 0)])
@pytest.mark.parametrize("sep", [False, True])
def test_attention_query_prefix(ops, L, sep, q, mask):
    B, n0, n1, H = GEOM["B"], GEOM["n0"], GEOM["n1"], GEOM["H"]
    c = attn_case(B, n0, n1, H, seed=300 + 10 * sep + q[0] + 3 * q[1] + mask, mask=mask)
    seq = ops.Seq(B, n0, n1)
    assert c["pos1"] == 40 and seq.rows == c["rows"]
    c["kept"] = kept_mask(B, n0, n1, q)
    c["dout_kept"] = torch.where(c["kept"][:, None], c["dout"], torch.zeros_like(c["dout"]))
    assert ops.attention_qkeep_served(c["qkv"], seq, H, bias_t=c["bias_t"], head_row0=H, rel_index=c["idx"], rel_index_t=c["idx_t"],
                                      keep0=c["keep0"], mode=L.ATTN_SEPARATE if sep else L.ATTN_JOINT)
    full = run_attention(ops, L, c, seq, H, sep, None)
    got = run_attention(ops, L, c, seq, H, sep, q)
    same = one_block_per_part(n0, n1, c["pos1"], q, sep)
    assert same == (q == (1, 0) or (q == (1, 1) and sep))  # the cases whose dK / dV are asserted byte-identical
    compare_attention(full, got, c, H, q, launched_mask(B, n0, n1, c["pos1"], q, sep), same)


@pytest.mark.parametrize("sep", [False, True])
def test_attention_query_prefix_with_a_dead_sample(ops, L, sep):
    """Dead + kept compose: sample 1 is dropped (both segments in JOINT mode, the text segment in SEPARATE mode) and the text
    prefix is kept.  Its rows get zeros from either rule, every other row is as in the unlimited call with the same vector."""
    B, n0, n1, H = GEOM["B"], GEOM["n0"], GEOM["n1"], GEOM["H"]
    q = (40, 0)
    c = attn_case(B, n0, n1, H, seed=77 + sep, mask=True)
    seq = ops.Seq(B, n0, n1)
    c["kept"] = kept_mask(B, n0, n1, q)
    dead = torch.zeros(c["rows"], dtype=torch.bool, device="cuda")
    dead[1 * n0:2 * n0] = True
    if not sep:
        dead[B * n0 + n1:B * n0 + 2 * n1] = True
    live = torch.full((c["rows"],), KEEP, device="cuda")
    live[dead] = 0.0
    c["dout_kept"] = torch.where((c["kept"] & ~dead)[:, None], c["dout"], torch.zeros_like(c["dout"]))
    full = run_attention(ops, L, c, seq, H, sep, None, live=live)
    got = run_attention(ops, L, c, seq, H, sep, q, live=live)
    compare_attention(full, got, c, H, q, launched_mask(B, n0, n1, c["pos1"], q, sep), False)
    assert bool((got["dqkv"][dead] == 0).all())


@pytest.mark.parametrize("q", [(72, 0), (1, 1)])
@pytest.mark.parametrize("sep", [False, True])
def test_attention_query_prefix_outside_the_hand_placed_kernels(ops, L, sep, q):
    """72 text positions: the image positions start past the first 64-key tile, which the hand-placed forward and dQ streams do not
    cover, so attn_fwd_kernel and attn_bwd_dq_kernel run -- and honour the limit like the streams (the fused dK / dV /
    bias-gradient kernel is the same one)."""
    B, n0, n1, H = 3, 72, 65, 2
    c = attn_case(B, n0, n1, H, seed=500 + sep + q[0], mask=True)
    seq = ops.Seq(B, n0, n1)
    assert c["pos1"] == 72
    c["kept"] = kept_mask(B, n0, n1, q)
    c["dout_kept"] = torch.where(c["kept"][:, None], c["dout"], torch.zeros_like(c["dout"]))
    full = run_attention(ops, L, c, seq, H, sep, None)
    got = run_attention(ops, L, c, seq, H, sep, q)
    compare_attention(full, got, c, H, q, launched_mask(B, n0, n1, c["pos1"], q, sep), one_block_per_part(n0, n1, 72, q, sep))


def test_attention_backward_without_a_table_gradient_ignores_the_limit(ops, L):
    """No bias-table gradient asked for: the plan has the separate dK / dV kernel, which does not take the limit.  The call says so
    (attention_qkeep_served) and computes everything: on a full forward and a dO that is zero outside the prefix it returns the
    bytes of the call without the limit."""
    B, n0, n1, H = 3, 40, 145, 2
    q = (40, 0)
    c = attn_case(B, n0, n1, H, seed=9, mask=True)
    seq = ops.Seq(B, n0, n1)
    c["kept"] = kept_mask(B, n0, n1, q)
    c["dout_kept"] = torch.where(c["kept"][:, None], c["dout"], torch.zeros_like(c["dout"]))
    assert not ops.attention_qkeep_served(c["qkv"], seq, H, bias_t=c["bias_t"], head_row0=H, rel_index=c["idx"],
                                          rel_index_t=c["idx_t"], keep0=c["keep0"], with_dbias=False)
    rows, D = c["rows"], c["D"]
    kw = dict(bias_t=c["bias_t"], head_row0=H, rel_index=c["idx"], rel_index_t=c["idx_t"], keep0=c["keep0"])
    out = torch.empty(rows, D, device="cuda", dtype=BF16)
    lse = torch.empty(H, rows, device="cuda")
    ops.attention_fwd(c["qkv"], out, lse, seq, H, **kw)
    res = []
    for lim in (None, q):
        dqkv = torch.full((rows, 3 * D), float("nan"), device="cuda", dtype=BF16)
        ops.attention_bwd(c["qkv"], out, c["dout_kept"], lse, dqkv, seq, H, q_keep=lim, **kw)
        torch.cuda.synchronize()
        res.append(dqkv)
    assert float(res[0].float().abs().max()) > 0 and same_bytes(res[0], res[1])


# ---- one block ---------------------------------------------------------------------------------------------------------------------
B_, T_, I_ = 12, 40, 197  # 2 844 rows at D = 768: the 256x256 GEMM kernel (forced, as in tests/test_rowskip_gpu.py) and the 768-wide row kernels
M_ = B_ * (T_ + I_)
WEIGHTS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")


@pytest.fixture
def big_tiles(L):
    assert L.get_lib().vlm_gemm_set_big_tile_mode(2) == 0
    yield
    L.get_lib().vlm_gemm_set_big_tile_mode(-1)


_MODELS = {}


def block_model(pkg, fold):
    """A ufo model at D = 768, 12 heads (built once per LayerScale form), block 6's parameters and the table perturbed so that
    every gradient path is non-trivial (the shipped init leaves biases at zero and gammas equal)."""
    if fold in _MODELS:
        return _MODELS[fold]
    engine = importlib.import_module("vl_merging_amd.engine")
    cfgmod = importlib.import_module("vl_merging_amd.vilt.config")
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    torch.manual_seed(11)
    prev = engine._FOLD_LS
    engine._FOLD_LS = fold
    try:
        cfg = cfgmod.make_config("ufo", vit="vit_base_patch16_224", hidden_size=768, num_heads=12, vocab_size=1024,
                                 max_text_len=T_, patch_size=16, vlffn_start_layer_index=10, image_size=224, max_vl_text_len=T_,
                                 tasks=["vl"], loss_names=cfgmod._loss_names({"itm": 1}), drop_rate=0.2)
        model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg)).cuda().train()
        with torch.no_grad():
            gen = torch.Generator(device="cuda"); gen.manual_seed(5)
            for n, p in model.named_parameters():
                if n.startswith("transformer.blocks.6.") or n == "relative_position_bias_table":
                    p.add_(0.02 * torch.randn(p.shape, device="cuda", generator=gen))
        model.setup_engine()
    finally:
        engine._FOLD_LS = prev
    _MODELS[fold] = model
    return model


def block_run(pkg, fold, keep, sep, on, twice=False):
    """Forward + backward of block 6 through engine.run_block(keep=...), the kept-row path on or off (off: every row is computed,
    the kept rows are handed out and their gradient is scattered into zeros -- the full block fed a gradient that is zero outside
    the kept rows).  The injected DropPath draws drop sample 1 at the first site and sample 2 at the second."""
    engine = importlib.import_module("vl_merging_amd.engine")
    ops = importlib.import_module("vl_merging_amd.ops")
    model = block_model(pkg, fold)
    H = 12
    prev, prev_fold = engine._TAILROWS["enabled"], engine._FOLD_LS
    engine._TAILROWS["enabled"], engine._FOLD_LS = on, fold
    try:
        blk = model.transformer.blocks[6]
        keep0 = torch.ones(B_, T_, device="cuda", dtype=torch.uint8)
        keep0[3, 30:] = 0
        pc = model._pass_ctx(ops.Seq(B_, T_, I_), H, model.get_rel_pos_bias(model.vl_text_imag_relative_position_index, T_), keep0=keep0)
        pc.independent_segments = sep

        def draws(pc_, S, streams):  # kept where u < keep
            u = torch.zeros(streams, S, B_)
            u[:, 0, 1] = 0.99
            u[:, 1, 2] = 0.99
            return u

        pc.uniform_source = draws
        pc.plan_drop_path([blk.drop_path_prob, blk.drop_path_prob])
        kr = engine.KeepRows.of(pc.seq, keep)
        gen = torch.Generator(device="cuda"); gen.manual_seed(17)
        x = torch.randn(M_, 768, device="cuda", generator=gen).requires_grad_(True)
        g = torch.randn(kr.count, 768, device="cuda", generator=gen)
        model.zero_grad()
        seen = []
        real = ops.attention_fwd
        ops.attention_fwd = lambda *a, **k: (seen.append(k.get("q_keep")), real(*a, **k))[1]
        try:
            y = blk.run(x, pc, 4 if sep else 2, keep=keep)
        finally:
            ops.attention_fwd = real
        folded = engine._folded(blk.plan(4 if sep else 2, pc.seq).ranges)
        first = None
        if twice:  # a second backward over the retained graph: the table's accumulator has been taken by then
            y.backward(g, retain_graph=True)
            first, x.grad = x.grad.detach().clone(), None
        y.backward(g)
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
                 if (n.startswith("transformer.blocks.6.") or n == "relative_position_bias_table") and p.grad is not None}
        weights = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith("transformer.blocks.6.")}
        return dict(y=y.detach().clone(), dx=x.grad.detach().clone(), grads=grads, w=weights, fold=folded, q=seen, rows=kr.count, first=first)
    finally:
        engine._TAILROWS["enabled"], engine._FOLD_LS = prev, prev_fold


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("keep,sep", [((T_, 0), False), ((1, 1), True)])
def test_block_with_kept_rows(pkg, big_tiles, keep, sep, fold):
    """x2 of the kept rows byte-identical (the forward of a kept row runs the same kernels on the same operands: a GEMM row does not
    depend on the launch's other rows).  Gradients: the bounds of tests/test_rowskip_gpu.py's block test, which are those of
    tests/test_wgrad_batch_gpu.py -- weight gradients rtol 1e-3 and atol 2e-3 sqrt(rows), column-sum gradients and the bias table
    1e-4 of the tensor's largest element, a folded gamma with the wgrad bound carried through dgamma[n] = sum_k W[n,k] raw_w[n,k] +
    b[n] raw_b[n]; the q / v bias gradients are column-sum gradients like the others (dQ rows are byte-identical or zero, only the
    order of the atomics differs).  dx is byte-identical, as there, where every part streams ONE kept query block ((1, 1), SEPARATE:
    dK / dV, and with them dqkv, receive the same products in the same order).  In the (T, 0) JOINT case dK / dV sum two kept blocks
    in an order that depends on the wave (tests above), an order-of-summation difference in fp32 ahead of a bf16 store: dx is held
    to the bound this file's sources state for such a difference, 1e-4 of the tensor's largest element.  The measured figure is
    printed."""
    on, off = block_run(pkg, fold, keep, sep, True), block_run(pkg, fold, keep, sep, False)
    assert on["fold"] == off["fold"] == fold
    assert on["q"] == [keep] and off["q"] == [None]  # the kept-row path ran with the limit, the other one computed everything
    assert on["y"].shape == (on["rows"], 768) and same_bytes(on["y"], off["y"]), "x2 of the kept rows differs"
    b = off["dx"]
    err = (on["dx"] - b).abs()
    print("dx max err %.4g of max %.4g (bound %.4g)" % (float(err.max()), float(b.abs().max()), 1e-4 * float(b.abs().max())))
    assert float(b.abs().max()) > 0
    if one_block_per_part(T_, I_, T_, keep, sep):
        assert torch.equal(on["dx"], off["dx"]), "dx differs"  # (==, as tests/test_rowskip_gpu.py asserts it)
    else:
        assert float(err.max()) <= 1e-4 * float(b.abs().max()), "dx"
    w = on["w"]
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


def test_second_backward_over_a_retained_graph(pkg, big_tiles):
    """The forward ran with the limit, so rows of out, lse and dO outside the prefix were never written; a second backward finds the
    bias table's accumulator gone and must still run the plan that honours the limit: its dx is the first one's."""
    r = block_run(pkg, True, (T_, 0), False, True, twice=True)
    assert r["q"] == [(T_, 0)] and bool(torch.isfinite(r["dx"]).all()) and float(r["dx"].abs().max()) > 0
    assert torch.equal(r["dx"], r["first"])


# ---- the model -------------------------------------------------------------------------------------------------------------------
def tiny_model(pkg, golden_dir, arch):
    from oracle.detweights import det_array
    cfgmod = importlib.import_module("vl_merging_amd.vilt.config")
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    cfg = cfgmod.make_config(arch, vit="vit_tiny_patch16_224", hidden_size=192, num_heads=3, vocab_size=1024, max_text_len=40,
                             patch_size=16, vlffn_start_layer_index=10, image_size=224, max_vl_text_len=40, tasks=["vl"],
                             loss_names=cfgmod._loss_names({"itm": 1, "mlm": 1, "ifm": 1}))
    model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg))
    meta = json.load(open(os.path.join(golden_dir, "keys_tiny_%s.json" % arch)))
    sd = {k: torch.from_numpy(det_array(k, s)) for k, (s, dt) in meta.items()
          if dt.startswith("float") and "index" not in k and "mask_for" not in k and not k.startswith(("train_", "val_"))}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    model = model.cuda().train()
    model.setup_engine()
    return model


def grad_norm_ok(got, ref):
    """tests/test_model_gpu.py's rule for a tensor's gradient norm: 2.5 %; 20 % where the norm is <= 0.05; 2.5e-4 absolute."""
    rel = abs(got - ref) / (ref + 1e-12)
    return rel <= 2.5e-2 or (ref <= 0.05 and rel <= 0.20) or abs(got - ref) <= 2.5e-4


@pytest.mark.parametrize("arch", ["ufo", "all_moe"])
def test_training_step_with_and_without_kept_rows(pkg, engine, golden_dir, arch):
    """One train-mode training_step + backward from one seed, kept rows on and off: the same losses (the existing train tests allow
    3e-2 per loss; the forward of a kept row is bit-equal, so they are expected equal and that is printed), every parameter's
    gradient norm by tests/test_model_gpu.py's rule, the same DropPath draws in number, order and shape, and the restricted reads
    really reached the last blocks."""
    from oracle.detweights import det_batch
    model = tiny_model(pkg, golden_dir, arch)
    nb = det_batch(4, 224, 40, 1024, seed=5)
    batch = {k: torch.from_numpy(v).cuda() for k, v in nb.items()}
    batch["image"] = [batch["image"]]
    ops = importlib.import_module("vl_merging_amd.ops")
    res = {}
    prev = engine._TAILROWS["enabled"]
    try:
        for on in (True, False):
            engine._TAILROWS["enabled"] = on
            draws, limits = [], []

            def source(pc, S, streams):
                draws.append((streams, S, pc.seq.B))
                return torch.rand(streams, S, pc.seq.B)

            model.droppath_uniform_source = source
            real = ops.attention_fwd
            ops.attention_fwd = lambda *a, **k: (limits.append(k.get("q_keep")), real(*a, **k))[1]
            torch.manual_seed(1234)
            model.zero_grad()
            try:
                loss = model.training_step({"vl": dict(batch)}, 0)
            finally:
                ops.attention_fwd = real
            loss.backward()
            torch.cuda.synchronize()
            res[on] = dict(loss=float(loss), draws=draws, limits=[q for q in limits if q is not None],
                           grads={n: p.grad.detach().float().norm().item() for n, p in model.named_parameters() if p.grad is not None},
                           touched=set(model._flat.touched))
    finally:
        engine._TAILROWS["enabled"] = prev
        model.droppath_uniform_source = None
    on, off = res[True], res[False]
    print("loss with kept rows %.9g, without %.9g, equal: %s" % (on["loss"], off["loss"], on["loss"] == off["loss"]))
    assert math.isfinite(off["loss"]) and abs(on["loss"] - off["loss"]) <= 3e-2
    assert on["draws"] == off["draws"] and len(on["draws"]) == 2
    # the pair pass: the x path's and the VL-FFN path's last block; the fused 4B pass: its last block.  (all_moe: the x path's last
    # block has one expert per modality, two groups of B gathered rows -- that one computes every row)
    if arch == "ufo":
        assert sorted(on["limits"]) == [(1, 1), (1, 1), (40, 0)]
    else:
        assert (40, 0) in on["limits"] and (1, 1) in on["limits"] and len(on["limits"]) <= 3
    assert off["limits"] == []
    assert on["touched"] == off["touched"] and sorted(on["grads"]) == sorted(off["grads"])
    bad = [(n, on["grads"][n], off["grads"][n]) for n in on["grads"] if not grad_norm_ok(on["grads"][n], off["grads"][n])]
    assert not bad, bad[:5]
    assert sum(1 for v in off["grads"].values() if v > 0) > 100
    # the default read is every row
    model.eval()
    with torch.no_grad():
        full = model.infer(dict(batch))
        text_only = model.infer(dict(batch), reads="text")
    assert full["image_feats"] is not None and full["image_feats"].shape[:2] == (4, 197) and text_only["image_feats"] is None
    assert full["text_feats"].shape == text_only["text_feats"].shape == (4, 40, 192)
    # nothing is differentiated here, so the forward's limit needs no backward plan: the last block ran on the text rows alone
    # and gave them the bytes of the full pass
    assert same_bytes(full["text_feats"], text_only["text_feats"]) and same_bytes(full["cls_feats"], text_only["cls_feats"])
    limits = []
    real = ops.attention_fwd
    ops.attention_fwd = lambda *a, **k: (limits.append(k.get("q_keep")), real(*a, **k))[1]
    try:
        with torch.no_grad():
            model.infer(dict(batch), reads="text")
    finally:
        ops.attention_fwd = real
    assert [q for q in limits if q is not None] == [(40, 0)]
