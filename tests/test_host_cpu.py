"""Host logic on CPU: config grammar, module tree / state_dict key parity with the reference, index buffers
bit-exact, optimizer grouping, loud failure without a GPU."""
import importlib
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def cfgmod(pkg):
    return importlib.import_module("vl_merging_amd.vilt.config")


@pytest.fixture(scope="module")
def vm(pkg):
    return importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")


def tiny_cfg(cfgmod, arch, **over):
    base = dict(vit="vit_tiny_patch16_224", hidden_size=192, num_heads=3, vocab_size=1024, max_text_len=40,
                patch_size=16, vlffn_start_layer_index=10, image_size=224)
    base.update(over)
    return cfgmod.make_config(arch, **base)


def test_cli_grammar_later_wins(cfgmod):
    c = cfgmod.parse_cli(["with", "task_mlm_itm_ifm_square_randaug_base_vl", "step200k", "all_moe", "per_gpu_batchsize=22",
                          "image_size=384", "loss_names.itm=0", "log_dir=/tmp/x"])
    assert c["max_steps"] == 200000 and c["warmup_steps"] == 2500 and c["use_moe"] and c["in_attn"]
    assert c["per_gpu_batchsize"] == 22 and c["image_size"] == 384 and c["loss_names"]["itm"] == 0
    assert c["log_dir"] == "/tmp/x" and c["vlffn_start_layer_index"] == 10
    with pytest.raises(KeyError):
        cfgmod.parse_cli(["no_such_config"])
    with pytest.raises(KeyError):
        cfgmod.parse_cli(["not_a_key=1"])


@pytest.mark.parametrize("arch,tag,losses", [("ufo", "tiny_ufo", {"itm": 1, "mlm": 1, "ifm": 1}),
                                             ("all_moe", "tiny_all_moe", {"itm": 1, "mlm": 1, "ifm": 1}),
                                             ("ufo", "tiny_irtr_ufo", {"irtr": 1, "itm": 0, "mlm": 0, "ifm": 0}),
                                             ("all_moe", "tiny_irtr_all_moe", {"irtr": 1, "itm": 0, "mlm": 0, "ifm": 0})])
def test_state_dict_keys_match_reference(cfgmod, vm, golden_dir, arch, tag, losses):
    meta = json.load(open(os.path.join(golden_dir, f"keys_{tag}.json")))
    # metric accumulators (torchmetrics states; not persistent in real checkpoints) are an artefact of the harness stub
    meta = {k: v for k, v in meta.items() if not k.startswith(("train_", "val_"))}
    cfg = tiny_cfg(cfgmod, arch, max_vl_text_len=40 if "irtr" not in tag else None,
                   loss_names=cfgmod._loss_names(losses))
    model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg))
    sd = model.state_dict()
    mine = {k: (list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in sd.items()}
    # transformers 4.x (what the reference's checkpoints were written with) keeps position_ids persistent
    extra = set(mine) - set(meta)
    assert extra <= {"text_embeddings.position_ids"}, extra
    assert not (set(meta) - set(mine)), set(meta) - set(mine)
    for k in meta:
        assert mine[k] == (meta[k][0], meta[k][1]), (k, mine[k], meta[k])
    assert sum(p.numel() for p in model.parameters()) == sum(
        int(np.prod(s)) for k, (s, dt) in meta.items() if k in dict(model.named_parameters()))


def test_index_buffers_bit_exact(vm, golden_dir):
    z = np.load(os.path.join(golden_dir, "index_buffers.npz"))
    # 480: README.md:194-223 of the reference runs VQA with image_size=480 (a 30 x 30 window on the 384 ViT, N = 941)
    for tag, g in (("224", 14), ("384", 24), ("480", 30)):
        idx, nrel, _, allrel = vm.build_relative_position_indices((g, g), 40, 196, 40)
        assert nrel == (2 * g - 1) ** 2 + 3 and allrel == nrel + 392 + 2
        for k, v in idx.items():
            ref = z[f"{k}_{tag}"]
            assert v.numpy().dtype == ref.dtype and v.numpy().tobytes() == ref.tobytes(), (k, tag)


def test_kernel_index_coordinates(vm):
    idx, *_ = vm.build_relative_position_indices((4, 4), 6, 196, None)
    m, mt = vm._index16(idx["text_imag_relative_position_index"], 6)
    assert m.dtype == torch.int16 and m.shape[1] % 4 == 0 and m.shape == mt.shape
    pos = torch.cat([torch.arange(6), 8 + torch.arange(17)])
    assert torch.equal(m[pos][:, pos].long(), 4 * idx["text_imag_relative_position_index"].long())
    assert torch.equal(mt[pos][:, pos].long(), 4 * idx["text_imag_relative_position_index"].long().t())


def test_gpu_only_is_loud(cfgmod, vm):
    cfg = tiny_cfg(cfgmod, "ufo")
    model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg))
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        model.setup_engine()
    batch = {"text_ids": torch.zeros(1, 40, dtype=torch.long), "text_labels": torch.zeros(1, 40, dtype=torch.long),
             "text_masks": torch.ones(1, 40, dtype=torch.long), "image": [torch.zeros(1, 3, 224, 224)]}
    with pytest.raises(L.VlmError):
        model.infer(batch)


def test_param_groups_follow_reference_rule(pkg):
    vu = importlib.import_module("vl_merging_amd.vilt.modules.vilt_utils")
    heads = vu.head_names(dict(all_mlp_mult=False, all_vl_mult=False, all_v_mult=False, all_l_mult=False))
    g = lambda n: vu.param_group_of(n, heads)  # noqa: E731
    assert g("transformer.blocks.0.attn.qkv.weight") == 0
    assert g("transformer.blocks.0.attn.q_bias") == 1          # contains "bias"
    # reference quirk kept: "norm1.v.weight" matches neither "norm1.weight" nor "norm.v.weight" -> it IS decayed
    assert g("transformer.blocks.3.norm1.v.weight") == 0
    assert g("transformer.blocks.3.norm1.v.bias") == 1
    assert g("transformer.blocks.3.norm1.weight") == 1
    assert g("transformer.blocks.0.gamma_1") == 0
    assert g("text_embeddings.LayerNorm.weight") == 1
    assert g("relative_position_bias_table") == 1               # the substring "bias" matches (reference quirk)
    assert g("mlm_score.bias") == 1
    lam = [vu.polynomial_decay_lambda(s, 10, 110, 1e-4) for s in (0, 5, 10, 60, 110, 200)]
    assert lam[0] == 0 and lam[1] == 0.5 and lam[2] == 1.0 and abs(lam[3] - 0.5) < 1e-12 and lam[4] == 0 and lam[5] == 0


def test_flat_params_qkv_bias_view():
    """FlatParams lays q_bias | zero gap | v_bias out back to back so cat(q_bias, 0, v_bias) (vision_transformer.py:335)
    is a view; the gap is part of q_bias' extent (optimizer ranges and DDP buckets stay contiguous)."""
    import torch
    import importlib
    import __graft_entry__ as ge
    ge.import_package()
    engine = importlib.import_module("vl_merging_amd.engine")

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.proj_bias = torch.nn.Parameter(torch.randn(128))
            self.q_bias = torch.nn.Parameter(torch.randn(128))
            self.v_bias = torch.nn.Parameter(torch.randn(128))
            self.w = torch.nn.Parameter(torch.randn(8, 8))

    top = torch.nn.Module()
    top.attn = Attn()
    m = top.attn
    q0, v0 = m.q_bias.detach().clone(), m.v_bias.detach().clone()
    flat = engine.FlatParams(top, order_key=lambda n: n)
    oq, kq = flat.offsets["attn.q_bias"]
    ov, _ = flat.offsets["attn.v_bias"]
    assert ov == oq + 2 * kq and flat.extent["attn.q_bias"] == 2 * kq
    view = m.q_bias._vlm_qkv_bias
    assert view.data_ptr() == m.q_bias.data_ptr() and view.numel() == 3 * kq
    assert torch.equal(view, torch.cat([q0, torch.zeros(128), v0]))
    assert flat.slice_of(["attn.q_bias"]) == (oq, oq + 2 * kq)


def test_param_groups_and_schedule_match_reference_set_schedule(pkg, cfgmod, vm, golden_dir):
    """The reference's own set_schedule (vilt_utils.py:225-359) on tiny models (tests/golden/schedule_groups.json, made by
    make_golden.py schedule): which parameter name lands in which of the four groups, each group's weight decay and
    learning rate, and the lr factor of the polynomial schedule at chosen steps (int and fractional warm-up, lr_mult,
    all_mlp_mult / all_vl_mult, decay_power 1 and 2, end_lr)."""
    import json
    vu = importlib.import_module("vl_merging_amd.vilt.modules.vilt_utils")
    gold = json.load(open(os.path.join(golden_dir, "schedule_groups.json")))
    assert set(gold) == {"pretrain_all_moe", "vqa_ufo_mult", "irtr_all_moe_vlmult"}
    for tag, g in gold.items():
        over = dict(g["config"])
        cfg = cfgmod.make_config(g["arch"], vit="vit_tiny_patch16_224", hidden_size=192, num_heads=3, vocab_size=64,
                                 max_text_len=40, patch_size=16, vlffn_start_layer_index=10, image_size=224,
                                 vqav2_label_size=37, loss_names=cfgmod._loss_names(g["loss_names"]), **over)
        model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg))
        heads = vu.head_names(cfg)
        mine = [[], [], [], []]
        for n, _ in model.named_parameters():
            mine[vu.param_group_of(n, heads)].append(n)
        spec = vu.group_spec(cfg)
        for gi, ref in enumerate(g["groups"]):
            assert sorted(mine[gi]) == ref["names"], (tag, gi, sorted(set(mine[gi]) ^ set(ref["names"]))[:6])
            assert spec[gi][0] == ref["weight_decay"] and abs(spec[gi][1] - ref["initial_lr"]) <= 1e-18, (tag, gi)
        lam = vu.schedule_lambda(cfg, cfg["max_steps"])
        for s_, want in zip(g["steps"], g["lr_factor"]):
            assert abs(lam(s_) - want) <= 1e-15, (tag, s_, lam(s_), want)


def test_modify_checkpoint_vlmo_matches_reference(cfgmod, vm, golden_dir):
    """A 224^2 checkpoint into a 384^2 model (vilt_module.py:749-806): bicubic 27x27 -> 47x47 resize of the table body,
    tail rows carried over, text positions truncated, index buffers dropped -- bit for bit what the reference's
    modify_checkpoint_vlmo returns on the same input (tests/golden/vlmo_resize.npz: sha256 of every tensor, sampled rows)."""
    import hashlib
    import json
    import sys
    sys.path.insert(0, golden_dir)
    from make_golden import vlmo_ckpt_inputs  # inputs only (seed-derived), no reference import at module scope
    gold = np.load(os.path.join(golden_dir, "vlmo_resize.npz"))
    cfg = cfgmod.make_config("ufo", vit="vit_base_patch16_384", hidden_size=768, num_heads=12, vocab_size=64,
                             max_text_len=40, patch_size=16, vlffn_start_layer_index=10, image_size=384,
                             loss_names=cfgmod._loss_names({"irtr": 1}))
    model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg))
    sd = {k: torch.from_numpy(v) for k, v in vlmo_ckpt_inputs().items()}
    res = model.modify_checkpoint_vlmo({"state_dict": sd})
    assert sorted(res.keys()) == json.loads(str(gold["__keys__"]))
    for k, v in res.items():
        a = np.ascontiguousarray(v.contiguous().numpy())
        assert list(a.shape) == list(gold[k + "/shape"]), k
        if k == "relative_position_bias_table":
            np.testing.assert_array_equal(a[::97], gold[k + "/rows"])
        assert hashlib.sha256(a.tobytes()).hexdigest() == str(gold[k + "/sha256"]), k


def test_reference_artefacts_load(tmp_path, cfgmod, vm):
    """The reference's own files are pickles of non-tensor objects: cache_gram_matrices.py saves a defaultdict(float)
    (:349), Lightning checkpoints carry hyper-parameter objects.  torch >= 2.6 refuses those under its weights_only
    default; the loaders here (checkpoint.load_file) read them."""
    import collections
    import types
    ck = importlib.import_module("vl_merging_amd.checkpoint")
    grams = collections.defaultdict(float)
    grams["transformer.blocks.0.attn.v"] += torch.eye(4, dtype=torch.float64)
    gp = os.path.join(tmp_path, "grams.pth")
    torch.save(grams, gp)
    with pytest.raises(Exception):
        torch.load(gp, map_location="cpu", weights_only=True)
    back = ck.load_file(gp)
    assert isinstance(back, collections.defaultdict) and torch.equal(back["transformer.blocks.0.attn.v"], torch.eye(4, dtype=torch.float64))
    cp = os.path.join(tmp_path, "model.ckpt")
    torch.save({"state_dict": {"w": torch.ones(3)}, "hyper_parameters": types.SimpleNamespace(config={"a": 1}),
                "callbacks": {collections.OrderedDict: 1}}, cp)
    assert torch.equal(ck.load_ckpt(cp)["w"], torch.ones(3))
    assert torch.equal(ck.load_file(cp)["state_dict"]["w"], torch.ones(3))


def test_every_named_config_of_the_reference_key_for_key(pkg):
    """config.py:25-711 of the reference: the default config and all 30 named configs, each entry equal to what the reference's
    own sacred functions produce (tests/golden/named_configs.json, written by `make_golden.py configs` from /root/reference)."""
    import json
    C = importlib.import_module("vl_merging_amd.vilt.config")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "named_configs.json")) as f:
        gold = json.load(f)
    assert C.default_config() == gold["default"]
    assert sorted(C.NAMED_CONFIGS) == sorted(gold["named"]) and len(gold["named"]) == 30
    for name, want in gold["named"].items():
        assert C.NAMED_CONFIGS[name]() == want, name
        merged = dict(gold["default"])
        merged.update(want)
        assert C.make_config(name) == merged, name
    # the README's merged-model evaluations (README.md:205-231) parse: later words win, like sacred
    cfg = C.parse_cli(["with", "task_finetune_vqa_square_randaug_base_image384_ufo", "ufo", "image_size=480", "merge_weights=True"])
    assert cfg["loss_names"]["vqa"] == 1 and cfg["use_ufo"] and cfg["image_size"] == 480 and cfg["lr_mult"] == 10


# ---- round 6: the host-side pieces around the front-end / head kernels (their CPU behaviour and dispatch rules) ---------------
def test_round6_host_fallbacks_and_dispatch_rules(pkg, cfgmod, vm):
    """What the one-launch paths fall back to, and when they refuse to engage, without a GPU:
    feature_views / row_range are plain views on CPU (values and autograd as the slices they replace); weighted_sum is the torch
    expression; the fused hard-negative draw engages only on CUDA (and never when torch.multinomial has been replaced); the text
    front end declines (TextSpec None) for CPU parameters or a replaced dropout module; an op called with CPU tensors raises."""
    engine = importlib.import_module("vl_merging_amd.engine")
    ops = importlib.import_module("vl_merging_amd.ops")
    L = importlib.import_module("vl_merging_amd._lib")
    obj = importlib.import_module("vl_merging_amd.vilt.modules.objectives")
    B, T, I, D = 2, 5, 3, 8
    x = torch.randn(B * T + B * I, D, requires_grad=True)
    text, image, tcls, icls = engine.feature_views(x, B, T, I)
    assert torch.equal(text, x[: B * T].view(B, T, D)) and torch.equal(image, x[B * T:].view(B, I, D))
    assert torch.equal(tcls, text[:, 0]) and torch.equal(icls, image[:, 0])
    (tcls.sum() * 2 + icls.sum()).backward()
    want = torch.zeros_like(x)
    want[0:B * T:T] = 2.0
    want[B * T::I] = 1.0
    assert torch.equal(x.grad, want)
    t = torch.randn(4, 3, 8, requires_grad=True)
    r = engine.row_range(t, 1, None)
    assert torch.equal(r, t[1:])
    r.sum().backward()
    assert float(t.grad[0].abs().max()) == 0.0 and float((t.grad[1:] - 1).abs().max()) == 0.0
    a, b = torch.tensor(1.5, requires_grad=True), torch.tensor(-2.0, requires_grad=True)
    s = engine.weighted_sum([a, b], [0.5, 2.0])
    assert abs(float(s.detach()) - (0.75 - 4.0)) < 1e-6
    s.backward()
    assert float(a.grad) == 0.5 and float(b.grad) == 2.0
    assert float(engine.weighted_sum([a.detach(), b.detach()])) == -0.5
    # the hard-negative draw on CPU: the torch formulation (own pair never drawn, forced choice at n = 2)
    sim = torch.randn(6, 6)
    for _ in range(5):
        ni, nt = obj._draw_negatives(sim, sim.t(), 6)
        assert bool((ni != torch.arange(6)).all()) and bool((nt != torch.arange(6)).all())
    two = torch.randn(2, 2)
    ni, nt = obj._draw_negatives(two, two.t(), 2)
    assert ni.tolist() == [1, 0] and nt.tolist() == [1, 0]
    # the text front end declines on CPU and for a replaced dropout
    cfg = tiny_cfg(cfgmod, "ufo")
    model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg))
    ids = torch.zeros(2, 40, dtype=torch.long)
    assert model._text_spec(ids) is None
    model.text_embeddings.dropout = torch.nn.Identity()
    assert model._text_spec(ids) is None
    # ops refuse CPU tensors loudly (no CPU fallback of a kernel)
    for call in (lambda: ops.tanh_fwd(torch.zeros(2, 8, dtype=torch.bfloat16)),
                 lambda: ops.scatter_rows(4, 8, torch.float32, [(torch.zeros(1, 8), 0, 1)], torch.device("cpu")),
                 lambda: ops.weighted_sum([torch.zeros(())], [1.0]),
                 lambda: ops.sample_negatives(sim, sim, 6, torch.rand(2, 6))):
        with pytest.raises(L.VlmError):
            call()


def test_pass_ends_keep_no_settled_switch_and_no_private_cache(pkg, cfgmod, vm, monkeypatch):
    """The two retired A/B switches are gone from the package (their records live in docs/experiments.md), the objectives
    reach the engine through public names only, ops keeps ONE scratch cache, and the environment no longer decides whether
    the unimodal passes are fused: fuse_unimodal_passes is a plain attribute, True by default."""
    engine = importlib.import_module("vl_merging_amd.engine")
    ops = importlib.import_module("vl_merging_amd.ops")
    root = os.path.dirname(os.path.abspath(pkg.__file__))
    gone = (b"VLM_FUSED_LOSS", b"VLM_FUSE_UNIMODAL", b"_FUSED_LOSS")
    seen = 0
    for d, dirs, files in os.walk(root):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        for f in files:
            data = open(os.path.join(d, f), "rb").read()
            seen += 1
            for word in gone:
                assert word not in data, (os.path.join(d, f), word)
    assert seen > 20
    src = open(os.path.join(root, "vilt", "modules", "objectives.py")).read()
    assert "engine._" not in src
    for name in ("_SPLITK_WS", "_ROW_WS", "_FRONT_WS", "_splitk_workspace", "_row_workspace", "_front_ws"):
        assert not hasattr(ops, name), name
    for name in ("_FUSED_LOSS", "_WVEC", "_KEEPS_CACHE"):
        assert not hasattr(engine, name), name
    monkeypatch.setenv("VLM_FUSE_UNIMODAL", "0")
    monkeypatch.setenv("VLM_FUSED_LOSS", "0")
    cfg = tiny_cfg(cfgmod, "ufo")
    model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg))
    assert model.fuse_unimodal_passes is True and model.fuse_joint_passes is True
    assert not hasattr(model, "_ones_cache")


def test_const_cache_is_bounded_and_zero_scalar_stays(pkg, monkeypatch):
    """engine.const builds a key's tensor once, holds at most CONST_MAX entries and drops the one that has been in longest;
    the placeholder zero of _TableT.backward lives outside it (one tensor per device, whatever is evicted)."""
    engine = importlib.import_module("vl_merging_amd.engine")
    monkeypatch.setattr(engine, "_CONSTS", {})
    built = []

    def make(i):
        def build():
            built.append(i)
            return torch.full((), float(i))
        return build

    z = engine._zero_scalar(torch.device("cpu"))
    first = engine.const(("k", 0), make(0))
    assert engine.const(("k", 0), make(0)) is first and built == [0]
    for i in range(1, engine.CONST_MAX + 3):
        assert float(engine.const(("k", i), make(i))) == i
    assert len(engine._CONSTS) == engine.CONST_MAX
    assert ("k", 0) not in engine._CONSTS and ("k", 2) not in engine._CONSTS and ("k", 3) in engine._CONSTS
    assert engine.const(("k", 0), make(0)) is not first and built[-1] == 0  # rebuilt after its eviction
    assert engine._zero_scalar(torch.device("cpu")) is z


def test_rows2d_matches_the_five_forms_it_replaced(pkg):
    """engine._rows2d(g, D, dtypes, contiguous) against the inline forms the backward functions used to carry, on every layout
    and dtype that tells them apart: same dtype, shape and strides, and a copy exactly where they made one."""
    engine = importlib.import_module("vl_merging_amd.engine")
    BF16, F32 = torch.bfloat16, torch.float32

    def old_rows2d(g, D):  # _FeatureViewsFn / _RowRangeFn / _LinearFn.backward
        g2 = g.reshape(-1, D)
        if g2.dtype not in (BF16, F32):
            g2 = g2.float()
        return g2 if g2.stride(1) == 1 else g2.contiguous()

    def old_l2norm(g, D):
        g2 = g.reshape(-1, D)
        return g2.float().contiguous() if g2.dtype != F32 or not g2.is_contiguous() else g2

    def old_layernorm(g, D):
        g2 = g.reshape(-1, D).contiguous()
        return g2 if g2.dtype in (BF16, F32) else g2.float()

    def old_front(g, D):  # _EmbeddingFn.backward / _PassRowsFn.backward
        g2 = g.reshape(-1, D)
        return g2.float().contiguous() if g2.dtype != F32 or g2.stride(1) != 1 else g2

    forms = ((old_rows2d, {}), (old_l2norm, dict(dtypes=(F32,), contiguous=True)), (old_layernorm, dict(contiguous=True)),
             (old_front, dict(dtypes=(F32,))))
    D = 8
    base = torch.randn(6, 2 * D)
    layouts = {"contiguous": lambda t: t[:, :D].contiguous(), "row-strided": lambda t: t[:, :D], "column-strided": lambda t: t[:, ::2],
               "transposed": lambda t: t[:, :D].contiguous().t().contiguous().t(), "3-d": lambda t: t[:, :D].contiguous().view(2, 3, D),
               "broadcast": lambda t: t[:1, :D].expand(6, D)}
    for dt in (F32, BF16, torch.float16, torch.float64):
        for lname, lay in layouts.items():
            g = lay(base.to(dt))
            for old, kw in forms:
                want, got = old(g, D), engine._rows2d(g, D, **kw)
                what = (old.__name__, lname, dt)
                assert got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride(), what
                assert (got.data_ptr() == g.data_ptr()) == (want.data_ptr() == g.data_ptr()), what
                assert torch.equal(got, want), what


def test_epilogue_builder_checks_in_the_old_order(pkg):
    """ops._epilogue (shared by gemm and gemm_grouped) fills vlm_epilogue_t and raises what the two used to raise, in their
    order: a strided residual / aux before a short col_sum before a wrong dtype, the dtypes in the order bias .. col_sum."""
    ops = importlib.import_module("vl_merging_amd.ops")
    L = importlib.import_module("vl_merging_amd._lib")
    N = 8
    f32, bf = torch.zeros(4, N), torch.zeros(4, N, dtype=torch.bfloat16)
    vec = torch.zeros(N)
    e = ops._epilogue(N, bias=vec, residual=f32[:, :4], aux=bf, act=L.ACT_GELU, alpha=0.5, accumulate=True, col_sum=vec)
    assert (e.bias, e.col_sum, e.residual, e.ld_res, e.aux, e.ld_aux) == (vec.data_ptr(), vec.data_ptr(), f32.data_ptr(), N, bf.data_ptr(), N)
    assert (e.act, e.alpha, e.accumulate, e.col_scale, e.row_scale, e.col_sum_ws, e.splitk_ws) == (L.ACT_GELU, 0.5, 1, None, None, None, None)
    e = ops._epilogue(N)
    assert (e.bias, e.residual, e.ld_res, e.aux, e.ld_aux, e.act, e.alpha, e.accumulate, e.col_sum) == (None, None, 0, None, 0, L.ACT_NONE, 1.0, 0, None)
    for kw, msg in ((dict(residual=f32[:, ::2], col_sum=vec[:4], bias=bf[0]), "unit inner stride"),
                    (dict(aux=bf[:, ::2], col_sum=vec[:4]), "unit inner stride"),
                    (dict(col_sum=vec[:4], bias=bf[0]), "col_sum must be"),
                    (dict(col_sum=torch.zeros(2 * N)[::2], aux=f32), "col_sum must be"),
                    (dict(bias=bf[0], aux=f32), "dtype torch.bfloat16, expected torch.float32"),
                    (dict(aux=f32, col_sum=vec.double()), "dtype torch.float32, expected torch.bfloat16"),
                    (dict(col_sum=vec.double()), "dtype torch.float64, expected torch.float32")):
        with pytest.raises(L.VlmError, match=msg):
            ops._epilogue(N, **kw)


def test_table_transpose_keeps_broadcast_gradients(pkg):
    """_TableT.backward drops only _BlockFn's placeholder (an expanded engine._zero_scalar); a genuine broadcast gradient
    of the transposed table, such as the one of bias_t.sum(), reaches the table."""
    engine = importlib.import_module("vl_merging_amd.engine")
    table = torch.randn(7, 6, requires_grad=True)
    rp = engine.make_relpos(table, None, None)
    rp.bias_t.sum().backward()
    assert table.grad is not None and torch.equal(table.grad, torch.ones(7, 6))
    # the placeholder carries nothing: only what the attention kernels accumulated in the holder arrives
    table.grad = None
    rp = engine.make_relpos(table, None, None)
    rp.holder["dbias_t"].fill_(2.0)
    rp.bias_t.backward(engine._zero_scalar(table.device).expand_as(rp.bias_t))
    assert torch.equal(table.grad, torch.full((7, 6), 2.0))


def test_big_tile_mode_range(pkg):
    """vlm_gemm_set_big_tile_mode takes 0..2 and -1 (back to the default, by shape); the removed tail-split mode 3 is an
    argument error.  Host state only: no GPU needed."""
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = L.get_lib()
    try:
        for mode in (0, 2, 1, -1):
            assert lib.vlm_gemm_set_big_tile_mode(mode) == 0, mode
        for mode in (3, -2):
            assert lib.vlm_gemm_set_big_tile_mode(mode) == -1, mode  # VLM_ERR_ARG
    finally:
        lib.vlm_gemm_set_big_tile_mode(-1)


def test_attention_bwd_workspace_size(pkg):
    """vlm_attention_bwd_ws_floats launches nothing and states one size per geometry, whatever `with_dbias` says: H * rows
    (delta) when there is no bias or the fused dK / dV / bias-gradient kernel's panel fits LDS (at most 1 024 positions in a
    part), 3 * H * rows (delta | nstat for the 16-wave bias-gradient kernel) when it does not.  Dummy non-null pointers, filled
    the way ops._attn_desc fills the descriptor.  Host arithmetic only: no GPU needed."""
    import ctypes
    L = importlib.import_module("vl_merging_amd._lib")
    ops = importlib.import_module("vl_merging_amd.ops")
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = L.get_lib()

    def size(B, n0, n1, H, mode, bias=True, with_dbias=0):
        seq = ops.Seq(B, n0, n1)
        NP = seq.pos1 + n1
        d = L.AttnDesc()
        d.qkv, d.ld_qkv, d.H, d.total_rows = 0x10000, 3 * H * 64, H, seq.rows
        if bias:
            d.R, d.bias_t = 300, 0x20000
            d.rel_index, d.ld_index, d.index_rows = 0x30000, (NP + 3) // 4 * 4, NP
            d.rel_index_t, d.ld_index_t, d.index_t_rows = 0x40000, (NP + 3) // 4 * 4, NP
            d.bias_dense, d.bias_dense_t = 0x50000, 0x60000
            d.dense_tiles = lib.vlm_bias_dense_bytes(n0, n1, seq.pos1, mode) // 4096
        d.mode = mode
        d.B, d.n0, d.n1, d.base0, d.base1, d.pos1 = seq.B, seq.n0, seq.n1, seq.base0, seq.base1, seq.pos1
        d.scale = 0.125
        return lib.vlm_attention_bwd_ws_floats(ctypes.byref(d), with_dbias), H * seq.rows

    for mode in (L.ATTN_JOINT, L.ATTN_SEPARATE):
        for B, n0, n1, H, bias, factor in ((22, 40, 577, 12, True, 1),     # 617 joint positions: the panel fits
                                           (2, 40, 901, 2, True, 1),       # 941 (480^2): fits with four waves
                                           (2, 40, 984, 2, True, 1),       # exactly 1 024 positions
                                           (1, 8, 1040, 1, True, 3),       # 1 048 joint / 1 040 image positions in one part: it does not
                                           (1, 8, 1040, 1, False, 1)):
            got0, hr = size(B, n0, n1, H, mode, bias, 0)
            got1, _ = size(B, n0, n1, H, mode, bias, 1)
            assert got0 == got1 == factor * hr, (mode, B, n0, n1, H, bias, got0, got1, hr)
    # SEPARATE looks at each part alone: 40 text + 1 000 image positions fit, the same 1 040 joint positions do not
    assert size(1, 40, 1000, 1, L.ATTN_SEPARATE)[0] == 1040
    assert size(1, 40, 1000, 1, L.ATTN_JOINT)[0] == 3 * 1040


def test_merge_variant_switch_is_retired():
    """The merge kernel's measurement switch and its sweep tool are gone (the sweep is recorded in docs/experiments.md): no
    source file under vl-merging_amd/, tools/ or include/ reads or names either.  Documents may."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    words = ("VLM_MERGE_VARIANT", "bench_merge_variants")
    hits = []
    for top in ("vl-merging_amd", "tools", "include"):
        for d, dirs, files in os.walk(os.path.join(root, top)):
            dirs[:] = [x for x in dirs if x not in ("_build", "__pycache__", "lib")]
            for f in files:
                if f.endswith((".md", ".rst", ".txt", ".pyc", ".so", ".o")):
                    continue
                path = os.path.join(d, f)
                with open(path, "rb") as fh:
                    text = fh.read().decode("utf-8", "replace")
                hits += [(os.path.relpath(path, root), w) for w in words if w in text]
    assert not hits, hits
    assert not os.path.exists(os.path.join(root, "tools", words[1] + ".py"))

