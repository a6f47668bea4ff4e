"""ops.gemm_wgrad_batch (vlm_gemm_wgrad_batch): up to four weight gradients over the same token rows in one launch of the 256x256
wgrad kernel plus one reduce launch.

Exact cases use integer-valued bf16 inputs in [-4, 4]: every product is an integer of magnitude <= 16 and every partial sum over
T <= 4 099 rows (plus the integer pre-fill of an accumulating gradient, <= 1 000) stays below 2^24, so fp32 addition is exact in ANY
order and the result must EQUAL the fp32 matmul bit for bit -- a wrong tile, slice, row bound or workspace offset is a mismatch,
not noise.  The random case uses the wgrad tolerance of tests/test_kernels_gpu.py (rtol 1e-3, atol 2e-3 sqrt(T))."""
import importlib
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SETS = {
    "four": [(256, 512), (512, 256), (256, 256), (768, 256)],
    "ragged_m": [(320, 256), (256, 768)],  # M = 320: rows >= M of the second row tile must be dropped
    "single": [(256, 512)],
}
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("vl_merging_amd.ops")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("vl_merging_amd._lib")


@pytest.fixture
def cu_budget(L):
    """set(n): plan for n compute units for the rest of the test; the previous plan comes back afterwards."""
    lib = L.get_lib()
    prev = lib.vlm_device_cus()

    def set_budget(n):
        assert lib.vlm_set_cu_budget(n) == 0 and lib.vlm_device_cus() == n

    yield set_budget
    lib.vlm_set_cu_budget(0)
    if prev != lib.vlm_device_cus():
        lib.vlm_set_cu_budget(prev)  # the previous value was itself a budget


def ints(gen, rows, cols, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, (rows, cols), device="cuda", generator=gen).to(torch.bfloat16)


def sliced_operand(gen, T, cols, make):
    """[T, cols] as a column slice (ld = cols + 16 > cols, 16-byte aligned start) of a wider buffer with a spare row at the end."""
    buf = make(gen, T + 1, cols + 16)
    return buf[:T, 8:8 + cols]


def build_problems(gen, T, shapes, make):
    """Per problem: dy, x (column slices of wider buffers), the gradient's whole buffer `big` (taller and wider than dW, full of a
    sentinel), dW = its [M, N] window, the accumulate flag (alternating) and the integer pre-fill."""
    out = []
    for i, (M, N) in enumerate(shapes):
        dy, x = sliced_operand(gen, T, M, make), sliced_operand(gen, T, N, make)
        wide = i == len(shapes) - 1  # one problem per call: ldc > N, a column slice of a wider gradient
        big = torch.full((M + 8, N + 16 if wide else N), SENTINEL, device="cuda")
        dW = big[:M, 8:8 + N] if wide else big[:M]
        pre = torch.randint(-1000, 1001, (M, N), device="cuda", generator=gen).float()
        dW.copy_(pre)
        out.append(dict(dy=dy, x=x, big=big, dW=dW, acc=(i % 2 == 0), pre=pre, wide=wide, M=M, N=N))
    return out


def want_of(p):
    w = p["dy"].float().t() @ p["x"].float()
    return w + p["pre"] if p["acc"] else w


def check_guard(p):
    """Nothing outside the [M, N] window moved: the rows below it (an M that is no multiple of 256) and the padding columns."""
    assert bool((p["big"][p["M"]:] == SENTINEL).all()), "rows >= M were written"
    if p["wide"]:
        assert bool((p["big"][:, :8] == SENTINEL).all()) and bool((p["big"][:, 8 + p["N"]:] == SENTINEL).all()), "padding columns moved"


@pytest.mark.parametrize("T,budget", [(2048, None), (2048, 16), (2048, 8), (2077, None), (4099, None)])
@pytest.mark.parametrize("name", sorted(SETS))
def test_exact_integers(ops, cu_budget, name, T, budget):
    """Bit-for-bit against the fp32 matmul.  T = 2 048: 64 K steps, at 256 CUs every tile gets its four 16-step slices; a budget of 16
    or 8 CUs cuts the slice count down to one per tile (8 CUs, the four-problem set of 8 tiles).  T = 2 077: T % 32 != 0, the last slice
    is ragged.  Accumulate on for problems 0 and 2 and off for 1 and 3 in the same call."""
    if budget is not None:
        cu_budget(budget)
    gen = torch.Generator(device="cuda"); gen.manual_seed(T * 31 + len(name) + (budget or 0))
    probs = build_problems(gen, T, SETS[name], ints)
    ops.gemm_wgrad_batch([(p["dy"], p["x"], p["dW"]) for p in probs], accumulate=[p["acc"] for p in probs])
    torch.cuda.synchronize()
    for i, p in enumerate(probs):
        want = want_of(p)
        assert float(want.abs().max()) < 2 ** 24
        bad = p["dW"] != want
        assert not bool(bad.any()), "problem %d (%d x %d): %d of %d elements differ, first at %s" % (
            i, p["M"], p["N"], int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()))
        check_guard(p)


def test_random_within_wgrad_tolerance_and_reproducible(ops):
    T = 2077
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    gauss = lambda g, r, c: torch.randn(r, c, device="cuda", generator=g).to(torch.bfloat16)  # noqa: E731
    probs = build_problems(gen, T, SETS["four"], gauss)
    for p in probs:
        p["pre"] = torch.randn(p["M"], p["N"], device="cuda", generator=gen)
    runs = []
    for _ in range(2):
        for p in probs:
            p["dW"].copy_(p["pre"])
        ops.gemm_wgrad_batch([(p["dy"], p["x"], p["dW"]) for p in probs], accumulate=[p["acc"] for p in probs])
        torch.cuda.synchronize()
        runs.append([p["dW"].clone() for p in probs])
    for p, a, b in zip(probs, runs[0], runs[1]):
        want = want_of(p)
        err = (a - want).abs()
        tol = 2e-3 * math.sqrt(T) + 1e-3 * want.abs()
        assert not bool((err > tol).any()), "max err %.4g" % float(err.max())
        assert torch.equal(a, b), "two calls on the same inputs differ: the reduction is not order-free"
        check_guard(p)


@pytest.mark.parametrize("T,shapes,exact", [(2077, [(256, 192), (256, 256)], True), (1000, [(256, 256), (512, 256)], False)])
def test_not_offered_equals_plain_calls(ops, T, shapes, exact):
    """N = 192 (no whole 256-column tiles) and T = 1 000 (below the workspace gate): bit for bit what one ops.gemm per problem gives.
    The plain path of the N = 192 problem at T >= 2 048 is the split-K kernel that adds its slices with fp32 atomics, whose result
    depends on arrival order (two plain calls differ from each other in the last bits): that case runs on integer inputs, whose
    sums are exact in any order, so equality is a statement about what is computed.  T = 1 000 takes no split: Gaussian inputs."""
    gen = torch.Generator(device="cuda"); gen.manual_seed(T)
    make = ints if exact else (lambda g, r, c: torch.randn(r, c, device="cuda", generator=g).to(torch.bfloat16))
    probs = []
    for M, N in shapes:
        pre = torch.randint(-1000, 1001, (M, N), device="cuda", generator=gen).float() if exact \
            else torch.randn(M, N, device="cuda", generator=gen)
        probs.append((make(gen, T, M), make(gen, T, N), pre))
    got = [w.clone() for _, _, w in probs]
    ops.gemm_wgrad_batch([(dy, x, g) for (dy, x, _), g in zip(probs, got)])
    for (dy, x, w), g in zip(probs, got):
        one = w.clone()
        ops.gemm(dy, x, one, ta=True, tb=True, accumulate=True)
        assert torch.equal(g, one)
        if exact:
            assert torch.equal(g, dy.float().t() @ x.float() + w)


def test_argument_errors(ops, L):
    dy = torch.zeros(2048, 256, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(256, 256, device="cuda")
    with pytest.raises(L.VlmError):
        ops.gemm_wgrad_batch([(dy, dy, w)] * 5)                 # too many problems
    with pytest.raises(L.VlmError):
        ops.gemm_wgrad_batch([(dy, dy[:1000], w)])              # token counts differ
    with pytest.raises(L.VlmError):
        ops.gemm_wgrad_batch([(dy, dy, w[:128])])               # gradient shape
    with pytest.raises(L.VlmError):
        ops.gemm_wgrad_batch([(dy.float(), dy, w)])             # dtype
    with pytest.raises(L.VlmError):
        ops.gemm_wgrad_batch([(dy, dy, w)], accumulate=[True, False])


# ---- engine wiring: _BlockFn.backward with the batch (side stream on) against the four plain calls (side stream off) ----------
def _block_run(pkg, fold, side):
    """Forward + backward of ONE base-width ufo block (D = 768, 12 heads) over 4 samples of 40 text + 577 image tokens (384^2:
    2 468 rows) with seeded inputs and injected DropPath draws.  -> {name: gradient} and dx."""
    engine = importlib.import_module("vl_merging_amd.engine")
    ops = importlib.import_module("vl_merging_amd.ops")
    cfgmod = importlib.import_module("vl_merging_amd.vilt.config")
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    B, T, I, D, H = 4, 40, 577, 768, 12
    torch.manual_seed(11)
    cfg = cfgmod.make_config("ufo", vit="vit_base_patch16_384", hidden_size=768, num_heads=12, vocab_size=1024,
                             max_text_len=40, patch_size=16, vlffn_start_layer_index=10, image_size=384, max_vl_text_len=40,
                             tasks=["vl"], loss_names=cfgmod._loss_names({"itm": 1}), drop_rate=0.2)
    model = vm.ViLTransformerSS(cfg, *cfgmod.routing_configs(cfg)).cuda().train()
    with torch.no_grad():  # the shipped init leaves biases at zero and gammas equal: make every gradient path non-trivial
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        for n, p in model.named_parameters():
            if n.startswith("transformer.blocks.6.") or n == "relative_position_bias_table":
                p.add_(0.02 * torch.randn(p.shape, device="cuda", generator=gen))
    prev_env = os.environ.get("VLM_FOLD_LAYERSCALE")
    os.environ["VLM_FOLD_LAYERSCALE"] = "1" if fold else "0"
    prev_side = engine._WGRAD["enabled"]
    try:
        model.setup_engine()
        engine._WGRAD["enabled"] = side
        blk = model.transformer.blocks[6]
        assert blk.drop_path_prob > 0
        keep0 = torch.ones(B, T, device="cuda", dtype=torch.uint8)
        pc = model._pass_ctx(ops.Seq(B, T, I), H, model.get_rel_pos_bias(model.vl_text_imag_relative_position_index, T), keep0=keep0)
        cpu = torch.Generator(); cpu.manual_seed(3)
        pc.uniform_source = lambda pc_, S, streams: torch.rand(streams, S, B, generator=cpu)
        pc.plan_drop_path([blk.drop_path_prob, blk.drop_path_prob])
        gen = torch.Generator(device="cuda"); gen.manual_seed(17)
        x = torch.randn(B * (T + I), D, device="cuda", generator=gen).requires_grad_(True)
        g = torch.randn(B * (T + I), D, device="cuda", generator=gen)
        model.zero_grad()
        y = blk.run(x, pc, 2)
        assert engine._folded(blk.plan(2, pc.seq).ranges) == fold
        y.backward(g)
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
                 if (n.startswith("transformer.blocks.6.") or n == "relative_position_bias_table") and p.grad is not None}
        weights = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith("transformer.blocks.6.")}
        return grads, x.grad.detach().clone(), weights, B * (T + I)
    finally:
        engine._WGRAD["enabled"] = prev_side
        if prev_env is None:
            os.environ.pop("VLM_FOLD_LAYERSCALE", None)
        else:
            os.environ["VLM_FOLD_LAYERSCALE"] = prev_env


WEIGHTS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")


@pytest.mark.parametrize("fold", [False, True])
def test_block_backward_batch_equals_plain_calls(pkg, fold):
    """Side stream on (one batched launch after the attention backward) against side stream off (the four plain calls in stream
    order).  dx is bit-identical.  The four weight gradients agree within the wgrad tolerance (rtol 1e-3, atol 2e-3 sqrt(rows)).
    Every other gradient of the block is a COLUMN SUM -- biases, LayerNorm weights, gammas, the bias table -- that the row kernels
    and the attention backward add up from per-workgroup partials with fp32 atomics, in arrival order: two runs of the SAME
    schedule already differ there (measured on this case, side stream off against off: 2e-8 of 0.37 for the bias table, 2e-6 of 24
    for proj.bias, 1.5e-5 of 77 for gamma_2; dx and the weight gradients 0), so bit-identity is not a property they have with or
    without the batch.  Their bound: a few hundred partials per element, each addition off by at most 2^-24 of a partial sum that
    is a small multiple of the tensor's largest element -- 1e-4 of that element leaves two orders of magnitude of room and still
    catches a lost or doubled contribution.
    Folded LayerScale: vlm_layerscale_finish computes dgamma[n] = sum_k W[n,k] raw_w[n,k] + b[n] raw_b[n] FROM the raw weight-gradient
    sums, and dW[n,:] = gamma[n] raw_w[n,:], so the gammas also inherit the summation-order difference of raw_w: on top of the
    above, the wgrad tolerance carried through that formula, sum_k |W[n,k]| tol(raw_w[n,k])."""
    on, dx_on, w, rows = _block_run(pkg, fold, True)
    off, dx_off, _, _ = _block_run(pkg, fold, False)
    assert sorted(on) == sorted(off) and len(on) == 16, sorted(on)  # the block's 15 parameters and the bias table
    assert torch.equal(dx_on, dx_off), "dx differs"
    atol = 2e-3 * math.sqrt(rows)
    pre = "transformer.blocks.6."
    seen = 0
    for n in sorted(on):
        a, b = on[n], off[n]
        assert float(b.abs().max()) > 0, n + ": zero gradient, the case checks nothing"
        short = n[len(pre):] if n.startswith(pre) else n
        err = (a - b).abs()
        if short in WEIGHTS:
            seen += 1
            gamma = {"attn.proj.weight": w[pre + "gamma_1"], "mlp.fc2.weight": w[pre + "gamma_2"]}.get(short) if fold else None
            scale = gamma.abs()[:, None] if gamma is not None else 1.0  # folded: dW = gamma * raw_w, the tolerance is raw_w's
            bound = scale * atol + 1e-3 * b.abs()
        else:
            bound = torch.full_like(b, 1e-4 * float(b.abs().max()))
            if fold and short in ("gamma_1", "gamma_2"):
                lin = "attn.proj" if short == "gamma_1" else "mlp.fc2"
                W, gm = w[pre + lin + ".weight"], w[pre + short]
                raw = off[pre + lin + ".weight"] / gm[:, None]
                bound = bound + (W.abs() * (atol + 1e-3 * raw.abs())).sum(1)
        assert not bool((err > bound).any()), "%s: max err %.4g of max %.4g" % (n, float(err.max()), float(b.abs().max()))
    assert seen == 4
