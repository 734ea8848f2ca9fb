"""Training path of the fused conv + bias + ReLU + 2x2 maxpool.

Forward: conv2d_relu_pool_fwd_idx gives the pooled output AND the u8
argmax plane bitwise as conv2d_fwd -> maxpool2d_fwd(want_idx=True) does,
on every fused route (thin, gemm256 in-kernel epilogue, gemm256 split-K
reduce), ties included.

Backward: the masked full-resolution gradient and db of the unpool
route are bitwise the maxpool2d_bwd -> relu_bwd_colsum chain
(mask-then-unpool == unpool-then-mask for a 2x2/stride-2 window, same
rows and trees), so by default every gradient of the model is bitwise
the two-op path's. The opt-in direct first-layer kernel
(BFLC_THIN_DIRECT_WGRAD=1, allow_direct in the native entry) sums
conv1 dW and db in its own order; each reordered tensor is held to

    max|new - ref| <= max(2 * max|parent - ref|, one bf16 ulp at max|ref|)

against an fp64 CPU reference built from the same bf16 inputs: parent
and new are both fp32 sums rounded once to bf16, so their errors are
the same size without being equal; the factor 2 covers the reordering,
the ulp floor a parent that happens to land exactly.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# name: (N, H, W, C, Kout, stride, pad) — all 3x3; the gemm256 shapes of
# test_conv_pool_fused_gpu.py (the small ones split K and pool in
# splitk_reduce_pool_kernel, n41 pools in the GEMM epilogue itself)
GEMM256_CASES = {
    "n8_8x8_c32_k64": (8, 8, 8, 32, 64, 1, 1),
    "n3_6x6_c32_k64": (3, 6, 6, 32, 64, 1, 1),
    "n5_12x12_c32_k64": (5, 12, 12, 32, 64, 1, 1),
    "n8_8x8_c8_k64": (8, 8, 8, 8, 64, 1, 1),
    "n8_8x8_c64_k64": (8, 8, 8, 64, 64, 1, 1),
    "n8_8x8_c32_k128": (8, 8, 8, 32, 128, 1, 1),
    "n8_4x4_c32_k64": (8, 4, 4, 32, 64, 1, 1),
    "n41_12x12_c32_k64": (41, 12, 12, 32, 64, 1, 1),
}


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def rand_inputs(n, h, w, c, kout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    wt = torch.randn(kout, 3, 3, c, generator=g) / math.sqrt(9 * c)
    b = torch.randn(kout, generator=g) * 0.5
    return bf(x), bf(wt), bf(b)


def fwd_route(x, w, stride, pad):
    return hip().conv2d_relu_pool_route(list(x.shape), list(w.shape),
                                        stride, pad)


def two_op_fwd(x, w, b, stride, pad):
    y = hip().conv2d_fwd(x, w, b, stride, pad, True)
    yp, idx = hip().maxpool2d_fwd(y, 2, 2, True)
    return y, yp, idx


def bf16_ulp(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 7) if v > 0 else 2.0 ** -133


def check_reordered(name, new, parent, ref64):
    """The tolerance of the module docstring, for one reordered tensor."""
    ref64 = ref64.reshape(-1)
    e_new = (new.detach().double().cpu().reshape(-1) - ref64).abs().max().item()
    e_par = (parent.detach().double().cpu().reshape(-1) - ref64).abs().max().item()
    ulp = bf16_ulp(ref64.abs().max().item())
    print(f"{name}: max|new-ref| {e_new:.3e}  max|parent-ref| {e_par:.3e}  "
          f"ulp@max|ref| {ulp:.3e}")
    assert e_new <= max(2 * e_par, ulp), name


# ---------------------------------------------------------------- forward

def _assert_fwd_idx_bitwise(x, w, b, stride, pad, want_route):
    assert fwd_route(x, w, stride, pad) == want_route
    y, idx = hip().conv2d_relu_pool_fwd_idx(x, w, b, stride, pad)
    yfull, ry, ridx = two_op_fwd(x, w, b, stride, pad)
    assert idx.dtype == torch.uint8 and idx.shape == y.shape == ry.shape
    assert torch.equal(y, ry)
    assert torch.equal(idx, ridx)
    return yfull, y, idx


@pytest.mark.parametrize("name", list(GEMM256_CASES))
def test_fwd_idx_gemm256_bitwise(name):
    n, h, w, c, kout, s, p = GEMM256_CASES[name]
    x, wt, b = rand_inputs(n, h, w, c, kout, seed=7)
    _, y, idx = _assert_fwd_idx_bitwise(x, wt, b, s, p, "gemm256_pool")
    assert y.float().abs().sum() > 0 and len(idx.unique()) == 4


@pytest.mark.parametrize("n,pad", [(84, 1), (97, 0)])
def test_fwd_idx_thin_bitwise(n, pad):
    x, wt, b = rand_inputs(n, 28, 28, 1, 32, seed=11)
    _, y, idx = _assert_fwd_idx_bitwise(x, wt, b, 1, pad, "thin_pool")
    assert y.float().abs().sum() > 0 and len(idx.unique()) == 4


TIE_SHAPES = {
    "gemm256": ((41, 12, 12, 32, 64), "gemm256_pool"),
    "gemm256_splitk": ((8, 8, 8, 32, 64), "gemm256_pool"),
    "thin": ((84, 28, 28, 1, 32), "thin_pool"),
}


@pytest.mark.parametrize("shape", list(TIE_SHAPES))
def test_fwd_idx_all_zero_windows(shape):
    """Bias -4: most windows are all-zero after ReLU; strict > from
    -inf keeps the first position, so idx must be 0 there."""
    (n, h, w, c, kout), rt = TIE_SHAPES[shape]
    x, wt, _ = rand_inputs(n, h, w, c, kout, seed=17)
    b = bf(torch.full((kout,), -4.0))
    yfull, y, idx = _assert_fwd_idx_bitwise(x, wt, b, 1, 1, rt)
    zero_win = y == 0
    assert zero_win.float().mean() > 0.5
    assert (idx[zero_win] == 0).all()


@pytest.mark.parametrize("shape", list(TIE_SHAPES))
def test_fwd_idx_positive_ties(shape):
    """Constant image: every interior window holds four equal values,
    positive for the channels whose taps sum above -bias; ties go to
    the first position."""
    (n, h, w, c, kout), rt = TIE_SHAPES[shape]
    _, wt, b = rand_inputs(n, h, w, c, kout, seed=19)
    x = bf(torch.ones(n, h, w, c))
    yfull, y, idx = _assert_fwd_idx_bitwise(x, wt, b, 1, 1, rt)
    win = yfull.view(n, h // 2, 2, w // 2, 2, kout)
    tie = ((win[:, :, 0, :, 0] == win[:, :, 0, :, 1]) &
           (win[:, :, 0, :, 0] == win[:, :, 1, :, 0]) &
           (win[:, :, 0, :, 0] == win[:, :, 1, :, 1]) & (y > 0))
    assert tie.any()
    assert (idx[tie] == 0).all()


# ----------------------------------------------------------------- unpool

UNPOOL_SHAPES = [(3, 3, 3, 64), (5, 6, 6, 64), (2, 7, 7, 32), (37, 7, 7, 8)]


def unpool_inputs(n, ph, pw, c, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(n, ph, pw, c, generator=g).abs()
    y[torch.rand(n, ph, pw, c, generator=g) < 0.2] = 0.0
    idx = torch.randint(0, 4, (n, ph, pw, c), generator=g, dtype=torch.uint8)
    idx[y == 0] = 0
    dy = torch.randn(n, ph, pw, c, generator=g)
    dy[torch.rand(n, ph, pw, c, generator=g) < 0.1] = -0.0
    return bf(y), idx.to(DEV).contiguous(), bf(dy)


@pytest.mark.parametrize("n,ph,pw,c", UNPOOL_SHAPES)
def test_unpool_relu_colsum(n, ph, pw, c):
    y, idx, dy = unpool_inputs(n, ph, pw, c, seed=23)
    assert (y == 0).float().mean() > 0.1
    assert (dy == 0).any()
    full = [n, 2 * ph, 2 * pw, c]
    dyf, db = hip().pool_relu_bwd_colsum(y, idx, dy, full)
    # the chain it replaces: only the selected position of a window
    # carries gradient, and there the activation is the pooled value
    yfull = hip().maxpool2d_bwd(y, idx, full, 2, 2)
    ref = hip().relu_bwd(yfull, hip().maxpool2d_bwd(dy, idx, full, 2, 2))
    assert list(dyf.shape) == full
    assert ref.float().abs().sum() > 0
    assert torch.equal(dyf, ref)
    _, db_parent = hip().relu_bwd_colsum(
        yfull, hip().maxpool2d_bwd(dy, idx, full, 2, 2))
    ref64 = (dy.double() * (y > 0)).sum(dim=(0, 1, 2)).cpu()
    check_reordered(f"unpool db {n}x{ph}x{pw}x{c}", db, db_parent, ref64)
    assert torch.equal(db, db_parent)  # same rows, chunks and trees
    # determinism
    dyf2, db2 = hip().pool_relu_bwd_colsum(y, idx, dy, full)
    assert torch.equal(dyf, dyf2) and torch.equal(db, db2)


# ----------------------------------------------------------- direct wgrad

# (N, H, Kout, pad)
WGRAD_SHAPES = [(3, 28, 32, 1), (2, 28, 32, 0), (5, 6, 8, 1), (2, 28, 64, 1),
                (84, 28, 32, 1)]


def wgrad_ref64(x, dy_masked_full, pad):
    """fp64 dW [Kout, 3, 3, 1] and db from the bf16 inputs on the CPU."""
    xn = x.double().cpu().permute(0, 3, 1, 2)
    dyn = dy_masked_full.double().cpu().permute(0, 3, 1, 2)
    kout = dyn.shape[1]
    dw = torch.nn.grad.conv2d_weight(xn, (kout, 1, 3, 3), dyn, stride=1,
                                     padding=pad)
    return dw.permute(0, 2, 3, 1).contiguous(), dyn.sum(dim=(0, 2, 3))


@pytest.mark.parametrize("n,h,kout,pad", WGRAD_SHAPES)
def test_thin_direct_wgrad(n, h, kout, pad):
    x, wt, b = rand_inputs(n, h, h, 1, kout, seed=29)
    yfull, yp, idx = two_op_fwd(x, wt, b, 1, pad)
    g = torch.Generator().manual_seed(31)
    dy = bf(torch.randn(yp.shape, generator=g))
    assert hip().conv2d_relu_pool_bwd_route(
        list(x.shape), list(wt.shape), 1, pad, False) == "thin_direct"
    dx, dw, db = hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, 1, pad,
                                            True, False)
    assert dx.numel() == 0 and dw.shape == wt.shape and db.shape == b.shape
    # parent chain on the same inputs
    dyf = hip().maxpool2d_bwd(dy, idx, list(yfull.shape), 2, 2)
    dym, db_parent = hip().relu_bwd_colsum(yfull, dyf)
    _, dw_parent, _ = hip().conv2d_bwd(x, wt, dym, 1, pad, None, False, False)
    dw64, db64 = wgrad_ref64(x, dym, pad)
    assert dw64.abs().max() > 0
    tag = f"thin {n}x{h}x{kout} pad{pad}"
    check_reordered(tag + " dW", dw, dw_parent, dw64)
    check_reordered(tag + " db", db, db_parent, db64)
    # determinism
    _, dw2, db2 = hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, 1, pad,
                                             True, False)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    # the two-kernel entry underneath gives the same pair
    dw3, db3 = hip().thin_conv_pool_wgrad(x, yp, idx, dy, 1, pad)
    assert torch.equal(dw, dw3.view(dw.shape)) and torch.equal(db, db3)
    # not allowed to go direct: the unpool route, bitwise the parent chain
    assert hip().conv2d_relu_pool_bwd_route(
        list(x.shape), list(wt.shape), 1, pad, False, False) == "unpool"
    _, dw4, db4 = hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, 1, pad,
                                             True, False, False)
    assert torch.equal(dw4, dw_parent) and torch.equal(db4, db_parent)


@pytest.mark.parametrize("name", ["n5_12x12_c32_k64", "n41_12x12_c32_k64"])
def test_unpool_route_bwd(name):
    """conv2-like stage: masked dy through the one-pass kernel, then the
    unchanged conv2d_bwd — dx, dW and db bitwise the parent chain; twice
    for determinism."""
    n, h, w, c, kout, s, p = GEMM256_CASES[name]
    x, wt, b = rand_inputs(n, h, w, c, kout, seed=37)
    yfull, yp, idx = two_op_fwd(x, wt, b, s, p)
    g = torch.Generator().manual_seed(41)
    dy = bf(torch.randn(yp.shape, generator=g))
    assert hip().conv2d_relu_pool_bwd_route(
        list(x.shape), list(wt.shape), s, p, True) == "unpool"
    dx, dw, db = hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, s, p,
                                            True, True)
    dyf = hip().maxpool2d_bwd(dy, idx, list(yfull.shape), 2, 2)
    dym, db_parent = hip().relu_bwd_colsum(yfull, dyf)
    dx_p, dw_p, _ = hip().conv2d_bwd(x, wt, dym, s, p, None, False, True)
    assert torch.equal(dx, dx_p) and torch.equal(dw, dw_p)
    check_reordered(name + " db", db, db_parent,
                    dym.double().sum(dim=(0, 1, 2)).cpu())
    assert torch.equal(db, db_parent)
    dx2, dw2, db2 = hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, s, p,
                                               True, True)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
    assert torch.equal(db, db2)


# ------------------------------------------------------------ model level

NAMES = ["c1w", "c1b", "c2w", "c2b", "f1w", "f1b", "f2w", "f2b"]


def _model_and_batch():
    from bflc_amd.config import FLConfig
    from bflc_amd.models import build_model
    cfg = FLConfig.for_world(1, model="femnist_cnn", n_class=62,
                             samples_per_client=64, batch_size=32,
                             eval_samples=64)
    m = build_model(cfg, torch.device(DEV))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():  # non-zero biases
        m.flat.add_(0.05 * torch.randn(m.numel, generator=g).to(DEV))
    m._sync_shadow()
    x = bf(torch.randn(96, 28, 28, 1, generator=g))
    y = torch.randint(0, 62, (96,), generator=g).to(DEV)
    return cfg, m, x, y


def _loss_backward(m, x, y, monkeypatch, gate, direct="0"):
    """One loss.backward() with the training gate set; also returns the
    logits, the two pooled stage outputs (with their grads retained) and
    the shapes each stage's autograd node saved."""
    from bflc_amd.ops import functional as fn
    monkeypatch.setenv("BFLC_FUSED_POOL_TRAIN", gate)
    monkeypatch.setenv("BFLC_THIN_DIRECT_WGRAD", direct)
    stages, logits = [], []
    orig = fn.conv2d_relu_pool
    orig_ce = fn.softmax_cross_entropy

    def recording(*a, **k):
        h = orig(*a, **k)
        h.retain_grad()
        stages.append(h)
        return h

    def recording_ce(lg, target):
        logits.append(lg.detach().clone())
        return orig_ce(lg, target)

    monkeypatch.setattr(fn, "conv2d_relu_pool", recording)
    monkeypatch.setattr(fn, "softmax_cross_entropy", recording_ce)
    m.zero_grad()
    loss = m.loss(x, y)
    monkeypatch.setattr(fn, "conv2d_relu_pool", orig)
    monkeypatch.setattr(fn, "softmax_cross_entropy", orig_ce)
    assert len(stages) == 2 and len(logits) == 1
    saved = [(type(h.grad_fn).__name__,
              [tuple(t.shape) for t in h.grad_fn.saved_tensors
               if t is not None]) for h in stages]
    loss.backward()
    grads = {k: m.p(k).grad.clone() for k in NAMES}
    return (loss.detach().clone(), logits[0]), grads, stages, saved


@pytest.mark.parametrize("direct", ["0", "1"])
def test_femnist_cnn_backward_gate_on_vs_off(monkeypatch, direct):
    """Gate on vs off. By default (direct "0") every gradient is bitwise
    equal; with the direct first-layer kernel opted in, c1w and c1b are
    held to the reordering tolerance and the rest stays bitwise.

    The forward is compared on the logits, bitwise. The scalar loss
    itself is NOT run-to-run bitwise on any path: softmax_ce_fwd adds
    the 96 per-row terms (all >= 0) into one fp32 with atomicAdd, in
    whatever order the waves retire (measured here: gate on vs off
    differed in the last bit, 30.9344 both). Any two orders of an fp32
    sum of M non-negative terms differ by at most 2 * (M - 1) * 2^-24 *
    sum, which is what the loss is held to; its gradient does not read
    the accumulated value, so every grad below is still exact."""
    _, m, x, y = _model_and_batch()
    assert fwd_route(x, m.p("c1w"), 1, 1) == "thin_pool"
    assert hip().conv2d_relu_pool_route(
        [96, 14, 14, 32], list(m.p("c2w").shape), 1, 1) == "gemm256_pool"
    (loss_on, lg_on), g_on, st_on, saved_on = _loss_backward(
        m, x, y, monkeypatch, "1", direct)
    (loss_off, lg_off), g_off, st_off, _ = _loss_backward(
        m, x, y, monkeypatch, "0")
    assert torch.isfinite(lg_on.float()).all() and torch.equal(lg_on, lg_off)
    print(f"loss gate on {loss_on.item():.9g} off {loss_off.item():.9g}")
    assert torch.isfinite(loss_on)
    assert abs(loss_on.item() - loss_off.item()) <= \
        2 * 95 * 2.0 ** -24 * abs(loss_off.item())
    exact = ("c2w", "c2b", "f1w", "f1b", "f2w", "f2b")
    for k in exact if direct == "1" else NAMES:
        assert g_on[k].float().abs().sum() > 0, k
        assert torch.equal(g_on[k], g_off[k]), k
    # gate on: only (x, w, y_pooled, idx) are saved, nothing at the
    # conv's full output resolution
    full = {(96, 28, 28, 32), (96, 14, 14, 64)}
    for fn_name, shapes in saved_on:
        assert "ConvReluPoolFn" in fn_name
        assert len(shapes) == 4 and not full & set(shapes), shapes
    assert set(saved_on[0][1]) == {(96, 28, 28, 1), (32, 3, 3, 1),
                                   (96, 14, 14, 32)}
    assert set(saved_on[1][1]) == {(96, 14, 14, 32), (64, 3, 3, 32),
                                   (96, 7, 7, 64)}
    # the pooled activations and the gradients reaching them are the
    # same under both gates, so one fp64 reference serves both paths
    for a, b in zip(st_on, st_off):
        assert torch.equal(a, b) and torch.equal(a.grad, b.grad)
    h1, h2 = (s.detach() for s in st_on)
    dh1, dh2 = st_on[0].grad, st_on[1].grad
    check_reordered("model c2b", g_on["c2b"], g_off["c2b"],
                    (dh2.double() * (h2 > 0)).sum(dim=(0, 1, 2)).cpu())
    yfull, yp, idx = two_op_fwd(x, m.p("c1w").detach(), m.p("c1b").detach(),
                                1, 1)
    assert torch.equal(yp, h1)
    dym = hip().relu_bwd(
        yfull, hip().maxpool2d_bwd(dh1.contiguous(), idx,
                                   list(yfull.shape), 2, 2))
    dw64, db64 = wgrad_ref64(x, dym, 1)
    check_reordered("model c1w", g_on["c1w"], g_off["c1w"], dw64)
    check_reordered("model c1b", g_on["c1b"], g_off["c1b"], db64)


@pytest.mark.parametrize("direct", ["0", "1"])
def test_graphed_train_step_matches_eager(monkeypatch, direct):
    from bflc_amd.fl.graphs import GraphedTrainStep
    monkeypatch.setenv("BFLC_FUSED_POOL_TRAIN", "1")
    monkeypatch.setenv("BFLC_THIN_DIRECT_WGRAD", direct)
    cfg, m, x, y = _model_and_batch()
    w0 = m.get_flat()
    lr = cfg.learning_rate
    step = GraphedTrainStep(m, lr, x, y)  # capture mutates the weights
    m.set_flat(w0)
    step.step(x, y)
    step.step(x, y)
    graphed = m.get_flat()
    m.set_flat(w0)
    for _ in range(2):
        m.zero_grad()
        m.loss(x, y).backward()
        m.sgd_step(lr)
    eager = m.get_flat()
    assert torch.isfinite(eager).all() and not torch.equal(eager, w0)
    assert torch.equal(graphed, eager)
