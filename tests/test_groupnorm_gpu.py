"""GPU numerics for the GroupNorm kernels (csrc/hip/groupnorm.hip): both
routes against an fp32 oracle on the same bf16-rounded inputs, fused
relu/residual, per-sample bitwise invariance, determinism, error paths,
and the ResNets / engine with norm_groups set."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5

# N, H, W, C, G — each chosen for a way the lane mapping can break
CASES = [
    (3, 8, 8, 16, 8),      # cpg = 2: four groups inside one 16-byte vector
    (2, 7, 7, 32, 8),      # cpg = 4, odd H*W (49 rows)
    (2, 8, 8, 64, 8),      # cpg = 8: group = vector
    (2, 4, 4, 64, 4),      # cpg = 16: group spans two vectors
    (1, 1, 1, 2048, 32),   # H*W = 1, N = 1, cpg = 64
    (5, 16, 16, 32, 8),    # ResNet-20 stage-2 slab, N not a power of two
    (2, 56, 56, 64, 32),   # split route, cpg = 2
    (1, 57, 57, 64, 8),    # split route, rows not a multiple of the chunk
]
SLAB_CASES = CASES[:6]
# further paths of the launcher: the deeper register slabs (8 and 16
# vectors per lane), and channel counts whose granule count is no power
# of two (split only), one with a group that straddles vectors unevenly
EXTRA_CASES = [
    (2, 32, 32, 16, 8),    # ResNet-20 stage-1 slab, 8 vectors per lane
    (1, 32, 32, 32, 8),    # 64 KiB: the largest slab, 16 vectors per lane
    (2, 5, 5, 24, 3),      # C/8 = 3 granules: split
    (2, 4, 4, 48, 4),      # cpg = 12: groups cut vectors at 4 and 8
    (1100, 2, 2, 16, 4),   # > 1024 partial rows: segmented dgamma/dbeta sum
]
INVARIANCE_CASES = [CASES[0], CASES[3], CASES[6]]


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def assert_close(y, ref, rel=0.03):
    y = y.float().cpu()
    ref = ref.float().cpu()
    scale = ref.abs().max().clamp_min(1.0)
    torch.testing.assert_close(y, ref, rtol=rel, atol=float(scale) * rel)


def rounded(x):
    """fp32 CPU copy of the bf16-rounded tensor the GPU sees."""
    return bf(x).float().cpu()


def oracle(xf, gf, bfl, groups, residual=None, relu=False):
    """fp32 torch GroupNorm on NHWC; returns (y, mean [N,G], rstd [N,G])."""
    n, h, w, c = xf.shape
    y = torch.nn.functional.group_norm(
        xf.permute(0, 3, 1, 2), groups, gf, bfl, eps=EPS).permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual
    if relu:
        y = torch.relu(y)
    xg = xf.detach().double().reshape(n, h * w, groups, c // groups)
    mean = xg.mean(dim=(1, 3))
    var = xg.var(dim=(1, 3), unbiased=False)
    return y, mean.float(), (var + EPS).rsqrt().float()


def run_case(n, h, w, c, groups, offset=0.0):
    torch.manual_seed(0)
    x = torch.randn(n, h, w, c) + offset
    g = torch.rand(c) + 0.5
    b = torch.randn(c)
    dy = torch.randn(n, h, w, c)
    y, mean, rstd = hip().groupnorm_fwd(bf(x), bf(g), bf(b), groups, EPS,
                                        False)
    x2 = rounded(x).requires_grad_(True)
    g2 = rounded(g).requires_grad_(True)
    b2 = rounded(b).requires_grad_(True)
    ref, rmean, rrstd = oracle(x2, g2, b2, groups)
    assert mean.shape == (n, groups) and mean.dtype == torch.float32
    assert_close(y, ref)
    # fp32 reductions of identical inputs against an fp64 oracle. Each
    # element passes through at most ~100 fp32 additions (a lane's rows,
    # the fixed tree, the cpg channel fold), so the worst-case error of a
    # mean is 100 * 2^-24 * mean|x| = 5e-6 * max(1, |offset|) and the
    # expected one orders of magnitude less; the absolute term only
    # serves group means that happen to fall near zero. The relative
    # bound is the issue's 1e-3 tightened to 1e-5 as the measured error
    # allows: the worst case here is the split route at mean = 8 sigma,
    # where E[x^2] - mean^2 on fp32 chunk sums (relative error ~1e-7 on
    # sums of size 65 and 64) leaves up to ~6e-6 on rstd. Measured on an
    # MI355X: |mean err| <= 1.5e-8 and rstd <= 1.3e-7 relative in every
    # case but that one, 1.4e-6 there.
    merr = (mean.cpu().double() - rmean.double()).abs()
    rerr = ((rstd.cpu().double() - rrstd.double()) / rrstd.double()).abs()
    print(f"gn stats {n}x{h}x{w}x{c} G={groups} offset={offset}: "
          f"max |mean err| {float(merr.max()):.3e} "
          f"max rel rstd err {float(rerr.max()):.3e}")
    torch.testing.assert_close(mean.cpu(), rmean, rtol=1e-5,
                               atol=1e-6 * max(1.0, abs(offset)))
    torch.testing.assert_close(rstd.cpu(), rrstd, rtol=1e-5, atol=0)
    dx, dgamma, dbeta = hip().groupnorm_bwd(bf(x), bf(dy), mean, rstd,
                                            bf(g), groups)
    assert dgamma.dtype == torch.bfloat16 and dbeta.dtype == torch.bfloat16
    (ref * rounded(dy)).sum().backward()
    assert_close(dx, x2.grad, rel=0.05)
    assert_close(dgamma, g2.grad, rel=0.05)
    assert_close(dbeta, b2.grad, rel=0.05)


class TestGroupNormKernels:
    def test_cases_cover_both_routes(self, monkeypatch):
        monkeypatch.delenv("BFLC_GN_ROUTE", raising=False)
        routes = [hip().groupnorm_route(h, w, c, g)
                  for _, h, w, c, g in CASES]
        assert routes[:6] == ["slab"] * 6 and routes[6:] == ["split"] * 2

    @pytest.mark.parametrize("n,h,w,c,groups", CASES + EXTRA_CASES)
    def test_fwd_bwd(self, monkeypatch, n, h, w, c, groups):
        monkeypatch.delenv("BFLC_GN_ROUTE", raising=False)
        run_case(n, h, w, c, groups)

    def test_extra_cases_routes(self, monkeypatch):
        monkeypatch.delenv("BFLC_GN_ROUTE", raising=False)
        routes = [hip().groupnorm_route(h, w, c, g)
                  for _, h, w, c, g in EXTRA_CASES]
        assert routes == ["slab", "slab", "split", "split", "slab"]

    @pytest.mark.parametrize("n,h,w,c,groups", SLAB_CASES)
    def test_fwd_bwd_forced_split(self, monkeypatch, n, h, w, c, groups):
        monkeypatch.setenv("BFLC_GN_ROUTE", "split")
        assert hip().groupnorm_route(h, w, c, groups) == "split"
        run_case(n, h, w, c, groups)

    @pytest.mark.parametrize("route", ["slab", "split"])
    def test_offset_inputs_exercise_variance(self, monkeypatch, route):
        # mean = 8 sigma: E[x^2] - mean^2 cancellation would show here
        monkeypatch.setenv("BFLC_GN_ROUTE", route)
        assert hip().groupnorm_route(16, 16, 32, 8) == route
        run_case(5, 16, 16, 32, 8, offset=8.0)

    @pytest.mark.parametrize("n,h,w,c,groups",
                             [CASES[0], CASES[3], CASES[5], CASES[7]])
    def test_fused_relu_residual(self, monkeypatch, n, h, w, c, groups):
        monkeypatch.delenv("BFLC_GN_ROUTE", raising=False)
        torch.manual_seed(3)
        x = torch.randn(n, h, w, c)
        g = torch.rand(c) + 0.5
        b = torch.randn(c)
        r = torch.randn(n, h, w, c)
        dy = torch.randn(n, h, w, c)
        y, mean, rstd = hip().groupnorm_fwd(bf(x), bf(g), bf(b), groups,
                                            EPS, True, bf(r))
        assert float(y.min()) >= 0.0
        x2 = rounded(x).requires_grad_(True)
        g2 = rounded(g).requires_grad_(True)
        b2 = rounded(b).requires_grad_(True)
        ref, _, _ = oracle(x2, g2, b2, groups, residual=rounded(r),
                           relu=True)
        assert_close(y, ref)
        dx, dgamma, dbeta = hip().groupnorm_bwd(bf(x), bf(dy), mean, rstd,
                                                bf(g), groups, y)
        # the kernel is specified to mask by its own y > 0: the oracle
        # takes exactly that mask, so no threshold-flip allowance
        mask = (y.float().cpu() > 0).float()
        pre, _, _ = oracle(x2, g2, b2, groups)
        (pre * (rounded(dy) * mask)).sum().backward()
        assert_close(dx, x2.grad, rel=0.05)
        assert_close(dgamma, g2.grad, rel=0.05)
        assert_close(dbeta, b2.grad, rel=0.05)
        # residual gradient = masked dy, through the autograd wrapper
        from bflc_amd.ops import functional as O
        xa = bf(x).requires_grad_(True)
        ra = bf(r).requires_grad_(True)
        ya = O.groupnorm2d(xa, bf(g), bf(b), groups, EPS, True, ra)
        assert torch.equal(ya, y)
        ya.backward(bf(dy))
        assert torch.equal(ra.grad.float().cpu(), rounded(dy) * mask)
        assert torch.equal(xa.grad, dx)

    @pytest.mark.parametrize("n,h,w,c,groups", INVARIANCE_CASES)
    def test_per_sample_bitwise_invariance(self, monkeypatch, n, h, w, c,
                                           groups):
        monkeypatch.delenv("BFLC_GN_ROUTE", raising=False)
        torch.manual_seed(5)
        x = bf(torch.randn(n, h, w, c))
        g, b = bf(torch.rand(c) + 0.5), bf(torch.randn(c))
        dy = bf(torch.randn(n, h, w, c))
        y, mean, rstd = hip().groupnorm_fwd(x, g, b, groups, EPS, False)
        dx, _, _ = hip().groupnorm_bwd(x, dy, mean, rstd, g, groups)
        for i in range(n):
            xi, dyi = x[i:i + 1].contiguous(), dy[i:i + 1].contiguous()
            yi, mi, ri = hip().groupnorm_fwd(xi, g, b, groups, EPS, False)
            dxi, _, _ = hip().groupnorm_bwd(xi, dyi, mi, ri, g, groups)
            assert torch.equal(y[i], yi[0]), i
            assert torch.equal(mean[i], mi[0]), i
            assert torch.equal(rstd[i], ri[0]), i
            assert torch.equal(dx[i], dxi[0]), i

    def test_deterministic(self, monkeypatch):
        monkeypatch.delenv("BFLC_GN_ROUTE", raising=False)
        torch.manual_seed(7)
        x = bf(torch.randn(8, 14, 14, 16))
        g, b = bf(torch.rand(16) + 0.5), bf(torch.randn(16))
        dy = bf(torch.randn(8, 14, 14, 16))
        f1 = hip().groupnorm_fwd(x, g, b, 4, EPS, False)
        f2 = hip().groupnorm_fwd(x, g, b, 4, EPS, False)
        assert all(torch.equal(a, c) for a, c in zip(f1, f2))
        b1 = hip().groupnorm_bwd(x, dy, f1[1], f1[2], g, 4)
        b2 = hip().groupnorm_bwd(x, dy, f1[1], f1[2], g, 4)
        assert all(torch.equal(a, c) for a, c in zip(b1, b2))

    def test_error_paths(self):
        x = bf(torch.randn(2, 4, 4, 12))
        g, b = bf(torch.ones(12)), bf(torch.zeros(12))
        with pytest.raises(RuntimeError, match="C % 8"):
            hip().groupnorm_fwd(x, g, b, 3, EPS, False)
        x = bf(torch.randn(2, 4, 4, 16))
        g, b = bf(torch.ones(16)), bf(torch.zeros(16))
        with pytest.raises(RuntimeError, match="divisible"):
            hip().groupnorm_fwd(x, g, b, 3, EPS, False)
        mean = torch.zeros(2, 3, device=DEV)
        with pytest.raises(RuntimeError, match="divisible"):
            hip().groupnorm_bwd(x, x, mean, mean, g, 3)


class TestResNetGroupNormGPU:
    @pytest.mark.parametrize("groups", [0, 8])
    def test_fresh_model_first_forward_uses_initialised_gammas(self, groups):
        """init_params fills the gammas (1.0) into the fp32 master after
        the base class synced the bf16 shadow; it must sync again, or a
        freshly built GPU ResNet runs its first forward with gamma = 0:
        all-zero logits and loss = ln(n_class). Holds for BatchNorm (0)
        and GroupNorm alike."""
        from bflc_amd.config import FLConfig
        from bflc_amd.models import build_model
        cfg = FLConfig(model="resnet20", n_class=10, client_num=1,
                       comm_count=1, needed_update_count=1,
                       aggregate_count=1, norm_groups=groups)
        m = build_model(cfg, torch.device(DEV))
        off, shape = m._offsets["stem_bn.g"]
        assert torch.equal(m.cflat[off:off + shape[0]].float().cpu(),
                           torch.ones(shape[0]))
        assert torch.equal(m.cflat.float(), m.flat.to(torch.bfloat16).float())
        torch.manual_seed(0)
        x = torch.randn(8, 32, 32, 3)
        with torch.no_grad():
            logits = m.forward(x.to(DEV, torch.bfloat16))
        assert float(logits.float().abs().max()) > 0.1

    @pytest.mark.parametrize("model,hw,groups,lr,steps", [
        ("resnet20", 32, 8, 0.05, 5),
        ("resnet50", 64, 32, 0.003, 10),
    ])
    def test_train_step_runs_and_learns(self, model, hw, groups, lr, steps):
        from bflc_amd.config import FLConfig
        from bflc_amd.models import build_model
        cfg = FLConfig(model=model, n_class=10, client_num=1, comm_count=1,
                       needed_update_count=1, aggregate_count=1,
                       learning_rate=lr, norm_groups=groups)
        m = build_model(cfg, torch.device(DEV))
        torch.manual_seed(0)
        x = torch.randn(16, hw, hw, 3)
        y = torch.randint(0, 10, (16,), device=DEV)
        losses = []
        for _ in range(steps):
            m.zero_grad()
            loss = m.loss(x, y)
            loss.backward()
            m.sgd_step(cfg.learning_rate)
            losses.append(float(loss.detach()))
        assert all(math.isfinite(v) for v in losses)
        assert min(losses[-3:]) < losses[0]


def _engine(cfg):
    from bflc_amd.comm import Transport
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    shards, test = make_federated(cfg)
    return FLEngine(cfg, Transport(device=torch.device(DEV)), shards, test)


class TestEngineGroupNormGPU:
    def test_one_client_round_with_eval(self):
        from bflc_amd.config import FLConfig
        cfg = FLConfig.for_world(1, model="resnet20", n_class=10,
                                 norm_groups=8, samples_per_client=256,
                                 batch_size=128, eval_samples=128)
        st = _engine(cfg).run_round(eval_global=True)
        assert st.epoch == 0 and st.test_acc is not None
        assert math.isfinite(st.global_loss)

    def test_four_client_round_concurrent_streams(self, monkeypatch):
        from bflc_amd.config import FLConfig
        monkeypatch.setenv("BFLC_STREAMS", "1")
        cfg = FLConfig.for_world(4, model="resnet20", n_class=10,
                                 norm_groups=8, samples_per_client=128,
                                 batch_size=64, eval_samples=128)
        eng = _engine(cfg)
        st = eng.run_round()
        assert math.isfinite(st.global_loss)
        assert len(eng._client_streams) > 1, "no per-client streams made"
        assert bool(torch.isfinite(eng.global_flat).all())

    def test_graph_capture_does_not_change_results(self):
        from bflc_amd.config import FLConfig
        runs = {}
        for graphs in (True, False):
            cfg = FLConfig.for_world(1, model="resnet20", n_class=10,
                                     norm_groups=8, samples_per_client=256,
                                     batch_size=128, eval_samples=128,
                                     use_graphs=graphs)
            eng = _engine(cfg)
            eng.run_round()
            runs[graphs] = eng.global_flat.clone()
        assert torch.equal(runs[True], runs[False])
