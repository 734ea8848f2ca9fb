"""GroupNorm on the CPU oracle path: op numerics against torch, config
round trip, ResNet-20 with norm_groups, batch independence, validation
errors and the (host-only) route function."""
import pytest
import torch
import torch.nn.functional as F

from bflc_amd.config import FLConfig
from bflc_amd.models import build_model
from bflc_amd.ops import functional as O

SHAPES = [(4, 7, 7, 8, 2), (2, 5, 5, 12, 3), (3, 1, 1, 16, 4)]


def _torch_gn(x, g, b, groups):
    return F.group_norm(x.permute(0, 3, 1, 2), groups, g, b,
                        eps=1e-5).permute(0, 2, 3, 1)


def _r20(norm_groups, n_class=10, lr=1e-3):
    cfg = FLConfig(model="resnet20", n_class=n_class, client_num=1,
                   comm_count=1, needed_update_count=1, aggregate_count=1,
                   learning_rate=lr, norm_groups=norm_groups)
    return build_model(cfg, torch.device("cpu"))


class TestGroupNormOracle:
    @pytest.mark.parametrize("n,h,w,c,groups", SHAPES)
    def test_fwd_bwd_matches_torch(self, n, h, w, c, groups):
        torch.manual_seed(0)
        x = torch.randn(n, h, w, c, requires_grad=True)  # NHWC
        g = torch.randn(c, requires_grad=True)
        b = torch.randn(c, requires_grad=True)
        y = O.groupnorm2d(x, g, b, groups)
        x2 = x.detach().clone().requires_grad_(True)
        g2 = g.detach().clone().requires_grad_(True)
        b2 = b.detach().clone().requires_grad_(True)
        ref = _torch_gn(x2, g2, b2, groups)
        assert torch.allclose(y, ref, atol=1e-5)
        dy = torch.randn_like(y)
        (y * dy).sum().backward()
        (ref * dy).sum().backward()
        assert torch.allclose(x.grad, x2.grad, atol=1e-4)
        assert torch.allclose(g.grad, g2.grad, atol=1e-4)
        assert torch.allclose(b.grad, b2.grad, atol=1e-4)

    @pytest.mark.parametrize("n,h,w,c,groups", SHAPES)
    def test_fused_relu_residual_matches_unfused(self, n, h, w, c, groups):
        torch.manual_seed(2)
        x = torch.randn(n, h, w, c, requires_grad=True)
        g = (torch.rand(c) + 0.5).requires_grad_(True)
        b = torch.randn(c, requires_grad=True)
        r = torch.randn(n, h, w, c, requires_grad=True)
        y = O.groupnorm2d(x, g, b, groups, relu=True, residual=r)
        dy = torch.randn_like(y)
        (y * dy).sum().backward()
        x2 = x.detach().clone().requires_grad_(True)
        g2 = g.detach().clone().requires_grad_(True)
        b2 = b.detach().clone().requires_grad_(True)
        r2 = r.detach().clone().requires_grad_(True)
        y2 = torch.relu(_torch_gn(x2, g2, b2, groups) + r2)
        assert torch.allclose(y, y2, atol=1e-5)
        (y2 * dy).sum().backward()
        assert torch.allclose(x.grad, x2.grad, atol=1e-4)
        assert torch.allclose(g.grad, g2.grad, atol=1e-4)
        assert torch.allclose(b.grad, b2.grad, atol=1e-4)
        assert torch.allclose(r.grad, r2.grad, atol=1e-4)

    def test_conv2d_gn_is_conv_then_gn(self):
        torch.manual_seed(4)
        x = torch.randn(2, 6, 6, 3)
        w = torch.randn(8, 3, 3, 3)
        g, b = torch.rand(8) + 0.5, torch.randn(8)
        y = O.conv2d_gn(x, w, g, b, 4, 1, 1, relu=True)
        ref = torch.relu(_torch_gn(O.conv2d(x, w, None, 1, 1), g, b, 4))
        assert torch.allclose(y, ref, atol=1e-5)


class TestConfig:
    def test_norm_groups_round_trip(self):
        cfg = FLConfig(model="resnet20", norm_groups=8)
        d = cfg.to_dict()
        assert d["norm_groups"] == 8
        assert FLConfig.from_dict(d).norm_groups == 8
        assert '"norm_groups": 8' in cfg.to_json()

    def test_missing_key_loads_as_zero(self):
        d = FLConfig(model="resnet20").to_dict()
        assert d["norm_groups"] == 0
        del d["norm_groups"]
        assert FLConfig.from_dict(d).norm_groups == 0


class TestResNet20GroupNorm:
    def test_forward_backward_and_layout(self):
        m = _r20(8)
        bn = _r20(0)
        assert m.numel == bn.numel
        assert m._offsets == bn._offsets
        torch.manual_seed(0)
        x = torch.randn(4, 32, 32, 3)
        y = torch.randint(0, 10, (4,))
        assert m.forward(x).shape == (4, 10)
        m.loss(x, y).backward()
        assert float(m.grad_flat().abs().sum()) > 0

    def test_loss_decreases_with_sgd(self):
        m = _r20(8, n_class=4, lr=0.05)
        torch.manual_seed(0)
        x = torch.randn(16, 32, 32, 3)
        y = torch.randint(0, 4, (16,))
        losses = []
        for _ in range(6):
            m.zero_grad()
            loss = m.loss(x, y)
            loss.backward()
            m.sgd_step(0.05)
            losses.append(float(loss.detach()))
        assert losses[-1] < losses[0]

    def test_batch_independence(self):
        """The point of the feature: a sample's logits do not depend on
        what shares its batch. BatchNorm (norm_groups=0) must fail the
        same comparison, or this test would be vacuous."""
        torch.manual_seed(1)
        x = torch.randn(6, 32, 32, 3)
        with torch.no_grad():
            gn = _r20(8)
            full = gn.forward(x)
            for i in range(6):
                alone = gn.forward(x[i:i + 1])[0]
                assert torch.allclose(full[i], alone, atol=1e-4), i
            bn = _r20(0)
            full = bn.forward(x)
            worst = max(float((full[i] - bn.forward(x[i:i + 1])[0])
                              .abs().max()) for i in range(6))
        assert worst > 1e-2


class TestValidation:
    def test_groups_must_divide_every_layer(self):
        with pytest.raises(ValueError, match="stem_bn"):
            _r20(32)

    def test_model_without_norm_layers_rejects_norm_groups(self):
        cfg = FLConfig(model="femnist_cnn", n_class=62, norm_groups=8)
        with pytest.raises(ValueError, match="norm_groups"):
            build_model(cfg, torch.device("cpu"))


@pytest.mark.skipif(not O.hip_available(),
                    reason="HIP extension not built")
class TestRoute:
    def test_resnet_shapes(self, monkeypatch):
        monkeypatch.delenv("BFLC_GN_ROUTE", raising=False)
        # ResNet-20 stages: 32 KB, 16 KB and 8 KB slabs per sample
        for h, c in [(32, 16), (16, 32), (8, 64)]:
            assert O.groupnorm_route(h, h, c, 8) == "slab"
        # ResNet-50 stage 1: 1.6 MB per sample
        assert O.groupnorm_route(56, 56, 256, 32) == "split"

    def test_route_takes_no_batch_size(self):
        import inspect
        params = list(inspect.signature(O.groupnorm_route).parameters)
        assert params == ["H", "W", "C", "groups"]

    def test_knob_forces_split_and_keeps_illegal_slab_out(self, monkeypatch):
        monkeypatch.setenv("BFLC_GN_ROUTE", "split")
        assert O.groupnorm_route(8, 8, 64, 8) == "split"
        monkeypatch.setenv("BFLC_GN_ROUTE", "slab")
        assert O.groupnorm_route(8, 8, 64, 8) == "slab"
        assert O.groupnorm_route(56, 56, 256, 32) == "split"

    def test_bad_shapes_raise(self):
        with pytest.raises(RuntimeError):
            O.groupnorm_route(4, 4, 12, 3)    # C % 8 != 0
        with pytest.raises(RuntimeError):
            O.groupnorm_route(4, 4, 16, 3)    # C % G != 0
