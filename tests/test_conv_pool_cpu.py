"""CPU path of O.conv2d_relu_pool: exactly the two-op sequence, with
and without grad mode (the fused kernel exists only for grad-free GPU
forwards)."""
import pytest
import torch

from bflc_amd.ops import functional as O


@pytest.mark.parametrize("h,stride,pad", [(8, 1, 1), (7, 1, 1), (10, 2, 1),
                                          (6, 1, 0)])
def test_conv2d_relu_pool_is_two_op_sequence(h, stride, pad):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, h, h, 4, generator=g)
    w = torch.randn(8, 3, 3, 4, generator=g)
    b = torch.randn(8, generator=g)
    ref = O.maxpool2d(O.conv2d(x, w, b, stride, pad, relu=True), 2)
    with torch.no_grad():
        y = O.conv2d_relu_pool(x, w, b, stride, pad)
    assert y.shape == ref.shape
    assert torch.equal(y, ref)
    assert torch.equal(O.conv2d_relu_pool(x, w, b, stride, pad), ref)


def test_conv2d_relu_pool_no_bias_and_grad():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, 8, 3, generator=g, requires_grad=True)
    w = torch.randn(4, 3, 3, 3, generator=g, requires_grad=True)
    y = O.conv2d_relu_pool(x, w, None, 1, 1)
    x2 = x.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    ref = O.maxpool2d(O.conv2d(x2, w2, None, 1, 1, relu=True), 2)
    assert torch.equal(y, ref)
    y.sum().backward()
    ref.sum().backward()
    assert torch.equal(x.grad, x2.grad) and torch.equal(w.grad, w2.grad)


def test_femnist_cnn_cpu_forward_unchanged():
    """The model's forward through the new op equals the explicit
    conv - pool - conv - pool stack it replaced."""
    from bflc_amd.config import FLConfig
    from bflc_amd.models import build_model
    cfg = FLConfig.for_world(1, model="femnist_cnn", n_class=62,
                             samples_per_client=8, batch_size=4,
                             eval_samples=8)
    m = build_model(cfg, torch.device("cpu"))
    x = torch.randn(4, 28, 28, 1, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        h = O.maxpool2d(O.conv2d(x, m.p("c1w"), m.p("c1b"), 1, 1, relu=True), 2)
        h = O.maxpool2d(O.conv2d(h, m.p("c2w"), m.p("c2b"), 1, 1, relu=True), 2)
        h = O.linear(h.reshape(4, -1), m.p("f1w"), m.p("f1b"), relu=True)
        ref = O.linear(h, m.p("f2w"), m.p("f2b"))
        assert torch.equal(m.forward(x), ref)
