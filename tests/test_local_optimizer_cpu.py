"""Extended local optimizer on CPU: config validation, the lr
schedules, the fp32-tensor oracles of the sgdm kernels against
torch.optim.SGD / clip_grad_norm_, and the engine's path selection and
checkpoint-free schedule."""
import math

import pytest
import torch

from bflc_amd.config import FLConfig
from bflc_amd.ops import functional as O


# ---------------------------------------------------------------- config
@pytest.mark.parametrize("kw", [
    dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(prox_mu=-0.01),
    dict(clip_norm=-1.0), dict(lr_gamma=-0.1), dict(lr_step_rounds=-1),
    dict(lr_total_rounds=-1), dict(lr_min=-1e-3),
    dict(nesterov=True),                          # no momentum
    dict(lr_schedule="step"),                     # no lr_step_rounds
    dict(lr_schedule="linear"),                   # unknown
    dict(optimizer="adam", momentum=0.9),
    dict(optimizer="adam", weight_decay=1e-4),
    dict(optimizer="adam", prox_mu=0.01),
    dict(optimizer="adam", clip_norm=1.0),
    dict(optimizer="adam", lr_schedule="cosine"),
])
def test_config_rejects(kw):
    with pytest.raises(ValueError):
        FLConfig(**kw)


def test_default_config_is_not_extended():
    cfg = FLConfig()
    assert cfg.extended_sgd is False
    assert cfg.local_lr(0) == cfg.learning_rate
    assert cfg.local_lr(999) == cfg.learning_rate
    assert FLConfig(optimizer="adam").extended_sgd is False


@pytest.mark.parametrize("kw", [
    dict(momentum=0.9), dict(momentum=0.9, nesterov=True),
    dict(weight_decay=1e-4), dict(prox_mu=0.01), dict(clip_norm=1.0),
    dict(lr_schedule="cosine"), dict(lr_schedule="step", lr_step_rounds=3),
    dict(lr_gamma=0.5), dict(lr_total_rounds=10), dict(lr_min=1e-4),
])
def test_any_field_makes_it_extended(kw):
    assert FLConfig(**kw).extended_sgd is True


def test_local_lr_constant():
    cfg = FLConfig(learning_rate=0.05, momentum=0.9)
    assert [cfg.local_lr(e) for e in (0, 1, 500)] == [0.05] * 3


def test_local_lr_step_boundaries():
    cfg = FLConfig(learning_rate=0.1, lr_schedule="step", lr_step_rounds=4,
                   lr_gamma=0.5)
    assert cfg.local_lr(0) == 0.1
    assert cfg.local_lr(3) == 0.1
    assert cfg.local_lr(4) == 0.1 * 0.5
    assert cfg.local_lr(7) == 0.1 * 0.5
    assert cfg.local_lr(8) == 0.1 * 0.5 ** 2


def test_local_lr_cosine_endpoints_and_midpoint():
    cfg = FLConfig(learning_rate=0.1, lr_schedule="cosine",
                   lr_total_rounds=10, lr_min=0.01)
    assert cfg.local_lr(0) == 0.1
    assert cfg.local_lr(5) == pytest.approx(0.055, rel=1e-12)
    assert cfg.local_lr(10) == pytest.approx(0.01, rel=1e-12)
    assert cfg.local_lr(25) == cfg.local_lr(10)  # clamped past T
    e = 3
    want = 0.01 + 0.5 * (0.1 - 0.01) * (1 + math.cos(math.pi * e / 10))
    assert cfg.local_lr(e) == want
    # lr_total_rounds == 0 means max_epoch
    cfg2 = FLConfig(learning_rate=0.1, lr_schedule="cosine", max_epoch=40)
    assert cfg2.local_lr(20) == pytest.approx(0.05, rel=1e-12)
    assert cfg2.local_lr(40) == pytest.approx(0.0, abs=1e-17)


def test_protocol_lr_is_not_scheduled():
    cfg = FLConfig(learning_rate=0.1, lr_schedule="cosine",
                   lr_total_rounds=4, momentum=0.9)
    assert cfg.ledger_config().learning_rate == pytest.approx(0.1)


# ---------------------------------------------------------------- oracle
def _scalars(lr, coef=1.0):
    return (torch.tensor([lr], dtype=torch.float32),
            torch.tensor([coef], dtype=torch.float32))


@pytest.mark.parametrize("mom,nest,wd", [
    (0.9, False, 0.0), (0.9, True, 0.0), (0.0, False, 1e-2),
    (0.9, True, 1e-2)])
def test_oracle_matches_torch_sgd(mom, nest, wd):
    """5 steps, 1000 elements, fp32. rtol 1e-6 / atol 1e-7: at most 4
    roundings of 2^-24 per step over 5 steps."""
    gen = torch.Generator().manual_seed(0)
    n, lr = 1000, 0.05
    p = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(5)]
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([ref], lr=lr, momentum=mom, nesterov=nest,
                          weight_decay=wd)
    buf = torch.zeros(n if mom > 0 else 1)
    lr_dev, coef_dev = _scalars(lr)
    dummy = torch.zeros(1)
    for g in grads:
        ref.grad = g.clone()
        opt.step()
        O.sgdm_step_(p, None, g, buf, dummy, lr_dev, coef_dev, mom, nest,
                     wd, 0.0)
    torch.testing.assert_close(p, ref.detach(), rtol=1e-6, atol=1e-7)
    if mom > 0:
        # the buffer is a cancelling sum, so its error scales with the
        # terms, not the result: same 4 roundings x 5 steps, relative
        # to sum_i |g_i| (+ the weight-decay term, bounded by |p|)
        scale = sum(g.abs() for g in grads) + 5 * wd * (p.abs() + 1)
        err = (buf - opt.state[ref]["momentum_buffer"]).abs()
        assert bool((err <= 20 * 2.0 ** -24 * scale).all())


def test_oracle_clip_coef_matches_clip_grad_norm():
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(1000, generator=gen)
    for clip in (0.5, 5.0, 1e3):
        leaf = torch.zeros(1000, requires_grad=True)
        leaf.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([leaf], clip)
        out = torch.zeros(2)
        O.grad_clip_coef_(g, clip, out)
        torch.testing.assert_close(out[0] * g, leaf.grad, rtol=1e-6,
                                   atol=1e-7)
        torch.testing.assert_close(out[1], g.square().sum(), rtol=1e-6,
                                   atol=1e-7)
    out = torch.zeros(1)
    O.grad_clip_coef_(g, 1e3, out)
    assert float(out[0]) == 1.0  # within the clip: exactly 1
    O.grad_clip_coef_(torch.zeros(10), 1.0, out)
    assert float(out[0]) == 1.0
    for bad in (float("inf"), float("nan")):
        gb = g.clone()
        gb[17] = bad
        O.grad_clip_coef_(gb, 1.0, out)
        assert float(out[0]) == 0.0


def test_oracle_skips_step_on_zero_coef():
    p = torch.randn(64)
    buf = torch.randn(64)
    sh = p.to(torch.bfloat16)
    p_in, buf_in, sh_in = p.clone(), buf.clone(), sh.clone()
    lr_dev, coef_dev = _scalars(0.1, coef=0.0)
    O.sgdm_step_(p, sh, torch.randn(64), buf, p.clone(), lr_dev, coef_dev,
                 0.9, True, 1e-2, 0.1)
    assert torch.equal(p, p_in) and torch.equal(buf, buf_in)
    assert torch.equal(sh, sh_in)


def test_oracle_prox_term():
    gen = torch.Generator().manual_seed(2)
    n, lr, mu = 257, 0.1, 0.25
    p = torch.randn(n, generator=gen)
    p0 = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    want = (p.double() - lr_f32(lr) * (g.double()
                                      + mu * (p.double() - p0.double())))
    p0_in = p0.clone()
    lr_dev, coef_dev = _scalars(lr)
    sh = torch.zeros(n, dtype=torch.bfloat16)
    O.sgdm_step_(p, sh, g, torch.zeros(1), p0, lr_dev, coef_dev, 0.0,
                 False, 0.0, mu)
    assert torch.equal(p, want.float())
    assert torch.equal(p0, p0_in)
    assert torch.equal(sh, p.to(torch.bfloat16))


def lr_f32(lr):
    return float(torch.tensor(lr, dtype=torch.float32))


def test_nesterov_without_momentum_raises():
    lr_dev, coef_dev = _scalars(0.1)
    with pytest.raises(ValueError):
        O.sgdm_step_(torch.zeros(8), None, torch.zeros(8), torch.zeros(1),
                     torch.zeros(1), lr_dev, coef_dev, 0.0, True, 0.0, 0.0)


# ---------------------------------------------------------------- engine
def _engine(cfg, metrics_path=None):
    from bflc_amd.comm import Transport
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    shards, test = make_federated(cfg)
    return FLEngine(cfg, Transport(), shards, test,
                    metrics_path=metrics_path)


_BASE = dict(model="mlp", n_features=16, n_class=4, samples_per_client=64,
             batch_size=32, eval_samples=64, learning_rate=0.05)
_EXT = dict(momentum=0.9, lr_schedule="cosine", lr_total_rounds=6,
            clip_norm=1.0, prox_mu=0.01)


def test_engine_reports_its_local_optimizer():
    assert _engine(FLConfig.for_world(1, **_BASE)).local_optimizer \
        == "sgd_legacy"
    assert _engine(FLConfig.for_world(1, **_BASE, **_EXT)).local_optimizer \
        == "sgdm"
    assert _engine(FLConfig.for_world(
        1, optimizer="adam", **_BASE)).local_optimizer == "adam"


def test_engine_schedule_needs_no_checkpoint_state(tmp_path):
    import json
    cfg = FLConfig.for_world(1, **_BASE, **_EXT)
    log = tmp_path / "m.jsonl"
    a = _engine(cfg, metrics_path=str(log))
    flat0 = a.global_flat.clone()
    a.run(6)
    assert not torch.equal(a.global_flat, flat0)
    assert bool(torch.isfinite(a.global_flat).all())
    recs = [json.loads(l) for l in log.read_text().splitlines()]
    assert [r["local_lr"] for r in recs] == [cfg.local_lr(e)
                                             for e in range(6)]

    b = _engine(cfg)
    b.run(3)
    ck = str(tmp_path / "ck.pt")
    b.save(ck)
    c = _engine(cfg)
    c.load(ck)
    c.run(3)
    assert c.ledger.epoch == 6
    assert torch.equal(c.global_flat, a.global_flat)


def test_engine_extended_differs_from_legacy_and_learns():
    """The extended step really runs (momentum changes the trajectory)
    and still trains the model."""
    legacy = _engine(FLConfig.for_world(1, **_BASE))
    ext = _engine(FLConfig.for_world(1, momentum=0.9, **_BASE))
    legacy.run(4)
    ext.run(4)
    assert not torch.equal(legacy.global_flat, ext.global_flat)
    assert ext.evaluate_global() > 0.5  # 4 classes, chance 0.25


# ------------------------------------------------------- optimizer object
@pytest.mark.parametrize("kind,kw", [
    ("adam", dict(optimizer="adam", learning_rate=0.001)),
    ("sgdm", dict(momentum=0.9)),
    ("sgd", {}),
])
def test_local_optimizer_reset_gives_a_fresh_pass(kind, kw):
    """Fresh state per client pass: two steps, reset(), two steps from
    the same restored weights must land on the same bits. A reset that
    forgets Adam's (m, v, step) or the momentum buffer carries one
    client's state into the next one's pass."""
    from bflc_amd.data import make_federated
    from bflc_amd.fl import graphs
    from bflc_amd.models import build_model
    cfg = FLConfig.for_world(1, **{**_BASE, **kw})
    shard = make_federated(cfg)[0][0]
    model = build_model(cfg, torch.device("cpu"))
    model.init_params(cfg.seed)
    start = model.get_flat()
    lr_dev = torch.full((1,), cfg.learning_rate)
    opt = graphs.LocalOptimizer(
        model, kind, cfg.learning_rate, False,
        **(dict(sgdm_cfg=cfg, lr_dev=lr_dev, p0=start)
           if kind == "sgdm" else {}))
    assert opt.kind == kind
    bs = cfg.batch_size

    def two_steps():
        model.set_flat(start)
        for b in range(2):
            graphs.train_step(model, opt, shard.x[b * bs:(b + 1) * bs],
                              shard.y[b * bs:(b + 1) * bs])
        return model.get_flat()

    first = two_steps()
    assert not torch.equal(first, start)
    if kind != "sgd":  # the state really carries over without a reset
        assert not torch.equal(two_steps(), first)
    opt.reset()
    assert torch.equal(two_steps(), first)


def test_local_optimizer_rejects_unknown_kind_and_fp32_graphed_adam():
    from bflc_amd.fl import graphs
    from bflc_amd.models import build_model
    cfg = FLConfig.for_world(1, **_BASE)
    model = build_model(cfg, torch.device("cpu"))
    with pytest.raises(ValueError):
        graphs.LocalOptimizer(model, "lion", 0.1, False)
    with pytest.raises(ValueError):  # sgdm without its device lr
        graphs.LocalOptimizer(model, "sgdm", 0.1, False)
    assert model.cflat is model.flat  # fp32 on the CPU: no bf16 shadow
    with pytest.raises(RuntimeError, match="bf16-shadow"):
        graphs.LocalOptimizer(model, "adam", 0.1, True)
