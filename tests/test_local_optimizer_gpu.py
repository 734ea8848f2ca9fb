"""Extended local optimizer on the GPU: the fused sgdm update, the
sum-of-squares / clip-coefficient pair, the binding guards, the graph
classes and the engine paths."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LR = 0.05


def _hip():
    from bflc_amd.ops.functional import hip_ops
    return hip_ops()


def _sizes():
    """Edge sizes + one n just above a full grid-stride pass of the
    update kernel (its loop then runs twice, with a ragged tail)."""
    blocks, threads, per_thread = _hip().sgdm_step_geom(1 << 40)
    return [1, 7, 8, 9, 1023, 8 * 1024 + 3,
            blocks * threads * per_thread + 8 * 37 + 5]


def _scal(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _inputs(n, gdtype, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen).to(gdtype)
    buf = torch.randn(n, generator=gen)
    p0 = p + 0.1 * torch.randn(n, generator=gen)
    return p.to(DEV), g.to(DEV), buf.to(DEV), p0.to(DEV)


def _ref64(p, g, buf, p0, lr, coef, mom, nest, wd, mu):
    """fp64 evaluation of the update formula on the same inputs:
    (p_ref, buf_ref, d_ref, sum of |terms| of buf)."""
    pd, gd = p.double(), coef * g.double()
    terms = gd.abs()
    if wd:
        gd = gd + wd * pd
        terms = terms + (wd * pd).abs()
    if mu:
        gd = gd + mu * (pd - p0.double())
        terms = terms + (mu * (pd - p0.double())).abs()
    b = gd
    if mom:
        b = mom * buf.double() + gd
        terms = terms + (mom * buf.double()).abs()
    d = gd + mom * b if nest else b
    return pd - lr * d, b, d, terms


# (grad dtype, shadow, momentum, nesterov, weight decay, mu): every
# boolean instantiation at least once
VARIANTS = [
    (torch.bfloat16, True, 0.9, True, 1e-2, 0.1),
    (torch.bfloat16, True, 0.9, False, 0.0, 0.0),
    (torch.bfloat16, True, 0.0, False, 1e-2, 0.0),
    (torch.bfloat16, True, 0.0, False, 0.0, 0.1),
    (torch.bfloat16, False, 0.9, True, 0.0, 0.0),
    (torch.float32, False, 0.9, False, 1e-2, 0.1),
    (torch.float32, False, 0.0, False, 0.0, 0.0),
    (torch.float32, True, 0.9, True, 0.0, 0.1),
]


@pytest.mark.parametrize("gdtype,shadow,mom,nest,wd,mu", VARIANTS)
def test_update_kernel_one_step(gdtype, shadow, mom, nest, wd, mu):
    from bflc_amd.ops import functional as O
    lr_dev, coef_dev = _scal(LR), _scal(1.0)
    lr = float(lr_dev)
    for n in _sizes():
        p, g, buf, p0 = _inputs(n, gdtype, seed=n % 1000)
        p_in, buf_in, p0_in = p.clone(), buf.clone(), p0.clone()
        sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV) \
            if shadow else None
        p0_arg = p0 if mu else torch.full((1,), 7.0, device=DEV)
        O.sgdm_step_(p, sh, g, buf, p0_arg, lr_dev, coef_dev, mom, nest,
                     wd, mu)
        p_ref, b_ref, d_ref, terms = _ref64(p_in, g, buf_in, p0_in, lr, 1.0,
                                            mom, nest, wd, mu)
        bound = 2.0 ** -22 * (p_in.double().abs() + lr * d_ref.abs())
        perr = (p.double() - p_ref).abs()
        print(f"n={n} max p err/bound "
              f"{float((perr / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((perr <= bound).all()), n
        if mom:
            berr = (buf.double() - b_ref).abs()
            assert bool((berr <= 2.0 ** -22 * terms).all()), n
        else:  # canary: buf is neither read nor written
            assert torch.equal(buf, buf_in), n
        if mu:
            assert torch.equal(p0, p0_in), n
        else:
            assert float(p0_arg[0]) == 7.0
        if shadow:
            assert torch.equal(sh, p.to(torch.bfloat16)), n


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_sumsq_and_coef(gdtype):
    from bflc_amd.ops import functional as O
    side = torch.cuda.Stream()
    for n in _sizes():
        _, g, _, _ = _inputs(n, gdtype, seed=n % 1000 + 1)
        out1 = torch.zeros(2, device=DEV)
        out2 = torch.zeros(2, device=DEV)
        out3 = torch.zeros(2, device=DEV)
        O.grad_clip_coef_(g, 0.5, out1)
        O.grad_clip_coef_(g, 0.5, out2)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            O.grad_clip_coef_(g, 0.5, out3)
        side.synchronize()
        assert torch.equal(out1, out2), n
        assert torch.equal(out1, out3), n
        _, per_lane, depth = O.grad_sumsq_geom(n)
        ss64 = float(g.double().square().sum())
        rel = abs(float(out1[1].double()) - ss64) / ss64
        print(f"n={n} sumsq rel err {rel:.3e} bound "
              f"{(per_lane + depth) * 2.0 ** -24:.3e}")
        assert rel <= (per_lane + depth) * 2.0 ** -24, n
        # the coefficient: torch.nn.utils.clip_grad_norm_'s formula, in
        # fp32 from the kernel's own ss (sqrt, add, divide: 3 roundings)
        want = min(1.0, 0.5 / (ss64 ** 0.5 + 1e-6))
        assert abs(float(out1[0]) - want) <= \
            want * ((per_lane + depth) / 2 + 3) * 2.0 ** -24, n
        # 1-element out: coefficient only
        out4 = torch.zeros(1, device=DEV)
        O.grad_clip_coef_(g, 0.5, out4)
        assert torch.equal(out4, out1[:1]), n


def test_sumsq_geom_is_a_function_of_n():
    from bflc_amd.ops import functional as O
    assert O.grad_sumsq_geom(1) == (1, 1, 24)
    assert O.grad_sumsq_geom(8) == (1, 8, 24)
    assert O.grad_sumsq_geom(9) == (1, 9, 24)
    assert O.grad_sumsq_geom(256 * 8 + 8) == (2, 8, 24)
    assert O.grad_sumsq_geom(1024 * 256 * 8) == (1024, 8, 24)
    assert O.grad_sumsq_geom(1024 * 256 * 8 + 9) == (1024, 17, 24)


def _step_args(n, clip_coef):
    p, g, buf, p0 = _inputs(n, torch.bfloat16, seed=11)
    sh = p.to(torch.bfloat16)
    return p, sh, g, buf, p0, _scal(LR), clip_coef


def test_coef_one_below_clip_and_zero_gradient():
    from bflc_amd.ops import functional as O
    n = 8 * 1024 + 3
    out = torch.zeros(2, device=DEV)
    O.grad_clip_coef_(torch.zeros(n, dtype=torch.bfloat16, device=DEV),
                      1.0, out)
    assert float(out[0]) == 1.0
    p, sh, g, buf, p0, lr_dev, _ = _step_args(n, None)
    norm = float(g.double().norm())
    O.grad_clip_coef_(g, 2.0 * norm, out)
    assert float(out[0]) == 1.0  # exactly
    a = [t.clone() for t in (p, sh, buf)]
    b = [t.clone() for t in (p, sh, buf)]
    O.sgdm_step_(a[0], a[1], g, a[2], p0, lr_dev, out, 0.9, True, 1e-2, 0.1)
    O.sgdm_step_(b[0], b[1], g, b[2], p0, lr_dev, _scal(1.0), 0.9, True,
                 1e-2, 0.1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], p)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_skips_the_step(bad):
    from bflc_amd.ops import functional as O
    n = 8 * 1024 + 3
    p, sh, g, buf, p0, lr_dev, _ = _step_args(n, None)
    g[n // 3] = bad
    out = torch.ones(2, device=DEV)
    O.grad_clip_coef_(g, 1.0, out)
    assert float(out[0]) == 0.0
    p_in, sh_in, buf_in = p.clone(), sh.clone(), buf.clone()
    O.sgdm_step_(p, sh, g, buf, p0, lr_dev, out, 0.9, True, 1e-2, 0.1)
    assert torch.equal(p, p_in)
    assert torch.equal(buf, buf_in)
    assert torch.equal(sh, sh_in)


def test_binding_guards():
    from bflc_amd.ops import functional as O
    n = 64
    p, sh, g, buf, p0, lr_dev, _ = _step_args(n, None)
    coef = _scal(1.0)
    big = torch.zeros(2 * n + 8, device=DEV)

    def step(p=p, sh=sh, g=g, buf=buf, p0=p0, lr_dev=lr_dev, coef=coef):
        O.sgdm_step_(p, sh, g, buf, p0, lr_dev, coef, 0.9, False, 0.0, 0.1)

    step()  # the well-formed call passes
    with pytest.raises(RuntimeError):  # misaligned views
        step(p=big[1:n + 1])
    with pytest.raises(RuntimeError):
        step(buf=big[1:n + 1])
    with pytest.raises(RuntimeError):
        step(p0=big[1:n + 1])
    with pytest.raises(RuntimeError):
        step(g=torch.zeros(n + 1, dtype=torch.bfloat16, device=DEV)[1:])
    with pytest.raises(RuntimeError):  # non-contiguous
        step(p=big[::2][:n])
    with pytest.raises(RuntimeError):
        step(g=torch.zeros(2 * n, dtype=torch.bfloat16, device=DEV)[::2])
    with pytest.raises(RuntimeError):  # dtypes
        step(p=p.double())
    with pytest.raises(RuntimeError):
        step(g=g.half())
    with pytest.raises(RuntimeError):
        step(sh=sh.float())
    with pytest.raises(RuntimeError):
        step(buf=buf.double())
    with pytest.raises(RuntimeError):
        step(lr_dev=lr_dev.double())
    with pytest.raises(RuntimeError):  # numel
        step(g=g[:n - 8])
    with pytest.raises(RuntimeError):
        step(buf=big[:n + 8])
    with pytest.raises(RuntimeError):  # host scalars
        step(coef=coef.cpu())
    out = torch.zeros(2, device=DEV)
    with pytest.raises(RuntimeError):
        O.grad_clip_coef_(big[1:n + 1], 1.0, out)
    with pytest.raises(RuntimeError):
        O.grad_clip_coef_(big[::2], 1.0, out)
    with pytest.raises(RuntimeError):
        O.grad_clip_coef_(g.half(), 1.0, out)
    with pytest.raises(RuntimeError):
        O.grad_clip_coef_(g, 1.0, out.double())


# ---------------------------------------------------------------- graphs
def _mlp_cfg():
    from bflc_amd.config import FLConfig
    return FLConfig.for_world(1, model="mlp", n_features=16, n_class=4,
                              samples_per_client=256, batch_size=128,
                              local_epochs=2, eval_samples=64,
                              learning_rate=LR, momentum=0.9, nesterov=True,
                              weight_decay=1e-4, prox_mu=0.01, clip_norm=1.0)


def _eager_pass(model, cfg, shard, start, lr_dev):
    from bflc_amd.models.base import SGDMState
    state = SGDMState.for_model(cfg, model, lr_dev, start)
    model.set_flat(start)
    bs = cfg.batch_size
    for _ in range(cfg.local_epochs):
        for b in range(shard.x.shape[0] // bs):
            model.zero_grad()
            model.loss(shard.x[b * bs:(b + 1) * bs],
                       shard.y[b * bs:(b + 1) * bs]).backward()
            model.sgdm_step(state)
    return model.get_flat()


def test_graphed_local_train_matches_eager_and_follows_lr_dev():
    from bflc_amd.data import make_federated
    from bflc_amd.fl.graphs import GraphedLocalTrain
    from bflc_amd.models import build_model
    cfg = _mlp_cfg()
    shards, _ = make_federated(cfg)
    shard = shards[0].to(DEV)
    model = build_model(cfg, DEV)
    model.init_params(cfg.seed)
    start = model.get_flat()
    lr_dev = _scal(LR)
    g = GraphedLocalTrain(model, cfg.learning_rate, shard.x, shard.y,
                          cfg.batch_size, cfg.local_epochs,
                          optimizer="sgdm", sgdm_cfg=cfg, lr_dev=lr_dev,
                          p0=start)
    assert g.n_steps == 4

    def graphed():
        model.set_flat(start)
        g.run()
        return model.get_flat()

    w1 = graphed()
    assert not torch.equal(w1, start)
    assert torch.equal(graphed(), w1)  # buf really is reset per run()
    assert torch.equal(_eager_pass(model, cfg, shard, start, lr_dev), w1)
    # refill lr_dev and replay the SAME graph object
    graph_obj = g.graph
    lr_dev.fill_(0.2 * LR)
    w2 = graphed()
    assert g.graph is graph_obj
    assert not torch.equal(w2, w1)
    assert torch.equal(_eager_pass(model, cfg, shard, start, lr_dev), w2)


def test_graphed_train_step_matches_eager():
    from bflc_amd.data import make_federated
    from bflc_amd.fl.graphs import GraphedTrainStep
    from bflc_amd.models import build_model
    cfg = _mlp_cfg()
    shards, _ = make_federated(cfg)
    shard = shards[0].to(DEV)
    model = build_model(cfg, DEV)
    model.init_params(cfg.seed)
    start = model.get_flat()
    lr_dev = _scal(LR)
    bs = cfg.batch_size
    st = GraphedTrainStep(model, cfg.learning_rate, shard.x[:bs],
                          shard.y[:bs], optimizer="sgdm", sgdm_cfg=cfg,
                          lr_dev=lr_dev, p0=start)
    model.set_flat(start)
    st.reset_state()
    for _ in range(cfg.local_epochs):
        for b in range(2):
            st.step(shard.x[b * bs:(b + 1) * bs],
                    shard.y[b * bs:(b + 1) * bs])
    w = model.get_flat()
    assert torch.equal(_eager_pass(model, cfg, shard, start, lr_dev), w)


# ---------------------------------------------------------------- engine
def _engine(cfg, metrics_path=None):
    from bflc_amd.comm import Transport
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    shards, test = make_federated(cfg)
    return FLEngine(cfg, Transport(device=DEV), shards, test,
                    metrics_path=metrics_path)


def _femnist_cfg(**kw):
    from bflc_amd.config import FLConfig
    return FLConfig.for_world(8, model="femnist_cnn", n_class=62,
                              samples_per_client=256, batch_size=128,
                              eval_samples=256, partition="dirichlet", **kw)


_EXT = dict(momentum=0.9, lr_schedule="cosine", lr_total_rounds=6,
            clip_norm=5.0, prox_mu=0.01)


def test_engine_sgdm_streams_graphs_and_eager_agree(monkeypatch, tmp_path):
    def run(streams, graphs, log=None):
        monkeypatch.setenv("BFLC_STREAMS", streams)
        cfg = _femnist_cfg(use_graphs=graphs, **_EXT)
        eng = _engine(cfg, metrics_path=log)
        assert eng.local_optimizer == "sgdm"
        sel = []
        for _ in range(4):
            eng.run_round()
            sel.append(tuple(o for o, _ in eng.last_decision.selected))
        return eng.global_flat.clone(), sel, eng, cfg

    log = str(tmp_path / "m.jsonl")
    flat_c, sel_c, eng_c, cfg = run("1", True, log)
    assert len(eng_c._client_streams) > 1 and len(eng_c._client_models) > 1
    assert any(g is not None for g in eng_c._train_graphs.values()), \
        "no whole-train graph captured"
    assert all(g.optimizer == "sgdm"
               for g in eng_c._train_graphs.values() if g is not None)
    recs = [json.loads(l) for l in open(log)]
    assert [r["local_lr"] for r in recs] == [cfg.local_lr(e)
                                             for e in range(4)]
    assert len(set(r["local_lr"] for r in recs)) == 4  # it really decays

    flat_s, sel_s, eng_s, _ = run("0", True)
    assert any(g is not None for g in eng_s._train_graphs.values())
    assert sel_c == sel_s
    assert torch.equal(flat_c, flat_s)

    flat_e, _, eng_e, _ = run("0", False)
    assert not eng_e._train_graphs and not eng_e._steppers
    assert torch.allclose(flat_s, flat_e, atol=1e-6, rtol=1e-5)


def test_engine_default_fields_stay_on_the_legacy_step():
    eng = _engine(_femnist_cfg())
    assert eng.local_optimizer == "sgd_legacy"
    assert eng._lr_dev is None
    eng.run(1)
    assert all(g.optimizer == "sgd"
               for g in eng._train_graphs.values() if g is not None)
