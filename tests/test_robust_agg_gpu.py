"""Robust aggregation on the GPU: the three gfx950 kernels against
their CPU oracles, and the engine under a model-poisoning attack."""
import numpy as np
import pytest
import torch

from bflc_amd.ops import functional as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _same_values(a: torch.Tensor, b: torch.Tensor) -> None:
    """Equal by value, NaN positions equal."""
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


# ------------------------------------------------------- order_stat_mean
OSM_K = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
OSM_P = (1, 3, 4, 5, 1023, 4099)


def _osm_inputs(K: int, P: int, gen: torch.Generator):
    plain = torch.randn(K, P, generator=gen)
    plain[:, P // 2] = plain[0, P // 2]        # a column of duplicates
    if K >= 3:
        plain[K - 1, 0] = plain[0, 0]          # one duplicated pair
    special = plain.clone()
    special[0] = float("inf")
    if K >= 2:
        special[K - 1] = float("-inf")
    if K >= 3:
        special[K // 2] = float("nan")
    return plain, special


@pytest.mark.parametrize("K", OSM_K)
def test_order_stat_mean_equals_cpu(K):
    gen = torch.Generator().manual_seed(100 + K)
    for P in OSM_P:
        for d in _osm_inputs(K, P, gen):
            dg = d.to(DEV)
            perm = torch.randperm(K, generator=gen)
            for t in sorted({0, 1, (K - 1) // 2}):
                if 2 * t >= K:
                    continue
                ref = O.order_stat_mean(d, t)
                got = O.order_stat_mean(dg, t)
                _same_values(got, ref)
                # sorted-order sum: row order cannot matter, bitwise
                again = O.order_stat_mean(dg[perm.to(DEV)].contiguous(), t)
                assert torch.equal(_bits(got), _bits(again)), (K, P, t)


@pytest.mark.parametrize("K,P,t", [(5, 4, 1), (9, 1024, 4), (32, 5, 1)])
def test_order_stat_mean_unaligned_base(K, P, t):
    """Rows sliced from a larger buffer: row 0 itself sits 4 bytes past
    a 16-byte boundary, so even P % 4 == 0 takes the dword path."""
    gen = torch.Generator().manual_seed(7)
    flat = torch.randn(K * P + 1, generator=gen)
    d = flat[1:].view(K, P)
    dg = flat.to(DEV)[1:].view(K, P)
    assert dg.data_ptr() % 16 == 4 and dg.is_contiguous()
    _same_values(O.order_stat_mean(dg, t), O.order_stat_mean(d, t))


def test_ops_raise_on_bad_arguments():
    d = torch.randn(4, 8, device=DEV)
    hip = O.hip_ops()
    for t in (-1, 2):
        with pytest.raises((RuntimeError, ValueError)):
            hip.order_stat_mean(d, t)
    big = torch.zeros(33, 8, device=DEV)
    for fn in (lambda: hip.order_stat_mean(big, 0),
               lambda: hip.delta_gram(big),
               lambda: hip.masked_wmean(big, torch.ones(33, device=DEV)),
               lambda: hip.delta_gram(d.double()),
               lambda: hip.delta_gram(d.t()),
               lambda: hip.order_stat_mean(d[:, ::2], 0),
               lambda: hip.masked_wmean(d, torch.ones(3, device=DEV)),
               lambda: hip.masked_wmean(d.cpu(), torch.ones(4))):
        with pytest.raises(RuntimeError):
            fn()


# ------------------------------------------------------------ delta_gram
GRAM_K = (1, 2, 3, 5, 10, 16, 17, 32)
GRAM_P = (1, 7, 64, 4099, 262147)


@pytest.mark.parametrize("K", GRAM_K)
def test_delta_gram(K):
    gen = torch.Generator().manual_seed(200 + K)
    for P in GRAM_P:
        d = torch.randn(K, P, generator=gen)
        # asymmetric row scales: a row/column swap cannot hide
        d *= (1.0 + torch.arange(K, dtype=torch.float32))[:, None]
        dg = d.to(DEV)
        G = O.delta_gram(dg)
        assert G.shape == (K, K) and G.dtype == torch.float32
        d64 = d.double()
        G64 = d64 @ d64.t()
        # fp32 fmaf chain of length <= P, factor 2 for the second stage
        bound = 2.0 * P * 2.0 ** -24 * (d64.abs() @ d64.abs().t())
        err = (G.cpu().double() - G64).abs()
        assert bool((err <= bound).all()), (K, P, float((err / bound).max()))
        assert torch.equal(_bits(G), _bits(G.t())), (K, P)
        assert torch.equal(_bits(G), _bits(O.delta_gram(dg))), (K, P)
        perm = torch.randperm(K, generator=gen).to(DEV)
        Gp = O.delta_gram(dg[perm].contiguous())
        assert torch.equal(_bits(Gp), _bits(G[perm][:, perm])), (K, P)
        # rows >= K are never read: NaN beyond them changes nothing
        buf = torch.full((32, P), float("nan"), device=DEV)
        buf[:K] = dg
        assert torch.equal(_bits(O.delta_gram(buf[:K])), _bits(G)), (K, P)


# ---------------------------------------------------------- masked_wmean
def _wmean_case(P: int):
    gen = torch.Generator().manual_seed(300 + P)
    d = torch.randn(6, P, generator=gen)
    w = torch.tensor([3.0, 0.0, 1.0, 2.0, 0.0, 5.0])
    return d, w


@pytest.mark.parametrize("P", [4, 4096])
def test_masked_wmean_is_fedavg_on_kept_rows(P):
    d, w = _wmean_case(P)
    keep = w != 0
    got = O.masked_wmean(d.to(DEV), w.to(DEV))
    ref = O.weighted_fedavg(d[keep].contiguous().to(DEV), w[keep].to(DEV))
    assert torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("P", [1, 5, 4099])
def test_masked_wmean_any_p(P):
    d, w = _wmean_case(P)
    d[1] = float("nan")   # zero weight: must not reach the output
    d[4] = float("nan")
    got = O.masked_wmean(d.to(DEV), w.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    keep = w != 0
    wd = w[keep, None].double() * d[keep].double()
    ref = wd.sum(0) / w.sum().double()
    tol = 1e-6 * wd.abs().sum(0) / w.sum().double()
    assert bool(((got.double() - ref).abs() <= tol).all())


# ---------------------------------------------------------------- engine
# Margin of the accuracy checks, fixed before any GPU run
# (profiles/r12_robust_agg_ab.md): the attack-free fedavg accuracy A0 of
# this config on the CPU fp32 engine was 1.0000 for seeds 42, 43 and 44 —
# a spread of 0, i.e. below the 1/1024 resolution of a 1024-sample
# evaluation. Twice that resolution stands in for twice the spread.
M_ACC = 2.0 / 1024.0

BASE = dict(client_num=8, comm_count=2, needed_update_count=6,
            aggregate_count=6, byzantine_clients=2, model="mlp",
            n_features=32, n_class=8, samples_per_client=256,
            batch_size=128, eval_samples=1024, learning_rate=0.05)
ATTACK = dict(byzantine_attack="scale", byzantine_scale=-4.0)
ATTACKERS = {"node_6", "node_7"}


def _run(**kw):
    from bflc_amd.comm import Transport
    from bflc_amd.config import FLConfig
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    cfg = FLConfig(**dict(BASE, **kw))
    shards, test = make_federated(cfg)
    eng = FLEngine(cfg, Transport(device=DEV), shards, test)
    kept, rows = [], []
    for _ in range(12):
        eng.run_round()
        rows += [o for o, _ in eng.last_decision.selected]
        kept += eng.last_aggregation.get("kept", [])
        assert eng.last_aggregation["aggregator"] == cfg.aggregator
    return eng.evaluate_global(), rows, kept


@pytest.fixture(scope="module")
def line():
    """A0 - m, with the attacked fedavg control checked against it."""
    a0, _, _ = _run(byzantine_clients=0)
    control, rows, _ = _run(**ATTACK)
    print(f"A0={a0:.4f} control={control:.4f} m={M_ACC:.4f}")
    assert set(rows) & ATTACKERS  # the committee passes attacker rows
    assert control < a0 - M_ACC, (control, a0)
    return a0 - M_ACC


@pytest.mark.parametrize("rule,extra", [
    ("trimmed_mean", dict(agg_trim=2)),
    ("median", {}),
    ("multi_krum", dict(agg_byzantine=2)),
])
def test_engine_rule_survives_scale_attack(line, rule, extra):
    """Each rule, standing alone (aggregate_count = needed_update_count),
    must hold the attack-free accuracy under two attackers publishing
    -4 * delta, and Krum must never keep an attacker. K = 6 rows, two of
    them attackers: trimmed mean and the median drop two per end, and
    multi-Krum assumes f = 2 (legal at K >= 2f + 2 = 6) and keeps four."""
    acc, rows, kept = _run(aggregator=rule, **extra, **ATTACK)
    print(f"{rule}: acc={acc:.4f} line={line:.4f}")
    assert set(rows) & ATTACKERS
    assert not set(kept) & ATTACKERS, sorted(set(kept) & ATTACKERS)
    assert acc >= line, (rule, acc, line)
