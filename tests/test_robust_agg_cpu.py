"""Robust aggregation on the CPU: config, the fallback oracles, the Krum
decision, and the engine (single process and world-2 gloo)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bflc_amd.config import FLConfig
from bflc_amd.fl.aggregate import (aggregate, effective_byzantine,
                                   effective_trim, krum_select)
from bflc_amd.ops import functional as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ---------------------------------------------------------------- config
def test_config_defaults_are_todays_behaviour():
    cfg = FLConfig()
    assert cfg.aggregator == "fedavg"
    assert cfg.agg_trim == 1 and cfg.agg_byzantine == 1
    assert cfg.byzantine_attack == "label_flip"
    assert cfg.byzantine_scale == -1.0


@pytest.mark.parametrize("kw", [
    dict(aggregator="krum"), dict(byzantine_attack="sign_flip"),
    dict(agg_trim=-1), dict(agg_byzantine=-1),
])
def test_config_rejects(kw):
    with pytest.raises(ValueError):
        FLConfig(**kw)


def test_config_robust_rules_limit_rows():
    big = dict(client_num=80, comm_count=4, needed_update_count=40,
               aggregate_count=33)
    FLConfig(**big)  # fedavg has no row limit
    for name in ("trimmed_mean", "median", "multi_krum"):
        with pytest.raises(ValueError):
            FLConfig(aggregator=name, **big)
        FLConfig(aggregator=name, **dict(big, aggregate_count=32))


def test_runtime_clamps():
    # trimmed mean: t = min(agg_trim, (K-1)//2)
    assert [effective_trim("trimmed_mean", K, 2) for K in range(1, 8)] == \
        [0, 0, 1, 1, 2, 2, 2]
    # median: t = (K-1)//2
    assert [effective_trim("median", K, 1) for K in range(1, 8)] == \
        [0, 0, 1, 1, 2, 2, 3]
    # multi-Krum: f = min(agg_byzantine, max(0, (K-2)//2)), K >= 2f + 2
    assert [effective_byzantine(K, 3) for K in range(1, 10)] == \
        [0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert effective_byzantine(6, 2) == 2   # two bad rows among six
    assert effective_byzantine(32, 1) == 1


# ------------------------------------------------------- order_stat_mean
def _osm_numpy(d: np.ndarray, t: int) -> np.ndarray:
    """Direct reference: per column sort (NaN last), fp32 ascending sum,
    fp32 division."""
    K, P = d.shape
    out = np.empty(P, dtype=np.float32)
    for i in range(P):
        col = d[:, i]
        s = np.concatenate([np.sort(col[~np.isnan(col)]),
                            col[np.isnan(col)]])
        acc = np.float32(0.0)
        for v in s[t:K - t]:
            acc = np.float32(acc + v)
        out[i] = np.float32(acc / np.float32(K - 2 * t))
    return out


@pytest.mark.parametrize("K,t", [(1, 0), (2, 0), (5, 0), (5, 1), (5, 2),
                                 (8, 3), (9, 4), (32, 1)])
def test_order_stat_mean_matches_numpy(K, t):
    g = torch.Generator().manual_seed(K * 10 + t)
    d = torch.randn(K, 37, generator=g)
    d[:, 3] = d[0, 3]          # a column of duplicates
    if K >= 3:
        d[2, 5] = d[0, 5]
    got = O.order_stat_mean(d, t).numpy()
    np.testing.assert_array_equal(got, _osm_numpy(d.numpy(), t))


def test_order_stat_mean_nan_rows():
    g = torch.Generator().manual_seed(1)
    d = torch.randn(5, 16, generator=g)
    one = d.clone()
    one[1] = float("nan")
    out = O.order_stat_mean(one, 1)
    assert torch.isfinite(out).all()     # the NaN row is trimmed away
    np.testing.assert_array_equal(out.numpy(), _osm_numpy(one.numpy(), 1))
    two = d.clone()
    two[1, 4:9] = float("nan")
    two[3, 4:9] = float("nan")
    out = O.order_stat_mean(two, 1)
    assert torch.isnan(out).tolist() == [4 <= i < 9 for i in range(16)]


def test_order_stat_mean_rejects_bad_t():
    d = torch.zeros(4, 3)
    for t in (-1, 2):
        with pytest.raises(ValueError):
            O.order_stat_mean(d, t)
    with pytest.raises(ValueError):
        O.order_stat_mean(torch.zeros(33, 3), 0)


def test_gram_and_wmean_fallbacks():
    g = torch.Generator().manual_seed(2)
    d = torch.randn(6, 11, generator=g)
    G = O.delta_gram(d)
    assert torch.equal(G, (d.double() @ d.double().t()).float())
    w = torch.tensor([1., 0., 2., 3., 0., 1.])
    bad = d.clone()
    bad[1] = float("nan")
    keep = w != 0
    got = O.masked_wmean(bad, w)
    ref = (w[keep, None].double() * d[keep].double()).sum(0) / w.sum().double()
    assert torch.isfinite(got).all()
    assert (got.double() - ref).abs().max() < 1e-6


# ------------------------------------------------------------------ Krum
def _gram(rows):
    d = torch.tensor(rows, dtype=torch.float64)
    return (d @ d.t()).tolist()


def test_krum_drops_outlier():
    rows = [[1.0, 0.0], [1.1, 0.0], [0.9, 0.1], [-40.0, 3.0], [1.0, 0.1]]
    assert krum_select(_gram(rows), 1) == [0, 1, 2, 4]


def test_krum_ties_resolve_by_position():
    # five identical rows: every score is 0, keep the first K - f
    rows = [[1.0, 2.0]] * 5
    assert krum_select(_gram(rows), 1) == [0, 1, 2, 3]
    # f is clamped to (K-2)//2 = 1 even when 2 are assumed
    assert krum_select(_gram(rows), 2) == [0, 1, 2, 3]


def test_krum_small_k_keeps_all():
    assert krum_select(_gram([[1.0]]), 1) == [0]
    assert krum_select(_gram([[1.0], [-50.0]]), 1) == [0, 1]
    # K = 3: f clamps to 0, all rows kept
    assert krum_select(_gram([[1.0], [2.0], [-50.0]]), 1) == [0, 1, 2]
    # K = 4: one bad row is the most that can be assumed
    assert krum_select(_gram([[1.0], [2.0], [-50.0], [1.5]]), 2) == [0, 1, 3]


def test_aggregate_rules_on_a_stack():
    g = torch.Generator().manual_seed(3)
    d = torch.randn(6, 10, generator=g)
    d[4] *= -30.0
    sel = [(f"node_{k}", float(k + 1)) for k in range(6)]
    w = torch.tensor([s[1] for s in sel])
    avg, info = aggregate(d, sel, FLConfig())
    assert torch.equal(avg, O.weighted_fedavg(d, w))
    assert info["aggregator"] == "fedavg"
    avg, info = aggregate(d, sel, FLConfig(aggregator="trimmed_mean",
                                           agg_trim=2))
    assert info["t"] == 2 and torch.equal(avg, O.order_stat_mean(d, 2))
    avg, info = aggregate(d, sel, FLConfig(aggregator="median"))
    assert info["t"] == 2 and torch.equal(avg, O.order_stat_mean(d, 2))
    avg, info = aggregate(d, sel, FLConfig(aggregator="multi_krum"))
    assert info["f"] == 1
    assert info["kept"] == ["node_0", "node_1", "node_2", "node_3", "node_5"]
    wk = w.clone()
    wk[4] = 0
    assert torch.equal(avg, O.masked_wmean(d, wk))


# ---------------------------------------------------------------- engine
MLP = dict(client_num=8, comm_count=2, needed_update_count=6,
           model="mlp", n_features=32, n_class=8, samples_per_client=256,
           batch_size=128, eval_samples=1024, learning_rate=0.05)


def _engine(cfg):
    from bflc_amd.comm import Transport
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    shards, test = make_federated(cfg)
    return FLEngine(cfg, Transport(device=CPU), shards, test), shards


def test_scale_attack_keeps_labels_and_marks_shards():
    from bflc_amd.data import make_federated
    honest, _ = make_federated(FLConfig(aggregate_count=6, **MLP))
    scaled, _ = make_federated(FLConfig(
        aggregate_count=6, byzantine_clients=2, byzantine_attack="scale",
        byzantine_scale=-4.0, **MLP))
    flipped, _ = make_federated(FLConfig(
        aggregate_count=6, byzantine_clients=2, **MLP))
    assert [s.byzantine for s in scaled] == [False] * 6 + [True] * 2
    for i in (6, 7):
        assert torch.equal(scaled[i].y, honest[i].y)
        assert not torch.equal(flipped[i].y, honest[i].y)


# one committee member, seven trainers: K = 7 rows, so multi-Krum may
# assume f = 2 = (7 - 3) // 2 and trimmed mean may drop 2 per end
WIDE = dict(MLP, comm_count=1, needed_update_count=7, aggregate_count=7)


@pytest.mark.parametrize("rule", ["trimmed_mean", "median", "multi_krum"])
def test_engine_cpu_scale_attack(rule):
    cfg = FLConfig(aggregator=rule, agg_trim=2, agg_byzantine=2,
                   byzantine_clients=2, byzantine_attack="scale",
                   byzantine_scale=-4.0, **WIDE)
    eng, shards = _engine(cfg)
    attackers = {"node_6", "node_7"}
    n_attacker_rows = 0
    for _ in range(6):
        eng.run_round()
        info = eng.last_aggregation
        assert info["aggregator"] == rule and info["rows"] == 7
        picked = {o for o, _ in eng.last_decision.selected}
        n_attacker_rows += len(picked & attackers)
        if rule == "multi_krum":
            assert info["f"] == 2
            assert len(info["kept"]) == 5
            assert not set(info["kept"]) & attackers, info
            assert set(info["kept"]) <= picked
        else:
            assert info["t"] == (2 if rule == "trimmed_mean" else 3)
    assert n_attacker_rows > 0  # the committee really passed attacker rows
    assert torch.isfinite(eng.global_flat).all()
    assert eng.evaluate_global() > 0.9  # the attack-free run reaches 1.0


def test_scale_attack_scales_the_published_delta():
    """Same seed, honest labels: with fedavg over every row the scaled
    run's first-round aggregate differs from the attack-free one by
    exactly the attackers' rows."""
    base = FLConfig(aggregate_count=6, **MLP)
    atk = FLConfig(aggregate_count=6, byzantine_clients=2,
                   byzantine_attack="scale", byzantine_scale=-4.0, **MLP)
    e0, _ = _engine(base)
    e1, _ = _engine(atk)
    e0.run_round()
    e1.run_round()
    assert {"node_6", "node_7"} & {o for o, _ in e1.last_decision.selected}
    assert not torch.equal(e0.global_flat, e1.global_flat)


def test_default_fields_leave_the_bits_alone():
    plain = FLConfig(aggregate_count=3, byzantine_clients=2, **MLP)
    spelled = FLConfig(aggregate_count=3, byzantine_clients=2,
                       aggregator="fedavg", agg_trim=1, agg_byzantine=1,
                       byzantine_attack="label_flip", byzantine_scale=-1.0,
                       **MLP)
    a, _ = _engine(plain)
    b, _ = _engine(spelled)
    a.run(3)
    b.run(3)
    assert torch.equal(a.global_flat, b.global_flat)
    # and they are the bits of the two lines aggregate() replaced
    c, _ = _engine(plain)
    for _ in range(3):
        c.run_round()
        sel = c.last_decision.selected
        assert c.last_aggregation == {"aggregator": "fedavg",
                                      "rows": len(sel)}
    assert torch.equal(a.global_flat, c.global_flat)


# ------------------------------------------------------------ world-2 gloo
WORKER = r"""
import json, os, sys
import torch
sys.path.insert(0, {repo!r})
from bflc_amd.config import FLConfig
from bflc_amd.comm import Transport
from bflc_amd.data import make_federated
from bflc_amd.fl import FLEngine

cfg = FLConfig(client_num=8, comm_count=1, needed_update_count=7,
               aggregate_count=7, aggregator="multi_krum", agg_byzantine=2,
               byzantine_clients=2, byzantine_attack="scale",
               byzantine_scale=-4.0, model="mlp", n_features=32, n_class=8,
               samples_per_client=64, batch_size=32, eval_samples=64,
               learning_rate=0.05)
shards, test = make_federated(cfg)
t = Transport(backend="gloo", device=torch.device("cpu"))
eng = FLEngine(cfg, t, shards, test)
kept = []
for _ in range(3):
    eng.run_round()
    kept.append(eng.last_aggregation["kept"])
torch.save(eng.global_flat, os.path.join({outdir!r}, f"flat{{t.rank}}.pt"))
with open(os.path.join({outdir!r}, f"rank{{t.rank}}.json"), "w") as f:
    json.dump({{"kept": kept, "epoch": eng.ledger.epoch}}, f)
t.barrier()
t.close()
"""


def test_world2_multi_krum_replicas_identical(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(repo=REPO, outdir=str(tmp_path)))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT="29561",
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen(
            [sys.executable, str(script)], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err.decode()[-3000:]
    r = [json.load(open(tmp_path / f"rank{i}.json")) for i in range(2)]
    assert r[0]["epoch"] == r[1]["epoch"] == 3
    assert r[0]["kept"] == r[1]["kept"]
    assert not {"node_6", "node_7"} & {o for k in r[0]["kept"] for o in k}
    f0 = torch.load(tmp_path / "flat0.pt")
    f1 = torch.load(tmp_path / "flat1.pt")
    assert torch.equal(f0, f1)  # bitwise
