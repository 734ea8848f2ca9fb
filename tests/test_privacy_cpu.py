"""Differential privacy without a GPU: the generator's known answers on
the CPU path, the accountant, the config checks, and the CPU engine with
the feature on (clip bound, determinism, key dependence, metrics, and a
two-process gloo run).

The float64 oracle of the noise is written out here from the definition
in DESIGN.md "Round-13"; it shares no code with bflc_amd.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF

# (counter, key) -> words
KNOWN = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_ref(ctr, key):
    """Philox4x32-10 on Python integers."""
    c, (k0, k1) = list(ctr), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1,
             p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return tuple(c)


def z_ref(n, seed, stream, epoch):
    """z(0..n-1) in float64, one coordinate at a time."""
    out = []
    for b in range((n + 3) // 4):
        x = philox_ref((b & M32, b >> 32, stream, epoch),
                       (seed & M32, (seed >> 32) & M32))
        u = [((w >> 8) + 0.5) * 2.0 ** -24 for w in x]
        r0 = math.sqrt(-2.0 * math.log(u[0]))
        r1 = math.sqrt(-2.0 * math.log(u[2]))
        out += [r0 * math.cos(2 * math.pi * u[1]),
                r0 * math.sin(2 * math.pi * u[1]),
                r1 * math.cos(2 * math.pi * u[3]),
                r1 * math.sin(2 * math.pi * u[3])]
    return np.array(out[:n])


# ------------------------------------------------------------------ ops
def test_oracle_reproduces_the_known_answers():
    for ctr, key, words in KNOWN:
        assert philox_ref(ctr, key) == words


def test_philox_known_answers_cpu_path():
    from bflc_amd.ops import dp_philox_words
    for ctr, key, words in KNOWN:
        got = dp_philox_words(torch.tensor([ctr], dtype=torch.int64), *key)
        assert got.dtype == torch.int64 and got.shape == (1, 4)
        assert tuple(got[0].tolist()) == words


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_privatize_cpu_follows_the_definition(n):
    from bflc_amd.ops import dp_privatize_
    one = torch.ones(1)
    d = torch.zeros(n)
    dp_privatize_(d, one, 1.0, 42, 7, 123)
    ref = z_ref(n, 42, 7, 123)
    # the CPU path rounds the float64 value once
    assert np.array_equal(d.numpy(), ref.astype(np.float32))
    # clip + noise: fmaf(coef, d, sigma * z) with one rounding
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    y = x.clone()
    coef = torch.tensor([0.25])
    dp_privatize_(y, coef, 0.5, 42, 7, 123)
    want = (0.25 * x.double().numpy()
            + (np.float32(0.5) * ref.astype(np.float32)).astype(np.float64))
    assert np.array_equal(y.numpy(), want.astype(np.float32))
    # sigma == 0: one multiply; coef == 0: the old value is not used
    y = x.clone()
    dp_privatize_(y, coef, 0.0, 42, 7, 123)
    assert torch.equal(y, x * 0.25)
    y = torch.full((n,), float("nan"))
    dp_privatize_(y, torch.zeros(1), 1.0, 42, 7, 123)
    assert torch.equal(y, d)


def test_extract_sumsq_and_clip_final_cpu_match_the_two_pass_chain():
    from bflc_amd import ops as O
    gen = torch.Generator().manual_seed(3)
    g, w = torch.randn(1025, generator=gen), torch.randn(1025, generator=gen)
    a, b = torch.empty(1025), torch.empty(1025)
    ca, cb = torch.empty(2), torch.empty(2)
    O.functional.delta_extract_(a, g, w, 0.05)
    O.grad_clip_coef_(a, 3.0, ca)
    part = torch.empty(O.functional.sumsq_partials(1025, "cpu"))
    O.delta_extract_sumsq_(b, g, w, 0.05, part)
    O.grad_clip_final_(part, 3.0, cb)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert 0 < float(ca[0]) < 1


# ----------------------------------------------------------- accountant
def test_gaussian_epsilon():
    from bflc_amd.fl.privacy import gaussian_epsilon
    assert abs(gaussian_epsilon(1.0, 1, 1e-5) - 5.2986) <= 1e-4
    for z, T, d in [(0.5, 3, 1e-5), (2.0, 100, 1e-6), (1.3, 17, 1e-3)]:
        closed = T / (2 * z * z) + math.sqrt(2 * T * math.log(1 / d)) / z
        assert gaussian_epsilon(z, T, d) == pytest.approx(closed, rel=1e-12)
    eps_t = [gaussian_epsilon(1.0, T, 1e-5) for T in (1, 2, 10, 100)]
    assert eps_t == sorted(eps_t) and len(set(eps_t)) == 4
    eps_z = [gaussian_epsilon(z, 10, 1e-5) for z in (0.25, 0.5, 1.0, 4.0)]
    assert eps_z == sorted(eps_z, reverse=True) and len(set(eps_z)) == 4
    assert gaussian_epsilon(0.0, 1, 1e-5) == math.inf


def test_central_sigma_and_noise_key():
    from bflc_amd.config import FLConfig
    from bflc_amd.fl.privacy import central_sigma, noise_key
    cfg = FLConfig(dp_clip=0.02, dp_noise_multiplier=1.5, dp_mode="central",
                   learning_rate=0.01)
    sel = [("node_1", 100.0), ("node_4", 300.0), ("node_2", 100.0)]
    assert central_sigma(sel, cfg) == pytest.approx(1.5 * 2.0 * 300 / 500)
    assert noise_key(FLConfig(dp_seed=12345)) == 12345
    keys = {noise_key(FLConfig(seed=s)) for s in range(8)}
    assert len(keys) == 8 and all(0 <= k < 1 << 64 for k in keys)
    assert noise_key(FLConfig(seed=3)) == noise_key(FLConfig(seed=3))


# --------------------------------------------------------------- config
def test_config_defaults_are_off():
    from bflc_amd.config import FLConfig
    cfg = FLConfig()
    assert cfg.dp_active is False
    assert (cfg.dp_clip, cfg.dp_noise_multiplier, cfg.dp_mode,
            cfg.dp_delta, cfg.dp_seed) == (0.0, 0.0, "local", 1e-5, None)
    assert FLConfig(dp_clip=0.1).dp_active is True
    assert FLConfig.from_dict(FLConfig(dp_clip=0.1, dp_seed=9).to_dict()
                              ).dp_seed == 9


@pytest.mark.parametrize("kw", [
    dict(dp_clip=-1.0),
    dict(dp_clip=1.0, dp_noise_multiplier=-0.5),
    dict(dp_noise_multiplier=1.0),                       # needs dp_clip
    dict(dp_clip=1.0, dp_mode="global"),
    dict(dp_clip=1.0, dp_mode="central", aggregator="median"),
    dict(dp_clip=1.0, dp_mode="central", aggregator="trimmed_mean"),
    dict(dp_clip=1.0, dp_mode="central", aggregator="multi_krum"),
    dict(dp_clip=1.0, dp_delta=0.0),
    dict(dp_clip=1.0, dp_delta=1.0),
    dict(dp_clip=1.0, dp_delta=-1e-5),
])
def test_config_rejections(kw):
    from bflc_amd.config import FLConfig
    with pytest.raises(ValueError):
        FLConfig(**kw)


# --------------------------------------------------------------- engine
LR = 0.05
S = 0.01           # model-space bound; the published rows see S / LR


def _cfg(**kw):
    from bflc_amd.config import FLConfig
    base = dict(model="mlp", n_features=16, n_class=4, learning_rate=LR,
                samples_per_client=64, batch_size=32, eval_samples=64,
                dp_clip=S)
    base.update(kw)
    return FLConfig.for_world(8, **base)


def _engine(cfg, metrics_path=None):
    from bflc_amd.comm import Transport
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    shards, test = make_federated(cfg)
    return FLEngine(cfg, Transport(device=torch.device("cpu")), shards, test,
                    metrics_path=metrics_path)


def test_engine_clip_bounds_every_gathered_row(tmp_path):
    """Every row the all-gather publishes has L2 norm <= S / lr, up to
    fp32 rounding: the sum of squares of P positive terms carries at most
    (P - 1) 2^-24 relative error in any order (half of it on the norm),
    sqrt, the divide and the multiply one rounding each."""
    log = str(tmp_path / "m.jsonl")
    eng = _engine(_cfg(), metrics_path=log)
    rows = []
    gather = eng.t.all_gather_tensor

    def spy(stack):
        out = gather(stack)
        rows.extend(r.clone() for rank_rows in out for r in rank_rows)
        return out

    eng.t.all_gather_tensor = spy
    coefs = []
    for _ in range(3):
        eng.run_round()
        assert eng.last_privacy["mode"] == "local"
        assert eng.last_privacy["clip"] == S
        coefs += list(eng.last_privacy["clip_coef"].values())
    P = eng.global_flat.numel()
    bound = (S / LR) * (1 + (P / 2 + 4) * 2.0 ** -24)
    assert len(rows) == 3 * eng.cfg.needed_update_count
    norms = [float(r.double().norm()) for r in rows]
    assert max(norms) <= bound, (max(norms), bound)
    # the bound was active (else the test shows nothing) and is reported
    assert len(coefs) == len(rows) and min(coefs) < 1.0
    assert all(0.0 < c <= 1.0 for c in coefs)
    # clip only: no noise, epsilon is infinite, and it is in the record
    recs = [json.loads(l) for l in open(log)]
    assert [r["privacy"]["epsilon"] for r in recs] == [math.inf] * 3


def test_engine_noise_is_reproducible_and_keyed(tmp_path):
    from bflc_amd.fl.privacy import gaussian_epsilon
    log = str(tmp_path / "m.jsonl")

    def run(path=None, **kw):
        eng = _engine(_cfg(dp_noise_multiplier=0.5, **kw), metrics_path=path)
        eng.run(3)
        return eng

    a, b = run(log), run()
    assert torch.equal(a.global_flat, b.global_flat)
    assert not torch.equal(a.global_flat, run(dp_seed=1).global_flat)
    assert not torch.equal(a.global_flat,
                           _run_plain(dp_noise_multiplier=0.0).global_flat)
    recs = [json.loads(l) for l in open(log)]
    assert [r["privacy"]["epsilon"] for r in recs] == \
        [gaussian_epsilon(0.5, T, 1e-5) for T in (1, 2, 3)]
    assert a.last_privacy["epsilon"] == gaussian_epsilon(0.5, 3, 1e-5)
    assert recs[-1]["privacy"]["noise_multiplier"] == 0.5


def _run_plain(**kw):
    eng = _engine(_cfg(**kw))
    eng.run(3)
    return eng


def test_engine_central_noise_is_the_defined_vector():
    """One round from the same state with z > 0 and z = 0: the two global
    models differ by lr * central_sigma * z(.; 0xFFFFFFFF, epoch)."""
    from bflc_amd.fl.privacy import central_sigma, noise_key
    a = _engine(_cfg(dp_mode="central", dp_noise_multiplier=2.0))
    b = _engine(_cfg(dp_mode="central"))
    a.run_round()
    b.run_round()
    assert a.last_decision.selected == b.last_decision.selected
    cs = central_sigma(a.last_decision.selected, a.cfg)
    assert cs > 0 and a.last_privacy["central_sigma"] == cs
    P = a.global_flat.numel()
    z = z_ref(P, noise_key(a.cfg), 0xFFFFFFFF, 0)
    diff = (b.global_flat.double() - a.global_flat.double()).numpy()
    # each model is rounded once (half an ulp each)
    ulp = np.spacing(np.maximum(np.abs(a.global_flat.numpy()),
                                np.abs(b.global_flat.numpy())))
    tol = 2e-5 * LR * cs + ulp.astype(np.float64)
    assert np.all(np.abs(diff - LR * cs * z) <= tol)


def test_default_engine_runs_no_privacy_code(monkeypatch):
    from bflc_amd.config import FLConfig
    from bflc_amd.ops import functional as F

    def boom(*a, **k):
        raise AssertionError("privacy op on the default path")

    for name in ("delta_extract_sumsq_", "dp_privatize_", "grad_clip_final_"):
        monkeypatch.setattr(F, name, boom)
    cfg = FLConfig.for_world(8, model="mlp", n_features=16, n_class=4,
                             samples_per_client=64, batch_size=32,
                             eval_samples=64)
    eng = _engine(cfg)
    eng.run(1)
    assert eng.last_privacy is None and not eng._dp_bufs


# ---------------------------------------------------------- distributed
WORKER = r"""
import json, os, sys
import torch
sys.path.insert(0, {repo!r})
from bflc_amd.config import FLConfig
from bflc_amd.comm import Transport
from bflc_amd.data import make_federated
from bflc_amd.fl import FLEngine

cfg = FLConfig.for_world(2, **{cfg_kw!r})
shards, test = make_federated(cfg)
t = Transport(backend="gloo", device=torch.device("cpu"))
eng = FLEngine(cfg, t, shards, test)
eng.run(3)
out = {{"rank": t.rank, "epoch": eng.ledger.epoch,
        "flat": eng.global_flat.view(torch.int32).tolist(),
        "epsilon": eng.last_privacy["epsilon"]}}
with open(os.path.join({outdir!r}, f"rank{{t.rank}}.json"), "w") as f:
    json.dump(out, f)
t.barrier()
t.close()
"""

W2_CFG = dict(model="mlp", n_features=16, n_class=4, samples_per_client=64,
              batch_size=32, eval_samples=64, learning_rate=LR, dp_clip=S,
              dp_noise_multiplier=0.5)


def test_world2_local_noise_replicas_identical(tmp_path):
    """Two gloo ranks with local noise on: bitwise identical replicas,
    equal to the single-process run — the noise is keyed by the client
    index, never by the rank or the world size."""
    from bflc_amd.config import FLConfig
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(repo=REPO, outdir=str(tmp_path),
                                    cfg_kw=W2_CFG))
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
    r0, r1 = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    assert r0["epoch"] == r1["epoch"] == 3
    assert r0["flat"] == r1["flat"]
    assert r0["epsilon"] == r1["epsilon"]
    eng = _engine(FLConfig.for_world(2, **W2_CFG))
    eng.run(3)
    assert eng.global_flat.view(torch.int32).tolist() == r0["flat"]
