"""Differential privacy on the GPU: the generator bitwise, the normal
transform against a float64 oracle, independence of launch geometry and
base alignment, first- and second-order statistics, the clip, and the
engine in local and central mode.

The float64 oracle of z(i) is written out here from the definition in
DESIGN.md "Round-13"; it shares no code with bflc_amd.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
M32 = 0xFFFFFFFF
CENTRAL = 0xFFFFFFFF
SIZES = [1, 3, 4, 5, 1023, 1025, 4099, 428350]
# z is within 2e-5 of the oracle: |z| <= sqrt(-2 ln 2^-25) = 5.89, and the
# fp32 errors of the angle, of sin/cos (<= 2 ulp) and of the radius (a few
# 1e-7 relative) sum to under 5e-6
Z_TOL = 2e-5

KNOWN = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_np(ctr, k0, k1):
    """Philox4x32-10 on an [N, 4] uint64 array of 32-bit counters."""
    c = [ctr[:, j].copy() for j in range(4)]
    mask, sh = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask,
             (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, axis=1)


def z_oracle(n, seed, stream, epoch, start=0):
    """z(start .. start + n - 1) in float64 (start a multiple of 4)."""
    assert start % 4 == 0
    b = np.arange(start // 4, (start + n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([b & np.uint64(M32), b >> np.uint64(32),
                    np.full(b.size, stream, dtype=np.uint64),
                    np.full(b.size, epoch, dtype=np.uint64)], axis=1)
    x = philox_np(ctr, seed & M32, (seed >> 32) & M32)
    u = ((x >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r0 = np.sqrt(-2.0 * np.log(u[:, 0]))
    r1 = np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0),
                  r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
    return z.reshape(-1)[:n]


def _ops():
    from bflc_amd import ops
    return ops


def _scal(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _noise(n, seed, stream, epoch, sigma=1.0):
    d = torch.zeros(n, device=DEV)
    _ops().dp_privatize_(d, _scal(1.0), sigma, seed, stream, epoch)
    return d


@pytest.fixture(scope="module")
def big():
    """One run above a full grid-stride pass of dp_privatize_ (2048
    blocks x 256 lanes x 4 coordinates = 2^21), with a ragged tail."""
    n = (1 << 21) + 4096 + 3
    return n, _noise(n, 42, 7, 123)


# ------------------------------------------------------------ generator
def test_oracle_reproduces_the_known_answers():
    for ctr, key, words in KNOWN:
        got = philox_np(np.array([ctr], dtype=np.uint64), *key)
        assert tuple(int(v) for v in got[0]) == words


def test_philox_words_known_answers_on_device():
    for ctr, key, words in KNOWN:
        c = torch.tensor([ctr] * 300, dtype=torch.int64, device=DEV)
        got = _ops().dp_philox_words(c, *key).cpu()
        assert got.shape == (300, 4)
        assert all(tuple(r) == words for r in got.tolist())


def test_philox_words_match_the_oracle_on_random_counters():
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64)
    got = _ops().dp_philox_words(
        torch.from_numpy(ctr.astype(np.int64)).to(DEV), 0xdeadbeef, 0x12345)
    assert np.array_equal(got.cpu().numpy().astype(np.uint64),
                          philox_np(ctr, 0xdeadbeef, 0x12345))


# ------------------------------------------------------------ transform
@pytest.mark.parametrize("n", SIZES)
def test_normals_match_the_float64_oracle(n):
    got = _noise(n, 42, 7, 123).cpu().double().numpy()
    err = np.abs(got - z_oracle(n, 42, 7, 123)).max()
    print(f"n={n}: max |z - oracle| = {err:.3e}")
    assert err <= Z_TOL


def test_normals_beyond_one_grid_stride_pass(big):
    n, d = big
    start = 1 << 21
    got = d[start:].cpu().double().numpy()
    err = np.abs(got - z_oracle(n - start, 42, 7, 123, start=start)).max()
    print(f"second pass: max |z - oracle| = {err:.3e}")
    assert err <= Z_TOL


def test_geometry_independence(big):
    """A coordinate's noise does not depend on the vector's length, hence
    not on the grid: bitwise equal prefixes."""
    _, d = big
    small = _noise(4099, 42, 7, 123)
    assert torch.equal(small, d[:4099])
    assert torch.equal(_noise(1 << 20, 42, 7, 123), d[:1 << 20])


@pytest.mark.parametrize("n", SIZES)
def test_base_alignment_independence(n):
    """A view one float into a buffer takes the dword path: same bits."""
    buf = torch.zeros(n + 1, device=DEV)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    _ops().dp_privatize_(view, _scal(1.0), 1.0, 42, 7, 123)
    assert torch.equal(view, _noise(n, 42, 7, 123))
    assert float(buf[0]) == 0.0


def test_row_view_of_a_stack():
    """Row 1 of a [2, 428350] stack starts 8 bytes off a 16-byte
    boundary (P % 4 == 2, the 62-class FEMNIST CNN)."""
    P = 428350
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, P, generator=gen).to(DEV)
    buf = x.clone()
    assert buf[1].data_ptr() % 16 == 8
    coef = _scal(0.5)
    _ops().dp_privatize_(buf[1], coef, 0.75, 42, 3, 9)
    want = x[1].clone()
    _ops().dp_privatize_(want, coef, 0.75, 42, 3, 9)
    assert torch.equal(buf[1], want)
    assert torch.equal(buf[0], x[0])
    ref = 0.5 * x[1].double().cpu().numpy() \
        + 0.75 * z_oracle(P, 42, 3, 9)
    err = np.abs(want.cpu().double().numpy() - ref)
    assert err.max() <= 0.75 * Z_TOL + 2.0 ** -24 * np.abs(ref).max()


# ----------------------------------------------------------- statistics
STREAMS = [(0, 0), (1, 0), (0, 1), (7, 123), (CENTRAL, 5)]


def test_statistics():
    """n = 2^20 per stream, fixed seeds (deterministic); the float64
    oracle passes the same bounds. 5-sigma bounds of the estimators."""
    n = 1 << 20
    zs = [_noise(n, 42, s, e).double() for s, e in STREAMS]
    b_mean, b_var, b_corr = 5 / math.sqrt(n), 5 * math.sqrt(2 / n), \
        5 / math.sqrt(n)
    for (s, e), z in zip(STREAMS, zs):
        mean, var = float(z.mean()), float(z.var(unbiased=False))
        print(f"stream {s:#x} epoch {e}: mean {mean:+.5f} var {var:.5f}")
        assert abs(mean) <= b_mean
        assert abs(var - 1.0) <= b_var
    zc = [(z - z.mean()) / z.std(unbiased=False) for z in zs]
    for i in range(len(zc)):
        for j in range(i + 1, len(zc)):
            c = float((zc[i] * zc[j]).mean())
            print(f"corr streams {i},{j}: {c:+.5f}")
            assert abs(c) <= b_corr
        for lag in (1, 4):
            c = float((zc[i][:-lag] * zc[i][lag:]).mean())
            print(f"corr stream {i} lag {lag}: {c:+.5f}")
            assert abs(c) <= b_corr


# ----------------------------------------------------------------- clip
def _sumsq_slack(n):
    """Relative slack of a norm computed through the fixed-order fp32 sum
    of squares: a lane chain of per_lane terms and depth further adds
    bound the sum's relative error by (per_lane + depth) 2^-24 (half of
    it on the norm); sqrt, the +1e-6, the divide and the final multiply
    round once each."""
    from bflc_amd.ops import functional as F
    _, per_lane, depth = F.grad_sumsq_geom(n)
    return ((per_lane + depth) / 2 + 4) * 2.0 ** -24


@pytest.mark.parametrize("n", SIZES)
def test_clip_only(n):
    O = _ops()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen).to(DEV)
    if n > 1:
        x[n - 1] = -0.0
    norm = float(x.double().norm())
    # within the bound: coef == 1 and the vector keeps its bits
    coef = torch.empty(2, device=DEV)
    O.grad_clip_coef_(x, 2.0 * norm + 1.0, coef)
    assert float(coef[0]) == 1.0
    y = x.clone()
    O.dp_privatize_(y, coef, 0.0, 42, 0, 0)
    assert torch.equal(y.view(torch.int32), x.view(torch.int32))
    # outside: one fp32 multiply per element, norm back inside the bound
    clip = 0.25 * norm
    O.grad_clip_coef_(x, clip, coef)
    c = coef[:1].clone()
    assert 0.0 < float(c) < 1.0
    O.dp_privatize_(y, coef, 0.0, 42, 0, 0)
    assert torch.equal(y.view(torch.int32), (x * c).view(torch.int32))
    assert float(y.double().norm()) <= clip * (1 + _sumsq_slack(n))


@pytest.mark.parametrize("n", [5, 4099])
def test_nonfinite_update_publishes_pure_noise(n):
    O = _ops()
    x = torch.randn(n, device=DEV)
    x[n // 2] = float("nan")
    coef = torch.empty(2, device=DEV)
    O.grad_clip_coef_(x, 1.0, coef)
    assert float(coef[0]) == 0.0
    O.dp_privatize_(x, coef, 0.5, 42, 2, 6)
    assert bool(torch.isfinite(x).all())
    assert torch.equal(x, _noise(n, 42, 2, 6, sigma=0.5))
    # and with no noise a non-finite update publishes zeros
    y = torch.full((n,), float("inf"), device=DEV)
    O.dp_privatize_(y, coef, 0.0, 42, 2, 6)
    assert torch.equal(y, torch.zeros(n, device=DEV))


def _grid_stride_size():
    from bflc_amd.ops import functional as F
    blocks, _, _ = F.grad_sumsq_geom(1 << 40)
    return blocks * 256 * 8 + 8 * 37 + 5   # second granule on some lanes


@pytest.mark.parametrize("n", SIZES + ["grid_stride"])
def test_extract_sumsq_matches_the_two_pass_chain(n):
    """delta_extract_sumsq_ + grad_clip_final_ == delta_extract_ +
    grad_clip_coef_: out, sum of squares and coefficient, bitwise."""
    O = _ops()
    if n == "grid_stride":
        n = _grid_stride_size()
    gen = torch.Generator().manual_seed(n % 1000)
    g = torch.randn(n, generator=gen).to(DEV)
    w = (g + 0.01 * torch.randn(n, generator=gen).to(DEV))
    lr = 0.003
    a, b = torch.empty_like(g), torch.empty_like(g)
    ca, cb = torch.empty(2, device=DEV), torch.empty(2, device=DEV)
    O.functional.delta_extract_(a, g, w, lr)
    clip = 0.5 * float(a.double().norm()) + 1e-3
    O.grad_clip_coef_(a, clip, ca)
    part = torch.empty(O.functional.sumsq_partials(n, DEV), device=DEV)
    O.delta_extract_sumsq_(b, g, w, lr, part)
    O.grad_clip_final_(part, clip, cb)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ca.view(torch.int32), cb.view(torch.int32))
    assert float(ca[1]) > 0 and 0 < float(ca[0]) <= 1


def test_binding_guards():
    O = _ops()
    d = torch.zeros(16, device=DEV)
    one = _scal(1.0)
    with pytest.raises((RuntimeError, ValueError)):
        O.dp_privatize_(d[::2], one, 1.0, 1, 0, 0)        # not contiguous
    with pytest.raises((RuntimeError, ValueError)):
        O.dp_privatize_(d.double(), one, 1.0, 1, 0, 0)
    with pytest.raises((RuntimeError, ValueError)):
        O.dp_privatize_(d, one, 1.0, 1, 1 << 32, 0)       # 32-bit stream
    with pytest.raises((RuntimeError, ValueError)):
        O.dp_privatize_(d, one, -1.0, 1, 0, 0)
    part = torch.empty(3, device=DEV)                     # wrong length
    with pytest.raises(RuntimeError):
        O.delta_extract_sumsq_(d, d.clone(), d.clone(), 0.1, part)
    big = torch.zeros(17, device=DEV)
    with pytest.raises(RuntimeError):                     # misaligned
        O.delta_extract_sumsq_(big[1:], d, d.clone(), 0.1,
                               torch.empty(1, device=DEV))


# --------------------------------------------------------------- engine
LR = 0.05
S = 0.025          # published rows are clipped to S / LR = 0.5


def _femnist_cfg(**kw):
    from bflc_amd.config import FLConfig
    base = dict(model="femnist_cnn", n_class=62, samples_per_client=128,
                batch_size=64, eval_samples=128, partition="dirichlet",
                comm_count=2, needed_update_count=6, aggregate_count=4,
                learning_rate=LR, dp_clip=S)
    base.update(kw)
    return FLConfig.for_world(8, **base)


def _engine(cfg):
    from bflc_amd.comm import Transport
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    shards, test = make_federated(cfg)
    return FLEngine(cfg, Transport(device=DEV), shards, test)


def test_engine_local_mode_is_reproducible():
    from bflc_amd.fl.privacy import gaussian_epsilon

    def run(**kw):
        eng = _engine(_femnist_cfg(dp_noise_multiplier=0.5, **kw))
        eng.run(2)
        return eng

    a, b = run(), run()
    assert torch.equal(a.global_flat, b.global_flat)
    assert bool(torch.isfinite(a.global_flat).all())
    assert not torch.equal(a.global_flat, run(dp_seed=7).global_flat)
    assert a.last_privacy["epsilon"] == gaussian_epsilon(0.5, 2, 1e-5)
    assert a.last_privacy["mode"] == "local"


def test_engine_published_rows_are_clipped():
    eng = _engine(_femnist_cfg())
    rows = []
    gather = eng.t.all_gather_tensor

    def spy(stack):
        out = gather(stack)
        rows.extend(r.clone() for rank_rows in out for r in rank_rows)
        return out

    eng.t.all_gather_tensor = spy
    coefs = []
    for _ in range(2):
        eng.run_round()
        coefs += list(eng.last_privacy["clip_coef"].values())
    assert len(rows) == 2 * eng.cfg.needed_update_count == len(coefs)
    bound = (S / LR) * (1 + _sumsq_slack(eng.global_flat.numel()))
    norms = [float(r.double().norm()) for r in rows]
    print("published norms", norms, "coefs", coefs)
    assert max(norms) <= bound
    assert min(coefs) < 1.0 and all(0.0 < c <= 1.0 for c in coefs)


def test_engine_central_noise_is_the_defined_vector():
    from bflc_amd.fl.privacy import (central_sigma, gaussian_epsilon,
                                     noise_key)
    z = 2.0
    a = _engine(_femnist_cfg(dp_mode="central", dp_noise_multiplier=z))
    b = _engine(_femnist_cfg(dp_mode="central"))
    a.run_round()
    b.run_round()
    assert a.last_decision.selected == b.last_decision.selected
    cs = central_sigma(a.last_decision.selected, a.cfg)
    assert cs > 0 and a.last_privacy["central_sigma"] == cs
    ga, gb = a.global_flat.cpu().numpy(), b.global_flat.cpu().numpy()
    zref = z_oracle(ga.size, noise_key(a.cfg), CENTRAL, 0)
    diff = gb.astype(np.float64) - ga.astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(ga), np.abs(gb))).astype(np.float64)
    err = np.abs(diff - LR * cs * zref)
    print(f"central: max err {err.max():.3e}, "
          f"noise scale {LR * cs:.3e}")
    assert np.all(err <= Z_TOL * LR * cs + ulp)
    assert a.last_privacy["epsilon"] == gaussian_epsilon(z, 1, 1e-5)
