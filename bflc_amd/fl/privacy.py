"""Differential privacy of the published updates (DP-FedAvg, McMahan et
al. 2018): host-side pieces. The kernels are in csrc/hip/privacy.hip,
the noise definition in DESIGN.md "Round-13".

A client's model-space update W0 - W is clipped to L2 norm S =
`dp_clip`; the published delta is (W0 - W) / lr, so the kernels clip to
S / lr. Gaussian noise of standard deviation z * S (z =
`dp_noise_multiplier`) is added either by every client to its own
clipped update (`dp_mode="local"`) or once, identically on every
replica, to the aggregate (`dp_mode="central"`).

Everything here is a pure function of the config, the ledger epoch and
the ledger's decision, so it is identical on every rank and needs no
checkpoint state.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

_M64 = (1 << 64) - 1


def noise_key(cfg) -> int:
    """The 64-bit Philox key. `dp_seed=None` derives it from `cfg.seed`
    (splitmix64 of the seed, so that seeds 0, 1, 2 give unrelated keys):
    every participant can compute that key — reproducible simulation,
    not secrecy."""
    if cfg.dp_seed is not None:
        return int(cfg.dp_seed) & _M64
    x = (int(cfg.seed) + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def kernel_clip(cfg) -> float:
    """The L2 bound in the published delta's units: S / lr."""
    return float(cfg.dp_clip) / float(cfg.learning_rate)


def local_sigma(cfg) -> float:
    """Noise standard deviation a client adds to its published delta:
    z * S / lr in local mode, 0 in central mode (clients only clip)."""
    if cfg.dp_mode != "local":
        return 0.0
    return float(cfg.dp_noise_multiplier) * kernel_clip(cfg)


def central_sigma(selected: Sequence[Tuple[str, float]], cfg) -> float:
    """Noise standard deviation on the weighted mean of the selected
    rows, in the delta's units: z * (S / lr) * max_k w_k / sum_k w_k.
    One client moves the mean by at most (S / lr) * w_k / sum(w), so
    this is z times the mean's sensitivity given the selection."""
    ws = [float(w) for _, w in selected]
    tot = sum(ws)
    if not ws or not tot > 0:
        return 0.0
    return float(cfg.dp_noise_multiplier) * kernel_clip(cfg) * max(ws) / tot


def gaussian_epsilon(z: float, rounds: int, delta: float) -> float:
    """epsilon at `delta` after `rounds` adaptive uses of the Gaussian
    mechanism with noise multiplier z (noise std / L2 sensitivity,
    add/remove of one client). Renyi DP: one use is (a, a / (2 z^2))-RDP,
    T uses add up, and (a, r)-RDP gives (r + ln(1/delta) / (a - 1),
    delta)-DP; minimising over the order a in closed form:

        eps = T / (2 z^2) + sqrt(2 T ln(1/delta)) / z

    No subsampling amplification: participants are chosen by the
    committee, not at random. z == 0 gives inf, rounds == 0 gives 0."""
    if not 0.0 < delta < 1.0:
        raise ValueError("delta must be in (0, 1)")
    if z < 0 or rounds < 0:
        raise ValueError("z and rounds must be >= 0")
    if rounds == 0:
        return 0.0
    if z == 0:
        return math.inf
    T = float(rounds)
    return T / (2.0 * z * z) + math.sqrt(2.0 * T * math.log(1.0 / delta)) / z
