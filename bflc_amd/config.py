"""Single source of truth for protocol + training configuration.

The reference scatters its constants across a C++ header
(reference CommitteePrecompiled.h:6-19: n_features=5, n_class=2,
COMM_COUNT=4, AGGREGATE_COUNT=6, NEEDED_UPDATE_COUNT=10, CLIENT_NUM=20,
learning_rate=0.001) and module-level Python constants
(reference python-sdk/main.py:52-69,87-88) with the learning rate
duplicated in both languages.  Here there is exactly one config object,
shared by the ledger, the engine, and the kernels, loadable from JSON
and overridable from the CLI.
"""
from __future__ import annotations

import dataclasses
import json
import math
from dataclasses import dataclass
from typing import Any, Dict, Optional


AGGREGATORS = ("fedavg", "trimmed_mean", "median", "multi_krum")
MAX_ROBUST_ROWS = 32  # K limit of the robust-aggregation kernels


@dataclass
class FLConfig:
    """Committee-consensus FL protocol + run configuration."""

    # --- protocol constants (reference CommitteePrecompiled.h:6-19) ---
    client_num: int = 20
    comm_count: int = 4
    needed_update_count: int = 10
    aggregate_count: int = 6
    learning_rate: float = 1e-3
    max_epoch: int = 1000          # reference main.py:65 (50 * CLIENT_NUM)

    # --- model / data ---
    model: str = "logreg"          # logreg | mlp | femnist_cnn | resnet20 | resnet50
    n_features: int = 5            # logreg/mlp input dim (reference main.py:68)
    n_class: int = 2
    batch_size: int = 100          # reference main.py:87
    local_epochs: int = 1          # passes over the local shard per round
    samples_per_client: int = 305  # synthetic shard size (reference ~8143*0.75/20)
    eval_samples: int = 2036       # held-out sponsor set (reference 8143*0.25)
    seed: int = 42
    dtype: str = "bf16"            # compute dtype on GPU; fp32 on CPU tests
    optimizer: str = "sgd"         # sgd | adam (reference main.py:126-127)
    norm_groups: int = 0           # ResNets: 0 = batch-stats BatchNorm,
                                   # > 0 = GroupNorm with that many groups

    # --- extended local SGD (all defaults mean "off": the legacy
    # sgd_master_ step). Only the LOCAL step is affected; delta
    # extraction, candidates, the server apply and the ledger keep the
    # constant `learning_rate` (DESIGN.md "Local optimizer") ---
    momentum: float = 0.0          # heavy ball, dampening 0 (torch.optim.SGD)
    nesterov: bool = False         # needs momentum > 0
    weight_decay: float = 0.0      # L2 added to the gradient, whole vector
    prox_mu: float = 0.0           # FedProx: + mu * (p - p_global)
    clip_norm: float = 0.0         # global L2 clip of the loss gradient; 0 = off
    lr_schedule: str = "constant"  # constant | step | cosine (by ledger epoch)
    lr_gamma: float = 0.1          # step: lr * gamma ** (epoch // lr_step_rounds)
    lr_step_rounds: int = 0
    lr_total_rounds: int = 0       # cosine horizon; 0 means max_epoch
    lr_min: float = 0.0            # cosine floor

    # --- sharding ---
    partition: str = "iid"         # iid | dirichlet (non-IID)
    dirichlet_alpha: float = 0.3
    byzantine_clients: int = 0     # attackers (BASELINE config 4)
    byzantine_attack: str = "label_flip"  # label_flip | scale: honest labels,
                                   # publishes byzantine_scale * delta
    byzantine_scale: float = -1.0  # scale attack multiplier (-4: boosted flip)

    # --- server-side aggregation rule over the ledger's selection (K
    # rows; fl/aggregate.py). "fedavg" is the reference's weighted
    # average; the robust rules need K <= 32. trimmed_mean and median are
    # unweighted (the ledger's weights are ignored), multi_krum keeps the
    # ledger's weights on the rows it retains ---
    aggregator: str = "fedavg"     # fedavg | trimmed_mean | median | multi_krum
    agg_trim: int = 1              # trimmed_mean: dropped at each end
    agg_byzantine: int = 1         # multi_krum: assumed bad rows f

    # --- differential privacy of the published update (fl/privacy.py,
    # DESIGN.md "Round-13"; all defaults mean "off"). The update W0 - W
    # is clipped to L2 norm dp_clip and Gaussian noise of standard
    # deviation dp_noise_multiplier * dp_clip is added: by every client
    # to its own update ("local") or once to the aggregate ("central") ---
    dp_clip: float = 0.0           # S, model space; the kernels see S / lr
    dp_noise_multiplier: float = 0.0  # z; needs dp_clip > 0
    dp_mode: str = "local"         # local | central (central: fedavg only)
    dp_delta: float = 1e-5         # the delta epsilon is reported for
    dp_seed: Optional[int] = None  # noise key; None derives it from `seed`

    # --- execution ---
    use_graphs: bool = True        # hipGraph-captured train step (GPU+SGD;
                                   # eager fallback elsewhere, fl/graphs.py)

    def __post_init__(self) -> None:
        if self.comm_count < 1 or self.client_num < 1:
            raise ValueError("comm_count and client_num must be >= 1")
        if self.aggregate_count > self.needed_update_count:
            raise ValueError("aggregate_count > needed_update_count")
        if self.comm_count >= self.client_num and self.client_num > 1:
            raise ValueError("comm_count must leave at least one trainer")
        if self.client_num > 1 and self.needed_update_count < self.comm_count:
            # rotation draws the next committee from scored trainers
            # (reference .cpp:443-455); fewer scored trainers than
            # comm_count would shrink the committee and deadlock scoring
            raise ValueError("needed_update_count must be >= comm_count")
        if self.client_num > 1 and \
                self.needed_update_count > self.client_num - self.comm_count:
            raise ValueError("needed_update_count exceeds trainer count")
        if self.norm_groups < 0:
            raise ValueError("norm_groups must be >= 0")
        for name in ("momentum", "weight_decay", "prox_mu", "clip_norm",
                     "lr_gamma", "lr_step_rounds", "lr_total_rounds",
                     "lr_min"):
            if getattr(self, name) < 0:
                raise ValueError(f"{name} must be >= 0")
        if self.nesterov and not self.momentum > 0:
            raise ValueError("nesterov needs momentum > 0")
        if self.lr_schedule not in ("constant", "step", "cosine"):
            raise ValueError(f"unknown lr_schedule {self.lr_schedule!r}")
        if self.lr_schedule == "step" and not self.lr_step_rounds > 0:
            raise ValueError("lr_schedule='step' needs lr_step_rounds > 0")
        if self.aggregator not in AGGREGATORS:
            raise ValueError(f"unknown aggregator {self.aggregator!r}")
        if self.byzantine_attack not in ("label_flip", "scale"):
            raise ValueError(
                f"unknown byzantine_attack {self.byzantine_attack!r}")
        if self.agg_trim < 0 or self.agg_byzantine < 0:
            raise ValueError("agg_trim and agg_byzantine must be >= 0")
        if self.aggregator != "fedavg" and \
                self.aggregate_count > MAX_ROBUST_ROWS:
            raise ValueError(
                f"aggregator {self.aggregator!r} needs aggregate_count <= "
                f"{MAX_ROBUST_ROWS} (the kernels hold K rows in registers)")
        if self.extended_sgd and self.optimizer == "adam":
            raise ValueError(
                "momentum / weight_decay / prox_mu / clip_norm / lr schedule "
                "fields extend optimizer='sgd' only")
        for name in ("dp_clip", "dp_noise_multiplier"):
            if getattr(self, name) < 0:
                raise ValueError(f"{name} must be >= 0")
        if self.dp_noise_multiplier > 0 and not self.dp_clip > 0:
            raise ValueError("dp_noise_multiplier needs dp_clip > 0")
        if self.dp_mode not in ("local", "central"):
            raise ValueError(f"unknown dp_mode {self.dp_mode!r}")
        if self.dp_mode == "central" and self.aggregator != "fedavg":
            raise ValueError(
                "dp_mode='central' needs aggregator='fedavg' (the noise is "
                "calibrated to the weighted mean's sensitivity)")
        if not 0.0 < self.dp_delta < 1.0:
            raise ValueError("dp_delta must be in (0, 1)")
        if self.dp_seed is not None and self.dp_seed < 0:
            raise ValueError("dp_seed must be >= 0")

    # ------------------------------------------------------------------
    _EXTENDED_DEFAULTS = dict(
        momentum=0.0, nesterov=False, weight_decay=0.0, prox_mu=0.0,
        clip_norm=0.0, lr_schedule="constant", lr_gamma=0.1,
        lr_step_rounds=0, lr_total_rounds=0, lr_min=0.0)

    @property
    def extended_sgd(self) -> bool:
        """True as soon as any extended-SGD field differs from its
        default: the local step then runs the sgdm kernels."""
        return any(getattr(self, k) != v
                   for k, v in self._EXTENDED_DEFAULTS.items())

    @property
    def dp_active(self) -> bool:
        """True when published updates are clipped (and, with
        dp_noise_multiplier > 0, noised): the engine then runs the
        privacy kernels."""
        return self.dp_clip > 0

    def local_lr(self, epoch: int) -> float:
        """Local step size at a ledger epoch (Python doubles; a pure
        function of the config, so it is identical on every rank and
        needs no checkpoint state). The protocol's `learning_rate`
        (delta scale, server apply, ledger) is NOT scheduled."""
        lr, e = float(self.learning_rate), int(epoch)
        if self.lr_schedule == "step":
            return lr * float(self.lr_gamma) ** (e // self.lr_step_rounds)
        if self.lr_schedule == "cosine":
            T = self.lr_total_rounds or self.max_epoch
            if T <= 0:
                return lr
            lo = float(self.lr_min)
            return lo + 0.5 * (lr - lo) * (
                1.0 + math.cos(math.pi * min(e, T) / T))
        return lr

    # ------------------------------------------------------------------
    @classmethod
    def reference_defaults(cls) -> "FLConfig":
        """The exact configuration of the reference demo."""
        return cls()

    @classmethod
    def for_world(cls, n_nodes: int, **overrides: Any) -> "FLConfig":
        """Scale the protocol sanely to n_nodes FL clients (1/2/4/8 GPUs).

        Keeps the committee/quota structure of the reference while making
        every world size well-formed:
          - committee = min(4, floor(n/2)) but at least 1 when n >= 2;
          - n == 1 degenerates to plain local SGD with self-scoring
            (committee == trainer on alternating epochs is meaningless at
            n == 1, so the single client both trains and scores).
        """
        n = int(n_nodes)
        if n < 1:
            raise ValueError("n_nodes >= 1 required")
        if n == 1:
            cfg = dict(client_num=1, comm_count=1, needed_update_count=1,
                       aggregate_count=1, self_score=True)
        else:
            comm = max(1, min(4, n // 2))
            trainers = n - comm
            # barrier-driven: every trainer submits each round; the quota
            # must be >= comm_count so rotation can always fill the
            # committee from scored trainers.
            needed = max(trainers, 1)
            agg = max(1, min(needed, -(-needed * 6 // 10)))  # ceil(0.6*needed)
            cfg = dict(client_num=n, comm_count=comm,
                       needed_update_count=needed, aggregate_count=agg)
        cfg.pop("self_score", None)
        cfg.update(overrides)
        return cls(**cfg)

    # n==1 special case: the lone node may both train and score.
    @property
    def self_scoring(self) -> bool:
        return self.client_num == 1

    # ------------------------------------------------------------------
    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)

    def to_json(self) -> str:
        return json.dumps(self.to_dict(), sort_keys=True)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "FLConfig":
        names = {f.name for f in dataclasses.fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in names})

    @classmethod
    def from_json_file(cls, path: str) -> "FLConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))

    def ledger_config(self):
        from bflc_amd._ledger import LedgerConfig  # lazy: built ext
        lc = LedgerConfig()
        lc.client_num = self.client_num
        lc.comm_count = self.comm_count
        lc.needed_update_count = self.needed_update_count
        lc.aggregate_count = self.aggregate_count
        lc.learning_rate = self.learning_rate
        lc.max_epoch = self.max_epoch
        return lc
