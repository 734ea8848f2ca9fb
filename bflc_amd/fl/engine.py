"""Barrier-driven committee-consensus FL round engine.

One process per GPU; each rank owns a contiguous slice of the FL
clients and a full replica of the deterministic ledger. A round replays
the reference protocol without any polling or sleeps,
one FLEngine method per phase:

  phase T  (_phase_train) designated trainers run the local HIP train
           step
  phase U  (_phase_publish) one rank-ordered all-gather publishes
           (meta, delta) updates; every rank feeds ALL submissions to
           its ledger replica in the same order => identical admission
           decisions (reference UploadLocalUpdate guards, .cpp:215-257)
  phase S  (_phase_score) committee clients score every accepted
           candidate on their own shard (reference local_scoring,
           main.py:196-217)
  phase V  (_phase_decide) one all-gather publishes score maps; the
           comm_count-th feed triggers the aggregation decision
           (.cpp:259-297)
  phase A  (_phase_aggregate) every rank applies the identical
           weighted-FedAvg kernel with a fixed accumulation order and
           commits (.cpp:349-455); or, opt-in, a robust rule over the
           same rows (fl/aggregate.py)

The reference resolves the 16-trainers-race-for-10-slots with
first-come PBFT ordering; here admission order is the deterministic
(rank, client) order, so ranks can PREDICT which updates would be
admitted and skip training the surplus trainers entirely — same
semantics (rejected updates never influence state), less wasted compute.

Execution model (GPU): each local client's ENTIRE training pass and
ENTIRE candidate-scoring sweep are captured once as hipGraphs
(fl/graphs.py, cached by _captured) against that client's own model
replica and private graph pool; within a phase, the participants'
replays run CONCURRENTLY on slot-indexed HIP streams and join at the
phase barrier (_run_on_slot_streams). Per-client kernel order is
unchanged, so results are bitwise-identical to the sequential path
(BFLC_STREAMS=0). The FL-model kernels are issue/launch-bound rather
than HBM-bound (profiles/r02_pmc_*.md), which is why overlap — not more
per-kernel bandwidth — is what shortens the round.

Data plane (flat fp32 delta tensors, the global model) stays resident on
the GPU; the ledger's blobs hold b"" markers in engine mode (the
ABI-compatible JSON blob path lives in bflc_amd.chain.client).
"""
from __future__ import annotations

import os
import time
import warnings
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from bflc_amd._ledger import Admit, CommitteeLedger
from bflc_amd.chain.identity import (KeyTable, scores_payload,
                                     update_payload)
from bflc_amd.comm import Transport
from bflc_amd.config import FLConfig
from bflc_amd.data.synthetic import Shard
from bflc_amd.fl import graphs, privacy
from bflc_amd.fl.aggregate import aggregate
from bflc_amd.models import build_model
from bflc_amd.ops import functional as O

# what flows between the phases of a round: an admitted (origin, delta)
# update — a local one also carries (n_samples, mean loss) — and a
# scorer's (origin, {candidate origin: accuracy}, HMAC tag)
Update = Tuple[str, torch.Tensor]
LocalUpdate = Tuple[str, torch.Tensor, int, float]
SignedScores = Tuple[str, Dict[str, float], bytes]


class StragglerError(RuntimeError):
    """A collective phase failed (dead or too-slow peer). The engine
    aborts the round cleanly after writing a rank-local checkpoint; the
    reference survived crashed trainers by quota over-provisioning
    (CommitteePrecompiled.h:15, only 10 of 16 need to upload) — a
    barrier-driven engine turns the hang into this diagnosable error
    instead, bounded by Transport.timeout_s."""


def client_rank(client_idx: int, n_clients: int, world: int) -> int:
    """Contiguous array_split-style client->rank assignment."""
    base, rem = divmod(n_clients, world)
    # ranks 0..rem-1 own (base+1) clients
    cut = rem * (base + 1)
    if client_idx < cut:
        return client_idx // (base + 1)
    return rem + (client_idx - cut) // max(base, 1)


@dataclass
class RoundStats:
    epoch: int
    wall_s: float
    train_s: float
    gather_s: float
    score_s: float
    aggregate_s: float
    global_loss: float
    n_updates: int
    n_selected: int
    samples_trained: int
    test_acc: Optional[float] = None


class FLEngine:
    def __init__(self, cfg: FLConfig, transport: Transport,
                 shards: List[Shard], test_shard: Optional[Shard] = None,
                 metrics_path: Optional[str] = None) -> None:
        from bflc_amd.utils import JsonlLogger
        self.cfg = cfg
        self.t = transport
        self.device = transport.device
        self.rank = transport.rank
        self.world = transport.world_size

        # client ownership
        self.origins = [f"node_{i}" for i in range(cfg.client_num)]
        self.local_clients = [i for i in range(cfg.client_num)
                              if client_rank(i, cfg.client_num, self.world)
                              == self.rank]
        self.shards = {i: shards[i].to(self.device) for i in self.local_clients}
        self.test_shard = test_shard.to(self.device) if test_shard else None

        # one shared model instance per rank (set_flat per client)
        self.model = build_model(cfg, self.device)
        self.global_flat = self.model.get_flat()  # device-resident fp32

        # per-origin HMAC keys (reference get_batch_accounts.sh: one
        # identity per client); every gathered submission is verified
        # before it reaches the ledger (chain/identity.py)
        self.keys = KeyTable(self.origins, cfg.seed)

        # replicated ledger: registration = deterministic replay of the
        # rank-ordered client lists (reference RegisterNode, .cpp:168-190)
        self.ledger = CommitteeLedger(cfg.ledger_config())
        gathered = self.t.all_gather_objects(self.local_clients)
        for rank_clients in gathered:
            for i in rank_clients:
                self.ledger.register_node(self.origins[i])
        assert self.ledger.epoch == 0, "registration did not start FL"
        self.ledger.set_global_model(b"")

        self._round = 0
        # info dict of the last round's aggregation (fl/aggregate.py):
        # rule, effective t or f, and for multi-Krum the origins kept
        self.last_aggregation: Optional[dict] = None
        self.metrics = JsonlLogger(metrics_path, rank=self.rank)

        # which fused local step this engine runs: the legacy
        # sgd_master_ step, the extended sgdm kernels (momentum / weight
        # decay / FedProx / clip / scheduled lr — cfg.extended_sgd) or
        # Adam. Public so tests cannot pass through the wrong path.
        self.local_optimizer = ("adam" if cfg.optimizer == "adam" else
                                "sgdm" if cfg.extended_sgd else "sgd_legacy")
        # sgdm: ONE device learning rate, refilled from
        # cfg.local_lr(epoch) at the top of every round on the main
        # stream (before the client streams fork); every captured step
        # reads it, so a schedule never forces a recapture. The
        # proximal anchor is global_flat itself (address-stable).
        self._lr_dev: Optional[torch.Tensor] = None
        if self.local_optimizer == "sgdm":
            self._lr_dev = torch.full(
                (1,), cfg.local_lr(self.ledger.epoch), dtype=torch.float32,
                device=self.device)
        # optimizer of the eager (ungraphed) local step, built on first
        # use and reset per client pass (graphs.LocalOptimizer)
        self._eager_opt: Optional[graphs.LocalOptimizer] = None

        # hipGraph-captured train step (fl/graphs.py): replay one
        # captured kernel DAG per minibatch instead of relaunching
        # ~dozens of kernels. SGD-only; falls back to eager on CPU, on
        # Adam, or if capture fails on this ROCm build.
        self._steppers: Dict[tuple, object] = {}
        self._scorers: Dict[int, object] = {}
        # whole-phase graphs: one per client (full local training pass)
        # and one per scorer (all quota candidates in one replay) —
        # launch/copy overhead per round collapses to one dispatch per
        # phase participant (fl/graphs.py)
        self._train_graphs: Dict[int, object] = {}
        self._score_graphs: Dict[int, object] = {}
        self._cand_stack: Optional[torch.Tensor] = None
        self._graph_pool = None  # shared by all serialized captures
        # concurrent client streams: the FL-model kernels are
        # issue/launch-bound, not HBM-bound (profiles/r02_pmc_femnist.md)
        # — so a rank hosting several clients overlaps their whole-phase
        # graph replays on concurrent HIP streams (slot-indexed per
        # phase participant, see _client_stream). That requires one
        # model replica and one private graph pool per local client
        # (concurrently-replaying graphs must not share weight buffers
        # or pool memory); the cost is #local_clients x (model +
        # activation footprint), sized for 288 GB HBM3E (ResNet-50 at 8
        # clients/rank ~ tens of GB). Per-client compute is unchanged
        # and each client's kernels stay serialized on its own stream,
        # so results are identical to the sequential path.
        self._client_models: Dict[int, object] = {}
        self._client_streams: Dict[int, object] = {}
        self._client_pools: Dict[int, object] = {}
        self._client_delta: Dict[int, torch.Tensor] = {}
        # round-persistent scratch (avoid per-round alloc/fill of
        # O(model)-sized tensors: the gather stack is ~400 MB/round on
        # ResNet-50)
        self._cand_buf: Optional[torch.Tensor] = None
        self._stack_buf: Optional[torch.Tensor] = None
        self._fedavg_buf: Optional[torch.Tensor] = None
        # differential privacy (cfg.dp_active; fl/privacy.py): per
        # client a (partials, [coef, sumsq]) pair of device buffers for
        # the update clip, the coefficients the local clients applied
        # this round, and the record of the last round (None when off)
        self._dp_bufs: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._dp_coefs: Dict[str, float] = {}
        self._dp_one: Optional[torch.Tensor] = None
        self.last_privacy: Optional[dict] = None
        self._use_graphs = (cfg.use_graphs and self.device.type == "cuda"
                            and os.environ.get("BFLC_GRAPHS", "1") != "0")
        self._concurrent = (self._use_graphs
                            and os.environ.get("BFLC_STREAMS", "1") != "0")
        self._phase_debug = os.environ.get("BFLC_PHASE_DEBUG", "0") == "1"

    # ------------------------------------------------------------------
    def _planned_submitters(self) -> List[int]:
        """The deterministic prefix of trainers whose updates will be
        admitted (first needed_update_count in (rank, client) order)."""
        roles = self.ledger.roles()
        # global (rank, client-index) order == client index order because
        # assignment is contiguous ascending (origins are id-sorted)
        order = [i for i in range(self.cfg.client_num)
                 if self.cfg.self_scoring
                 or roles.get(self.origins[i], "trainer") == "trainer"]
        return order[: self.cfg.needed_update_count]

    def _fence(self) -> None:
        """Phase boundary: the device is idle when the phase's
        timestamp is taken."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------
    def _graph_optimizer(self) -> dict:
        """Optimizer arguments of graphs.LocalOptimizer and of the graph
        classes that build one (fl/graphs.py)."""
        if self.local_optimizer == "sgdm":
            return dict(optimizer="sgdm", sgdm_cfg=self.cfg,
                        lr_dev=self._lr_dev, p0=self.global_flat)
        return dict(optimizer=self.cfg.optimizer)

    def _eager_optimizer(self) -> graphs.LocalOptimizer:
        """Optimizer of the eager (ungraphed) local step: one per
        engine, reset at the start of every client pass."""
        if self._eager_opt is None:
            self._eager_opt = graphs.LocalOptimizer(
                self.model, lr=self.cfg.learning_rate, capturable=False,
                **self._graph_optimizer())
        return self._eager_opt

    # ------------------------------------------------------------------
    def _client_model(self, client: int):
        """Per-client model replica (concurrent mode): each local
        client's graphs capture against their OWN flat/cflat buffers so
        their replays can overlap on per-client streams."""
        if client not in self._client_models:
            self._client_models[client] = build_model(self.cfg, self.device)
        return self._client_models[client]

    def _client_stream(self, slot: int):
        """Stream for the slot-th CONCURRENT participant of the current
        phase (NOT per client): ROCm multiplexes streams onto
        GPU_MAX_HW_QUEUES (default 4) hardware queues and streams
        sharing a queue serialize — with one stream per CLIENT (8
        streams, roles rotating), a phase's 4 participants could land
        2-per-queue and run pairwise-serial (per-client stream timings
        showed exactly that). At most max-participants-per-phase
        streams ever exist, so each phase's replays map to distinct
        queues. Safe because phases are joined before the next launch
        and a client appears at most once per phase."""
        if slot not in self._client_streams:
            self._client_streams[slot] = torch.cuda.Stream()
        return self._client_streams[slot]

    def _captured(self, cache: dict, key, build: Callable, failure: str,
                  client: Optional[int] = None,
                  disable_graphs: bool = False):
        """The lazily captured graph cache[key]: on first use
        ``build(model, pool)`` captures it; a capture that raises warns
        ``failure`` and is remembered as None for this key — or, with
        ``disable_graphs``, stops the engine trying graphs at all.

        Model and pool: the whole-phase graphs name their ``client`` and
        in concurrent mode capture against that client's own replica
        and one PRIVATE pool per client (graphs replaying in parallel
        must not share weight buffers or pool memory). Everything else
        — sequential mode, the per-batch stepper, the per-candidate
        scorer — replays serialized and captures against self.model in
        the one shared pool (round-1 ADVICE — serialized replays can
        share). A pool is the pool of its first capture."""
        if key in cache:
            return cache[key]
        private = self._concurrent and client is not None
        try:
            if private:
                model = self._client_model(client)
                pool = self._client_pools.get(client)
            else:
                model, pool = self.model, self._graph_pool
            g = build(model, pool)
            if pool is None and private:
                self._client_pools[client] = g.pool()
            elif pool is None:
                self._graph_pool = g.pool()
        except Exception as e:
            warnings.warn(f"{failure}: {e}")
            if disable_graphs:
                self._use_graphs = False
                return None
            g = None
        cache[key] = g
        return g

    def _graphed_stepper(self, shard: Shard, bs: int):
        """Lazily capture the train-step hipGraph (fl/graphs.py), one
        stepper per batch shape (heterogeneous shard sizes each get
        their own capture instead of silently running eager — round-1
        ADVICE item). Returns None — and stops trying — if capture is
        unavailable."""
        xb, yb = shard.x[:bs], shard.y[:bs]
        return self._captured(
            self._steppers, (tuple(xb.shape), xb.dtype, tuple(yb.shape)),
            lambda model, pool: graphs.GraphedTrainStep(
                model, self.cfg.learning_rate, xb, yb, pool=pool,
                **self._graph_optimizer()),
            "hipGraph capture failed, running eager", disable_graphs=True)

    def _whole_train_graph(self, client: int):
        """Per-client whole-local-training graph (shard slices baked in,
        zero per-batch copies); None if capture is unavailable. In
        concurrent mode the graph is captured against the client's own
        model replica (g.model) so replays can overlap."""
        return self._captured(
            self._train_graphs, client,
            lambda model, pool: graphs.GraphedLocalTrain(
                model, self.cfg.learning_rate, self.shards[client].x,
                self.shards[client].y, self.cfg.batch_size,
                self.cfg.local_epochs, pool=pool,
                **self._graph_optimizer()),
            f"whole-train graph capture failed for client {client}, "
            "using per-batch path", client=client)

    def _phase_scorer(self, scorer: int):
        """Per-scorer whole-phase scoring graph (all quota candidates in
        one replay); None if capture is unavailable."""
        return self._captured(
            self._score_graphs, scorer,
            lambda model, pool: graphs.GraphedScorePhase(
                model, self.shards[scorer].x, self.shards[scorer].y,
                self._cand_stack, self.global_flat, self.cfg.learning_rate,
                pool=pool),
            f"whole-scoring graph capture failed for scorer {scorer}, "
            "per-candidate path", client=scorer)

    def _graphed_scorer(self, scorer: int):
        """Per-scorer captured scoring graph (fl/graphs.py); capture
        mutates the scratch model, which every phase reloads anyway."""
        return self._captured(
            self._scorers, scorer,
            lambda model, pool: graphs.GraphedScore(
                model, self.shards[scorer].x, self.shards[scorer].y,
                pool=pool),
            "score-graph capture failed, running eager")

    # ------------------------------------------------------------------
    def _run_on_slot_streams(self, label: str, participants: List[int],
                             enqueue: Callable[[int], torch.Tensor]
                             ) -> List[torch.Tensor]:
        """Fork/join of one concurrent phase: ``enqueue(i)`` runs under
        the stream of participant i's SLOT (its position in the phase,
        see _client_stream) and returns the device tensor the caller
        will read back; they come back in participant order. The
        ordering rules this owns:
          * every slot stream first waits for the current stream, so
            whatever the caller allocated or enqueued before the fork
            (deltas, DP buffers, the lr refill, the packed candidates)
            is ready — callers allocate BEFORE calling, on the main
            stream, never inside ``enqueue``;
          * every slot stream is joined into the current stream before
            this returns, so the caller's one stacked host read (and
            the next phase) sees all of them. The host read itself is
            the caller's.
        BFLC_PHASE_DEBUG=1 adds per-client device timings (and a device
        synchronize, so that they can be read)."""
        cur = torch.cuda.current_stream()
        out, evs = {}, {}
        th0 = time.perf_counter()
        for j, i in enumerate(participants):
            s = self._client_stream(j)
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                if self._phase_debug:
                    evs[i] = (torch.cuda.Event(enable_timing=True),
                              torch.cuda.Event(enable_timing=True))
                    evs[i][0].record(s)
                out[i] = enqueue(i)
                if self._phase_debug:
                    evs[i][1].record(s)
        th1 = time.perf_counter()
        for j in range(len(participants)):
            cur.wait_stream(self._client_streams[j])
        if self._phase_debug:
            torch.cuda.synchronize(self.device)
            th2 = time.perf_counter()
            tt = " ".join(f"c{i}:{evs[i][0].elapsed_time(evs[i][1]):.1f}"
                          for i in participants)
            print(f"# [debug] epoch {self.ledger.epoch} {label} per-client "
                  f"ms: {tt} | host enqueue {1e3*(th1-th0):.2f} "
                  f"join {1e3*(th2-th1):.2f}", flush=True)
        return [out[i] for i in participants]

    # ------------------------------------------------------------------
    def _dp_buffers(self, client: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The client's clip buffers, allocated on first use (on the
        main stream: the concurrent path asks before it forks)."""
        if client not in self._dp_bufs:
            P = self.global_flat.numel()
            self._dp_bufs[client] = (
                torch.empty(O.sumsq_partials(P, self.device),
                            dtype=torch.float32, device=self.device),
                torch.empty(2, dtype=torch.float32, device=self.device))
        return self._dp_bufs[client]

    def _publish_delta(self, client: int, out: torch.Tensor,
                       w: torch.Tensor) -> None:
        """out = the update client `client` publishes from its trained
        weights `w`, on the current stream: (W0 - W)/lr (reference
        main.py:153-154), and with cfg.dp_active clipped to S/lr and, in
        local mode, noised (fl/privacy.py) — extraction with the sum of
        squares in the same pass, the clip coefficient on the device,
        one in-place pass for clip and noise."""
        cfg = self.cfg
        if not cfg.dp_active:
            O.delta_extract_(out, self.global_flat, w, cfg.learning_rate)
            return
        part, coef = self._dp_buffers(client)
        O.delta_extract_sumsq_(out, self.global_flat, w, cfg.learning_rate,
                               part)
        O.grad_clip_final_(part, privacy.kernel_clip(cfg), coef)
        O.dp_privatize_(out, coef, privacy.local_sigma(cfg),
                        privacy.noise_key(cfg), client, self.ledger.epoch)

    def _read_losses(self, clients: List[int],
                     costs: List[torch.Tensor]) -> List[float]:
        """ONE host sync for the listed clients' summed losses; with
        cfg.dp_active the clip coefficients they applied ride along
        (and are kept for the round's privacy record). Every cost is
        a detached fp32 scalar: a graph's `.cost` or the eager loop's
        accumulator."""
        fetch = list(costs)
        if self.cfg.dp_active:
            fetch += [self._dp_bufs[i][1][0] for i in clients]
        host = torch.stack(fetch).tolist()
        if self.cfg.dp_active:
            for i, coef in zip(clients, host[len(clients):]):
                self._dp_coefs[self.origins[i]] = coef
        return host[:len(clients)]

    def _extract_update(self, client: int, w: torch.Tensor,
                        cost: torch.Tensor) -> Tuple[torch.Tensor, float]:
        """(published delta, summed loss on the host) of the sequential
        training paths: publish, then the one host read."""
        delta = torch.empty_like(self.global_flat)
        self._publish_delta(client, delta, w)
        return delta, self._read_losses([client], [cost])[0]

    def _local_train(self, client: int) -> Tuple[torch.Tensor, int, float]:
        """Local train step (reference local_training, main.py:103-158):
        start from the global model, run local_epochs passes of
        minibatch SGD/Adam, return pseudo-gradient delta=(W0-W)/lr."""
        cfg = self.cfg
        shard = self.shards[client]
        n = shard.n
        # whole-pass graph: capture BEFORE loading the round's weights
        # (capture executes real steps and mutates flat/cflat)
        wg = self._whole_train_graph(client) if self._use_graphs else None
        if wg is not None:
            wg.model.set_flat(self.global_flat)
            delta, cost = self._extract_update(client, wg.model.flat.data,
                                               wg.run())
            return delta, n, cost / wg.n_steps
        bs = min(cfg.batch_size, n)
        batches = [(shard.x[bi * bs:(bi + 1) * bs],
                    shard.y[bi * bs:(bi + 1) * bs])
                   for bi in range(max(n // bs, 1))] * cfg.local_epochs
        # capture BEFORE loading the round's weights: graph warmup and
        # capture execute real SGD steps and mutate flat/cflat
        stepper = self._graphed_stepper(shard, bs) if self._use_graphs \
            else None
        self.model.set_flat(self.global_flat)
        # either way: fresh optimizer state per client pass (Adam's
        # (m, v, step), sgdm's momentum) and the loss accumulated
        # on-device — ONE host sync per client per round
        if stepper is not None:
            stepper.cost.zero_()
            stepper.reset_state()
            for xb, yb in batches:
                stepper.step(xb, yb)
            cost_accum = stepper.cost
        else:
            opt = self._eager_optimizer()
            opt.reset()
            cost_accum = torch.zeros((), device=self.device)
            for xb, yb in batches:
                graphs.train_step(self.model, opt, xb, yb, cost_accum)
        delta, cost = self._extract_update(client, self.model.flat.data,
                                           cost_accum)
        return delta, n, cost / len(batches)

    # ------------------------------------------------------------------
    def _pack_candidates(self, updates: List[Update]) -> bool:
        """Pack the admitted deltas into the persistent [quota, P]
        buffer the whole-scoring graphs bake in; False when the shape
        doesn't fit (degraded round) => per-candidate fallback."""
        K = len(updates)
        if not self._use_graphs or K != self.cfg.needed_update_count \
                or K == 0 or self.device.type != "cuda":
            return False
        if self._cand_stack is None:
            self._cand_stack = torch.empty(
                K, self.global_flat.numel(), dtype=torch.float32,
                device=self.device)
        for k, (_, delta) in enumerate(updates):
            self._cand_stack[k].copy_(delta)
        return True

    def _score_candidates(self, scorer: int, updates: List[Update],
                          packed: bool = False) -> List[float]:
        """Committee scoring (reference local_scoring, main.py:196-217):
        candidate = W0 - lr*delta, scored by accuracy on the scorer's own
        local shard; one accuracy per update, in their order."""
        if packed:
            g = self._phase_scorer(scorer)
            if g is not None:
                return g.run().tolist()  # one host sync for all K
        shard = self.shards[scorer]
        gs = self._graphed_scorer(scorer) if self._use_graphs else None
        lr = self.cfg.learning_rate
        accs: List[torch.Tensor] = []
        if gs is not None:
            for _, delta in updates:
                # candidate built in the graph's own input buffer — no
                # per-candidate clone
                accs.append(gs.score_candidate(self.global_flat, lr, delta))
        else:
            if self._cand_buf is None:
                self._cand_buf = torch.empty_like(self.global_flat)
            for _, delta in updates:
                self._cand_buf.copy_(self.global_flat)
                O.axpy_(self._cand_buf, -lr, delta)
                self.model.set_flat(self._cand_buf)
                # device-resident: ONE host sync per scorer (below),
                # not one per candidate
                accs.append(self.model.accuracy_t(shard.x, shard.y))
        return [float(a) for a in accs]

    # ------------------------------------------------------------------
    def _gather(self, phase: str, fn, *args):
        """Run one collective phase; a dead or timed-out peer becomes a
        clean StragglerError after a rank-local checkpoint (path:
        $BFLC_ABORT_CHECKPOINT, default under the system temp dir)."""
        try:
            return fn(*args)
        except StragglerError:
            raise
        except Exception as e:
            import tempfile
            path = os.environ.get(
                "BFLC_ABORT_CHECKPOINT",
                os.path.join(tempfile.gettempdir(),
                             f"bflc_abort_rank{self.rank}.pt"))
            note = ""
            try:
                self.save(path)
                note = f"; state checkpointed to {path}"
            except Exception:
                note = "; checkpoint write also failed"
            raise StragglerError(
                f"collective phase '{phase}' failed at epoch "
                f"{self.ledger.epoch} on rank {self.rank}/{self.world} "
                f"(dead or >={self.t.timeout_s:.0f}s-slow peer?): "
                f"{e}{note}") from e

    # ------------------------------------------------------------------
    def _phase_train(self) -> List[LocalUpdate]:
        """Phase T: local training on the designated submitters that
        this rank owns.

        Concurrent path: each local trainer's whole-training graph
        replays on its own HIP stream (its own model replica and
        private pool) — set_flat, the replay, and the fused delta
        extraction are all enqueued per stream, joined once at the
        phase end. Falls back to the sequential loop if any capture is
        unavailable."""
        cfg = self.cfg
        local_subs = [i for i in self._planned_submitters()
                      if i in self.shards]
        if self._concurrent and self._round == 0:
            # Pre-capture EVERY local client's training graph now:
            # committee rotation means each client eventually trains,
            # and a lazy capture during a later (timed/steady-state)
            # round would put one-time capture cost inside it.
            for i in self.local_clients:
                self._whole_train_graph(i)
        conc = self._concurrent and len(local_subs) > 1 and all(
            self._whole_train_graph(i) is not None for i in local_subs)
        if conc:
            for i in local_subs:  # allocate on the main stream
                if i not in self._client_delta:
                    self._client_delta[i] = torch.empty_like(
                        self.global_flat)
                if cfg.dp_active:
                    self._dp_buffers(i)

            def replay(i: int) -> torch.Tensor:
                g = self._train_graphs[i]
                g.model.set_flat(self.global_flat)
                cost = g.run()
                self._publish_delta(i, self._client_delta[i],
                                    g.model.flat.data)
                return cost

            costs = self._read_losses(
                local_subs,
                self._run_on_slot_streams("train", local_subs, replay))
            local_updates = [
                (self.origins[i], self._client_delta[i], self.shards[i].n,
                 cost / self._train_graphs[i].n_steps)
                for i, cost in zip(local_subs, costs)]
        else:
            local_updates = []
            for i in local_subs:
                delta, n, cost = self._local_train(i)
                local_updates.append((self.origins[i], delta, n, cost))
        if cfg.byzantine_attack == "scale":
            # model-poisoning adversary: an attacker trains honestly and
            # publishes byzantine_scale * delta. Done on the owning rank,
            # after the client streams joined, for both training paths;
            # plain torch on purpose (simulation glue, not a hot path)
            for (_, delta, _, _), i in zip(local_updates, local_subs):
                if self.shards[i].byzantine:
                    delta.mul_(float(cfg.byzantine_scale))
        return local_updates

    def _phase_publish(self, epoch: int, local_updates: List[LocalUpdate]
                       ) -> Tuple[List[Update], int]:
        """Phase U: publish updates (one RCCL all-gather). Returns the
        admitted updates and the number of bad signatures.

        Each submission carries an HMAC tag binding (origin, epoch,
        meta) to the origin's bootstrap key (chain/identity.py); every
        replica verifies before feeding its ledger, so a forged origin
        is rejected deterministically on all ranks (reference: one
        ECDSA key per client, get_batch_accounts.sh)."""
        metas = [(o, epoch, n, c,
                  self.keys.sign("update", o, epoch, update_payload(n, c)))
                 for (o, delta, n, c) in local_updates]
        all_metas = self._gather("updates", self.t.all_gather_objects, metas)
        max_subs = max((len(m) for m in all_metas), default=0)
        rows = max(max_subs, 1)
        # cached, never zeroed: rows beyond a rank's own submission count
        # are never read back (unpack walks rank_metas, not the padding)
        if self._stack_buf is None or self._stack_buf.shape[0] < rows:
            self._stack_buf = torch.empty(
                rows, self.global_flat.numel(), dtype=torch.float32,
                device=self.global_flat.device)
        stack = self._stack_buf[:rows]
        for j, (_, delta, _, _) in enumerate(local_updates):
            stack[j] = delta
        gathered = self._gather("update-deltas", self.t.all_gather_tensor,
                                stack)
        updates: List[Update] = []
        n_bad_sig = 0
        for r, rank_metas in enumerate(all_metas):
            for j, (origin, ep, n, c, tag) in enumerate(rank_metas):
                if not self.keys.verify("update", origin, ep,
                                        update_payload(n, c), tag):
                    n_bad_sig += 1
                    continue
                code = self.ledger.upload_local_update(origin, b"", ep, n, c)
                if code == Admit.ACCEPTED:
                    updates.append((origin, gathered[r][j].to(self.device)))
        return updates, n_bad_sig

    def _phase_score(self, epoch: int, updates: List[Update]
                     ) -> List[SignedScores]:
        """Phase S: committee scoring; the signed score map of every
        local scorer.

        Concurrent path: every local scorer's whole-scoring graph (all
        K candidates in one replay) runs on its own slot stream; scores
        are read back once after the join."""
        roles = self.ledger.roles()
        if self.cfg.self_scoring:
            local_scorers = list(self.shards.keys())
        else:
            local_scorers = [i for i in self.local_clients
                             if roles.get(self.origins[i]) == "comm"]
        packed = bool(local_scorers) and self._pack_candidates(updates)
        if self._concurrent and packed and self._round == 0:
            # pre-capture every local client's scoring graph (rotation:
            # each client eventually sits on the committee) so later
            # rounds never pay capture cost
            for i in self.local_clients:
                self._phase_scorer(i)
        conc = self._concurrent and packed and len(local_scorers) > 1 \
            and all(self._phase_scorer(i) is not None for i in local_scorers)
        if conc:
            # ONE host sync for all scorers' [K] accuracy vectors
            all_accs = torch.stack(self._run_on_slot_streams(
                "score", local_scorers,
                lambda i: self._score_graphs[i].run_inplace())).tolist()
        else:
            all_accs = [self._score_candidates(i, updates, packed=packed)
                        for i in local_scorers]
        my_scores = []
        for i, accs in zip(local_scorers, all_accs):
            o = self.origins[i]
            smap = {origin: acc for (origin, _), acc in zip(updates, accs)}
            my_scores.append((o, smap, self.keys.sign(
                "scores", o, epoch, scores_payload(smap))))
        return my_scores

    def _phase_decide(self, epoch: int, my_scores: List[SignedScores]):
        """Phase V: publish scores, decide. Returns the ledger's
        aggregation decision and the number of bad signatures."""
        all_scores = self._gather("scores", self.t.all_gather_objects,
                                  my_scores)
        decision = None
        n_bad_sig = 0
        for rank_scores in all_scores:
            for origin, smap, tag in rank_scores:
                if not self.keys.verify("scores", origin, epoch,
                                        scores_payload(smap), tag):
                    n_bad_sig += 1
                    continue
                d = self.ledger.upload_scores(origin, epoch, smap)
                if d is not None:
                    decision = d
        if decision is None:
            raise RuntimeError(
                f"round {epoch}: no aggregation decision "
                f"(scores={self.ledger.score_count}/{self.cfg.comm_count})")
        return decision, n_bad_sig

    def _phase_aggregate(self, epoch: int, updates: List[Update],
                         decision) -> Tuple[dict, dict]:
        """Phase A: weighted FedAvg (or a robust rule) + commit. Returns
        the aggregation info and the extra fields of the round's metrics
        record."""
        cfg = self.cfg
        by_origin = dict(updates)
        sel = decision.selected
        K = len(sel)
        self.last_decision = decision
        agg_info = {"aggregator": cfg.aggregator, "rows": 0}
        central_sigma = 0.0
        if K > 0:
            if self._fedavg_buf is None or self._fedavg_buf.shape[0] < K:
                self._fedavg_buf = torch.empty(
                    K, self.global_flat.numel(), dtype=torch.float32,
                    device=self.global_flat.device)
            deltas = self._fedavg_buf[:K]
            for k, (origin, _) in enumerate(sel):
                deltas[k] = by_origin[origin]
            # cfg.aggregator: weighted FedAvg (default) or a robust rule
            # over the same K rows (fl/aggregate.py)
            avg, agg_info = aggregate(deltas, sel, cfg)
            if cfg.dp_active and cfg.dp_mode == "central" \
                    and cfg.dp_noise_multiplier > 0:
                # one noise vector on the aggregate, a function of (key,
                # epoch, coordinate) and the host weights: the same bits
                # on every replica
                if self._dp_one is None:
                    self._dp_one = torch.ones(1, dtype=torch.float32,
                                              device=self.device)
                central_sigma = privacy.central_sigma(sel, cfg)
                O.dp_privatize_(avg, self._dp_one, central_sigma,
                                privacy.noise_key(cfg), O.DP_CENTRAL_STREAM,
                                epoch)
            # global -= lr * avg  (reference .cpp:403-414)
            O.axpy_(self.global_flat, -cfg.learning_rate, avg)
        # K == 0 (no admitted updates survived): the model is unchanged
        # but the epoch still advances and the committee rotates/refills
        # — the round degrades instead of wedging every replica
        self.last_aggregation = agg_info
        extra = {}
        if cfg.dp_active:
            # epsilon is a function of the config and the epoch alone
            # (epoch + 1 rounds done), so checkpoints carry nothing new
            self.last_privacy = extra["privacy"] = {
                "mode": cfg.dp_mode, "clip": cfg.dp_clip,
                "noise_multiplier": cfg.dp_noise_multiplier,
                "central_sigma": central_sigma,
                "clip_coef": dict(self._dp_coefs),
                "delta": cfg.dp_delta,
                "epsilon": privacy.gaussian_epsilon(
                    cfg.dp_noise_multiplier, epoch + 1, cfg.dp_delta)}
        self.ledger.commit_aggregate(b"")
        return agg_info, extra

    def run_round(self, eval_global: bool = False) -> RoundStats:
        cfg, led = self.cfg, self.ledger
        if led.finished:
            raise RuntimeError(
                f"FL run finished: epoch {led.epoch} > max_epoch "
                f"{cfg.max_epoch} (reference clients exit here, "
                "main.py:251-252)")
        epoch = led.epoch
        t0 = time.perf_counter()
        # only the LOCAL step size is scheduled; delta extraction,
        # candidates and the server apply keep cfg.learning_rate
        local_lr = cfg.local_lr(epoch)
        if self._lr_dev is not None:
            self._lr_dev.fill_(local_lr)
        self._dp_coefs.clear()

        local_updates = self._phase_train()
        self._fence()
        t1 = time.perf_counter()
        updates, bad_update_sigs = self._phase_publish(epoch, local_updates)
        t2 = time.perf_counter()
        my_scores = self._phase_score(epoch, updates)
        self._fence()
        t3 = time.perf_counter()
        decision, bad_score_sigs = self._phase_decide(epoch, my_scores)
        agg_info, extra = self._phase_aggregate(epoch, updates, decision)
        self._fence()
        t4 = time.perf_counter()

        acc = None
        if eval_global and self.test_shard is not None:
            acc = self.evaluate_global()
        self._round += 1
        stats = RoundStats(
            epoch=epoch, wall_s=t4 - t0, train_s=t1 - t0, gather_s=t2 - t1,
            score_s=t3 - t2, aggregate_s=t4 - t3,
            global_loss=led.global_loss, n_updates=len(updates),
            n_selected=len(decision.selected),
            samples_trained=sum(n for _, _, n, _ in local_updates)
            * cfg.local_epochs, test_acc=acc)
        self.metrics.log("round", stats,
                         selected=[o for o, _ in decision.selected],
                         bad_signatures=bad_update_sigs + bad_score_sigs,
                         local_lr=local_lr, aggregation=agg_info, **extra)
        return stats

    # ------------------------------------------------------------------
    def evaluate_global(self) -> float:
        """Sponsor evaluation (reference run_sponsor, main.py:280-340)."""
        assert self.test_shard is not None
        self.model.set_flat(self.global_flat)
        return self.model.accuracy(self.test_shard.x, self.test_shard.y)

    def run(self, rounds: int, eval_every: int = 0) -> List[RoundStats]:
        out = []
        for r in range(rounds):
            if self.ledger.finished:  # max_epoch reached (main.py:251)
                break
            ev = eval_every > 0 and (r + 1) % eval_every == 0
            out.append(self.run_round(eval_global=ev))
        return out

    # ------------------------------------------------------------------
    # checkpoint / resume (chain persistence -> snapshot)
    def save(self, path: str) -> None:
        torch.save({
            "config": self.cfg.to_dict(),
            "ledger": self.ledger.snapshot(),
            "global_flat": self.global_flat.cpu(),
            "round": self._round,
        }, path)

    def load(self, path: str) -> None:
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert ck["config"]["model"] == self.cfg.model
        self.ledger.restore(ck["ledger"])
        # copy INTO the existing buffer: captured graphs bake its
        # device pointer (global_flat must never reallocate)
        with torch.no_grad():
            self.global_flat.copy_(ck["global_flat"].to(self.device))
        self._round = ck["round"]
