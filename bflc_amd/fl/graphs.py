"""hipGraph-captured local-train step.

The FL local-train inner loop is a fixed kernel DAG: parameters are
per-parameter autograd leaves ALIASING one flat compute buffer at fixed
device addresses (models/base.py), the optimizer is one fused flat
kernel, and every minibatch has the same shape (the trainer drops the
ragged tail, engine.py). A profiled round is made of many 8-25 us
kernels (profiles/r01_kernel_stats_nhwc.md), so per-kernel launch gaps
are a real cost; capturing one

    zero-visible-state -> forward -> backward -> fused optimizer -> loss+=

step into a hipGraph and replaying it once per batch launches the whole
step as a single unit.

Capture safety relies on invariants the rest of the framework already
guarantees:
  * ``model.flat`` / ``model.cflat`` never reallocate — ``set_flat``
    copies INTO them — so kernel pointers baked at capture stay valid
    across rounds and clients;
  * the train step performs no host sync (the loss accumulates into a
    device scalar; ``accuracy_t`` is device-resident; the only
    ``.item()`` calls in the stack are in FedAvg, outside this region);
  * intermediate/grad tensors allocated during capture live in the
    graph's private memory pool and are rewritten in place on replay.

SGD captures trivially. Adam captures through the graph-safe kernel
pair ``adam_tick`` + ``adam_master_dev`` (csrc/hip/elementwise.hip):
the step counter and the bias corrections (1-beta^t) live in DEVICE
buffers advanced inside the captured step, so nothing epoch-dependent
is baked in; ``reset_state()`` zeroes (m, v, step) between clients —
the reference builds a fresh optimizer per round (main.py:109,126).
Adam-on-GPU-fp32 (no bf16 shadow) stays eager: only the master+shadow
kernel has the device-step variant, and fp32 compute is a test-only
configuration.

The extended SGD step (``optimizer="sgdm"``: momentum, weight decay,
FedProx, clipping, scheduled lr) captures the same way: its learning
rate and clip coefficient are DEVICE floats (csrc/hip/optimizer.hip), so
the caller refills ``lr_dev`` between replays and the same graph runs at
the new step size. The optimizer object owns the momentum buffer and
the coefficient; ``lr_dev`` and the proximal anchor ``p0`` are the
caller's and must keep their addresses.

The optimizer kind is dispatched, and its per-pass state allocated and
reset, in ONE place: ``LocalOptimizer``. Both train graphs hold a
capturable one; the engine's eager loop holds a non-capturable one.

Capture executes real kernels, so construction MUTATES the weights —
callers build the stepper before loading the round's global weights
(engine.py does this), or snapshot/restore around construction.

Graph memory pools are the caller's choice (``pool=`` of every class,
``graph.pool()`` of an earlier capture). Graphs that only ever replay
one after another share ONE pool — per-scorer private pools each held
full-shard forward activations and grew GPU memory with the number of
local scorers (round-1 ADVICE item) — which is what the engine does for
the per-batch stepper, the per-candidate scorer and everything in
sequential mode. Graphs that replay CONCURRENTLY must not share pool
memory: in concurrent mode the engine gives each local client's
whole-phase graphs one private pool per client.
"""
from __future__ import annotations

import torch


class LocalOptimizer:
    """The local step's optimizer: per-pass state, ``step()`` and
    ``reset()`` for ``sgd | sgdm | adam``. ``capturable`` picks the
    Adam form: the device-step kernel pair (hipGraph-safe) or the eager
    kernel with a host step counter — two kernels on purpose, they
    differ in where 1 - beta^t is computed. sgdm owns a fresh buf +
    coef_dev and uses the caller's lr_dev / p0 (fixed addresses, baked
    into a capture)."""

    def __init__(self, model, optimizer: str, lr: float, capturable: bool,
                 sgdm_cfg=None, lr_dev=None, p0=None) -> None:
        self.model = model
        self.kind = optimizer
        self.capturable = capturable
        self.lr = float(lr)
        if optimizer == "adam":
            if capturable and model.cflat is model.flat:
                raise RuntimeError(
                    "graphed Adam needs the bf16-shadow model (the "
                    "device-step kernel is adam_master_graph_)")
            self.m = torch.zeros_like(model.flat)
            self.v = torch.zeros_like(model.flat)
            self.step_n = 0  # host step counter of the eager form
            if capturable:
                self.step_t = torch.zeros(1, device=model.device,
                                          dtype=torch.int32)
                self.bc = torch.zeros(2, device=model.device,
                                      dtype=torch.float32)
        elif optimizer == "sgdm":
            from bflc_amd.models.base import SGDMState
            if sgdm_cfg is None or lr_dev is None:
                raise ValueError("optimizer='sgdm' needs sgdm_cfg and lr_dev")
            self.sgdm = SGDMState.for_model(sgdm_cfg, model, lr_dev, p0)
        elif optimizer != "sgd":
            raise ValueError(optimizer)

    def step(self) -> None:
        if self.kind == "sgd":
            self.model.sgd_step(self.lr)
        elif self.kind == "sgdm":
            self.model.sgdm_step(self.sgdm)
        elif self.capturable:
            self.model.adam_step_graph(self.m, self.v, self.step_t,
                                       self.bc, self.lr)
        else:
            self.step_n += 1
            self.model.adam_step(self.m, self.v, self.step_n, self.lr)

    def reset(self) -> None:
        """Fresh state for a new client pass, on the current stream
        (the reference builds a new optimizer per round, main.py:109)."""
        if self.kind == "adam":
            self.m.zero_()
            self.v.zero_()
            self.step_n = 0
            if self.capturable:
                self.step_t.zero_()
        elif self.kind == "sgdm":
            self.sgdm.reset()


def train_step(model, opt: LocalOptimizer, xb, yb, cost=None):
    """One local minibatch step, in the order every path keeps:
    zero_grad, loss, backward, optimizer step, then (only when
    accumulating) cost += loss."""
    model.zero_grad()
    loss = model.loss(xb, yb)
    loss.backward()
    opt.step()
    if cost is not None:
        cost.add_(loss.detach().float())


def _capture(warm, body, pool, zero_grad_of=None):
    """Run ``warm()`` on a side stream (materializes autograd engine
    state and cat/workspace allocations so none of it happens
    mid-capture), join, then capture ``body()`` into a new graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm()
    torch.cuda.current_stream().wait_stream(side)
    if zero_grad_of is not None:
        # grads=None at capture: backward's grad tensors are allocated
        # from the graph pool and rewritten in place on every replay
        zero_grad_of.zero_grad()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=pool):
        body()
    return graph


class GraphedTrainStep:
    """One captured (forward, backward, fused-optimizer) step over
    static input buffers; ``step()`` copies a batch in and replays."""

    def __init__(self, model, lr: float, x_proto: torch.Tensor,
                 y_proto: torch.Tensor, optimizer: str = "sgd",
                 warmup: int = 2, pool=None, sgdm_cfg=None, lr_dev=None,
                 p0=None) -> None:
        self.model = model
        self.optimizer = optimizer
        self.sx = torch.empty_like(x_proto)
        self.sy = torch.empty_like(y_proto)
        self.cost = torch.zeros((), device=model.device,
                                dtype=torch.float32)
        self.sx.copy_(x_proto)
        self.sy.copy_(y_proto)
        self.opt = LocalOptimizer(model, optimizer, lr, True, sgdm_cfg,
                                  lr_dev, p0)

        def warm():
            for _ in range(max(warmup, 1)):
                train_step(model, self.opt, self.sx, self.sy)

        self.graph = _capture(
            warm, lambda: train_step(model, self.opt, self.sx, self.sy,
                                     self.cost),
            pool, zero_grad_of=model)

    def reset_state(self) -> None:
        """Fresh optimizer for a new client/round (reference builds a
        new TF graph per round, main.py:109)."""
        self.opt.reset()

    def pool(self):
        return self.graph.pool()

    def matches(self, xb: torch.Tensor, yb: torch.Tensor) -> bool:
        return (xb.shape == self.sx.shape and xb.dtype == self.sx.dtype
                and yb.shape == self.sy.shape)

    def step(self, xb: torch.Tensor, yb: torch.Tensor) -> None:
        self.sx.copy_(xb)
        self.sy.copy_(yb)
        self.graph.replay()


class GraphedLocalTrain:
    """A client's ENTIRE local training pass as one graph: every
    minibatch step (forward, backward, fused optimizer, loss
    accumulate) of `local_epochs x total_batches` captured back to back
    with the client's OWN shard slices baked in (shard tensors are
    engine-lifetime persistent, so no per-batch input copies at all).
    One replay per client per round instead of one per batch — the
    per-round launch/copy overhead of the train phase collapses to a
    single dispatch."""

    def __init__(self, model, lr: float, shard_x: torch.Tensor,
                 shard_y: torch.Tensor, batch_size: int,
                 local_epochs: int, optimizer: str = "sgd",
                 pool=None, sgdm_cfg=None, lr_dev=None, p0=None) -> None:
        self.model = model
        self.optimizer = optimizer
        self.cost = torch.zeros((), device=model.device,
                                dtype=torch.float32)
        n = shard_x.shape[0]
        bs = min(batch_size, n)
        self.total_batches = max(n // bs, 1)
        self.n_steps = self.total_batches * local_epochs
        self.opt = LocalOptimizer(model, optimizer, lr, True, sgdm_cfg,
                                  lr_dev, p0)
        batches = [(shard_x[b * bs:(b + 1) * bs],
                    shard_y[b * bs:(b + 1) * bs])
                   for b in range(self.total_batches)] * local_epochs

        def warm():
            for _ in range(2):
                train_step(model, self.opt, *batches[0])

        def whole_pass():
            for xb, yb in batches:
                train_step(model, self.opt, xb, yb, self.cost)

        self.graph = _capture(warm, whole_pass, pool, zero_grad_of=model)

    def pool(self):
        return self.graph.pool()

    def run(self) -> torch.Tensor:
        """One replay = the whole local training pass. Caller loads the
        round's global weights first (set_flat). Returns the summed
        per-batch loss (device scalar)."""
        self.cost.zero_()
        self.opt.reset()
        self.graph.replay()
        return self.cost


class GraphedScorePhase:
    """One scorer's ENTIRE committee-scoring pass as one graph: for
    each of the K quota slots, build candidate = global - lr*stack[k]
    in place, load it, and evaluate accuracy on the scorer's shard —
    K candidate evaluations and their accuracy reads in a single
    replay. `cand_stack` must be the engine's persistent [K, P] packed
    buffer (same device pointers every round)."""

    def __init__(self, model, shard_x: torch.Tensor,
                 shard_y: torch.Tensor, cand_stack: torch.Tensor,
                 global_flat: torch.Tensor, lr: float, pool=None) -> None:
        from bflc_amd.ops import functional as O
        self.model = model
        self.K = cand_stack.shape[0]
        self.accs = torch.zeros(self.K, device=model.device,
                                dtype=torch.float32)
        lr = float(lr)

        # candidate load is ONE fused kernel writing the compute-dtype
        # shadow directly (the eval forward's only weight consumer);
        # the fp32 master stays stale during scoring — every later
        # phase reloads it via set_flat (ops/functional.py score_load_)
        def score_slot(k: int) -> torch.Tensor:
            O.score_load_(model.cflat.data, global_flat, cand_stack[k], lr)
            return model.accuracy_t(shard_x, shard_y)

        def all_slots():
            for k in range(self.K):
                self.accs[k] = score_slot(k)

        self.graph = _capture(lambda: score_slot(0), all_slots, pool)

    def pool(self):
        return self.graph.pool()

    def run(self) -> torch.Tensor:
        """Replay; returns a snapshot of the K accuracies (device)."""
        self.graph.replay()
        return self.accs.clone()

    def run_inplace(self) -> torch.Tensor:
        """Replay; returns the live accs buffer (no allocation) — for
        concurrent per-scorer stream replays, where the caller reads
        the buffer only after joining all scorer streams."""
        self.graph.replay()
        return self.accs


class GraphedScore:
    """Captured committee-scoring evaluation: load a candidate flat
    vector into the model (copy + shadow refresh) and run accuracy over
    the scorer's own shard — the shard tensors are baked into the graph
    (they never change), only the candidate is copied in per replay.
    The per-round scoring cost scales with the number of admitted
    candidates (committee size x quota at 8 nodes), so this is the
    phase that grows with world size."""

    def __init__(self, model, shard_x: torch.Tensor,
                 shard_y: torch.Tensor, pool=None) -> None:
        self.model = model
        self.cand = torch.empty_like(model.flat)
        self.cand.copy_(model.flat.detach())

        def load_and_score():
            model.set_flat(self.cand)
            return model.accuracy_t(shard_x, shard_y)

        def captured():
            self.acc = load_and_score()

        self.graph = _capture(load_and_score, captured, pool)

    def pool(self):
        return self.graph.pool()

    def score(self, cand: torch.Tensor) -> torch.Tensor:
        """Returns a device scalar snapshot (no host sync)."""
        self.cand.copy_(cand)
        self.graph.replay()
        return self.acc.clone()

    def score_candidate(self, global_flat: torch.Tensor, lr: float,
                        delta: torch.Tensor) -> torch.Tensor:
        """Build candidate = global - lr*delta DIRECTLY in the graph's
        input buffer (reference main.py:215-216) — no per-candidate
        clone+copy round trip (the engine's scoring loop runs
        committee x quota of these per round)."""
        from bflc_amd.ops import functional as O
        self.cand.copy_(global_flat)
        O.axpy_(self.cand, -lr, delta)
        self.graph.replay()
        return self.acc.clone()
