"""Server-side aggregation rules over the ledger's selection.

`aggregate(deltas, selected, cfg)` turns the [K, P] fp32 stack of the
rows the ledger selected (`decision.selected`, in that order) into the
averaged pseudo-gradient the engine applies with `axpy_`:

  fedavg        the reference's weighted average (weighted_fedavg),
                exactly the call the engine made before this module
  trimmed_mean  coordinate-wise, t = min(agg_trim, (K-1)//2) values
                dropped at each end; UNWEIGHTED (the ledger's weights
                are ignored, as in the literature)
  median        coordinate-wise, t = (K-1)//2: the middle value or the
                mean of the two middle values; unweighted
  multi_krum    keeps the K - f rows of lowest Krum score,
                f = min(agg_byzantine, max(0, (K-2)//2)), and averages
                them with the ledger's weights (masked_wmean)

Runtime K may be below aggregate_count (fewer admitted updates); the
clamps above make every rule degrade deterministically instead of
raising. None of the rules carries state across rounds.

Krum's decision is taken on the host from the K x K Gram matrix
(ops.delta_gram): every replica computes the same G bits, hence the
same float64 distances, scores and kept set. Distances come from
d2 = G_ii + G_jj - 2 G_ij, which cancels: differences below about
1e-7 * ||d||^2 are rounding noise, far under the spread of honest
updates — and the reason equal scores resolve by position in
`selected`, never by rounding.
"""
from __future__ import annotations

from typing import Any, Dict, List, Sequence, Tuple

import torch

from bflc_amd.ops import functional as O


def effective_trim(aggregator: str, K: int, agg_trim: int) -> int:
    """Values dropped at each end by the coordinate-wise rules at K rows."""
    if aggregator == "median":
        return (K - 1) // 2
    return min(int(agg_trim), (K - 1) // 2)


def effective_byzantine(K: int, agg_byzantine: int) -> int:
    """Multi-Krum's f at K rows: the largest f <= agg_byzantine with
    K >= 2f + 2. Under that condition every honest row can fill its
    K - f - 2 scored neighbours with honest rows, while an attacker, with
    at most f - 1 colluders, must count at least K - 2f - 1 >= 1 honest
    row: colluding rows cannot score among themselves alone. It is one
    row weaker than the K >= 2f + 3 of Krum's convergence proof, so that
    two bad rows among six are still handled."""
    return min(int(agg_byzantine), max(0, (K - 2) // 2))


def krum_select(G: Sequence[Sequence[float]], f: int) -> List[int]:
    """Positions kept by multi-Krum from the K x K Gram matrix, in
    ascending position order. Python float64 throughout:
    d2[i][j] = G[i][i] + G[j][j] - 2 G[i][j] clamped at 0, score[i] = sum
    of the K - f - 2 smallest d2[i][j] (j != i), keep the K - f lowest
    scores, ties by position. K <= 2 keeps every row."""
    K = len(G)
    if K <= 2:
        return list(range(K))
    f = effective_byzantine(K, f)
    g = [[float(G[i][j]) for j in range(K)] for i in range(K)]
    m = K - f - 2  # neighbours scored; >= f >= 0, and >= 1 for K >= 3
    scores = []
    for i in range(K):
        d2 = sorted(max(g[i][i] + g[j][j] - 2.0 * g[i][j], 0.0)
                    for j in range(K) if j != i)
        s = 0.0
        for v in d2[:m]:  # ascending: a fixed summation order
            s += v
        scores.append(s)
    # NaN scores (a non-finite row) rank last; sorted() is stable, so
    # equal scores keep their position order
    def rank(i: int):
        nan = scores[i] != scores[i]
        return (nan, 0.0 if nan else scores[i], i)

    order = sorted(range(K), key=rank)
    return sorted(order[: K - f])


def aggregate(deltas: torch.Tensor, selected: Sequence[Tuple[str, float]],
              cfg) -> Tuple[torch.Tensor, Dict[str, Any]]:
    """(avg[P], info) for the rows of `deltas` ([K, P] fp32, row k the
    update of selected[k] = (origin, weight))."""
    K = deltas.shape[0]
    assert K == len(selected) and K > 0
    name = cfg.aggregator
    info: Dict[str, Any] = {"aggregator": name, "rows": K}
    if name == "fedavg":
        weights = torch.empty(K, dtype=torch.float32, device=deltas.device)
        for k, (_, w) in enumerate(selected):
            weights[k] = float(w)
        return O.weighted_fedavg(deltas, weights), info
    if name in ("trimmed_mean", "median"):
        t = effective_trim(name, K, cfg.agg_trim)
        info["t"] = t
        return O.order_stat_mean(deltas, t), info
    if name == "multi_krum":
        f = effective_byzantine(K, cfg.agg_byzantine) if K > 2 else 0
        G = O.delta_gram(deltas).cpu().tolist()  # <= 4 KiB, one sync
        kept = krum_select(G, f)
        w = [0.0] * K
        for k in kept:
            w[k] = float(selected[k][1])
        weights = torch.tensor(w, dtype=torch.float32, device=deltas.device)
        info["f"] = f
        info["kept"] = [selected[k][0] for k in kept]
        return O.masked_wmean(deltas, weights), info
    raise ValueError(f"unknown aggregator {name!r}")
