"""Batched exact linear sum assignment on the device (include/pq3d_hip.h: pq3d_lsap_batched; csrc/lsap.hip).

``linear_sum_assignment_batched`` solves G independent problems in one launch, each exactly as
``scipy.optimize.linear_sum_assignment`` solves its block in float64, with device inputs and outputs and no host sync, so
it can be captured into a graph.  ``check_errors`` reads the per-matrix error codes once and raises scipy's messages."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib as L

MAX_DIM = L.H.PQ3D_LSAP_MAX_DIM      # rows and columns of every matrix of a launch
INVALID, INFEASIBLE, BAD_SIZE = L.H.PQ3D_LSAP_INVALID, L.H.PQ3D_LSAP_INFEASIBLE, L.H.PQ3D_LSAP_BAD_SIZE
_MESSAGES = {INVALID: "matrix contains invalid numeric entries", INFEASIBLE: "cost matrix is infeasible",
             BAD_SIZE: "n_rows / n_cols outside [0, R] / [0, Cmax]"}


def _sizes(t: Optional[torch.Tensor], G: int, dev, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != dev or t.shape != (G,):
        raise ValueError(f"{what} must be an int32 tensor [{G}] on {dev}")
    return t.contiguous()


def linear_sum_assignment_batched(cost: torch.Tensor, n_rows: Optional[torch.Tensor] = None,
                                  n_cols: Optional[torch.Tensor] = None
                                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Assignments of the G matrices ``cost[g, :n_rows[g], :n_cols[g]]`` (``cost`` fp32 [G, R, Cmax] on the device;
    ``n_rows`` / ``n_cols`` int32 [G] device tensors, None = R / Cmax for every matrix).

    Returns int32 device tensors ``row_idx`` [G, M], ``col_idx`` [G, M] (M = min(R, Cmax); pair k < n_match[g] of matrix g,
    in scipy's order; 0 past it), ``n_match`` [G] and ``err`` [G] (0, or INVALID / INFEASIBLE / BAD_SIZE with n_match = 0)."""
    if not isinstance(cost, torch.Tensor) or cost.dtype != torch.float32 or not cost.is_cuda:
        raise ValueError("cost must be a float32 device tensor")
    if cost.dim() != 3:
        raise ValueError(f"cost must be [G, R, Cmax], got {tuple(cost.shape)}")
    G, R, Cm = cost.shape
    if not (1 <= R <= MAX_DIM and 1 <= Cm <= MAX_DIM):
        raise ValueError(f"cost matrices must have 1 to {MAX_DIM} rows and columns, got {R} x {Cm}")
    dev = cost.device
    n_rows, n_cols = _sizes(n_rows, G, dev, "n_rows"), _sizes(n_cols, G, dev, "n_cols")
    if cost.stride(2) != 1 or cost.stride(0) != R * cost.stride(1) or cost.stride(1) < Cm:
        cost = cost.contiguous()
    M = min(R, Cm)
    idx = torch.empty(2, G, M, dtype=torch.int32, device=dev)
    stats = torch.empty(2, G, dtype=torch.int32, device=dev)
    if G:
        L.call("pq3d_lsap_batched", cost, G, R, Cm, cost.stride(1), n_rows, n_cols, idx[0], idx[1], stats[0], stats[1])
    return idx[0], idx[1], stats[0], stats[1]


def check_errors(err: torch.Tensor) -> None:
    """Read the error codes of a launch (one device-to-host copy) and raise scipy's ValueError for the first bad matrix."""
    codes = err.cpu().tolist()
    for g, c in enumerate(codes):
        if c:
            raise ValueError(f"{_MESSAGES.get(c, f'error code {c}')} (matrix {g})")
