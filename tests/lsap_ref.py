"""CPU restatement of the batched linear-sum-assignment kernel (pq3d_amd/csrc/lsap.hip): scipy's shortest-augmenting-path
solver (rectangular_lsap.cpp, Crouse) in float64, with the Dijkstra step's sequential column choice replaced by the
order-independent rule the kernel reduces with.  Let m be the least shortest-path cost over the remaining columns:
  - if a column with cost m is unassigned, take the one at the LARGEST position in `remaining`;
  - otherwise take the column with cost m at the SMALLEST position.
Returns (rows, cols) as int64 arrays, or raises ValueError with scipy's messages."""
from __future__ import annotations

import numpy as np

INVALID = "matrix contains invalid numeric entries"
INFEASIBLE = "cost matrix is infeasible"


def select(spc_rem: np.ndarray, unassigned: np.ndarray) -> int:
    """Position in `remaining` the kernel's reduction picks (spc_rem / unassigned indexed by position)."""
    m = spc_rem.min()
    tie = spc_rem == m
    free = np.flatnonzero(tie & unassigned)
    return int(free[-1]) if free.size else int(np.flatnonzero(tie)[0])


def lsap(cost) -> tuple:
    c = np.asarray(cost, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError("expected a matrix (2-D array)")
    nr, nc = c.shape
    if nr == 0 or nc == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    tr = nc < nr
    if tr:
        c = c.T
        nr, nc = nc, nr
    if np.isnan(c).any() or (c == -np.inf).any():
        raise ValueError(INVALID)
    u = np.zeros(nr)
    v = np.zeros(nc)
    col4row = np.full(nr, -1, np.int64)
    row4col = np.full(nc, -1, np.int64)
    path = np.full(nc, -1, np.int64)
    for cur in range(nr):
        remaining = np.arange(nc - 1, -1, -1, dtype=np.int64)
        num = nc
        SR = np.zeros(nr, bool)
        SC = np.zeros(nc, bool)
        spc = np.full(nc, np.inf)
        i, min_val, sink = cur, 0.0, -1
        while sink == -1:
            SR[i] = True
            js = remaining[:num]
            r = ((min_val + c[i, js]) - u[i]) - v[js]
            better = r < spc[js]
            path[js[better]] = i
            spc[js[better]] = r[better]
            idx = select(spc[js], row4col[js] == -1)
            min_val = spc[js[idx]]
            if min_val == np.inf:
                raise ValueError(INFEASIBLE)
            j = int(js[idx])
            if row4col[j] == -1:
                sink = j
            else:
                i = int(row4col[j])
            SC[j] = True
            num -= 1
            remaining[idx] = remaining[num]
        others = SR.copy()
        others[cur] = False
        u[others] += min_val - spc[col4row[others]]
        u[cur] += min_val
        v[SC] -= min_val - spc[SC]
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            if i == cur:
                break
    if tr:
        order = np.argsort(col4row)
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.copy()
