"""Topologies and Metropolis-Hastings mixing weights in CSR form.

Replaces the dense construction of DecentralizedTrainer._create_mixing_matrix
(trainer.py:91-136), which needs two N x N float64 matrices (64 GiB at
N = 65536).  Here a topology is a list of sorted neighbour ids per worker and
W is built directly in CSR with the diagonal included.

Bit-exactness with the reference: W_ij = 1 / (1 + max(d_i, d_j)) is one IEEE
division, and W_ii = 1 - np.sum(W[i, neighbours]) is evaluated with the same
numpy call on the same float64 vector the reference sums (neighbour weights in
ascending column order, 0.0 in the slot of a self loop), so every entry equals
the reference's W to the bit (tests/test_topology.py checks the fixtures).

Topologies:
  ring              trainer.py:95-98 (N = 1 gives a self loop, N = 2 degree 1)
  grid              trainer.py:99-108, nx.grid_2d_graph(side, side, periodic=True)
                    with row-major ids over sorted (r, c) nodes; side 2 has degree 2
  fully_connected   trainer.py:109-110
  random_regular    not in the reference: the random k-regular graph of
                    BASELINE.json config C3 (pairing model, fixed seed)

Directed topologies (not in the reference; push-sum, trainer algorithm='push_sum'): a
DirectedTopology is built from sorted OUT-neighbour lists and carries the COLUMN-stochastic
matrix A_ij = 1 / (1 + outdeg_j) on the edges j -> i and on the diagonal, in CSR by rows.
  directed_ring     i -> i+1
  exponential       i -> (i + 2^k) mod n for every 2^k < n
  random_digraph    the directed ring plus k - 1 further distinct random out-neighbours per
                    node (fixed seed): unbalanced in-degrees
"""
from __future__ import annotations

import numpy as np


class Topology:
    """Neighbour lists + MH weights.  `row_ptr`, `col`, `w` include the diagonal."""

    def __init__(self, name, neighbours):
        self.name = name
        self.n = len(neighbours)
        self.neighbours = neighbours
        # reference degrees = row sums of the 0/1 adjacency (float64), self loop included
        self.degrees = np.array([float(len(nb)) for nb in neighbours], dtype=np.float64)
        self.row_ptr, self.col, self.w = _mh_csr(neighbours, self.degrees)

    @property
    def nnz(self):
        return int(self.row_ptr[-1])

    def dense_adjacency(self):
        adj = np.zeros((self.n, self.n))
        for i, nb in enumerate(self.neighbours):
            adj[i, nb] = 1.0
        return adj

    def dense_W(self):
        W = np.zeros((self.n, self.n))
        for i in range(self.n):
            s, e = self.row_ptr[i], self.row_ptr[i + 1]
            W[i, self.col[s:e]] = self.w[s:e]
        return W

    def sparse_W(self):
        from scipy.sparse import csr_matrix

        return csr_matrix((self.w, self.col, self.row_ptr), shape=(self.n, self.n))

    def uniform_offdiag(self):
        """(w_off, diag) when every off-diagonal weight is present and equal (the
        complete graph), else None: then sum_j W_ij x_j = w_off (S - x_i) + W_ii x_i."""
        n = self.n
        if n < 2 or self.nnz != n * n:
            return None
        diag_mask = self.col == np.repeat(np.arange(n), n)
        off = self.w[~diag_mask]
        if not np.all(off == off[0]):
            return None
        return float(off[0]), self.w[diag_mask].copy()

    def check(self):
        """trainer.py:129-131 on the CSR form: rows sum to 1 and W is symmetric."""
        if self.n == 0:
            return
        rs = np.add.reduceat(self.w, self.row_ptr[:-1]) if self.nnz else np.zeros(self.n)
        assert np.allclose(rs, 1.0), f"Rows of W do not sum to 1 (Topology: {self.name})"
        S = self.sparse_W()
        assert abs(S - S.T).max() <= 1e-8 + 1e-5 * abs(S).max(), f"W is not symmetric (Topology: {self.name})"

    def spectral_gap(self, dense_limit=4096):
        """trainer.py:133-135: 1 - (second largest |eigenvalue|).  Dense eigvalsh up to
        `dense_limit` workers, Lanczos (scipy eigsh) on the CSR matrix above it."""
        if self.n <= 1:
            return None
        if self.n <= dense_limit:
            ev = np.linalg.eigvalsh(self.dense_W())
            return 1.0 - np.sort(np.abs(ev))[-2]
        from scipy.sparse.linalg import eigsh

        ev = eigsh(self.sparse_W(), k=2, which="LM", return_eigenvectors=False, tol=1e-10)
        return 1.0 - np.sort(np.abs(ev))[0]


def _mh_csr(neighbours, degrees):
    n = len(neighbours)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    cols, vals = [], []
    for i, nb in enumerate(neighbours):
        nb = np.asarray(nb, dtype=np.int64)
        # off-diagonal weights, one IEEE division each (trainer.py:125)
        wn = 1.0 / (1.0 + np.maximum(degrees[i], degrees[nb]))
        wn[nb == i] = 0.0  # W[i, i] is still 0 when the reference sums the row
        wii = 1.0 - np.sum(wn)  # trainer.py:126, same numpy reduction on the same vector
        if np.any(nb == i):
            row_c, row_w = nb, wn.copy()
            row_w[nb == i] = wii
        else:
            pos = int(np.searchsorted(nb, i))
            row_c = np.concatenate([nb[:pos], [i], nb[pos:]])
            row_w = np.concatenate([wn[:pos], [wii], wn[pos:]])
        cols.append(row_c)
        vals.append(row_w)
        row_ptr[i + 1] = row_ptr[i] + len(row_c)
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    w = np.concatenate(vals).astype(np.float64) if vals else np.zeros(0)
    return row_ptr, col, w


def ring(n):
    nbrs = []
    for i in range(n):
        nbrs.append(sorted({(i + 1) % n, (i - 1 + n) % n}))
    return Topology("ring", nbrs)


def grid(n):
    side = int(np.sqrt(n))
    if side * side != n:
        raise ValueError(f"Warning: N_WORKERS ({n}) is not a perfect square.")
    nbrs = [set() for _ in range(n)]
    for r in range(side):
        for c in range(side):
            u = r * side + c
            for v in (((r + 1) % side) * side + c, r * side + (c + 1) % side):
                if u != v:  # nx.grid_2d_graph has no self loops
                    nbrs[u].add(v)
                    nbrs[v].add(u)
    return Topology("grid", [sorted(s) for s in nbrs])


def fully_connected(n):
    allv = np.arange(n)
    return Topology("fully_connected", [np.delete(allv, i) for i in range(n)])


def random_regular(n, k, seed=0, max_tries=10000):
    """Uniform-ish random simple k-regular graph by the pairing model with restarts."""
    if (n * k) % 2 or k >= n:
        raise ValueError(f"no simple {k}-regular graph on {n} vertices")
    rng = np.random.default_rng(seed)
    stubs = np.repeat(np.arange(n), k)
    for _ in range(max_tries):
        p = rng.permutation(stubs).reshape(-1, 2)
        a, b = p[:, 0], p[:, 1]
        if np.any(a == b):
            continue
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        key = lo.astype(np.int64) * n + hi
        if len(np.unique(key)) != len(key):
            continue
        nbrs = [[] for _ in range(n)]
        for u, v in zip(lo.tolist(), hi.tolist()):
            nbrs[u].append(v)
            nbrs[v].append(u)
        return Topology("random_regular", [sorted(x) for x in nbrs])
    raise RuntimeError("random_regular: no simple graph found")


class DirectedTopology:
    """Out-neighbour lists + push-sum weights.  `row_ptr`, `col`, `w`: row i holds the
    in-neighbours of i plus i, ascending, with A_ij = 1 / (1 + outdeg_j) (one IEEE division),
    so every COLUMN of A sums to 1."""

    directed = True

    def __init__(self, name, out_neighbours):
        self.name = name
        self.n = n = len(out_neighbours)
        self.out_neighbours = [np.asarray(nb, dtype=np.int64) for nb in out_neighbours]
        self.out_degrees = np.array([float(len(nb)) for nb in self.out_neighbours], dtype=np.float64)
        self.degrees = self.out_degrees
        src = np.concatenate([np.full(len(nb), j, dtype=np.int64) for j, nb in enumerate(self.out_neighbours)] +
                             [np.arange(n, dtype=np.int64)])
        dst = np.concatenate(self.out_neighbours + [np.arange(n, dtype=np.int64)])
        if len(np.unique(dst * max(n, 1) + src)) != len(src):
            raise ValueError(f"out-neighbour lists with a self loop or a repeated edge (Topology: {name})")
        order = np.lexsort((src, dst))  # by row, columns ascending
        self.col = src[order].astype(np.int32)
        self.w = 1.0 / (1.0 + self.out_degrees[src[order]])
        self.row_ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(dst, minlength=n), out=self.row_ptr[1:])

    nnz = Topology.nnz
    dense_W = Topology.dense_W
    sparse_W = Topology.sparse_W

    @classmethod
    def from_undirected(cls, topo):
        """The directed form of an undirected Topology: the same neighbour lists read as
        out-neighbours (every edge both ways), out-degree weights."""
        return cls(topo.name, [np.asarray(nb, dtype=np.int64)[np.asarray(nb, dtype=np.int64) != i]
                               for i, nb in enumerate(topo.neighbours)])

    def dense_adjacency(self):
        """adj[j, i] = 1 for every edge j -> i."""
        adj = np.zeros((self.n, self.n))
        for j, nb in enumerate(self.out_neighbours):
            adj[j, nb] = 1.0
        return adj

    def check(self):
        """Columns of A sum to 1 and the graph is strongly connected."""
        if self.n == 0:
            return
        cs = np.bincount(self.col, weights=self.w, minlength=self.n)
        assert np.allclose(cs, 1.0), f"Columns of A do not sum to 1 (Topology: {self.name})"
        from scipy.sparse.csgraph import connected_components

        nc, _ = connected_components(self.sparse_W(), directed=True, connection="strong")
        assert nc == 1, f"The graph is not strongly connected (Topology: {self.name})"


def directed_ring(n):
    return DirectedTopology("directed_ring", [[(i + 1) % n] if n > 1 else [] for i in range(n)])


def exponential(n):
    hops = [1 << k for k in range(max(n, 1).bit_length()) if (1 << k) < n]
    return DirectedTopology("exponential", [sorted({(i + h) % n for h in hops}) for i in range(n)])


def random_digraph(n, k, seed=0):
    """The directed ring plus k - 1 further distinct random out-neighbours per node (no self
    loops): out-degree k everywhere, in-degrees unbalanced, so the push-sum weights leave 1."""
    if n > 1 and not 1 <= k <= n - 1:
        raise ValueError(f"no simple digraph of out-degree {k} on {n} vertices")
    rng = np.random.default_rng(seed)
    nbrs = []
    for i in range(n):
        if n == 1:
            nbrs.append([])
            continue
        ring_nb = (i + 1) % n
        others = np.delete(np.arange(n, dtype=np.int64), [i, ring_nb])
        extra = rng.choice(others, size=k - 1, replace=False) if k > 1 else np.zeros(0, np.int64)
        nbrs.append(sorted([ring_nb] + extra.tolist()))
    return DirectedTopology("random_digraph", nbrs)


DIRECTED = ("directed_ring", "exponential", "random_digraph")


def relabel(topo, order):
    """The same graph with new vertex ids: new id k is old vertex order[k] (a permutation).
    MH weights are recomputed on the new ids (per edge the same value; W_ii can differ in
    the last bit, as it sums the row in the new column order)."""
    order = np.asarray(order, dtype=np.int64)
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    nbrs = [np.sort(inv[np.asarray(topo.neighbours[o], dtype=np.int64)]) for o in order]
    return Topology(topo.name, nbrs)


def build(name, n, config=None):
    """trainer.py:95-112 dispatch; unknown names raise the reference's ValueError."""
    config = config or {}
    if name == "ring":
        return ring(n)
    if name == "grid":
        return grid(n)
    if name == "fully_connected":
        return fully_connected(n)
    if name == "random_regular":
        return random_regular(n, int(config.get("regular_degree", 4)), int(config.get("topology_seed", 0)))
    if name == "directed_ring":
        return directed_ring(n)
    if name == "exponential":
        return exponential(n)
    if name == "random_digraph":
        return random_digraph(n, int(config.get("regular_degree", 4)), int(config.get("topology_seed", 0)))
    raise ValueError(f"Wrong topology: {name}")
