"""Graph automorphisms of one molecule, for the symmetry-aware RMSD (``Engine.pair_rmsd``, ``FlowMol.rmsd_matrix``).  Pure Python / torch on the host.

DEFINITION.  ``automorphisms`` returns the automorphisms of the SELECTED, COLOURED bond graph: the vertices are the selected atoms, two of them are joined
when their pair token is a bond (an edge's colour is that token), and a vertex's colour is (atom token, charge token, sorted multiset of (bond token, atom
token) over its UNSELECTED neighbours).  With the heavy atoms selected the last term carries the hydrogen counts, so a CH3 carbon is never mapped onto a CH2
carbon, while the hydrogens themselves are not permuted.  When every unselected neighbour is a leaf (hydrogens) each such automorphism extends to one of the
whole molecule; for other selections this is a definition, not a theorem about the whole molecule."""
from __future__ import annotations

from typing import List, Optional

import torch


def _bond_matrix(e_upper, n: int, mask_token: Optional[int]) -> List[List[int]]:
    e = [int(v) for v in torch.as_tensor(e_upper).reshape(-1).tolist()]
    if len(e) != n * (n - 1) // 2:
        raise ValueError(f'e_upper has {len(e)} entries, {n} atoms have {n * (n - 1) // 2} unordered pairs')
    bond = [[0] * n for _ in range(n)]
    k = 0
    for i in range(n):
        for j in range(i + 1, n):
            t = e[k]
            k += 1
            bond[i][j] = bond[j][i] = 0 if (mask_token is not None and t == mask_token) else t
    return bond


def _refine(colour: List[int], nodes: List[int], bond: List[List[int]]) -> List[int]:
    """Colour refinement (1-WL with edge colours) over the induced subgraph of ``nodes``: stable colours as dense integers, numbered in a way that depends
    on the colours' contents only."""
    ids = sorted(set(colour[v] for v in nodes))
    col = {v: ids.index(colour[v]) for v in nodes}
    while True:
        sig = {v: (col[v], tuple(sorted((bond[v][u], col[u]) for u in nodes if u != v and bond[v][u] != 0))) for v in nodes}
        ids = sorted(set(sig.values()))
        index = {s: i for i, s in enumerate(ids)}
        new = {v: index[sig[v]] for v in nodes}
        if len(ids) == len(set(col.values())):
            return [new.get(v, -1) for v in range(len(colour))]
        col = new


def automorphisms(a, c, e_upper, select=None, max_perms: int = 256, mask_token: Optional[int] = None) -> torch.Tensor:
    """The automorphisms of the selected, coloured bond graph of one molecule (module docstring) as a (P, n) int64 tensor of full-length rows: row[i] is
    the atom that atom i is mapped onto, the identity on unselected atoms; the identity comes first and the rows are in lexicographic order.

    ``a``, ``c`` (n,): atom and charge tokens; ``e_upper`` (n (n - 1) / 2,): pair tokens in upper-triangle order (row-major, i < j).  Pair token 0 and
    ``mask_token`` (the model's n_bond_types, when given) mean "no bond", as in the valence check; every other token is an edge colour.  ``select`` (n,) bool,
    None = all atoms.  More than ``max_perms`` automorphisms raise ValueError naming the count reached: pass ``symmetry=False`` or a smaller selection."""
    a = [int(v) for v in torch.as_tensor(a).reshape(-1).tolist()]
    c = [int(v) for v in torch.as_tensor(c).reshape(-1).tolist()]
    n = len(a)
    if len(c) != n:
        raise ValueError(f'a has {n} entries, c {len(c)}')
    bond = _bond_matrix(e_upper, n, mask_token)
    if select is None:
        sel = [True] * n
    else:
        sel = [bool(v) for v in torch.as_tensor(select).reshape(-1).tolist()]
        if len(sel) != n:
            raise ValueError(f'select has {len(sel)} entries, the molecule {n} atoms')
    nodes = [v for v in range(n) if sel[v]]
    start = {}
    for v in nodes:
        start[v] = (a[v], c[v], tuple(sorted((bond[v][u], a[u]) for u in range(n) if not sel[u] and bond[v][u] != 0)))
    ids = sorted(set(start.values()))
    colour = _refine([ids.index(start[v]) if sel[v] else -1 for v in range(n)], nodes, bond)
    rows: List[List[int]] = []
    image = list(range(n))
    used = [False] * n

    def extend(k: int):
        if k == len(nodes):
            if len(rows) >= max_perms:
                raise ValueError(f'more than max_perms = {max_perms} automorphisms ({len(rows) + 1} reached): pass symmetry=False, a smaller selection or a '
                                 f'larger max_perms')
            rows.append(list(image))
            return
        v = nodes[k]
        for w in nodes:          # ascending candidates for ascending atoms: the rows come out in lexicographic order
            if used[w] or colour[w] != colour[v]:
                continue
            if any(bond[v][nodes[q]] != bond[w][image[nodes[q]]] for q in range(k)):
                continue
            used[w], image[v] = True, w
            extend(k + 1)
            used[w], image[v] = False, v

    extend(0)
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), n)
