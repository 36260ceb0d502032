"""Stereo elements of one molecular graph, for the stereo check of conformers (``Engine.stereo``, ``FlowMol.match_stereo``).  Pure Python / torch on the host.

DEFINITION.  ``stereo_elements`` lists the places of a token graph where two arrangements of the same graph in space differ by more than a rotation about
single bonds: tetrahedral centres (kind 0) and double bonds (kind 1).  Whether two substituents are "different" is decided by colour refinement
(``symmetry._refine``, 1-WL with bond tokens as edge colours) over the whole molecule, started from (atom token, charge token): two neighbours count as
different when their stable colours differ.  This is a definition over the labelling the project already shares with ``symmetry.automorphisms``; it is NOT the
CIP system, assigns no R/S or E/Z label, and only says where a sign is to be compared between two coordinate sets of ONE graph.

WHAT IT LEAVES OUT.
  * three-coordinate centres: N, P and S with three neighbours (and a lone pair) are never listed, whether or not they invert;
  * centres whose inequivalence colour refinement cannot see: cis/trans substitution of a ring (the two ring branches of such a carbon refine to one colour),
    pseudo-asymmetric centres, and anything else where the substituents differ only in their own stereo state;
  * allenes and other cumulenes (an end with a second double or a triple bond is skipped), and atropisomers (hindered rotation about a single bond).
A molecule whose only stereo lies in these passes the check whatever its coordinates."""
from __future__ import annotations

from typing import List, Optional

import torch

from .symmetry import _bond_matrix, _refine

TETRA, DOUBLE_BOND = 0, 1


def _ring_path(bond: List[List[int]], nodes: List[int], a: int, b: int, limit: int) -> bool:
    """Is there a path from ``a`` to ``b`` of at most ``limit`` bonds that avoids the bond a-b itself?  Breadth first."""
    seen, front = {a}, [a]
    for depth in range(1, limit + 1):
        nxt = []
        for v in front:
            for u in nodes:
                if bond[v][u] == 0 or u in seen or (v == a and u == b):
                    continue
                if u == b:
                    return True
                seen.add(u)
                nxt.append(u)
        front = nxt
    return False


def stereo_elements(a, c, e_upper, mask_token: Optional[int] = None, fake_token: Optional[int] = None, max_ring: int = 8) -> torch.Tensor:
    """The stereo elements of one molecule as a (Q, 5) int64 tensor of rows ``[kind, i0, i1, i2, i3]`` with local atom indices, sorted, so that the
    result is a function of the graph alone (module docstring: the definition and what it leaves out).

    ``a``, ``c`` (n,): atom and charge tokens; ``e_upper`` (n (n - 1) / 2,): pair tokens in upper-triangle order (row-major, i < j), read as
    ``extract_moldata`` reads them: 0 and ``mask_token`` (the model's n_bond_types, when given) mean no bond, 1 / 2 / 3 are bond orders, 4 (models with
    explicit aromaticity) is aromatic.  Atoms whose token is ``fake_token`` (when given) and their pairs are ignored.

    kind 0, tetrahedral centre: an atom with exactly four neighbours, all four bonds of token 1, the four neighbours of pairwise distinct colours.  Row
    ``(centre, n1, n2, n3)``: the three lowest-index neighbours; the fourth is implied.

    kind 1, double bond: a pair a < b with bond token 2 where neither end has another bond of token 2 or 3, each end has one or two further neighbours,
    two further neighbours of one end have distinct colours, and the bond lies in no ring of at most ``max_ring`` atoms (the shortest path from a to b
    that avoids the bond has more than ``max_ring - 1`` bonds, or there is none): a kekulized aromatic ring or a small ring fixes its double bonds.  Row
    ``(s_a, a, b, s_b)``: ``s_a`` / ``s_b`` the lowest-index further neighbour of each end."""
    a = [int(v) for v in torch.as_tensor(a).reshape(-1).tolist()]
    c = [int(v) for v in torch.as_tensor(c).reshape(-1).tolist()]
    n = len(a)
    if len(c) != n:
        raise ValueError(f'a has {n} entries, c {len(c)}')
    bond = _bond_matrix(e_upper, n, mask_token)
    nodes = [v for v in range(n) if fake_token is None or a[v] != fake_token]
    real = set(nodes)
    for v in range(n):
        if v not in real:
            for u in range(n):
                bond[v][u] = bond[u][v] = 0
    if not nodes:
        return torch.zeros(0, 5, dtype=torch.int64)
    ids = sorted(set((a[v], c[v]) for v in nodes))
    colour = _refine([ids.index((a[v], c[v])) if v in real else -1 for v in range(n)], nodes, bond)
    nbrs = {v: [u for u in nodes if bond[v][u] != 0] for v in nodes}
    rows = []
    for v in nodes:
        nb = nbrs[v]
        if len(nb) == 4 and all(bond[v][u] == 1 for u in nb) and len(set(colour[u] for u in nb)) == 4:
            rows.append([TETRA, v, nb[0], nb[1], nb[2]])
    for p in nodes:
        for q in nbrs[p]:
            if q < p or bond[p][q] != 2:
                continue
            subs = []
            for end, other in ((p, q), (q, p)):
                rest = [u for u in nbrs[end] if u != other]
                if any(bond[end][u] in (2, 3) for u in rest) or not 1 <= len(rest) <= 2 or (len(rest) == 2 and colour[rest[0]] == colour[rest[1]]):
                    break
                subs.append(rest[0])
            if len(subs) == 2 and not _ring_path(bond, nodes, p, q, max_ring - 1):
                rows.append([DOUBLE_BOND, subs[0], p, q, subs[1]])
    return torch.tensor(sorted(rows), dtype=torch.int64).reshape(len(rows), 5)
