"""flowmol_amd.symmetry.automorphisms against a brute-force enumeration (CPU only): every permutation of the selected atoms that preserves the vertex colours
-- (atom token, charge token, sorted multiset of (bond token, atom token) over the UNSELECTED neighbours) -- and every bond token between selected atoms."""
import itertools

import pytest
import torch

from flowmol_amd.symmetry import automorphisms

from test_pair_rmsd import BTB_BONDS, RING_BONDS


def upper(n, bonds):
    """Pair tokens in upper-triangle order from {(i, j): token}; 0 elsewhere."""
    return torch.tensor([bonds.get((i, j), bonds.get((j, i), 0)) for i in range(n) for j in range(i + 1, n)], dtype=torch.int64)


def brute_force(a, c, e, select=None, mask_token=None):
    n = len(a)
    tok = [[0] * n for _ in range(n)]
    k = 0
    for i in range(n):
        for j in range(i + 1, n):
            t = int(e[k])
            tok[i][j] = tok[j][i] = 0 if t == mask_token else t
            k += 1
    sel = [True] * n if select is None else [bool(s) for s in select]
    nodes = [i for i in range(n) if sel[i]]
    colour = {v: (int(a[v]), int(c[v]), tuple(sorted((tok[v][u], int(a[u])) for u in range(n) if not sel[u] and tok[v][u]))) for v in nodes}
    rows = []
    for image in itertools.permutations(nodes):
        p = dict(zip(nodes, image))
        if all(colour[v] == colour[p[v]] for v in nodes) and all(tok[u][v] == tok[p[u]][p[v]] for u in nodes for v in nodes if u < v):
            rows.append([p.get(i, i) for i in range(n)])
    return sorted(rows)


def chain(n):
    return {(i, i + 1): 1 for i in range(n - 1)}


ONES = {b: 1 for b in RING_BONDS}
# name: (atom tokens, charge tokens, {bond: token}, select or None, automorphisms expected)
CASES = {
    'one': ([0], [0], {}, None, 1),
    'two': ([0, 1], [0, 0], {(0, 1): 1}, None, 1),
    'two_alike': ([0, 0], [1, 1], {(0, 1): 2}, None, 2),
    'line': ([0, 1, 2, 1, 3], [0] * 5, chain(5), None, 1),
    'ring': ([0] * 6, [0] * 6, ONES, None, 12),
    'btb': ([0] * 8, [0] * 8, {b: 1 for b in BTB_BONDS}, None, 72),
    'chain_distinct_ends': ([1, 0, 0, 0, 2], [0] * 5, chain(5), None, 1),
    'chain_alike_ends': ([1, 0, 0, 0, 1], [0] * 5, chain(5), None, 2),
    'chain_charged_end': ([1, 0, 0, 0, 1], [0, 0, 0, 0, 1], chain(5), None, 1),
    'star_one_double_arm': ([0, 1, 1, 1], [0] * 4, {(0, 1): 1, (0, 2): 1, (0, 3): 2}, None, 2),
    'star': ([0, 1, 1, 1], [0] * 4, {(0, 1): 1, (0, 2): 1, (0, 3): 1}, None, 6),
    'ring_one_hetero': ([2, 0, 0, 0, 0, 0], [0] * 6, ONES, None, 2),
    'ring_alternating_bonds': ([0] * 6, [0] * 6, {(i, (i + 1) % 6): 1 + i % 2 for i in range(6)}, None, 6),
    # C0 (three H) - C1 (two H, one F): the carbons are selected, and only their unselected neighbours tell them apart
    'ch3_ch2': ([0, 0, 3, 3, 3, 3, 3, 4], [0] * 8, {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1, (1, 5): 1, (1, 6): 1, (1, 7): 1},
                [True, True] + [False] * 6, 1),
    'ch3_ch3': ([0, 0, 3, 3, 3, 3, 3, 3], [0] * 8, {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1, (1, 5): 1, (1, 6): 1, (1, 7): 1},
                [True, True] + [False] * 6, 2),
    'mask_token_is_no_bond': ([0, 0, 0], [0] * 3, {(0, 1): 1, (1, 2): 1, (0, 2): 5}, None, 2),
}


@pytest.mark.parametrize('name', list(CASES))
def test_automorphisms_equal_the_brute_force_enumeration(name):
    a, c, bonds, select, count = CASES[name]
    n = len(a)
    e = upper(n, bonds)
    got = automorphisms(torch.tensor(a), torch.tensor(c), e, None if select is None else torch.tensor(select), mask_token=5)
    want = brute_force(a, c, e.tolist(), select, mask_token=5)
    assert got.dtype == torch.int64 and tuple(got.shape) == (count, n)
    assert got.tolist() == want                                  # the same set, in lexicographic order
    assert got[0].tolist() == list(range(n))                     # the identity comes first
    if select is not None:
        fixed = ~torch.tensor(select)
        assert bool((got[:, fixed] == torch.arange(n)[fixed]).all())


def test_more_than_max_perms_is_refused_with_the_count():
    a, c, bonds, _, _ = CASES['btb']
    with pytest.raises(ValueError, match='72 reached'):
        automorphisms(torch.tensor(a), torch.tensor(c), upper(8, bonds), max_perms=71)
    assert automorphisms(torch.tensor(a), torch.tensor(c), upper(8, bonds), max_perms=72).shape[0] == 72


def test_argument_shapes_are_checked():
    with pytest.raises(ValueError, match='unordered pairs'):
        automorphisms(torch.zeros(3), torch.zeros(3), torch.zeros(2))
    with pytest.raises(ValueError, match='select'):
        automorphisms(torch.zeros(3), torch.zeros(3), torch.zeros(3), select=torch.ones(2, dtype=torch.bool))


def test_a_larger_graph_stays_fast():
    """A 30-atom chain with a methyl-like fork at either end: 2 x 2 x 2 automorphisms, found without enumerating 30! candidates."""
    n = 30
    bonds = chain(n - 4)
    bonds.update({(0, n - 4): 1, (0, n - 3): 1, (n - 5, n - 2): 1, (n - 5, n - 1): 1})
    got = automorphisms(torch.zeros(n), torch.zeros(n), upper(n, bonds))
    assert got.shape == (8, n) and got[0].tolist() == list(range(n))
