"""The stereo check at the model level: FlowMol.match_stereo and conformer_ensembles(stereo=...) (ABI 15) on the `qm9` preset with synthetic weights.

match_stereo runs on the constructed molecules of tests/test_stereo.py (a rigid copy, a mirror image, a centre with two leaves swapped, a flipped double
bond).  conformer_ensembles runs on two input molecules, K = 4 conformers each, 5 time points: C(F)(OH)(NH2)H (one tetrahedral centre, so a mismatch is a
mirror image) and but-2-ene with its hydrogens (one double bond, no centre, so nothing is ever a mirror image).  Synthetic weights place the atoms anywhere:
about half the conformers come back with the other sign, which is what the filter is for.  The conformers are computed once per library and shared.
SEED was picked on the emulation so that 'match' keeps at least one and drops at least one conformer of each molecule; the emulation run asserts that.  On the
device only the consistency relations are asserted: the sampler's last bits are not pinned between the two.
Every check runs on the CPU emulation and, marked gpu, on the device."""
import math

import pytest
import torch

import mixed_util as mu
from test_conformer_ensembles import same, triangles
from test_stereo import BASE_ATOMS, BASE_BONDS, GRAPHS, _tetra, batch, graph

K, T, SEED = 4, 5, 22


# ------------------------------------------------------------------------------------------------------------------ match_stereo
def constructed():
    """The cases a .. d of tests/test_stereo.py and their reference as the (tensors, n_atoms) form."""
    B = batch()
    a, c, e, _ = graph(BASE_ATOMS, BASE_BONDS)
    tens = lambda key: {'x': torch.cat([B[k][key] for k in 'abcd']), 'a': a.repeat(4), 'c': c.repeat(4), 'e': e.repeat(4)}
    return (tens('x'), torch.tensor([15] * 4)), (tens('ref'), torch.tensor([15] * 4))


def _check_match_stereo(lib, device):
    mdl = mu.model('qm9', lib, device)
    (mt, n), (rt, _) = constructed()
    want = torch.tensor([[2, 2, 0, 1, 1, 0, 1, 0], [2, 2, 2, 1, 1, 0, 0, 1], [2, 2, 1, 1, 1, 0, 0, 0], [2, 2, 0, 1, 1, 1, 0, 0]], dtype=torch.int32)
    out, match, table = mdl.match_stereo((mt, n), (rt, n))
    assert match.dtype == torch.bool and match.tolist() == [True, False, False, False] and table.dtype == torch.int32 and torch.equal(table, want)
    assert out[0] is mt          # the full list, unfiltered and unaltered
    out, match, table = mdl.match_stereo((mt, n), (rt, n), mirror=True)
    assert match.tolist() == [True, True, False, False] and torch.equal(table, want)
    flip = torch.tensor([1.0, -1.0, 1.0, 1.0]).repeat_interleave(15)[:, None]
    assert torch.equal(out[0]['x'], mt['x'] * flip) and all(torch.equal(out[0][k], mt[k]) for k in 'ace') and out[1].tolist() == [15] * 4
    # the same as SampledMolecule lists
    mols = mdl._package(dict(mt), n, None, False, False)
    refs = mdl._package(dict(rt), n, None, False, False)
    out, match, table = mdl.match_stereo(mols, refs)
    assert match.tolist() == [True, False, False, False] and torch.equal(table, want) and all(o is m for o, m in zip(out, mols))
    out, match, table = mdl.match_stereo(mols, refs, mirror=True)
    assert match.tolist() == [True, True, False, False] and torch.equal(table, want)
    assert all(out[i] is mols[i] for i in (0, 2, 3)) and out[1] is not mols[1]
    assert torch.equal(out[1].x_1, -mols[1].x_1) and torch.equal(out[1].a_1, mols[1].a_1) and torch.equal(out[1].c_1, mols[1].c_1)
    assert torch.equal(out[1].e_1, mols[1].e_1)
    assert mdl.match_stereo(out, refs)[1].tolist() == [True, True, False, False]          # what was inverted now matches as it stands
    # mixed forms, and a flat_tol above every value: nothing is defined, nothing matches
    assert mdl.match_stereo(mols, (rt, n))[1].tolist() == [True, False, False, False]
    assert mdl.match_stereo(mols, refs, flat_tol=1.5)[1].tolist() == [False] * 4
    # refusals
    with pytest.raises(ValueError, match='size'):
        mdl.match_stereo(mols[:3], refs)
    with pytest.raises(ValueError, match='size'):
        mdl.match_stereo(mols[:1], mdl._package({'x': torch.zeros(4, 3), 'a': torch.zeros(4), 'c': torch.ones(4), 'e': torch.zeros(6)}, torch.tensor([4]), None,
                                                False, False))
    for key, row, what in (('a', 7, 'atom type'), ('c', 20, 'charge'), ('e', 3, 'bond order')):
        odd = {k: v.clone() for k, v in mt.items()}
        odd[key][row] = 2 if key != 'c' else 0
        with pytest.raises(ValueError, match=what):
            mdl.match_stereo((odd, n), (rt, n))
    with pytest.raises(ValueError, match='flat_tol'):
        mdl.match_stereo(mols, refs, flat_tol=-0.1)


def test_match_stereo_on_emulation(emu_lib):
    _check_match_stereo(emu_lib, 'cpu')


@pytest.mark.gpu
def test_match_stereo_on_gpu():
    _check_match_stereo(None, 'cuda:0')


# ------------------------------------------------------------------------------------------------------------------ conformer_ensembles
def given():
    """C(F)(OH)(NH2)H and but-2-ene (the cis isomer) with coordinates, as the (tensors, n_atoms) form."""
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    (a1, c1, e1, _), _ = GRAPHS['cfonh']          # C0 F1 O2 N3, H4 on C, H5 on O, H6 H7 on N
    x1 = torch.zeros(8, 3, dtype=torch.float64)
    x1[1] = t(0.0, 0.0, 1.35)
    x1[2], x1[3], x1[4] = _tetra(x1[0], x1[1], [1.43, 1.47, 1.09], 0.2)
    x1[5] = x1[2] + 0.96 * t(0.6, 0.64, 0.48)
    x1[6], x1[7] = x1[3] + 1.01 * t(0.0, -0.6, 0.8), x1[3] + 1.01 * t(-0.8, 0.0, -0.6)
    (a2, c2, e2, _), _ = GRAPHS['but-2-ene']      # C0 C1 = C2 C3, H4..6 on C0, H7 on C1, H8 on C2, H9..11 on C3
    c60, s60 = 0.5, math.sqrt(3.0) / 2
    x2 = torch.zeros(12, 3, dtype=torch.float64)
    x2[2] = t(1.34, 0, 0)
    x2[0], x2[7] = 1.5 * t(-c60, s60, 0), 1.09 * t(-c60, -s60, 0)
    x2[3], x2[8] = x2[2] + 1.5 * t(c60, s60, 0), x2[2] + 1.09 * t(c60, -s60, 0)
    x2[4], x2[5], x2[6] = _tetra(x2[0], x2[1], [1.09] * 3, 0.3)
    x2[9], x2[10], x2[11] = _tetra(x2[3], x2[2], [1.09] * 3, 0.9)
    return ({'x': torch.cat([x1, x2]).float(), 'a': torch.cat([a1, a2]), 'c': torch.cat([c1, c2]), 'e': torch.cat([e1, e2])}, torch.tensor([8, 12]))


def references():
    t, n = given()
    cut = lambda v, sizes: [p for p in torch.split(v, sizes) for _ in range(K)]
    return ({'x': torch.cat(cut(t['x'], [8, 12])), 'a': torch.cat(cut(t['a'], [8, 12])), 'c': torch.cat(cut(t['c'], [8, 12])),
             'e': torch.cat(cut(t['e'], [28, 66]))}, n.repeat_interleave(K))


_CACHE = {}


def conformers(lib, device, seed=SEED):
    key = (id(lib), str(device), seed)
    if key not in _CACHE:
        mdl = mu.model('qm9', lib, device)
        _CACHE[key] = (mdl, mdl.conformers(given(), n_conformers=K, n_timesteps=T, seed=seed))
    return _CACHE[key]


def flat(groups):
    return [m for g in groups for m in g]


def _check_ensembles(lib, device, pinned):
    mdl, confs = conformers(lib, device)
    out, match, table = mdl.match_stereo(confs, references())
    assert table[:K, 0].tolist() == [1] * K and table[:K, 3].tolist() == [0] * K and table[K:, 0].tolist() == [0] * K and table[K:, 3].tolist() == [1] * K
    assert all(o is c for o, c in zip(out, confs))
    sizes = [int(match[:K].sum()), int(match[K:].sum())]
    print('match', match.tolist(), 'table', table.tolist())
    if pinned:          # the seed's purpose
        assert all(0 < s < K for s in sizes), sizes
    # 'match', no pruning: conformers(...) filtered by match_stereo's match
    filtered = [c for c, k in zip(confs, match.tolist()) if k]
    ens = mdl.conformer_ensembles(given(), K, T, SEED, stereo='match')
    assert [len(g) for g in ens] == sizes and all(same(m, w) for m, w in zip(flat(ens), filtered))
    # 'mirror': the same filter after the inversion; every inverted member is exactly the negative of its original
    out2, match2, table2 = mdl.match_stereo(confs, references(), mirror=True)
    assert torch.equal(table2, table) and torch.equal(match2, match | (table[:, 7] != 0)) and not bool(table[K:, 7].any())
    inverted = (table[:, 7] != 0).tolist()
    for i, (o, c) in enumerate(zip(out2, confs)):
        assert (torch.equal(o.x_1, -c.x_1) and torch.equal(o.a_1, c.a_1) and torch.equal(o.e_1, c.e_1)) if inverted[i] else o is c
    if pinned:
        assert any(inverted) and match2[:K].all() and match2[K:].tolist() == match[K:].tolist()          # a lone centre that mismatches is a mirror image
    filtered2 = [m for m, k in zip(out2, match2.tolist()) if k]
    ens2 = mdl.conformer_ensembles(given(), K, T, SEED, stereo='mirror')
    assert [len(g) for g in ens2] == [int(match2[:K].sum()), int(match2[K:].sum())] and all(same(m, w) for m, w in zip(flat(ens2), filtered2))
    # with a threshold: prune_conformers of the filtered list, the groups now of unequal sizes
    for mode, kept, gs in (('match', filtered, sizes), ('mirror', filtered2, [len(g) for g in ens2])):
        if not kept:          # possible on the device only, where the seed pins nothing
            assert mdl.conformer_ensembles(given(), K, T, SEED, stereo=mode, prune_rmsd=0.5) == [[], []]
            continue
        d = triangles(mdl.rmsd_matrix(kept, groups=gs, heavy=True, symmetry=True))
        thr = float(d.sort().values[d.numel() // 2]) if d.numel() else 0.5          # the median pair distance of what the filter left; equal to it stays
        want = mdl.prune_conformers(kept, groups=gs, threshold=thr)[0]
        got = mdl.conformer_ensembles(given(), K, T, SEED, stereo=mode, prune_rmsd=thr)
        assert [len(g) for g in got] == [len(g) for g in want] and all(same(m, w) for m, w in zip(flat(got), flat(want))), mode
        if pinned:
            assert sum(len(g) for g in got) < len(kept)          # the threshold does drop something
    # stereo=None is the call without the argument
    every = mdl.conformer_ensembles(given(), K, T, SEED, stereo=None)
    assert [len(g) for g in every] == [K, K] and all(same(m, w) for m, w in zip(flat(every), confs))
    # refusals
    with pytest.raises(ValueError, match='stereo must be'):
        mdl.conformer_ensembles(given(), K, T, SEED, stereo='flip')
    with pytest.raises(ValueError, match='return_tensors'):
        mdl.conformer_ensembles(given(), K, T, SEED, stereo='match', return_tensors=True)
    with pytest.raises(ValueError, match='trajectories'):
        mdl.conformer_ensembles(given(), K, T, SEED, stereo='mirror', xt_traj=True)


def test_conformer_ensembles_stereo_on_emulation(emu_lib):
    _check_ensembles(emu_lib, 'cpu', pinned=True)


@pytest.mark.gpu
def test_conformer_ensembles_stereo_on_gpu():
    _check_ensembles(None, 'cuda:0', pinned=False)
