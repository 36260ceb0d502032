"""Conformer ensembles end to end: FlowMol.rmsd_matrix, prune_conformers and conformer_ensembles (ABI 14) on the `qm9` preset with synthetic weights.

Two input molecules, K = 4 conformers each, 5 time points: a six-ring of carbons (12 automorphisms over its heavy atoms) and a seven-atom chain with four
hydrogens (the identity only).  The conformers are computed once per library and shared.  Every check runs on the CPU emulation and, marked gpu, on the device."""
import pytest
import torch

import mixed_util as mu
from test_pair_rmsd import prune_loop

K, T, SEED = 4, 5, 23
SIZES = [6, 7]


def upper(n, bonds):
    return torch.tensor([bonds.get((i, j), 0) for i in range(n) for j in range(i + 1, n)], dtype=torch.int64)


def given():
    """The two graphs as the (tensors, n_atoms) form; qm9 tokens: C 0, H 1, O 3."""
    gen = torch.Generator().manual_seed(5)
    ring = {(i, i + 1): 1 for i in range(5)}
    ring[(0, 5)] = 1
    chain = {(0, 1): 1, (1, 2): 2, (0, 3): 1, (0, 4): 1, (0, 5): 1, (1, 6): 1}
    a = torch.tensor([0] * 6 + [0, 0, 3, 1, 1, 1, 1])
    return ({'x': torch.randn(13, 3, generator=gen) * 1.5, 'a': a, 'c': torch.ones(13, dtype=torch.int64), 'e': torch.cat([upper(6, ring), upper(7, chain)])},
            torch.tensor(SIZES))


_CACHE = {}


def conformers(lib, device):
    key = (id(lib), str(device))
    if key not in _CACHE:
        mdl = mu.model('qm9', lib, device)
        _CACHE[key] = (mdl, mdl.conformers(given(), n_conformers=K, n_timesteps=T, seed=SEED))
    return _CACHE[key]


def same(m, w):
    return torch.equal(m.x_1, w.x_1) and torch.equal(m.a_1, w.a_1) and torch.equal(m.c_1, w.c_1) and torch.equal(m.e_1, w.e_1)


def triangles(mats):
    return torch.cat([m[tuple(torch.triu_indices(m.shape[0], m.shape[0], 1))] for m in mats])


def _check_matrices(lib, device):
    mdl, confs = conformers(lib, device)
    assert len(confs) == 2 * K
    plain = mdl.rmsd_matrix(confs, n_conformers=K, heavy=True)
    sym = mdl.rmsd_matrix(confs, n_conformers=K, heavy=True, symmetry=True)
    for m in plain + sym:
        assert m.shape == (K, K) and m.dtype == torch.float32 and torch.equal(m, m.T) and bool((m.diagonal() == 0).all())
        assert bool((m[~torch.eye(K, dtype=torch.bool)] > 0).all())
    for p, s in zip(plain, sym):
        assert bool((s <= p).all())          # the identity is among the rows, and the arithmetic per row is the same
    assert torch.equal(sym[1], plain[1])     # the chain's heavy atoms have no symmetry
    # groups=[sizes] is n_conformers in its general form; the (tensors, n_atoms) form is the list's
    assert all(torch.equal(a, b) for a, b in zip(mdl.rmsd_matrix(confs, groups=[K, K], heavy=True), plain))
    both = mdl.rmsd_matrix(confs[:3] + confs[K:], groups=[3, K], heavy=True, symmetry=True)
    assert torch.equal(both[0], sym[0][:3, :3]) and torch.equal(both[1], sym[1])
    sel = [[True] * 6] * K + [[True, True, True, False, False, False, False]] * K
    assert all(torch.equal(a, b) for a, b in zip(mdl.rmsd_matrix(confs, n_conformers=K, select=sel), plain))
    # refusals
    with pytest.raises(ValueError, match='differ in size'):
        mdl.rmsd_matrix(confs, groups=[K + 1, K - 1])
    with pytest.raises(ValueError, match='groups'):
        mdl.rmsd_matrix(confs, groups=[K, K - 1])
    with pytest.raises(ValueError, match='n_conformers'):
        mdl.rmsd_matrix(confs, n_conformers=3)
    with pytest.raises(ValueError, match='max_perms'):
        mdl.rmsd_matrix(confs, n_conformers=K, heavy=True, symmetry=True, max_perms=11)
    t, n = mdl._given_molecules(confs)
    odd = {k[0]: v.clone() for k, v in t.items()}
    odd['c'][6] = 0          # one charge token of the ring's second conformer
    with pytest.raises(ValueError, match='ONE graph'):
        mdl.rmsd_matrix((odd, n), n_conformers=K, symmetry=True)
    assert len(mdl.rmsd_matrix((odd, n), n_conformers=K)) == 2          # without symmetry only the sizes must agree
    odd['a'][6] = 1          # ... and one atom becomes a hydrogen: heavy flags differ inside the group
    with pytest.raises(ValueError, match='flag different atoms'):
        mdl.rmsd_matrix((odd, n), n_conformers=K, heavy=True)


def test_rmsd_matrix_on_emulation(emu_lib):
    _check_matrices(emu_lib, 'cpu')


@pytest.mark.gpu
def test_rmsd_matrix_on_gpu():
    _check_matrices(None, 'cuda:0')


def _check_ensembles(lib, device):
    mdl, confs = conformers(lib, device)
    every = mdl.conformer_ensembles(given(), K, T, SEED, prune_rmsd=None)
    assert [len(g) for g in every] == [K, K]
    assert all(same(m, w) for m, w in zip([m for g in every for m in g], confs))
    mats = mdl.rmsd_matrix(confs, n_conformers=K, heavy=True, symmetry=True)
    d = triangles(mats)
    thr = float(d.sort().values[d.numel() // 2])          # the median pair distance: some conformers go, some stay; a value equal to it stays
    want_keep, want_rep = prune_loop(d, [K, K], thr)
    assert 2 < int(want_keep.sum()) < 2 * K
    kept, keep, rep = mdl.prune_conformers(confs, n_conformers=K, threshold=thr)
    assert torch.equal(keep, want_keep) and torch.equal(rep, want_rep)
    assert [len(g) for g in kept] == [int(want_keep[:K].sum()), int(want_keep[K:].sum())]
    assert all(m is confs[i] for m, i in zip([m for g in kept for m in g], want_keep.nonzero().reshape(-1).tolist()))
    ens = mdl.conformer_ensembles(given(), K, T, SEED, prune_rmsd=thr)
    assert [len(g) for g in ens] == [len(g) for g in kept]
    assert all(same(m, w) for m, w in zip([m for g in ens for m in g], [m for g in kept for m in g]))          # pruning selects, it never alters
    assert [len(g) for g in mdl.conformer_ensembles(given(), K, T, SEED, prune_rmsd=float('inf'))] == [1, 1]
    assert [len(g) for g in mdl.prune_conformers(confs, n_conformers=K, threshold=0.0)[0]] == [K, K]
    assert [len(g) for g in mdl.prune_conformers(confs, n_conformers=K, threshold=float('inf'))[0]] == [1, 1]
    t, n = mdl._given_molecules(confs)
    idx, keep_t, _ = mdl.prune_conformers(({k[0]: v for k, v in t.items()}, n), n_conformers=K, threshold=thr)          # the tensor form: indices, not objects
    assert torch.equal(keep_t, want_keep) and [i for g in idx for i in g] == want_keep.nonzero().reshape(-1).tolist()
    with pytest.raises(ValueError, match='return_tensors'):
        mdl.conformer_ensembles(given(), K, T, SEED, prune_rmsd=thr, return_tensors=True)
    with pytest.raises(ValueError, match='seed'):
        mdl.conformer_ensembles(given(), K, T, prune_rmsd=thr)


def test_conformer_ensembles_on_emulation(emu_lib):
    _check_ensembles(emu_lib, 'cpu')


@pytest.mark.gpu
def test_conformer_ensembles_on_gpu():
    _check_ensembles(None, 'cuda:0')
