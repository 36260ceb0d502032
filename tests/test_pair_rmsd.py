"""Symmetry-aware pair RMSD and threshold pruning on the device: fm_pair_rmsd / Engine.pair_rmsd, fm_prune_rmsd / Engine.prune_rmsd (ABI 14).

INPUTS (float32, one fixed generator; `graphs()`): the smallest sizes at which each mechanism can break.
  one      1 atom, two: 2 atoms                               identity only
  line     5 collinear atoms (a degenerate top eigenspace)      identity only
  ring     a 6-cycle of one atom type, 12 automorphisms; a strongly puckered, irregular geometry
  btb      the 8 heavy atoms of (CH3)3C-C(CH3)3, 3! 3! 2 = 72 automorphisms: more rows than lanes, so the lane stride wraps
  cloud47  a 47-atom Gaussian cloud, identity only
  big70    a 70-atom cloud shifted by 500, identity and one transposition: more atoms than lanes, so the strided means wrap
Every graph has 3 to 5 conformers: the base geometry under random proper rotations and translations plus 0.1 noise.  cloud47's conformer 2 is an exact rigid
copy (rmsd ~ 0, the cancellation case); ring's, btb's and big70's conformer 2 are exact rigid copies with the atoms relabelled by a non-identity automorphism
(far under the identity labelling, ~ 0 under the right row); ring's conformer 3 is the base mirrored through the ring plane (chiral: not 0).  The cases are all
pairs i < j of conformers of one graph, named 'graph:i-j'.

REFERENCE, written here: the float64 SVD Kabsch with the determinant correction of tests/test_align_rmsd.py, minimised over the permutation rows.
TOLERANCE (derived as in that file, not tuned): `reference(..., torch.float32)` restates it in float32; its error against float64 on these inputs, measured once
on the host (`f32_errors()`; recorded in DESIGN_LOG.md, 2026-10, "conformer ensembles"), is F32_ERR per case: (identity only, with the graph's rows).  The
kernel gets 8x that (a different eigen-solver with a fixed sweep count).  fm_align_rmsd's bound on the same input is, by its file's derivation, the same
8 x F32_ERR[case][0]; "the sum of the two bounds" of the comparison with that kernel is therefore 16 x F32_ERR[case][0].
Every device check runs on the CPU emulation and, marked gpu, on the device."""
import math

import pytest
import torch

from flowmol_amd.engine import _ptr
from flowmol_amd.symmetry import automorphisms
from hygiene_util import GuardSet

import mixed_util as mu

GRAPHS = ('one', 'two', 'line', 'ring', 'btb', 'cloud47', 'big70')
N_CONF = {'one': 3, 'two': 3, 'line': 3, 'ring': 5, 'btb': 4, 'cloud47': 4, 'big70': 3}

# |float32 restatement - float64 reference| of the aligned rmsd per case: (identity only, over the graph's permutation rows); measured, see the module docstring
F32_ERR = {
    'one:0-1': (0.0, 0.0), 'one:0-2': (0.0, 0.0), 'one:1-2': (0.0, 0.0),
    'two:0-1': (4.25e-08, 4.25e-08), 'two:0-2': (2.77e-08, 2.77e-08), 'two:1-2': (7.46e-08, 7.46e-08),
    'line:0-1': (1.13e-08, 1.13e-08), 'line:0-2': (3.08e-09, 3.08e-09), 'line:1-2': (4.55e-08, 4.55e-08),
    'ring:0-1': (7.11e-09, 7.11e-09), 'ring:0-2': (2.96e-08, 2.70e-07), 'ring:0-3': (3.89e-08, 2.91e-08), 'ring:0-4': (5.58e-08, 5.58e-08),
    'ring:1-2': (2.79e-09, 7.39e-08), 'ring:1-3': (8.72e-08, 3.95e-08), 'ring:1-4': (5.42e-08, 5.42e-08), 'ring:2-3': (2.71e-08, 2.81e-08),
    'ring:2-4': (3.52e-08, 5.36e-08), 'ring:3-4': (8.70e-09, 5.54e-08),
    'btb:0-1': (1.13e-07, 1.13e-07), 'btb:0-2': (6.23e-08, 3.39e-07), 'btb:0-3': (5.60e-09, 5.60e-09), 'btb:1-2': (3.09e-08, 3.90e-08),
    'btb:1-3': (2.79e-08, 2.79e-08), 'btb:2-3': (1.86e-08, 1.05e-07),
    'cloud47:0-1': (1.57e-08, 1.57e-08), 'cloud47:0-2': (3.96e-07, 3.96e-07), 'cloud47:0-3': (6.33e-08, 6.33e-08), 'cloud47:1-2': (5.96e-09, 5.96e-09),
    'cloud47:1-3': (3.28e-08, 3.28e-08), 'cloud47:2-3': (3.00e-08, 3.00e-08),
    'big70:0-1': (2.61e-08, 2.61e-08), 'big70:0-2': (3.21e-08, 2.39e-05), 'big70:1-2': (1.16e-07, 1.98e-08),
}
BOUND = {k: tuple(8.0 * e for e in v) for k, v in F32_ERR.items()}
# the same for the clouds with every third atom dropped from the fit (`sel_of`), over the graph's rows
SEL_GRAPHS = ('cloud47', 'big70')
SEL_F32_ERR = {
    'cloud47:0-1': 2.81e-08, 'cloud47:0-2': 4.70e-07, 'cloud47:0-3': 3.99e-08, 'cloud47:1-2': 1.35e-08, 'cloud47:1-3': 1.12e-07, 'cloud47:2-3': 3.41e-08,
    'big70:0-1': 8.61e-08, 'big70:0-2': 3.19e-05, 'big70:1-2': 1.12e-08,
}


def _rotation(gen):
    q = torch.randn(4, generator=gen, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def _upper(n, bonds):
    """Pair tokens in upper-triangle order: 1 on the listed bonds, 0 elsewhere."""
    e = []
    for i in range(n):
        for j in range(i + 1, n):
            e.append(1 if (i, j) in bonds or (j, i) in bonds else 0)
    return torch.tensor(e, dtype=torch.int64)


RING_BONDS = {(i, (i + 1) % 6) for i in range(6)}
BTB_BONDS = {(0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (1, 6), (1, 7)}          # 0, 1 the quaternary carbons; 2..4 and 5..7 their methyls
RING_RELABEL = [0, 5, 4, 3, 2, 1]          # a reflection of the cycle
BTB_RELABEL = [0, 1, 2, 4, 3, 6, 7, 5]     # two methyls of one end swapped, the other end's cycled
BIG_RELABEL = [68 if i == 3 else 3 if i == 68 else i for i in range(70)]

_GRAPHS = {}


def graphs():
    """{name: {'x': [conformers, (n,3) float32], 'rows': (P,n) int64 or None}}, built once."""
    if _GRAPHS:
        return _GRAPHS
    gen = torch.Generator().manual_seed(1409)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    move = lambda x: x @ _rotation(gen).T + rnd(1, 3) * 2.0
    noisy = lambda x: move(x) + 0.1 * rnd(*x.shape)

    def relabelled(x, g):          # an exact rigid copy whose atom g[i] is atom i of x
        y = torch.empty_like(x)
        y[torch.tensor(g)] = move(x)
        return y
    base = {'one': rnd(1, 3), 'two': rnd(2, 3), 'cloud47': rnd(47, 3) * 1.5, 'big70': rnd(70, 3) * 1.8 + 500.0}
    base['line'] = torch.tensor([-2.0, -0.7, 0.1, 1.2, 2.5], dtype=torch.float64)[:, None] * torch.tensor([[0.6, -0.3, 0.74]], dtype=torch.float64)
    ang = torch.arange(6, dtype=torch.float64) * (math.pi / 3)
    rad = torch.tensor([1.4, 0.8, 1.9, 1.0, 1.7, 0.7], dtype=torch.float64)
    base['ring'] = torch.stack([rad * ang.cos(), rad * ang.sin(), torch.tensor([0.6, -0.5, 0.4, 0.3, -0.7, 0.2], dtype=torch.float64)], dim=1)
    t = 1.54 * math.sqrt(8.0 / 9.0)
    arm = lambda k, up, twist: [t * math.cos(2 * math.pi * k / 3 + twist), t * math.sin(2 * math.pi * k / 3 + twist), up * (0.77 + 1.54 / 3)]
    btb = torch.tensor([[0.0, 0.0, 0.77], [0.0, 0.0, -0.77]] + [arm(k, 1.0, 0.0) for k in range(3)] + [arm(k, -1.0, math.pi / 3) for k in range(3)],
                       dtype=torch.float64)
    base['btb'] = btb + 0.15 * rnd(8, 3)
    conf = {k: [v] + [noisy(v) for _ in range(N_CONF[k] - 1)] for k, v in base.items()}
    conf['cloud47'][2] = move(base['cloud47'])
    conf['ring'][2] = relabelled(base['ring'], RING_RELABEL)
    conf['ring'][3] = move(base['ring'] * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))
    conf['btb'][2] = relabelled(base['btb'], BTB_RELABEL)
    conf['big70'][2] = relabelled(base['big70'], BIG_RELABEL)
    rows = {k: None for k in GRAPHS}
    rows['ring'] = automorphisms(torch.zeros(6), torch.zeros(6), _upper(6, RING_BONDS))
    rows['btb'] = automorphisms(torch.zeros(8), torch.zeros(8), _upper(8, BTB_BONDS), max_perms=72)
    rows['big70'] = torch.tensor([list(range(70)), BIG_RELABEL])
    assert rows['ring'].shape[0] == 12 and rows['btb'].shape[0] == 72
    for k in GRAPHS:
        _GRAPHS[k] = {'x': [c.float() for c in conf[k]], 'rows': rows[k]}
    return _GRAPHS


def cases():
    """[(case name, graph, i, j)]: every pair of conformers of one graph."""
    return [(f'{g}:{i}-{j}', g, i, j) for g in GRAPHS for i in range(N_CONF[g]) for j in range(i + 1, N_CONF[g])]


def reference(xa, xb, sel, dtype, rows=None):
    """min over the rows (None: the identity) of the Kabsch rmsd in ``dtype`` of a[i] onto b[row[i]], proper rotations only: R = V diag(1, 1, det) U^T.
    -> (the minimum, the rmsd of every row)."""
    a, b0 = xa.to(dtype), xb.to(dtype)
    s = torch.ones(a.shape[0], dtype=torch.bool) if sel is None else sel
    per_row = []
    for row in ([None] if rows is None else rows):
        b = b0 if row is None else b0[row]
        ac, bc = a - a[s].mean(0, keepdim=True), b - b[s].mean(0, keepdim=True)
        U, _, Vh = torch.linalg.svd(ac[s].T @ bc[s])
        D = torch.eye(3, dtype=dtype)
        D[2, 2] = torch.sign(torch.linalg.det(Vh.T @ U.T))
        R = Vh.T @ D @ U.T
        per_row.append(float((((ac @ R.T - bc)[s]) ** 2).sum(1).mean().sqrt()))
    return min(per_row), per_row


def f32_errors():
    """The measurement behind F32_ERR."""
    out, G = {}, graphs()
    for name, g, i, j in cases():
        xa, xb, rows = G[g]['x'][i], G[g]['x'][j], G[g]['rows']
        out[name] = (abs(reference(xa, xb, None, torch.float32)[0] - reference(xa, xb, None, torch.float64)[0]),
                     abs(reference(xa, xb, None, torch.float32, rows)[0] - reference(xa, xb, None, torch.float64, rows)[0]))
    return out


def sel_of(n):
    return torch.tensor([k % 3 != 1 for k in range(n)])


def f32_errors_select():
    """The measurement behind SEL_F32_ERR."""
    out, G = {}, graphs()
    for name, g, i, j in cases():
        if g in SEL_GRAPHS:
            xa, xb, rows, s = G[g]['x'][i], G[g]['x'][j], G[g]['rows'], sel_of(G[g]['x'][i].shape[0])
            out[name] = abs(reference(xa, xb, s, torch.float32, rows)[0] - reference(xa, xb, s, torch.float64, rows)[0])
    return out


_REF64 = {}


def ref64():
    """{case: ((identity rmsd, [it]), (rmsd over the rows, per row))} in float64, computed once."""
    if not _REF64:
        G = graphs()
        for name, g, i, j in cases():
            xa, xb = G[g]['x'][i], G[g]['x'][j]
            _REF64[name] = (reference(xa, xb, None, torch.float64), reference(xa, xb, None, torch.float64, G[g]['rows']))
    return _REF64


# ------------------------------------------------------------------------------------------------------------------ the batch
def layout(order=GRAPHS):
    """The batch of every conformer of the graphs in ``order`` -> (sizes, x (N,3), {(graph, conformer): molecule index}, perm_sets)."""
    G = graphs()
    sizes, xs, index, perm_set, rows = [], [], {}, [], []
    for g in order:
        sid = -1
        if G[g]['rows'] is not None:
            rows.append(G[g]['rows'])
            sid = len(rows) - 1
        for k, x in enumerate(G[g]['x']):
            index[(g, k)] = len(sizes)
            sizes.append(x.shape[0])
            xs.append(x)
            perm_set.append(sid)
    return sizes, torch.cat(xs), index, (torch.tensor(perm_set, dtype=torch.int32), rows)


def run(eng, case_list, order=GRAPHS, symmetry=True, select=None, shuffle_rows=False, x=None):
    """One Engine.pair_rmsd call on the batch of ``order`` for the cases of ``case_list`` -> (out (P,2), best (P,)) on the cpu."""
    sizes, x0, index, perm_sets = layout(order)
    eng.bind(torch.tensor(sizes))
    pairs = torch.tensor([[index[(g, i)], index[(g, j)]] for _, g, i, j in case_list], dtype=torch.int32).reshape(-1, 2)
    if shuffle_rows:
        gen = torch.Generator().manual_seed(77)
        perm_sets = (perm_sets[0], [r[torch.randperm(r.shape[0], generator=gen)] for r in perm_sets[1]])
    out, best = eng.pair_rmsd(x0 if x is None else x, pairs, select, perm_sets if symmetry else None, best=True)
    eng.synchronize()
    return out.cpu(), best.cpu()


_RESULTS = {}


def results(lib, device):
    """The kernel on all cases, with the rows and with the identity only: computed once per library and shared by the tests that read it."""
    key = (id(lib), str(device))
    if key not in _RESULTS:
        eng = mu.engine('qm9', lib, device)[0]
        _RESULTS[key] = (run(eng, cases(), symmetry=False), run(eng, cases(), symmetry=True))
    return _RESULTS[key]


# ------------------------------------------------------------------------------------------------------------------ 1. against float64
def test_every_case_has_a_recorded_bound():
    assert set(F32_ERR) == {c[0] for c in cases()} and set(SEL_F32_ERR) == {c[0] for c in cases() if c[1] in SEL_GRAPHS}


def _check_against_reference(lib, device):
    """Every case against float64, the identity alone and over the graph's rows, within 8 x F32_ERR."""
    (plain, _), (sym, best) = results(lib, device)
    ref, G, bad = ref64(), graphs(), []
    for p, (name, g, i, j) in enumerate(cases()):
        n = G[g]['x'][i].shape[0]
        assert float(plain[p, 0]) == n and float(sym[p, 0]) == n, name
        e0, e1 = abs(float(plain[p, 1]) - ref[name][0][0]), abs(float(sym[p, 1]) - ref[name][1][0])
        print(f'{name}: identity {e0:.3g} (bound {BOUND[name][0]:.3g}), rows {e1:.3g} (bound {BOUND[name][1]:.3g})')
        if not e0 <= BOUND[name][0]:
            bad.append((name, 'identity', e0, BOUND[name][0]))
        if not e1 <= BOUND[name][1]:
            bad.append((name, 'rows', e1, BOUND[name][1]))
        n_rows = 1 if G[g]['rows'] is None else G[g]['rows'].shape[0]
        assert 0 <= int(best[p]) < n_rows, name
    assert bad == [], bad


def test_pair_rmsd_against_float64_kabsch_on_emulation(emu_lib):
    _check_against_reference(emu_lib, 'cpu')


@pytest.mark.gpu
def test_pair_rmsd_against_float64_kabsch_on_gpu():
    _check_against_reference(None, 'cuda:0')


# ------------------------------------------------------------------------------------------------------------------ 2. symmetry discriminates
def test_the_relabelled_conformers_discriminate_in_the_reference():
    ref = ref64()
    for name in ('ring:0-2', 'btb:0-2'):
        assert ref[name][0][0] > 0.5 and ref[name][1][0] < 1e-6, (name, ref[name][0][0], ref[name][1][0])
    assert ref['ring:0-3'][1][0] > 0.1 and ref['cloud47:0-2'][0][0] < 1e-6          # the mirrored ring is no conformer under any row; the rigid copy is one


def _check_symmetry(lib, device):
    (plain, _), (sym, best) = results(lib, device)
    ref, G = ref64(), graphs()
    names = [c[0] for c in cases()]
    for name, relabel in (('ring:0-2', RING_RELABEL), ('btb:0-2', BTB_RELABEL)):
        p, g = names.index(name), name.split(':')[0]
        assert float(plain[p, 1]) > 0.5, (name, float(plain[p, 1]))
        assert float(sym[p, 1]) <= BOUND[name][1], (name, float(sym[p, 1]), BOUND[name][1])
        per_row = ref[name][1][1]
        assert per_row[int(best[p])] <= ref[name][1][0] + BOUND[name][1], (name, int(best[p]))
        assert G[g]['rows'][int(best[p])].tolist() == relabel, name
    assert bool((sym[:, 1] <= plain[:, 1]).all())          # the identity is among the rows and the arithmetic per row is the same


def test_symmetry_discriminates_on_emulation(emu_lib):
    _check_symmetry(emu_lib, 'cpu')


@pytest.mark.gpu
def test_symmetry_discriminates_on_gpu():
    _check_symmetry(None, 'cuda:0')


# ------------------------------------------------------------------------------------------------------------------ 3. canonical arithmetic
CANON = ('ring:0-2', 'ring:1-3', 'btb:0-1', 'cloud47:0-1', 'big70:0-1', 'two:0-1')


def _check_canonical(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    all_cases = cases()
    names = [c[0] for c in all_cases]
    full, best = results(lib, device)[1]
    back = run(eng, all_cases[::-1])[0].flip(0)
    assert torch.equal(back, full)                                              # the pair list reversed
    assert torch.equal(run(eng, all_cases, shuffle_rows=True)[0], full)           # the permutation rows shuffled
    assert torch.equal(run(eng, all_cases, order=GRAPHS[::-1])[0], full)          # the batch reordered
    for name in CANON:
        alone, alone_best = run(eng, [all_cases[names.index(name)]])
        assert torch.equal(alone[0], full[names.index(name)]) and int(alone_best[0]) == int(best[names.index(name)]), name      # a pair alone
    assert float(full[names.index('cloud47:0-1'), 1]) > 0.05


def test_a_pair_alone_reversed_shuffled_and_reordered_on_emulation(emu_lib):
    _check_canonical(emu_lib, 'cpu')


@pytest.mark.gpu
def test_a_pair_alone_reversed_shuffled_and_reordered_on_gpu():
    _check_canonical(None, 'cuda:0')


# ------------------------------------------------------------------------------------------------------------------ 4. against fm_align_rmsd
def _check_against_align(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    plain = results(lib, device)[0][0]
    G, all_cases = graphs(), cases()
    sizes = [G[g]['x'][i].shape[0] for _, g, i, _ in all_cases]
    eng.bind(torch.tensor(sizes))
    xa, xb = torch.cat([G[g]['x'][i] for _, g, i, _ in all_cases]), torch.cat([G[g]['x'][j] for _, g, _, j in all_cases])
    al = eng.align_rmsd(xa, xb).cpu()
    bad = []
    for p, (name, _, _, _) in enumerate(all_cases):
        assert float(al[p, 0]) == float(plain[p, 0]), name
        diff = abs(float(al[p, 2]) - float(plain[p, 1]))
        if not diff <= 2 * BOUND[name][0]:
            bad.append((name, diff, 2 * BOUND[name][0]))
    assert bad == [], bad
    # select: every third atom of the clouds dropped from the fit; the dropped atoms displaced by 3 must not enter
    sizes, x, index, _ = layout()
    sel = torch.cat([sel_of(n) if n >= 47 else torch.ones(n, dtype=torch.bool) for n in sizes])
    sub = [c for c in all_cases if c[1] in SEL_GRAPHS]
    got = run(eng, sub, select=sel)[0]
    moved = x.clone()
    moved[~sel] += 3.0
    assert torch.equal(run(eng, sub, select=sel, x=moved)[0], got)
    names = [c[0] for c in all_cases]
    assert not torch.equal(got[:, 1], results(lib, device)[1][0][[names.index(c[0]) for c in sub], 1])
    for p, (name, g, i, j) in enumerate(sub):
        s = sel_of(G[g]['x'][i].shape[0])
        want = reference(G[g]['x'][i], G[g]['x'][j], s, torch.float64, G[g]['rows'])[0]
        assert float(got[p, 0]) == int(s.sum()), name
        assert abs(float(got[p, 1]) - want) <= 8 * SEL_F32_ERR[name], (name, abs(float(got[p, 1]) - want), 8 * SEL_F32_ERR[name])


def test_identity_only_agrees_with_align_rmsd_on_emulation(emu_lib):
    _check_against_align(emu_lib, 'cpu')


@pytest.mark.gpu
def test_identity_only_agrees_with_align_rmsd_on_gpu():
    _check_against_align(None, 'cuda:0')


# ------------------------------------------------------------------------------------------------------------------ 5. hygiene and refusals
def _check_hygiene(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    order = ('two', 'ring', 'btb', 'one')
    sizes, x0, index, (perm_set, rows) = layout(order)
    eng.bind(torch.tensor(sizes))
    N = sum(sizes)
    sub = [c for c in cases() if c[1] in order]
    pr = torch.tensor([[index[(g, i)], index[(g, j)]] for _, g, i, j in sub], dtype=torch.int32)
    P = pr.shape[0]
    sel = torch.ones(N, dtype=torch.bool)
    sel[:6] = False                                  # the three conformers of 'two': nothing selected
    set_off = torch.tensor([0, rows[0].numel(), rows[0].numel() + rows[1].numel()], dtype=torch.int32)
    gs = GuardSet(eng.device)
    x = gs.inp('x', x0)
    prd = gs.inp('pairs', pr)
    sl = gs.inp('select', sel.to(torch.uint8))
    ps, so = gs.inp('perm_set', perm_set), gs.inp('set_off', set_off)
    pm = gs.inp('perms', torch.cat([r.reshape(-1) for r in rows]).to(torch.int32))
    out, best = gs.out('out', (P, 2)), gs.out('best', (P,), torch.int32)
    call = lambda x_, n, ph, pd, s, a, b, c, ns, o, bp: eng.lib.fm_pair_rmsd(eng._ctx, eng._stream(), _ptr(x_), n, _ptr(ph), _ptr(pd), _ptr(s), _ptr(a), _ptr(b),
                                                                            _ptr(c), ns, _ptr(o), _ptr(bp))
    assert call(x, P, pr, prd, sl, ps, so, pm, 2, out, best) == 0
    eng.synchronize()
    assert gs.check() == [] and gs.unwritten() == [], (gs.check(), gs.unwritten())
    want, want_best = run(eng, sub, order=order, select=sel)
    eng.bind(torch.tensor(sizes))
    assert torch.equal(out.cpu(), want) and torch.equal(best.cpu(), want_best)
    names = [c[0] for c in sub]
    assert torch.equal(out.cpu()[names.index('two:0-1')], torch.zeros(2)) and int(best.cpu()[names.index('two:0-1')]) == 0          # no atom selected
    # without best_perm, and without a table, the call writes out alone
    gs2 = GuardSet(eng.device)
    out2 = gs2.out('out', (P, 2))
    assert call(x, P, pr, prd, sl, ps, so, pm, 2, out2, None) == 0
    eng.synchronize()
    assert gs2.check() == [] and gs.check() == [] and torch.equal(out2.cpu(), out.cpu())
    err = lambda: eng.lib.fm_last_error(eng._ctx)
    before = (out.cpu().clone(), best.cpu().clone())
    unequal = torch.tensor([[index[('two', 0)], index[('ring', 0)]]], dtype=torch.int32)
    assert call(x, 1, unequal, prd, sl, ps, so, pm, 2, out, best) == -1 and b'unequal size' in err(), err()
    for bad_index in (len(sizes), -1):
        outside = torch.tensor([[0, bad_index]], dtype=torch.int32)
        assert call(x, 1, outside, prd, sl, ps, so, pm, 2, out, best) == -1 and b'outside' in err(), err()
    for args in ((x, P, pr, prd, sl, ps, so, pm, 2, x, best), (x, P, pr, prd, sl, ps, so, pm, 2, out, out), (x, P, pr, prd, sl, ps, so, pm, 2, out, pm),
                 (x, P, pr, prd, sl, ps, so, pm, 2, prd, best)):
        assert call(*args) == -1 and b'alias' in err(), err()
    assert call(x, P, pr, prd, sl, ps, None, pm, 2, out, best) == -1 and call(None, P, pr, prd, sl, ps, so, pm, 2, out, best) == -1
    assert call(x, P, None, prd, sl, ps, so, pm, 2, out, best) == -1
    eng.synchronize()
    assert gs.check() == [] and torch.equal(out.cpu(), before[0]) and torch.equal(best.cpu(), before[1])          # a refused call enqueues nothing
    # Engine.pair_rmsd: what it refuses before the call
    ring0 = index[('ring', 0)]
    pair = torch.tensor([[ring0, ring0 + 1]])
    one_set = lambda r: (torch.tensor([0 if k in (ring0, ring0 + 1) else -1 for k in range(len(sizes))]), [r])
    with pytest.raises(ValueError, match='not a permutation'):
        eng.pair_rmsd(x0, pair, None, one_set(torch.tensor([[0, 1, 2, 3, 4, 4]])))
    part = torch.ones(N, dtype=torch.bool)
    n0 = sum(sizes[:ring0])
    part[n0 + 5] = part[n0 + 6 + 5] = False
    with pytest.raises(ValueError, match='unselected'):
        eng.pair_rmsd(x0, pair, part, one_set(torch.tensor([[0, 1, 2, 3, 5, 4]])))
    with pytest.raises(ValueError, match='sizes of a pair differ'):
        eng.pair_rmsd(x0, unequal)
    with pytest.raises(ValueError, match='select'):
        eng.pair_rmsd(x0, pair, torch.ones(N + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match='bound batch'):
        eng.pair_rmsd(x0[:-1], pair)
    assert eng.pair_rmsd(x0, torch.zeros(0, 2, dtype=torch.int32)).shape == (0, 2)          # no pair: legal, nothing launched


def test_pair_rmsd_between_guard_bands_and_refusals_on_emulation(emu_lib):
    _check_hygiene(emu_lib, 'cpu')


@pytest.mark.gpu
def test_pair_rmsd_between_guard_bands_and_refusals_on_gpu():
    _check_hygiene(None, 'cuda:0')


# ------------------------------------------------------------------------------------------------------------------ 6. pruning
PRUNE_SIZES = (0, 1, 2, 5, 65, 130)
THR = 0.5


def prune_inputs():
    """Hand-built triangles of the groups PRUNE_SIZES (row-major, i < j), concatenated, in float32."""
    gen = torch.Generator().manual_seed(99)
    tris = []
    for K in PRUNE_SIZES:
        m = torch.full((K, K), 2.0)
        if K == 2:
            m[0, 1] = THR                          # equal to the threshold: kept
        if K == 5:
            m[0, 1], m[1, 2], m[0, 2] = 0.1, 0.1, 0.9          # the chain: 1 is dropped for 0, so 2 is kept
            m[0, 3], m[2, 3] = 0.25, 0.25          # a tie between the kept 0 and 2: the lowest index wins
            m[1, 3] = 0.01                         # the dropped 1 is nearer still and must not count
            m[0, 4], m[2, 4] = float('nan'), 0.7   # a NaN drops nothing
        if K >= 65:
            m = torch.rand(K, K, generator=gen) * 1.2 + 0.2          # about a quarter of the values under the threshold
            if K == 130:
                m[0, 1], m[:64, 64] = 2.0, 2.0         # 1 and 64 are kept ...
                m[1, K - 1], m[64, K - 1] = 0.05, 0.05 # ... and tie as the nearest of the last conformer, from two lanes and two strides: 1 wins
                m[3, 100] = float('nan')
        i, j = torch.triu_indices(K, K, 1)
        tris.append(m[i, j])
    return torch.cat(tris).float()


def prune_loop(d, sizes, thr):
    """The rule in ten lines of Python: (keep, rep) over the concatenated conformers."""
    keep, rep, m0, t0 = [], [], 0, 0
    for K in sizes:
        at = lambda j, i: float(d[t0 + j * (2 * K - j - 1) // 2 + (i - j - 1)])
        for i in range(K):
            cand = [(at(j, i), j) for j in range(i) if keep[m0 + j] and at(j, i) == at(j, i)]
            v, j = min(cand) if cand else (float('inf'), i)
            keep.append(not v < thr)
            rep.append(m0 + (j if v < thr else i))
        m0, t0 = m0 + K, t0 + K * (K - 1) // 2
    return torch.tensor(keep, dtype=torch.bool), torch.tensor(rep, dtype=torch.int64)


def _check_prune(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    d = prune_inputs()
    want_keep, want_rep = prune_loop(d, PRUNE_SIZES, THR)
    keep, rep = eng.prune_rmsd(d, PRUNE_SIZES, THR)
    eng.synchronize()
    assert torch.equal(keep.cpu(), want_keep) and torch.equal(rep.cpu(), want_rep)
    five = sum(PRUNE_SIZES[:3])
    assert want_keep[five:five + 5].tolist() == [True, False, True, False, True] and want_rep[five:five + 5].tolist() == [five, five, five + 2, five, five + 4]
    assert want_keep[1:3].tolist() == [True, True] and 0 < int(want_keep[8:].sum()) < 190
    # the raw call between guard bands
    M, G = sum(PRUNE_SIZES), len(PRUNE_SIZES)
    off = lambda v: torch.tensor([0] + torch.cumsum(torch.tensor(v), 0).tolist(), dtype=torch.int32)
    gs = GuardSet(eng.device)
    go, to = gs.inp('group_off', off(list(PRUNE_SIZES))), gs.inp('tri_off', off([K * (K - 1) // 2 for K in PRUNE_SIZES]))
    dd = gs.inp('d', d)
    kp, rp = gs.out('keep', (M,), torch.uint8), gs.out('rep', (M,), torch.int32)
    call = lambda a, b, c, k, r: eng.lib.fm_prune_rmsd(eng._ctx, eng._stream(), G, _ptr(a), _ptr(b), _ptr(c), THR, _ptr(k), _ptr(r))
    assert call(go, dd, to, kp, rp) == 0
    eng.synchronize()
    assert gs.check() == [] and gs.unwritten() == [], (gs.check(), gs.unwritten())
    assert torch.equal(kp.cpu() != 0, want_keep) and torch.equal(rp.cpu().long(), want_rep)
    assert call(go, dd, to, kp, go) == -1 and b'alias' in eng.lib.fm_last_error(eng._ctx)
    assert call(go, dd, to, None, rp) == -1
    with pytest.raises(ValueError, match='pairs'):
        eng.prune_rmsd(d[:-1], PRUNE_SIZES, THR)
    k0, r0 = eng.prune_rmsd(torch.zeros(0), [0, 0], THR)
    assert k0.shape == (0,) and r0.shape == (0,)
    k1, r1 = eng.prune_rmsd(d, PRUNE_SIZES, float('inf'))          # everything is nearer than inf, except a NaN: one survivor per group and the NaN's row
    eng.synchronize()
    assert torch.equal(k1.cpu(), prune_loop(d, PRUNE_SIZES, float('inf'))[0])


def test_prune_rmsd_equals_the_python_loop_on_emulation(emu_lib):
    _check_prune(emu_lib, 'cpu')


@pytest.mark.gpu
def test_prune_rmsd_equals_the_python_loop_on_gpu():
    _check_prune(None, 'cuda:0')
