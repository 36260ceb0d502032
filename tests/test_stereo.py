"""Stereo elements on the host and the stereo check on the device: flowmol_amd/stereo.py, fm_stereo / Engine.stereo (ABI 15).

PERCEPTION: hand-built token graphs with QM9 tokens (C 0, H 1, N 2, O 3, F 4), `GRAPHS`.

KERNEL INPUTS (float32, one fixed generator; `batch()`).  BASE is a 15-atom molecule with two tetrahedral centres and one double bond,
    F1, O2(H12), Ca3 and C8 on the centre C0;  Ca3(H5) = Cb4(F6)(H7);  C0, F9, N10(H13, H14) and H11 on the centre C8,
in a near-ideal geometry plus 0.05 noise; `stereo_elements` gives its three rows.  The molecules of the batch, each against the reference in brackets:
  a       BASE under a proper rotation and a translation [BASE]                                   match
  b       -BASE under a proper rotation and a translation [BASE]                                  mirror
  c       a with the positions of F9 and H11, two leaves of the centre C8, swapped [BASE]         1 tetra mismatch, neither flag
  d       a with the positions of F6 and H7, the substituents of Cb4, swapped [BASE]              1 double-bond mismatch
  e       BASE with C8 and its listed neighbours C0, F9, N10 at z = 0 [BASE]                      that value exactly 0: undefined, no match
  f       BASE with F1 on top of C0 [BASE]                                                        a zero-length bond: value 0, no NaN
  one     one atom, set -1;  free: a with set -1;  empty: a with a set of no rows                 no element: zeros and match
  cloud70 70 atoms, a Gaussian cloud shifted by 500, against a moved copy with 0.3 noise, 130 caller-made rows of both kinds: more rows and more atoms than
          lanes, so both strides wrap.  Rows are drawn until every value keeps its distance (below).
a .. f share one set.

REFERENCE, written here (`value`, `ref64`): the two formulas in float64 and the integer table from them.
DECIDABILITY: every float64 |value|, in x and in x_ref, is exactly 0 by construction (`ZERO`) or farther than 1e-3 from both 0 and flat_tol -- asserted
for every element in `test_every_value_is_decidable`; the float32 error is 1e-6 at most, so every integer of the table is then determined.
TOLERANCE of the values (derived as in tests/test_pair_rmsd.py, not tuned): `value(..., torch.float32)` restates the formulas in float32; its largest error
against float64 over a molecule's rows, measured once on the host (`f32_errors()`; recorded in DESIGN_LOG.md, 2026-10, "stereo check"), is F32_ERR.  The kernel
gets 8x that: it may order the normalisation differently.
Every device check runs on the CPU emulation and, marked gpu, on the device."""
import math

import pytest
import torch

from flowmol_amd.engine import _ptr
from flowmol_amd.stereo import stereo_elements
import hygiene_util as hu
from hygiene_util import GuardSet

import mixed_util as mu
from test_pair_rmsd import _rotation

C_, H_, N_, O_, F_ = 0, 1, 2, 3, 4
FAKE, MASK = 5, 4          # the qm9 preset: five atom types and the fake atom; bond orders 0..3 and the mask token
TOL = 0.05


# ------------------------------------------------------------------------------------------------------------------ graphs
def graph(atoms, bonds, hydrogens=()):
    """(a, c, e_upper, bonds) of the atoms (tokens) and bonds {(i, j): order}; ``hydrogens``: how many H to hang on each atom, appended in atom order."""
    atoms, bonds = list(atoms), dict(bonds)
    for v, k in enumerate(hydrogens):
        for _ in range(k):
            bonds[(v, len(atoms))] = 1
            atoms.append(H_)
    n = len(atoms)
    full = {}
    for (i, j), o in bonds.items():
        full[(min(i, j), max(i, j))] = o
    e = torch.tensor([full.get((i, j), 0) for i in range(n) for j in range(i + 1, n)], dtype=torch.int64)
    return torch.tensor(atoms), torch.ones(n, dtype=torch.int64), e, full


def ring(n, double=()):
    return {(i, (i + 1) % n): (2 if i in double else 1) for i in range(n)}


BASE_ATOMS = [C_, F_, O_, C_, C_, H_, F_, H_, C_, F_, N_, H_, H_, H_, H_]
BASE_BONDS = {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 8): 1, (3, 4): 2, (3, 5): 1, (4, 6): 1, (4, 7): 1, (8, 9): 1, (8, 10): 1, (8, 11): 1, (2, 12): 1, (10, 13): 1,
              (10, 14): 1}
BASE_ROWS = [[0, 0, 1, 2, 3], [0, 8, 0, 9, 10], [1, 0, 3, 4, 6]]

GRAPHS = {
    # C(F)(OH)(NH2)H: C0 F1 O2 N3, then H on C, on O, two on N
    'cfonh': (graph([C_, F_, O_, N_], {(0, 1): 1, (0, 2): 1, (0, 3): 1}, [1, 0, 1, 2]), [[0, 0, 1, 2, 3]]),
    'propane': (graph([C_, C_, C_], {(0, 1): 1, (1, 2): 1}, [3, 2, 3]), []),
    'but-2-ene': (graph([C_] * 4, {(0, 1): 1, (1, 2): 2, (2, 3): 1}, [3, 1, 1, 3]), [[1, 0, 1, 2, 3]]),
    'propene': (graph([C_] * 3, {(0, 1): 1, (1, 2): 2}, [3, 1, 2]), []),
    'cyclohexene': (graph([C_] * 6, ring(6, [0]), [1, 1, 2, 2, 2, 2]), []),
    'benzene': (graph([C_] * 6, ring(6, [0, 2, 4]), [1] * 6), []),
    'allene': (graph([C_] * 5, {(0, 1): 1, (1, 2): 2, (2, 3): 2, (3, 4): 1}, [3, 1, 0, 1, 3]), []),
    'cyclodecene': (graph([C_] * 10, ring(10, [0]), [1, 1] + [2] * 8), [[1, 9, 0, 1, 2]]),
    'cyclooctene': (graph([C_] * 8, ring(8, [0]), [1, 1] + [2] * 6), []),          # a ring of exactly max_ring atoms is still excluded
    'base': (graph(BASE_ATOMS, BASE_BONDS), BASE_ROWS),
}


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_stereo_elements_of_hand_built_graphs(name):
    (a, c, e, _), want = GRAPHS[name]
    got = stereo_elements(a, c, e, mask_token=MASK, fake_token=FAKE)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(want), 5) and got.tolist() == want


def test_max_ring_is_the_ring_size_that_still_fixes_a_double_bond():
    a, c, e, _ = GRAPHS['cyclooctene'][0]
    assert stereo_elements(a, c, e, max_ring=7).tolist() == [[1, 7, 0, 1, 2]]
    a, c, e, _ = GRAPHS['cyclodecene'][0]
    assert stereo_elements(a, c, e, max_ring=10).tolist() == []


def test_charge_tokens_distinguish_substituents():
    """C(NH3+)(NH2)(F)H-like: two nitrogens that differ in their charge token only are different substituents; with equal tokens the centre is none."""
    a, c, e, _ = graph([C_, N_, N_, F_, H_], {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1})
    assert stereo_elements(a, c, e).tolist() == []
    c2 = c.clone()
    c2[1] = 3
    assert stereo_elements(a, c2, e).tolist() == [[0, 0, 1, 2, 3]]


def test_fake_atoms_and_mask_token_pairs_are_ignored():
    (a, c, e, bonds), want = GRAPHS['cfonh']
    n = a.shape[0]
    bonds = dict(bonds)
    bonds[(0, n)] = 1          # a fake atom 'bonded' to the centre: a fifth neighbour if it were counted
    bonds[(0, 5)] = MASK       # the mask token between the centre and the hydroxyl hydrogen: another one
    atoms = a.tolist() + [FAKE]
    e2 = torch.tensor([bonds.get((i, j), 0) for i in range(n + 1) for j in range(i + 1, n + 1)])
    got = stereo_elements(torch.tensor(atoms), torch.ones(n + 1, dtype=torch.int64), e2, mask_token=MASK, fake_token=FAKE)
    assert got.tolist() == want
    assert stereo_elements(torch.tensor(atoms), torch.ones(n + 1, dtype=torch.int64), e2).tolist() == []          # without the two tokens named, both count


def test_a_relabelled_graph_gives_the_relabelled_rows():
    (a, c, e, bonds), rows = GRAPHS['base']
    n = a.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).tolist()          # old atom i becomes perm[i]
    assert perm != list(range(n))
    a2 = torch.empty_like(a)
    a2[torch.tensor(perm)] = a
    bonds2 = {(perm[i], perm[j]): o for (i, j), o in bonds.items()}
    _, _, e2, _ = graph(a2.tolist(), bonds2)
    nbrs = lambda v: [j if i == v else i for (i, j) in bonds if v in (i, j)]
    want = []
    for kind, i0, i1, i2, i3 in rows:
        if kind == 0:
            want.append([0, perm[i0]] + sorted(perm[u] for u in nbrs(i0))[:3])
        else:
            ends = sorted((perm[v], min(perm[u] for u in nbrs(v) if u != w)) for v, w in ((i1, i2), (i2, i1)))
            want.append([1, ends[0][1], ends[0][0], ends[1][0], ends[1][1]])
    assert stereo_elements(a2, c, e2, mask_token=MASK, fake_token=FAKE).tolist() == sorted(want)


# ------------------------------------------------------------------------------------------------------------------ geometry
def _tetra(centre, toward, lengths, twist):
    """Three positions around ``centre`` that complete a tetrahedron whose fourth bond points at ``toward``."""
    d = (toward - centre) / (toward - centre).norm()
    h = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    e1 = h - (h @ d) * d
    e1 = e1 / e1.norm()
    e2 = torch.linalg.cross(d, e1)
    out = []
    for k, l in enumerate(lengths):
        ph = twist + 2 * math.pi * k / 3
        out.append(centre + l * (-d / 3 + math.sqrt(8.0) / 3 * (math.cos(ph) * e1 + math.sin(ph) * e2)))
    return out


def base_geometry(gen):
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    x = torch.zeros(15, 3, dtype=torch.float64)
    c60, s60 = 0.5, math.sqrt(3.0) / 2
    x[3], x[4] = t(0, 0, 0), t(1.34, 0, 0)                                # Ca = Cb in the xy plane
    x[0], x[5] = 1.5 * t(-c60, s60, 0), 1.09 * t(-c60, -s60, 0)           # C0 and H5 on Ca
    x[6], x[7] = x[4] + 1.35 * t(c60, s60, 0), x[4] + 1.09 * t(c60, -s60, 0)      # F6 (cis to C0) and H7 on Cb
    x[1], x[2], x[8] = _tetra(x[0], x[3], [1.35, 1.43, 1.54], 0.4)
    x[9], x[10], x[11] = _tetra(x[8], x[0], [1.35, 1.47, 1.09], 1.1)
    x[12] = x[2] + 0.96 * t(0.5, 0.3, 0.81)
    x[13], x[14] = x[10] + 1.01 * t(0.7, -0.6, 0.39), x[10] + 1.01 * t(-0.5, -0.2, 0.84)
    return x + 0.05 * torch.randn(15, 3, generator=gen, dtype=torch.float64)


_BATCH = {}
NAMES = ('a', 'b', 'one', 'c', 'd', 'free', 'e', 'empty', 'f', 'cloud70')
ZERO = {('e', 1), ('f', 0)}          # (molecule, row) whose value in x is exactly 0 by construction


def batch():
    """{name: {'x', 'ref' (n,3) float32, 'rows' (Q,5) int64 or None for set -1}} in the order NAMES, built once."""
    if _BATCH:
        return _BATCH
    gen = torch.Generator().manual_seed(2215)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    move = lambda x: x @ _rotation(gen).T + rnd(1, 3) * 2.0
    base = base_geometry(gen)
    rows = torch.tensor(BASE_ROWS)

    def swapped(x, i, j):
        y = x.clone()
        y[i], y[j] = x[j], x[i]
        return y
    a = move(base)
    flat = base.clone()
    flat[[8, 0, 9, 10], 2] = 0.0
    on_top = base.clone()
    on_top[1] = on_top[0]
    mols = {'a': (a, base, rows), 'b': (move(-base), base, rows), 'c': (swapped(a, 9, 11), base, rows), 'd': (swapped(a, 6, 7), base, rows),
            'e': (flat, base, rows), 'f': (on_top, base, rows), 'one': (rnd(1, 3), rnd(1, 3), None), 'free': (a, base, None),
            'empty': (a, base, torch.zeros(0, 5, dtype=torch.int64))}
    cloud = rnd(70, 3) * 1.8 + 500.0
    cref = move(cloud - 500.0) + 0.3 * rnd(70, 3) + 500.0
    cx, cr = cloud.float(), cref.float()
    crow = []
    while len(crow) < 130:          # rows whose value keeps its distance from 0 and from the tolerance in both coordinate sets
        r = [len(crow) % 2] + torch.randperm(70, generator=gen)[:4].tolist()
        if len(crow) < 20:
            r[1] = 64 + int(torch.randint(6, (1,), generator=gen))          # atoms beyond the first 64 for certain
        if len(set(r[1:])) == 4 and all(min(abs(abs(float(value(v, r, torch.float64))) - t) for t in (0.0, TOL)) > 2e-3 for v in (cx, cr)):
            crow.append(r)
    mols['cloud70'] = (cloud, cref, torch.tensor(crow))
    for k in NAMES:
        x, ref, r = mols[k]
        _BATCH[k] = {'x': x.float(), 'ref': ref.float(), 'rows': r}
    return _BATCH


# ------------------------------------------------------------------------------------------------------------------ the reference
def value(x, row, dtype):
    """The value of one element row in the coordinates ``x``, every operation in ``dtype``; a zero length gives 0."""
    kind, i0, i1, i2, i3 = [int(v) for v in row]
    p = x.to(dtype)
    zero = torch.zeros((), dtype=dtype)

    def unit(v):
        l = (v * v).sum().sqrt()
        return None if float(l) == 0.0 else v / l
    if kind == 0:
        u = [unit(p[j] - p[i0]) for j in (i1, i2, i3)]
        return zero if any(v is None for v in u) else (torch.linalg.cross(u[0], u[1]) * u[2]).sum()
    b1, b2, b3 = p[i1] - p[i0], p[i2] - p[i1], p[i3] - p[i2]
    n1, n2 = unit(torch.linalg.cross(b1, b2)), unit(torch.linalg.cross(b2, b3))
    return zero if n1 is None or n2 is None else (n1 * n2).sum()


_REF = {}


def ref64():
    """{name: (values of x, values of ref, both float64 lists, the 8 integers)}."""
    if not _REF:
        for name, m in batch().items():
            rows = [] if m['rows'] is None else m['rows'].tolist()
            va, vb = [float(value(m['x'], r, torch.float64)) for r in rows], [float(value(m['ref'], r, torch.float64)) for r in rows]
            cnt = [0] * 6
            for r, p, q in zip(rows, va, vb):
                both = abs(p) >= TOL and abs(q) >= TOL
                cnt[3 * r[0]] += 1
                cnt[3 * r[0] + 1] += both
                cnt[3 * r[0] + 2] += both and (p < 0) != (q < 0)
            defined = cnt[1] == cnt[0] and cnt[4] == cnt[3]
            match = defined and cnt[2] == 0 and cnt[5] == 0
            mirror = cnt[0] > 0 and defined and cnt[2] == cnt[0] and cnt[5] == 0
            _REF[name] = (va, vb, cnt + [int(match), int(mirror)])
    return _REF


def f32_errors():
    """The measurement behind F32_ERR: per molecule, the largest |float32 restatement - float64| over its rows."""
    out = {}
    for name, m in batch().items():
        rows = [] if m['rows'] is None else m['rows'].tolist()
        out[name] = max([abs(float(value(m['x'], r, torch.float32)) - float(value(m['x'], r, torch.float64))) for r in rows], default=0.0)
    return out


F32_ERR = {'a': 7.05e-08, 'b': 1.40e-07, 'c': 7.05e-08, 'd': 7.05e-08, 'e': 6.16e-08, 'f': 2.73e-08, 'one': 0.0, 'free': 0.0, 'empty': 0.0, 'cloud70': 1.53e-07}


def test_every_value_is_decidable():
    """No element exempted: exactly 0 where the construction says so, else farther than 1e-3 from 0 and from flat_tol, in x and in the reference."""
    ref = ref64()
    for name in NAMES:
        va, vb, _ = ref[name]
        for q, (p, r) in enumerate(zip(va, vb)):
            if (name, q) in ZERO:
                assert p == 0.0, (name, q, p)
            else:
                assert min(abs(abs(p) - 0.0), abs(abs(p) - TOL)) > 1e-3, (name, q, p)
            assert min(abs(abs(r) - 0.0), abs(abs(r) - TOL)) > 1e-3, (name, q, r)
    assert set(F32_ERR) == set(NAMES)
    assert sum(r[1] >= 64 or r[2] >= 64 for r in batch()['cloud70']['rows'].tolist()) > 10 and batch()['cloud70']['rows'].shape[0] == 130


def test_the_cases_are_what_they_claim_in_the_reference():
    ref = ref64()
    want = {'a': [2, 2, 0, 1, 1, 0, 1, 0], 'b': [2, 2, 2, 1, 1, 0, 0, 1], 'c': [2, 2, 1, 1, 1, 0, 0, 0], 'd': [2, 2, 0, 1, 1, 1, 0, 0],
            'e': [2, 1, 0, 1, 1, 0, 0, 0], 'f': [2, 1, 0, 1, 1, 0, 0, 0], 'one': [0] * 6 + [1, 0], 'free': [0] * 6 + [1, 0], 'empty': [0] * 6 + [1, 0]}
    for k, w in want.items():
        assert ref[k][2] == w, (k, ref[k][2])
    t = ref['cloud70'][2]
    assert t[0] == 65 and t[3] == 65 and 0 < t[2] < t[1] and 0 < t[5] < t[4]          # both kinds, matches and mismatches among the defined ones


# ------------------------------------------------------------------------------------------------------------------ the batch on the device
def layout(names=NAMES, permute_rows=False):
    """-> (sizes, x, x_ref, (elem_set, [rows])): a .. f share one set."""
    B = batch()
    sets, elem_set, shared = [], [], None
    gen = torch.Generator().manual_seed(8)
    for k in names:
        r = B[k]['rows']
        if r is None:
            elem_set.append(-1)
        elif k in tuple('abcdef'):
            if shared is None:
                sets.append(r[torch.randperm(r.shape[0], generator=gen)] if permute_rows else r)
                shared = len(sets) - 1
            elem_set.append(shared)
        else:
            sets.append(r[torch.randperm(r.shape[0], generator=gen)] if permute_rows and r.shape[0] else r)
            elem_set.append(len(sets) - 1)
    return ([B[k]['x'].shape[0] for k in names], torch.cat([B[k]['x'] for k in names]), torch.cat([B[k]['ref'] for k in names]),
            (torch.tensor(elem_set, dtype=torch.int32), sets))


def run(eng, names=NAMES, permute_rows=False, flat_tol=TOL):
    """One Engine.stereo call -> (out (B,8), [values per molecule], x_out, the sets) on the cpu."""
    sizes, x, xr, sets = layout(names, permute_rows)
    eng.bind(torch.tensor(sizes))
    out, (vals, off), xo = eng.stereo(x, xr, sets, flat_tol, values=True, fixed=True)
    eng.synchronize()
    vals = vals.cpu()
    return out.cpu(), [vals[int(off[m]):int(off[m + 1])] for m in range(len(sizes))], xo.cpu(), sets


_RESULTS = {}


def results(lib, device):
    key = (id(lib), str(device))
    if key not in _RESULTS:
        _RESULTS[key] = run(mu.engine('qm9', lib, device)[0])
    return _RESULTS[key]


def _check_against_reference(lib, device):
    out, vals, xo, _ = results(lib, device)
    ref, B, bad = ref64(), batch(), []
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(NAMES), 8)
    for m, name in enumerate(NAMES):
        assert out[m].tolist() == ref[name][2], (name, out[m].tolist(), ref[name][2])
        assert vals[m].shape[0] == len(ref[name][0]) and not bool(torch.isnan(vals[m]).any()), name
        for q, (got, want) in enumerate(zip(vals[m].tolist(), ref[name][0])):
            err = abs(got - want)
            print(f'{name}[{q}]: {got:+.7f} against {want:+.7f}, error {err:.3g} (bound {8 * F32_ERR[name]:.3g})')
            if (name, q) in ZERO:
                assert got == 0.0 and math.copysign(1.0, got) == 1.0, (name, q, got)
            if not err <= 8 * F32_ERR[name]:
                bad.append((name, q, err, 8 * F32_ERR[name]))
    assert bad == [], bad
    assert not bool(torch.isnan(xo).any())
    for name, piece in zip(NAMES, torch.split(xo, [B[k]['x'].shape[0] for k in NAMES])):
        assert torch.equal(piece, -B[name]['x'] if ref[name][2][7] else B[name]['x']), name
    assert ref['b'][2][7] == 1


def test_stereo_against_the_float64_oracle_on_emulation(emu_lib):
    _check_against_reference(emu_lib, 'cpu')


@pytest.mark.gpu
def test_stereo_against_the_float64_oracle_on_gpu():
    _check_against_reference(None, 'cuda:0')


def _check_canonical(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    out, vals, xo, _ = results(lib, device)
    B = batch()
    x_parts = torch.split(xo, [B[k]['x'].shape[0] for k in NAMES])
    for m, name in enumerate(NAMES):          # each molecule alone: the bits it gives inside the batch
        o1, v1, x1, _ = run(eng, (name,))
        assert torch.equal(o1[0], out[m]) and torch.equal(v1[0], vals[m]) and torch.equal(x1, x_parts[m]), name
    o2, v2, x2, _ = run(eng, NAMES[::-1])          # the batch reversed
    assert torch.equal(o2.flip(0), out) and all(torch.equal(p, q) for p, q in zip(v2[::-1], vals))
    # a set's rows permuted: only the order of the values changes
    o3, v3, x3, (_, sets3) = run(eng, permute_rows=True)
    sets = layout()[3][1]
    assert torch.equal(o3, out) and torch.equal(x3, xo)
    seen = 0
    for m, name in enumerate(NAMES):
        s = int(layout()[3][0][m])
        if s < 0 or not sets[s].shape[0]:
            continue
        old, new = sets[s].tolist(), sets3[s].tolist()
        assert sorted(old) == sorted(new)
        seen += old != new
        assert torch.equal(v3[m], vals[m][torch.tensor([old.index(r) for r in new])]), name
    assert seen >= 1
    # fixed applied twice returns the input: the mirror image, inverted, is a match, and inverting back needs the inverted reference
    mb = NAMES.index('b')
    eng.bind(torch.tensor([15]))
    rows = (torch.zeros(1, dtype=torch.int32), [B['b']['rows']])
    t1, once = eng.stereo(B['b']['x'], B['b']['ref'], rows, TOL, fixed=True)
    t2, same = eng.stereo(once, B['b']['ref'], rows, TOL, fixed=True)
    t3, twice = eng.stereo(once, -B['b']['ref'], rows, TOL, fixed=True)
    eng.synchronize()
    assert t1.cpu()[0].tolist() == out[mb].tolist() and torch.equal(once.cpu(), -B['b']['x'])
    assert t2.cpu()[0, 6:].tolist() == [1, 0] and torch.equal(same.cpu(), once.cpu())
    assert t3.cpu()[0, 6:].tolist() == [0, 1] and torch.equal(twice.cpu(), B['b']['x'])
    # flat_tol moves the line between defined and flat, nothing else
    va = ref64()['a'][0]
    big = min(abs(v) for v in va + ref64()['a'][1]) + 0.01
    o4 = run(eng, ('a',), flat_tol=big)[0]
    assert o4[0].tolist()[6:] == [0, 0] and o4[0, 1] + o4[0, 4] < 3
    o5 = run(eng, ('e', 'f'), flat_tol=0.0)[0]          # with a tolerance of 0 everything is defined and a value of +0 counts as positive
    assert o5[:, [1, 4]].tolist() == [[2, 1], [2, 1]]


def test_alone_reversed_and_permuted_on_emulation(emu_lib):
    _check_canonical(emu_lib, 'cpu')


@pytest.mark.gpu
def test_alone_reversed_and_permuted_on_gpu():
    _check_canonical(None, 'cuda:0')


# ------------------------------------------------------------------------------------------------------------------ hygiene and refusals
def _check_hygiene(lib, device):
    eng = hu.engine('qm9', lib, device, fresh=True)[0]
    err = lambda: eng.lib.fm_last_error(eng._ctx)
    sizes, x0, r0, (elem_set, sets) = layout()
    M, N = len(sizes), sum(sizes)
    per_set = [s.shape[0] for s in sets]
    set_off = torch.tensor([0] + torch.cumsum(torch.tensor(per_set), 0).tolist(), dtype=torch.int32)
    n_rows = [per_set[s] if s >= 0 else 0 for s in elem_set.tolist()]
    val_off = torch.tensor([0] + torch.cumsum(torch.tensor(n_rows), 0).tolist(), dtype=torch.int32)
    gs = GuardSet(eng.device)
    x, xr = gs.inp('x', x0), gs.inp('x_ref', r0)
    es, so, el = gs.inp('elem_set', elem_set), gs.inp('set_off', set_off), gs.inp('elems', torch.cat([s.reshape(-1) for s in sets]).to(torch.int32))
    vo = gs.inp('val_off', val_off)
    out, vals, xo = gs.out('out', (M, 8), torch.int32), gs.out('values', (int(val_off[-1]),)), gs.out('x_out', (N, 3))
    call = lambda x_, r_, a, b, c, ns, tol, o, v_off, v, f: eng.lib.fm_stereo(eng._ctx, eng._stream(), _ptr(x_), _ptr(r_), _ptr(a), _ptr(b), _ptr(c), ns, tol,
                                                                           _ptr(o), _ptr(v_off), _ptr(v), _ptr(f))
    ok = (x, xr, es, so, el, len(sets), TOL, out, vo, vals, xo)
    assert call(*ok) == -1 and b'no batch bound' in err(), err()          # a fresh engine: nothing bound yet
    ws, guards_intact = hu.arena(eng, [sizes], 'ones')                    # every float32 of the workspace a NaN, filled before the bind
    eng.bind(torch.tensor(sizes), workspace=ws)
    assert call(*ok) == 0
    eng.synchronize()
    assert gs.check() == [] and gs.unwritten() == [] and guards_intact(), (gs.check(), gs.unwritten())
    want_out, want_vals, want_xo, _ = results(lib, device)
    assert torch.equal(out.cpu(), want_out) and torch.equal(vals.cpu(), torch.cat(want_vals)) and torch.equal(xo.cpu(), want_xo)
    # without the optional outputs, and without a table, the call writes out alone
    gs2 = GuardSet(eng.device)
    out2, out3 = gs2.out('out', (M, 8), torch.int32), gs2.out('out.no-table', (M, 8), torch.int32)
    assert call(x, xr, es, so, el, len(sets), TOL, out2, None, None, None) == 0 and call(x, xr, None, None, None, 0, TOL, out3, None, None, None) == 0
    eng.synchronize()
    assert gs2.check() == [] and gs.check() == [] and torch.equal(out2.cpu(), out.cpu())
    assert out3.cpu().tolist() == [[0] * 6 + [1, 0]] * M
    before = (out.cpu().clone(), vals.cpu().clone(), xo.cpu().clone())
    swap = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for args in (swap(7, x), swap(9, xr), swap(10, x), swap(7, el), swap(10, so), swap(9, vo)):
        assert call(*args) == -1 and b'aliases an input' in err(), err()
    for args in (swap(10, vals), swap(9, xo)):
        assert call(*args) == -1 and b'another output' in err(), err()
    assert call(*swap(8, None)) == -1 and b'without val_off' in err(), err()
    for args in (swap(2, None), swap(3, None), swap(4, None), swap(5, 0)):
        assert call(*args) == -1 and b'come together' in err(), err()
    assert call(x, xr, None, None, None, 2, TOL, out, vo, vals, xo) == -1 and b'without an element table' in err(), err()
    for tol in (-0.01, float('nan')):
        assert call(*swap(6, tol)) == -1 and b'flat_tol' in err(), err()
    assert call(*swap(0, None)) == -1 and call(*swap(1, None)) == -1 and call(*swap(7, None)) == -1
    eng.synchronize()
    assert gs.check() == [] and all(torch.equal(a, b) for a, b in zip((out.cpu(), vals.cpu(), xo.cpu()), before))          # a refused call enqueues nothing
    # Engine.stereo: what it refuses before the call
    only = lambda r: (torch.tensor([0 if k == 0 else -1 for k in range(M)]), [torch.tensor(r)])
    with pytest.raises(ValueError, match='index outside'):
        eng.stereo(x0, r0, only([[0, 0, 1, 2, 15]]))
    with pytest.raises(ValueError, match='index outside'):
        eng.stereo(x0, r0, only([[0, -1, 1, 2, 3]]))
    with pytest.raises(ValueError, match='index outside'):          # the set named by the one-atom molecule too
        eng.stereo(x0, r0, (torch.tensor([0 if NAMES[k] in ('a', 'one') else -1 for k in range(M)]), [torch.tensor([[0, 0, 1, 2, 3]])]))
    with pytest.raises(ValueError, match='twice'):
        eng.stereo(x0, r0, only([[1, 0, 3, 4, 3]]))
    with pytest.raises(ValueError, match='kind'):
        eng.stereo(x0, r0, only([[2, 0, 1, 2, 3]]))
    with pytest.raises(ValueError, match=r'\(rows, 5\)'):
        eng.stereo(x0, r0, only([[0, 1, 2, 3]]))
    with pytest.raises(ValueError, match='set id'):
        eng.stereo(x0, r0, (torch.tensor([1] + [-1] * (M - 1)), [torch.tensor(BASE_ROWS)]))
    with pytest.raises(ValueError, match='flat_tol'):
        eng.stereo(x0, r0, None, flat_tol=-1.0)
    with pytest.raises(ValueError, match='flat_tol'):
        eng.stereo(x0, r0, None, flat_tol=float('nan'))
    with pytest.raises(ValueError, match='bound batch'):
        eng.stereo(x0[:-1], r0, None)
    none = eng.stereo(x0, r0, None)
    eng.synchronize()
    assert none.cpu().tolist() == [[0] * 6 + [1, 0]] * M


def test_stereo_between_guard_bands_and_refusals_on_emulation(emu_lib):
    _check_hygiene(emu_lib, 'cpu')


@pytest.mark.gpu
def test_stereo_between_guard_bands_and_refusals_on_gpu():
    _check_hygiene(None, 'cuda:0')
