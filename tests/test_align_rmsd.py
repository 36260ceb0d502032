"""Aligned RMSD on the device: fm_align_rmsd, Engine.align_rmsd, FlowMol.rmsd.

The reference is written here: a float64 torch Kabsch with the determinant correction (the optimal PROPER rotation; molecule.rigid_alignment has no
correction and may reflect).  Inputs (float32, the reference reads the same float32 values):
  cloud    a 47-atom Gaussian cloud against itself rotated, translated and perturbed by 0.1
  rigid    the same cloud against an exact rigid copy (rmsd ~ 0: the case a residual sum must survive and Ga + Gb - 2 lambda does not)
  one, two 1 and 2 atoms;  line: 5 collinear atoms (a degenerate top eigenspace)
  ring     a planar 6-ring whose atoms are pushed out of the plane, against its mirror image through that plane: chiral, so the proper-rotation answer is not
           zero while the determinant-free alignment reflects it onto itself -- asserted on the two references
  select   the cloud with every third atom dropped from the fit (the dropped atoms of xb displaced by 3: they must not enter) -- they move with the fitted transform
  far      both clouds shifted by 500

TOLERANCE (derived, not tuned).  `reference(..., torch.float32)` restates the reference in float32 -- centring, SVD, residuals.  Its error against float64 on
these inputs, measured once on the host and recorded in DESIGN_LOG.md (2026-10, "aligned RMSD on the device"), is F32_ERR below per input and output: 'c' the
centred rmsd, 'r' the aligned rmsd, 'x' the largest coordinate error of the aligned atoms.  The kernel gets 8x that (a different eigen-solver with a fixed
sweep count): BOUND = 8 * F32_ERR.  Every check runs on the CPU emulation and, marked gpu, on the device."""
import ctypes as C
import math

import pytest
import torch

from flowmol_amd.engine import _ptr
from flowmol_amd.molecule import rigid_alignment
from hygiene_util import GuardSet

import mixed_util as mu
import resample_util as ru

NAMES = ('cloud', 'rigid', 'one', 'two', 'line', 'ring', 'select', 'far')
BATCH5 = ('cloud', 'one', 'two', 'line', 'ring')          # the 5-molecule batch of the canonical-arithmetic check

# |float32 restatement - float64 reference| on the inputs below: (centred rmsd, aligned rmsd, aligned coordinates); measured, see the module docstring
F32_ERR = {
    'cloud': (1.39e-07, 4.82e-09, 1.10e-06),
    'rigid': (1.81e-07, 4.69e-07, 8.94e-07),
    'one': (0.0, 0.0, 0.0),
    'two': (1.01e-07, 2.42e-08, 1.98e-07),
    'line': (7.87e-08, 1.16e-07, 3.09e-07),
    'ring': (5.00e-08, 7.89e-08, 4.10e-07),
    'select': (8.92e-08, 7.16e-08, 1.01e-06),
    'far': (7.92e-08, 3.64e-08, 6.77e-05),
}
BOUND = {k: tuple(8.0 * e for e in v) for k, v in F32_ERR.items()}


def _rotation(gen):
    q = torch.randn(4, generator=gen, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def inputs():
    """{name: (xa, xb, select or None)} in float32, from one fixed generator."""
    gen = torch.Generator().manual_seed(4711)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    move = lambda x: x @ _rotation(gen).T + rnd(1, 3) * 2.0
    cloud = rnd(47, 3) * 1.5
    out = {'cloud': (cloud, move(cloud) + 0.1 * rnd(47, 3), None), 'rigid': (cloud, move(cloud), None)}
    out['one'] = (rnd(1, 3), rnd(1, 3), None)
    two = rnd(2, 3)
    out['two'] = (two, move(two) + 0.1 * rnd(2, 3), None)
    line = torch.tensor([-2.0, -0.7, 0.1, 1.2, 2.5], dtype=torch.float64)[:, None] * torch.tensor([[0.6, -0.3, 0.74]], dtype=torch.float64)
    out['line'] = (line, move(line) + 0.05 * rnd(5, 3), None)
    ang = torch.arange(6, dtype=torch.float64) * (math.pi / 3)
    rad = torch.tensor([1.4, 1.1, 1.5, 1.2, 1.45, 1.0], dtype=torch.float64)
    ring = torch.stack([rad * ang.cos(), rad * ang.sin(), torch.tensor([0.3, -0.2, 0.25, 0.1, -0.35, 0.15], dtype=torch.float64)], dim=1)
    out['ring'] = (ring, move(ring * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)), None)
    sel = torch.tensor([i % 3 != 1 for i in range(47)])
    xb = move(cloud) + 0.1 * rnd(47, 3)
    xb[~sel] += 3.0
    out['select'] = (cloud, xb, sel)
    out['far'] = (cloud + 500.0, move(cloud) + 0.1 * rnd(47, 3) + 500.0, None)
    return {k: (a.float(), b.float(), s) for k, (a, b, s) in out.items()}


def reference(xa, xb, sel, dtype, proper=True):
    """Kabsch in ``dtype``: (centred rmsd, aligned rmsd, all atoms of xa under the fitted transform).  proper: R = V diag(1, 1, det) U^T."""
    a, b = xa.to(dtype), xb.to(dtype)
    s = torch.ones(a.shape[0], dtype=torch.bool) if sel is None else sel
    ma, mb = a[s].mean(0, keepdim=True), b[s].mean(0, keepdim=True)
    ac, bc = a - ma, b - mb
    U, _, Vh = torch.linalg.svd(ac[s].T @ bc[s])
    D = torch.eye(3, dtype=dtype)
    if proper:
        D[2, 2] = torch.sign(torch.linalg.det(Vh.T @ U.T))
    R = Vh.T @ D @ U.T
    moved = ac @ R.T
    rms = lambda d: (d[s] ** 2).sum(1).mean().sqrt()
    return float(rms(ac - bc)), float(rms(moved - bc)), moved + mb


def f32_errors():
    """The measurement behind F32_ERR."""
    out = {}
    for name, (xa, xb, sel) in inputs().items():
        c64, r64, x64 = reference(xa, xb, sel, torch.float64)
        c32, r32, x32 = reference(xa, xb, sel, torch.float32)
        out[name] = (abs(c32 - c64), abs(r32 - r64), float((x32.double() - x64).abs().max()))
    return out


def run(eng, names, aligned=True):
    """One Engine.align_rmsd call on the molecules ``names`` -> {name: (out row (4,), its aligned rows)} on the cpu."""
    inp = inputs()
    sizes = [inp[n][0].shape[0] for n in names]
    eng.bind(torch.tensor(sizes))
    xa, xb = torch.cat([inp[n][0] for n in names]), torch.cat([inp[n][1] for n in names])
    use_sel = any(inp[n][2] is not None for n in names)
    sel = torch.cat([inp[n][2] if inp[n][2] is not None else torch.ones(k, dtype=torch.bool) for n, k in zip(names, sizes)]) if use_sel else None
    out, moved = eng.align_rmsd(xa, xb, sel, aligned=True)
    eng.synchronize()
    return {n: (o, m) for n, o, m in zip(names, out.cpu(), torch.split(moved.cpu(), sizes))}


def errors(eng):
    """{name: (centred, aligned, coordinates)}: the kernel's distance from the float64 reference, the molecules in one batch without ``select`` and one with."""
    inp, got = inputs(), {}
    got.update(run(eng, [n for n in NAMES if inp[n][2] is None]))
    got.update(run(eng, ['select', 'ring', 'one']))          # a batch with a select array: its other molecules are fully selected
    res = {}
    for name in NAMES:
        xa, xb, sel = inp[name]
        c64, r64, x64 = reference(xa, xb, sel, torch.float64)
        o, m = got[name]
        assert float(o[0]) == (xa.shape[0] if sel is None else int(sel.sum())) and float(o[3]) == 0.0, name
        res[name] = (abs(float(o[1]) - c64), abs(float(o[2]) - r64), float((m.double() - x64).abs().max()))
    return res


def _check_against_reference(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    err = errors(eng)
    print({k: tuple(f'{e:.3g}' for e in v) for k, v in err.items()})
    print({k: tuple(f'{e:.3g}' for e in v) for k, v in BOUND.items()})
    bad = [(name, 'crx'[i], err[name][i], BOUND[name][i]) for name in NAMES for i in range(3) if not err[name][i] <= BOUND[name][i]]
    assert bad == [], bad


def test_the_references_differ_on_the_mirrored_ring():
    xa, xb, _ = inputs()['ring']
    _, proper, _ = reference(xa, xb, None, torch.float64)
    _, free, _ = reference(xa, xb, None, torch.float64, proper=False)
    centre = lambda x: x - x.mean(0, keepdim=True)          # rigid_alignment's translation is the reference's own: compare the rotated shapes
    lib_free = float(((centre(rigid_alignment(xa.double(), xb.double())) - centre(xb.double())) ** 2).sum(1).mean().sqrt())
    assert free < 1e-6 and lib_free < 1e-6 and proper > 0.1, (free, lib_free, proper)          # a reflection fits the mirror image; no rotation does
    _, rigid, _ = reference(*inputs()['rigid'][:2], None, torch.float64)
    assert rigid < 1e-6


def test_align_rmsd_against_float64_kabsch_on_emulation(emu_lib):
    _check_against_reference(emu_lib, 'cpu')


@pytest.mark.gpu
def test_align_rmsd_against_float64_kabsch_on_gpu():
    _check_against_reference(None, 'cuda:0')


def _check_canonical(lib, device):
    """A molecule alone and inside the 5-molecule batch: the same bits, in the numbers and in the aligned rows."""
    eng = mu.engine('qm9', lib, device)[0]
    batch = run(eng, list(BATCH5))
    back = run(eng, list(BATCH5[::-1]))
    for name in BATCH5:
        alone = run(eng, [name])[name]
        for got in (batch[name], back[name]):
            assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1]), name
    assert float(batch['ring'][0][2]) > 0.1 and float(batch['cloud'][0][2]) > 0.05


def test_a_molecule_alone_and_in_a_batch_on_emulation(emu_lib):
    _check_canonical(emu_lib, 'cpu')


@pytest.mark.gpu
def test_a_molecule_alone_and_in_a_batch_on_gpu():
    _check_canonical(None, 'cuda:0')


def _check_hygiene(lib, device):
    """The raw call between guard bands; nothing selected; the refusals."""
    eng = mu.engine('qm9', lib, device)[0]
    inp = inputs()
    names = ['select', 'two', 'one', 'ring']
    sizes = [inp[n][0].shape[0] for n in names]
    eng.bind(torch.tensor(sizes))
    N, B = sum(sizes), len(sizes)
    sel = torch.cat([inp['select'][2], torch.zeros(2, dtype=torch.bool), torch.ones(1, dtype=torch.bool), torch.ones(6, dtype=torch.bool)])
    gs = GuardSet(eng.device)
    xa = gs.inp('xa', torch.cat([inp[n][0] for n in names]))
    xb = gs.inp('xb', torch.cat([inp[n][1] for n in names]))
    sl = gs.inp('select', sel.to(torch.uint8))
    out, moved = gs.out('out', (B, 4)), gs.out('moved', (N, 3))
    call = lambda a, b, s, o, m: eng.lib.fm_align_rmsd(eng._ctx, eng._stream(), _ptr(a), _ptr(b), _ptr(s), _ptr(o), _ptr(m))
    assert call(xa, xb, sl, out, moved) == 0
    eng.synchronize()
    assert gs.check() == [] and gs.unwritten() == [], (gs.check(), gs.unwritten())
    want = run(eng, ['select', 'ring', 'one'])
    eng.bind(torch.tensor(sizes))
    rows = torch.split(moved.cpu(), sizes)
    for i, name in ((0, 'select'), (3, 'ring'), (2, 'one')):
        assert torch.equal(out.cpu()[i], want[name][0]) and torch.equal(rows[i], want[name][1]), name
    assert torch.equal(out.cpu()[1], torch.zeros(4)) and torch.equal(rows[1], inp['two'][0])          # no atom selected: zeros, and its rows are xa's
    # without the aligned output the numbers are the same
    gs2 = GuardSet(eng.device)
    out2 = gs2.out('out', (B, 4))
    assert call(xa, xb, sl, out2, None) == 0
    eng.synchronize()
    assert gs2.check() == [] and gs.check() == [] and torch.equal(out2.cpu(), out.cpu())
    err = lambda: eng.lib.fm_last_error(eng._ctx)
    before = (out.cpu().clone(), moved.cpu().clone())
    for args in ((xa, xb, sl, out, xa), (xa, xb, sl, out, xb), (xa, xb, moved, out, moved), (xa, xb, sl, xa, moved), (xa, xb, sl, out, out)):
        assert call(*args) == -1 and b'alias' in err(), err()
    assert call(None, xb, sl, out, moved) == -1 and call(xa, xb, sl, None, moved) == -1
    eng.synchronize()
    assert gs.check() == [] and torch.equal(out.cpu(), before[0]) and torch.equal(moved.cpu(), before[1])          # a refused call enqueues nothing
    with pytest.raises(ValueError, match='select'):
        eng.align_rmsd(xa, xb, torch.ones(N + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match='bound batch'):
        eng.align_rmsd(xa[:-1], xb[:-1])


def test_align_rmsd_between_guard_bands_and_refusals_on_emulation(emu_lib):
    _check_hygiene(emu_lib, 'cpu')


@pytest.mark.gpu
def test_align_rmsd_between_guard_bands_and_refusals_on_gpu():
    _check_hygiene(None, 'cuda:0')


def _check_model_rmsd(lib, device):
    """FlowMol.rmsd: the aligned column of one launch over the molecules; heavy=True drops 'H' and the fake atom of molecules_b; sizes must match."""
    mdl = mu.model('dev', lib, device)
    cfg = mdl.cfg
    inp = inputs()
    names = ['cloud', 'ring', 'two']
    sizes = [inp[n][0].shape[0] for n in names]
    gen = torch.Generator().manual_seed(3)
    N, U = sum(sizes), sum(n * (n - 1) // 2 for n in sizes)
    tok = {'a': torch.randint(0, cfg.n_atom_types, (N,), generator=gen), 'c': torch.randint(0, cfg.n_charges, (N,), generator=gen),
           'e': torch.randint(0, cfg.n_bond_types, (U,), generator=gen)}
    n = torch.tensor(sizes)
    ma = ({'x': torch.cat([inp[k][0] for k in names]), **tok}, n)
    mb = ({'x': torch.cat([inp[k][1] for k in names]), **tok}, n)
    got = mdl.rmsd(ma, mb)
    want = run(mdl.engine, names)
    assert got.shape == (3,) and torch.equal(got, torch.stack([want[k][0][2] for k in names]))
    amap = list(cfg.atom_type_map)
    light = torch.tensor([amap.index('H'), len(amap)] if cfg.fake_atoms else [amap.index('H')])
    heavy = ~torch.isin(tok['a'], light)
    assert bool(heavy.any()) and bool((~heavy).any())
    mdl.engine.bind(n)
    ref = mdl.engine.align_rmsd(ma[0]['x'], mb[0]['x'], heavy)[:, 2].cpu()
    assert torch.equal(mdl.rmsd(ma, mb, heavy=True), ref) and not torch.equal(ref, got)
    per_mol = [list(r) for r in torch.split(heavy, sizes)]
    assert torch.equal(mdl.rmsd(ma, mb, select=[[bool(v) for v in r] for r in per_mol]), ref)
    with pytest.raises(ValueError, match='size'):
        mdl.rmsd(ma, ru.take(mb, [0, 2, 1]))
    with pytest.raises(ValueError, match='select'):
        mdl.rmsd(ma, mb, select=torch.ones(N - 1, dtype=torch.bool))


def test_model_rmsd_on_emulation(emu_lib):
    _check_model_rmsd(emu_lib, 'cpu')


@pytest.mark.gpu
def test_model_rmsd_on_gpu():
    _check_model_rmsd(None, 'cuda:0')
