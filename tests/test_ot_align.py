"""The equivariant-OT coupling of the position prior on the device (ABI 16): fm_ot_align / Engine.ot_align, fm_conditional_path_x0,
Engine.conditional_path(coupling='ot') and the ``coupling`` argument of denoising_loss, resample, conformers and the sampling queue.

INPUTS (tests/ot_util.py, float32 from one generator): one, two, three, five atoms; cloud47 (a sigma = 1.5 cloud against an N(0, I) prior: the workload);
n65 and n130 (second and third lane stride of the column scan); mirror (x0 = a row-shuffled mirror image of a chiral 12-ring); ties (two coincident prior rows,
x1c on a lattice: the optimum is not unique); far (both clouds shifted by 500).

ASSIGNMENT.  The reference is scipy's linear_sum_assignment on the kernel's float32 cost matrix restated in torch (ot_util.cost_f32), in float64.  The kernel's
duals are float64 and exact, so perm is an optimum of that matrix: equal to scipy's where the optimum is unique (asserted here, on the host, for every input
but two, three and ties), of equal cost everywhere.  Against the reference's own recipe, torch.cdist in float32 (the matmul form above 25 rows), the
kernel's assignment costed in float64 may exceed scipy's optimum on the cdist matrix by 2 n eps c_max, eps = max(2^-21, the measured relative error of cdist
on that input): every entry of either matrix is within eps c_max of the true distance (the kernel's within 2^-23), and both are optimal for their own matrix.
Measured eps: 2^-21 or less on every input but far, where the matmul form cancels (|x|^2 = 750000) and cdist is off by 4.4e-2 c_max.

RIGID FIT.  The reference is the Kabsch of priors.py:128-169 (R = V U^T, no determinant correction; allow_reflection = 0: R = V diag(1, 1, det) U^T) in
float64 on x0[perm] (ot_util.rigid_reference).  Restated in float32, its error against float64 on these inputs, measured once on the host
(ot_util.f32_errors, the larger of the two settings; DESIGN_LOG.md "OT coupling on the device"), is F32_ERR: rmsd after the permutation, rmsd after the
fit, largest coordinate error.  The kernel gets 8x that (a different eigen-solver with a fixed sweep count).  one, two, three and ties: the rmsds only, the
optimal transform is not unique.  Every check runs on the CPU emulation and, marked gpu, on the device."""
import ctypes as C

import pytest
import torch

from flowmol_amd import _lib
from flowmol_amd.engine import _ptr, alpha_tables
from flowmol_amd.molecule import rigid_alignment
from hygiene_util import GuardSet, cpu

import mixed_util as mu
import ot_util as ou
import resample_util as ru

SEED = 777

# |float32 restatement - float64 reference|: (rmsd after the permutation, rmsd after the fit, coordinates); measured, see the module docstring
F32_ERR = {
    'one': (1.27e-07, 0.00e+00, 0.00e+00),
    'two': (5.07e-08, 4.19e-08, 8.30e-08),
    'three': (1.65e-08, 4.31e-08, 9.92e-08),
    'five': (2.36e-08, 1.43e-08, 6.15e-07),
    'cloud47': (7.00e-08, 3.18e-08, 6.30e-07),
    'n65': (4.59e-08, 7.00e-08, 7.01e-07),
    'n130': (2.20e-08, 1.15e-07, 1.04e-06),
    'mirror': (1.59e-08, 7.06e-07, 7.45e-07),
    'ties': (7.29e-08, 7.37e-08, 1.62e-07),
    'far': (3.85e-09, 1.86e-07, 4.63e-05),
}
BOUND = {k: tuple(8.0 * e for e in v) for k, v in F32_ERR.items()}


def run(eng, names, reflect=True):
    """One Engine.ot_align call on the molecules ``names`` -> {name: (perm (n,) int64, moved (n,3), out row (4,))} on the cpu."""
    inp = ou.inputs()
    sizes = [inp[n][0].shape[0] for n in names]
    eng.bind(torch.tensor(sizes))
    moved, out, perm = eng.ot_align(torch.cat([inp[n][0] for n in names]), torch.cat([inp[n][1] for n in names]), reflect=reflect, perm=True)
    eng.synchronize()
    return {n: (p.long(), m, o) for n, p, m, o in zip(names, torch.split(perm.cpu(), sizes), torch.split(moved.cpu(), sizes), out.cpu())}


def all_runs(lib, device):
    """Every input in one batch, with and without reflection: computed once per library and shared."""
    eng = mu.engine('qm9', lib, device)[0]
    return mu.cached(('ot-runs', id(lib), str(device)), lambda: {r: run(eng, list(ou.NAMES), r) for r in (True, False)})


# ---------------------------------------------------------------------------------------------------------------- 0. the references, on the host
def test_the_optimum_is_unique_where_perm_is_compared():
    inp = ou.inputs()
    assert all(ou.is_unique(*inp[n]) for n in ou.UNIQUE)
    assert not ou.is_unique(*inp['ties'])


def test_the_references_differ_on_the_mirror_image():
    x0, x1c = ou.inputs()['mirror']
    cols, _ = ou.assignment(x0, x1c)
    _, free, _ = ou.rigid_reference(x0[cols], x1c, torch.float64, True)
    _, proper, _ = ou.rigid_reference(x0[cols], x1c, torch.float64, False)
    assert free <= BOUND['mirror'][1] and proper > 10 * BOUND['mirror'][1], (free, proper)


def test_reference_translation_on_centred_priors():
    """molecule.rigid_alignment, the reference's code, ends with + mean0 + (mean1 - R mean0): R (x0 - mean0) + mean1 displaced by mean0 - R mean0, at most
    2 |mean0|, which is rounding for a COM-free prior."""
    inp = ou.inputs()
    for name in ou.COORDS:
        if name == 'far':
            continue
        x0, x1c = inp[name]
        x0p = x0[ou.assignment(x0, x1c)[0]].double()
        want = ou.rigid_reference(x0p, x1c, torch.float64, True)[2]
        got = rigid_alignment(x0p, x1c.double())
        assert float((got - want).abs().max()) <= 2 * float(x0p.mean(0).norm()) + 1e-12, name


# ---------------------------------------------------------------------------------------------------------------- 1. the assignment
def _check_assignment(lib, device):
    inp, got = ou.inputs(), all_runs(lib, device)
    for name in ou.NAMES:
        x0, x1c = inp[name]
        n = x0.shape[0]
        perm, _, out = got[True][name]
        cols, best = ou.assignment(x0, x1c)
        assert sorted(perm.tolist()) == list(range(n)), name
        assert torch.equal(perm, got[False][name][0]), name          # the assignment does not depend on the reflection flag
        if name in ou.UNIQUE:
            assert torch.equal(perm, cols), name
        c = ou.cost_f32(x0, x1c).double()
        mine = float(c[torch.arange(n), perm].sum())
        assert abs(mine - best) <= n * 2.0 ** -52 * best, (name, mine, best)
        assert float(out[0]) == n and float(out[1]) == float(torch.tensor(mine, dtype=torch.float64).float()), (name, out, mine)
        # against the reference's recipe: scipy on torch.cdist in float32
        true = torch.cdist(x1c.double(), x0.double(), p=2, compute_mode='donot_use_mm_for_euclid_dist')
        cd = torch.cdist(x1c, x0, p=2).double()
        eps = max(2.0 ** -21, float((cd - true).abs().max() / true.max()))
        _, best_cd = ou.assignment_of(cd)
        excess = float(true[torch.arange(n), perm].sum()) - best_cd
        print(f'{name}: cdist eps {eps:.3g}, excess over the cdist optimum {excess:.3g}, allowed {2 * n * eps * float(true.max()):.3g}')
        assert excess <= 2 * n * eps * float(true.max()), name


def test_assignment_is_scipys_optimum_on_emulation(emu_lib):
    _check_assignment(emu_lib, 'cpu')


@pytest.mark.gpu
def test_assignment_is_scipys_optimum_on_gpu():
    _check_assignment(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 2. the rigid fit
def _check_fit(lib, device):
    inp, got = ou.inputs(), all_runs(lib, device)
    bad = []
    for reflect in (True, False):
        for name in ou.NAMES:
            x0, x1c = inp[name]
            perm, moved, out = got[reflect][name]
            p64, r64, x64 = ou.rigid_reference(x0[perm], x1c, torch.float64, reflect)
            err = (abs(float(out[2]) - p64), abs(float(out[3]) - r64), float((moved.double() - x64).abs().max()) if name in ou.COORDS else 0.0)
            print(name, reflect, tuple(f'{e:.3g}' for e in err), tuple(f'{b:.3g}' for b in BOUND[name]))
            bad += [(name, reflect, 'prx'[i], err[i], BOUND[name][i]) for i in range(3) if not err[i] <= BOUND[name][i]]
    assert bad == [], bad
    assert torch.equal(got[True]['one'][1], inp['one'][1]) and got[True]['one'][0].tolist() == [0]          # n = 1: the identity, and x1c's row
    # the mirror image: a reflection fits it, no rotation does
    assert float(got[True]['mirror'][2][3]) <= BOUND['mirror'][1] and float(got[False]['mirror'][2][3]) > 10 * BOUND['mirror'][1]


def test_rigid_fit_against_float64_kabsch_on_emulation(emu_lib):
    _check_fit(emu_lib, 'cpu')


@pytest.mark.gpu
def test_rigid_fit_against_float64_kabsch_on_gpu():
    _check_fit(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 3. batch independence
def _check_canonical(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    for reflect in (True, False):
        batch, back = run(eng, list(ou.BATCH5), reflect), run(eng, list(ou.BATCH5[::-1]), reflect)
        for name in ou.BATCH5:
            alone = run(eng, [name], reflect)[name]
            for got in (batch[name], back[name], all_runs(lib, device)[reflect][name]):
                assert all(torch.equal(g, a) for g, a in zip(got, alone)), (name, reflect)


def test_a_molecule_alone_and_in_a_batch_on_emulation(emu_lib):
    _check_canonical(emu_lib, 'cpu')


@pytest.mark.gpu
def test_a_molecule_alone_and_in_a_batch_on_gpu():
    _check_canonical(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 4. the conditional path on a given prior
def _path_x0(eng, x1, alphas, groups, seed, x0_in):
    """fm_conditional_path_x0 through ctypes -> (state, tape) on the cpu."""
    d, i32 = eng.device, dict(dtype=torch.int32, device=eng.device)
    out = {'x_t': torch.empty(eng.N, 3, device=d), 'a_t': torch.empty(eng.N, **i32), 'c_t': torch.empty(eng.N, **i32), 'e_t': torch.empty(eng.U, **i32)}
    tape = {'x0': torch.empty(eng.N, 3, device=d), 'u_a': torch.empty(eng.N, device=d), 'u_c': torch.empty(eng.N, device=d), 'u_e': torch.empty(eng.U, device=d)}
    cs = _lib.fm_cond_tape()
    cs.x0, cs.u_a, cs.u_c, cs.u_e = _ptr(tape['x0']), _ptr(tape['u_a']), _ptr(tape['u_c']), _ptr(tape['u_e'])
    al = torch.tensor(alphas, dtype=torch.float32).to(d)
    grp = torch.tensor(groups, dtype=torch.int32).to(d)
    s1, so = eng._state_struct(x1), eng._state_struct(out)
    with eng._dev():
        rc = eng.lib.fm_conditional_path_x0(eng._ctx, eng._stream(), C.c_uint64(seed), C.byref(s1), len(alphas), _ptr(grp), _ptr(al), C.byref(so), C.byref(cs),
                                            _ptr(x0_in))
    eng._check(rc, 'fm_conditional_path_x0')
    eng.synchronize()
    return cpu(out), cpu(tape)


def _check_path_x0(lib, device):
    case = ru.kernel_case('qm9', lib, device)
    eng = ru.rebind(case)
    x1 = {k: v.to(eng.device) for k, v in case['x1'].items()}
    args = (case['alphas'], case['groups'], case['seed'])
    plain = {**case['out'], **case['tape']}
    for x0_in in (None, eng.prior_philox(case['seed'])):          # no prior given, and the prior the call would have drawn: fm_conditional_path bit for bit
        out, tape = _path_x0(eng, x1, *args, x0_in)
        assert mu.first_difference({**out, **tape}, plain) is None
    x1c = eng.remove_com(x1['x_t'].clone())
    x0a, _ = eng.ot_align(eng.prior_philox(case['seed']), x1c)
    out, tape = _path_x0(eng, x1, *args, x0a)
    al = ru.node_alpha(case['sizes'], case['groups'], case['alphas'], 0).unsqueeze(-1)
    assert torch.equal(out['x_t'], (1 - al) * x0a.cpu() + al * x1c.cpu())          # reference line 112 on the coupled prior: three separately rounded operations
    assert torch.equal(tape['x0'], x0a.cpu()) and not torch.equal(tape['x0'], case['tape']['x0'])
    assert all(torch.equal(out[k], case['out'][k]) for k in ('a_t', 'c_t', 'e_t')) and all(torch.equal(tape[k], case['tape'][k]) for k in ('u_a', 'u_c', 'u_e'))
    # Engine.conditional_path(coupling='ot') is that chain, and its tape replays on the host with the reference's recipe: scipy, then rigid_alignment
    st, tp = eng.conditional_path(x1, *args[:2], seed=case['seed'], tape=True, coupling='ot')
    eng.synchronize()
    assert mu.first_difference(cpu(st), out) is None and torch.equal(tp['x0'].cpu(), tape['x0']) and torch.equal(tp['x0_raw'].cpu(), case['tape']['x0'])
    raw, x0c, perm = tp['x0_raw'].cpu(), tp['x0'].cpu(), tp['perm'].cpu().long()
    for r, c, a, p, n in zip(*(torch.split(v, case['sizes']) for v in (raw, x1c.cpu(), x0c, perm)), case['sizes']):
        cols, _ = ou.assignment(r, c)
        assert torch.equal(p, cols)
        if n < 5:
            continue          # one, two atoms: the transform is not unique
        want = rigid_alignment(r[cols].double(), c.double())
        f32 = float((rigid_alignment(r[cols], c).double() - want).abs().max())
        bound = 8 * max(f32, F32_ERR['cloud47'][2]) + 2 * float(r.double().mean(0).norm())          # 8x the float32 restatement on this very input; the translation term
        assert float((a.double() - want).abs().max()) <= bound, (n, float((a.double() - want).abs().max()), bound)


def test_conditional_path_on_a_given_prior_on_emulation(emu_lib):
    _check_path_x0(emu_lib, 'cpu')


@pytest.mark.gpu
def test_conditional_path_on_a_given_prior_on_gpu():
    _check_path_x0(None, 'cuda:0')


def _check_coupling_shortens_the_path(lib, device):
    """At t = 0.1 the corrupted cloud47 lies closer to the molecule under the coupled prior: a property of the coupling, read off the states."""
    eng, cfg, _ = mu.engine('flowmol3', lib, device)
    x1c = ou.inputs()['cloud47'][1]
    n = x1c.shape[0]
    eng.bind(torch.tensor([n]))
    eng.set_molecule_ids(torch.tensor([5]))
    x1 = eng.make_state(x1c, torch.zeros(n), torch.zeros(n), torch.zeros(n * (n - 1) // 2))
    al = alpha_tables(torch.tensor([0.1]), cfg.schedule_type, cfg.cosine_params)[0]
    dist = {c: float((eng.conditional_path(x1, al, seed=SEED, coupling=c)['x_t'].cpu() - x1c).norm()) for c in ('independent', 'ot')}
    print(dist)
    assert dist['ot'] < dist['independent']


def test_coupling_shortens_the_path_on_emulation(emu_lib):
    _check_coupling_shortens_the_path(emu_lib, 'cpu')


@pytest.mark.gpu
def test_coupling_shortens_the_path_on_gpu():
    _check_coupling_shortens_the_path(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 5. the public interface
def _same_molecule(batch, sizes, i, alone):
    n = [int(v) for v in sizes]
    p = [k * (k - 1) // 2 for k in n]
    if not torch.equal(batch['per_molecule'][i:i + 1], alone['per_molecule']):
        return False
    return all(torch.equal(batch['rows'][k][sum((p if k == 'e' else n)[:i]):sum((p if k == 'e' else n)[:i + 1])], alone['rows'][k]) for k in 'xace')


def _check_denoising_loss(lib, device):
    mdl = mu.model('dev', lib, device)
    sizes, t, ids = [5, 3, 4], torch.tensor([0.3, 0.7, 0.3]), [40, 2, 9]
    mols = ru.given(mdl.cfg, sizes)
    kw = dict(seed=SEED, mol_ids=ids)
    plain = mdl.denoising_loss(mols, t, **kw)
    same = lambda a, b: torch.equal(a['per_molecule'], b['per_molecule']) and all(torch.equal(a['rows'][k], b['rows'][k]) for k in 'xace')
    assert same(mdl.denoising_loss(mols, t, coupling='independent', **kw), plain)
    ot = mdl.denoising_loss(mols, t, coupling='ot', **kw)
    assert not torch.equal(ot['rows']['x'], plain['rows']['x']) and all(torch.equal(ot['rows'][k] == 0, plain['rows'][k] == 0) for k in 'ace')
    for i in range(3):
        assert _same_molecule(ot, sizes, i, mdl.denoising_loss(ru.take(mols, [i]), float(t[i]), seed=SEED, mol_ids=[ids[i]], coupling='ot')), i
    try:          # None follows the checkpoint
        mdl.loss_hparams = {'prior_align_x': True}
        assert same(mdl.denoising_loss(mols, t, **kw), ot)
        mdl.loss_hparams = {'prior_align_x': False}
        assert same(mdl.denoising_loss(mols, t, **kw), plain)
    finally:
        mdl.loss_hparams = {}
    with pytest.raises(ValueError, match='coupling'):
        mdl.denoising_loss(mols, t, coupling='sinkhorn', **kw)


def test_denoising_loss_coupling_on_emulation(emu_lib):
    _check_denoising_loss(emu_lib, 'cpu')


@pytest.mark.gpu
def test_denoising_loss_coupling_on_gpu():
    _check_denoising_loss(None, 'cuda:0')


def test_checkpoint_hparams_set_the_default_coupling(tmp_path):
    """load_from_checkpoint reads prior_config.x.align into loss_hparams['prior_align_x'] (the pattern of distort_p); a missing key is the reference's False."""
    from flowmol_amd import FlowMol, presets, weights
    cfg = presets.flowmol3()
    sd = {'vector_field.' + k: v for k, v in weights.synth_state_dict(cfg, 0).items()}
    hp = {'atom_type_map': presets.GEOM_ATOMS, 'n_atoms_hist_file': 'data/geom_full_kekulized/train_data_n_atoms_histogram.pt',
          'marginal_dists_file': 'x', 'n_atom_charges': 6, 'parameterization': 'ctmc', 'fake_atom_p': 0.3, 'default_n_timesteps': 250,
          'interpolant_scheduler_config': {'schedule_type': {k: 'linear' for k in 'xace'}},
          'vector_field_config': dict(self_conditioning=True, stochasticity=30.0, high_confidence_threshold=0.9, n_vec_channels=32,
                                      update_edge_w_distance=True, n_hidden_scalars=256, n_hidden_edge_feats=128, s_message_dim=None,
                                      v_message_dim=None, n_expansion_gvps=3, attention=False, n_heads=32, n_recycles=1,
                                      separate_mol_updaters=True, n_molecule_updates=6, convs_per_update=1, n_cp_feats=4, n_message_gvps=3,
                                      n_update_gvps=3, message_norm='sum', rbf_dmax=10, rbf_dim=32, time_embedding_dim=64, a_token_dim=64,
                                      c_token_dim=64, e_token_dim=64)}
    for align in (True, False, None):
        px = {'type': 'centered-normal', 'kwargs': {'std': 1.0}, **({} if align is None else {'align': align})}          # configs/flowmol3.yml:62-66
        path = tmp_path / f'align_{align}.ckpt'
        torch.save({'state_dict': sd, 'hyper_parameters': {**hp, 'prior_config': {**{k: {'type': 'ctmc', 'align': False} for k in 'ace'}, 'x': px}}}, path)
        assert FlowMol.load_from_checkpoint(path).loss_hparams['prior_align_x'] is bool(align)
    assert 'prior_align_x' not in FlowMol.from_preset('dev').loss_hparams


def _check_resample(lib, device, T=4):
    mdl = mu.model('dev', lib, device)
    sizes, ids = [4, 3, 2], [40, 2, 9]
    mols = ru.given(mdl.cfg, sizes)
    plain = ru.resample_tensors(mdl, mols, 2, T, SEED, ids)
    assert all(mu.first_difference(a, b) is None for a, b in zip(ru.resample_tensors(mdl, mols, 2, T, SEED, ids, coupling='independent'), plain))
    ot = ru.resample_tensors(mdl, mols, [2, 1, 2], T, SEED, ids, coupling='ot')
    assert not torch.equal(ot[0]['x'], plain[0]['x'])
    for i, k in enumerate([2, 1, 2]):
        assert mu.first_difference(ot[i], ru.resample_alone(mdl, mols, i, k, T, SEED, ids[i], coupling='ot')) is None, i
    two = ru.take(mols, [0, 1])
    conf, n_rep = mdl.conformers(two, n_conformers=2, n_timesteps=T, seed=SEED, start_step=2, coupling='ot', return_tensors=True)
    rep = [0, 0, 1, 1]
    given = ru.take(mols, rep)[0]
    assert n_rep.tolist() == [sizes[i] for i in rep] and all(torch.equal(conf[k].long(), given[k].long()) for k in 'ace')
    free = mdl.conformers(two, n_conformers=2, n_timesteps=T, seed=SEED, start_step=2, return_tensors=True)[0]
    assert not torch.equal(conf['x'], free['x'])
    # a frozen pose follows the coupled path: the result holds the centred input rows either way, the free rows differ
    first = ru.take(mols, [0])
    keep = {'x': torch.tensor([True, True, False, False])}
    a = ru.resample_tensors(mdl, first, 1, T, SEED, ids[:1], keep=keep, coupling='ot')[0]
    b = ru.resample_tensors(mdl, first, 1, T, SEED, ids[:1], keep=keep)[0]
    assert torch.equal(a['x'][:2], b['x'][:2]) and not torch.equal(a['x'][2:], b['x'][2:])
    # the queue admits requests of both couplings into one batch; each is its resample call alone
    q = mdl.sampling_queue(seed=SEED)
    tk = q.submit_from(ru.take(mols, [0]), 2, T, mol_ids=[ids[0]], coupling='ot') + q.submit_from(ru.take(mols, [1]), 2, T, mol_ids=[ids[1]])
    q.run()          # admission takes the first step, here the last one of T = 4
    assert q.idle
    done = q.pop_finished()
    got = [{'x': done[t].x_1, 'a': done[t].a_1, 'c': done[t].c_1, 'e': done[t].e_1} for t in tk]
    assert mu.molecule_differences(got, [ot[0], plain[1]]) == []


def test_resample_and_conformers_coupling_on_emulation(emu_lib):
    _check_resample(emu_lib, 'cpu')


@pytest.mark.gpu
def test_resample_and_conformers_coupling_on_gpu():
    _check_resample(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 6. hygiene and refusals
def _check_hygiene(lib, device):
    eng = mu.engine('qm9', lib, device)[0]
    inp = ou.inputs()
    names = ['five', 'one', 'n65', 'mirror']
    sizes = [inp[n][0].shape[0] for n in names]
    eng.bind(torch.tensor(sizes))
    N, B = sum(sizes), len(sizes)
    call = lambda a, b, r, m, p, o: eng.lib.fm_ot_align(eng._ctx, eng._stream(), _ptr(a), _ptr(b), r, _ptr(m), _ptr(p), _ptr(o))
    results = []
    for fill in (None, 0.0, float('nan')):          # whatever the outputs held before
        gs = GuardSet(eng.device)
        x0, x1c = gs.inp('x0', torch.cat([inp[n][0] for n in names])), gs.inp('x1c', torch.cat([inp[n][1] for n in names]))
        init = (lambda shape, dt: None) if fill is None else (lambda shape, dt: torch.full(shape, fill if dt == torch.float32 else -7, dtype=dt))
        moved, perm = gs.out('moved', (N, 3), init=init((N, 3), torch.float32)), gs.out('perm', (N,), torch.int32, init=init((N,), torch.int32))
        out = gs.out('out', (B, 4), init=init((B, 4), torch.float32))
        assert call(x0, x1c, 1, moved, perm, out) == 0
        eng.synchronize()
        assert gs.check() == [] and gs.unwritten() == [], (gs.check(), gs.unwritten())
        results.append({'moved': moved.cpu().clone(), 'perm': perm.cpu().clone(), 'out': out.cpu().clone()})
    assert all(mu.first_difference(r, results[0]) is None for r in results[1:])
    want = run(eng, names)
    eng.bind(torch.tensor(sizes))
    for i, name in enumerate(names):
        assert torch.equal(torch.split(results[0]['perm'], sizes)[i].long(), want[name][0]) and torch.equal(torch.split(results[0]['moved'], sizes)[i], want[name][1])
        assert torch.equal(results[0]['out'][i], want[name][2])
    # without perm the other outputs are the same
    gs2 = GuardSet(eng.device)
    moved2, out2 = gs2.out('moved', (N, 3)), gs2.out('out', (B, 4))
    assert call(x0, x1c, 1, moved2, None, out2) == 0
    eng.synchronize()
    assert gs2.check() == [] and torch.equal(moved2.cpu(), results[0]['moved']) and torch.equal(out2.cpu(), results[0]['out'])
    # refusals: FM_ERR_INVALID with a message, nothing enqueued
    err = lambda: eng.lib.fm_last_error(eng._ctx)
    for args in ((x0, x1c, 1, x0, perm, out), (x0, x1c, 1, x1c, perm, out), (x0, x1c, 1, moved, perm, x0), (x0, x1c, 1, moved, moved, out), (x0, x1c, 1, moved, perm, moved),
                 (x0, x1c, 1, moved, out, out)):
        assert call(*args) == -1 and b'alias' in err(), err()
    assert call(None, x1c, 1, moved, perm, out) == -1 and call(x0, x1c, 1, None, perm, out) == -1 and call(x0, x1c, 1, moved, perm, None) == -1
    assert call(x0, x1c, 2, moved, perm, out) == -1 and b'allow_reflection' in err()
    eng.synchronize()
    assert gs.check() == [] and torch.equal(moved.cpu(), results[-1]['moved']) and torch.equal(out.cpu(), results[-1]['out'])
    with pytest.raises(ValueError, match='bound batch'):
        eng.ot_align(x0[:-1], x1c[:-1])
    with pytest.raises(ValueError, match='coupling'):
        eng.conditional_path({}, [1.0] * 4, seed=1, coupling='greedy')
    # fm_conditional_path_x0: the prior may not be an output
    case = ru.kernel_case('qm9', lib, device)
    eng = ru.rebind(case)
    x1 = {k: v.to(eng.device) for k, v in case['x1'].items()}
    buf = torch.zeros(eng.N, 3, device=eng.device)
    i32 = dict(dtype=torch.int32, device=eng.device)
    o = {'x_t': buf, 'a_t': torch.empty(eng.N, **i32), 'c_t': torch.empty(eng.N, **i32), 'e_t': torch.empty(eng.U, **i32)}
    al = torch.tensor([1.0, 1.0, 1.0, 1.0], device=eng.device)
    cs = _lib.fm_cond_tape()
    cs.x0 = _ptr(buf)
    s1, so = eng._state_struct(x1), eng._state_struct(o)
    assert eng.lib.fm_conditional_path_x0(eng._ctx, eng._stream(), C.c_uint64(1), C.byref(s1), 1, None, _ptr(al), C.byref(so), None, _ptr(buf)) == -1 and b'alias' in err()
    o['x_t'] = torch.empty(eng.N, 3, device=eng.device)
    so = eng._state_struct(o)
    assert eng.lib.fm_conditional_path_x0(eng._ctx, eng._stream(), C.c_uint64(1), C.byref(s1), 1, None, _ptr(al), C.byref(so), C.byref(cs), _ptr(buf)) == -1 and b'alias' in err()
    eng.synchronize()
    assert torch.equal(buf.cpu(), torch.zeros(eng.N, 3))


def test_ot_align_between_guard_bands_and_refusals_on_emulation(emu_lib):
    _check_hygiene(emu_lib, 'cpu')


@pytest.mark.gpu
def test_ot_align_between_guard_bands_and_refusals_on_gpu():
    _check_hygiene(None, 'cuda:0')


def _check_size_cap_and_state(lib, device):
    """A 257-atom molecule is refused from the bind's host-side sizes -- nothing is launched, the outputs stay untouched -- and so is a context without a batch."""
    from flowmol_amd import presets, weights
    from flowmol_amd.engine import Engine
    cfg = presets.PRESETS['qm9']()
    fresh = Engine(cfg, weights.synth_state_dict(cfg, 0), device=device, lib=lib)
    buf = lambda *s: torch.zeros(*s, device=fresh.device)
    call = lambda e, a, b, m, o: e.lib.fm_ot_align(e._ctx, e._stream(), _ptr(a), _ptr(b), 1, _ptr(m), None, _ptr(o))
    assert call(fresh, buf(4, 3), buf(4, 3), buf(4, 3), buf(1, 4)) == -1 and b'no batch bound' in fresh.lib.fm_last_error(fresh._ctx)
    sizes = [3, _lib.FM_OT_MAX_ATOMS + 1]
    fresh.bind(torch.tensor(sizes))
    gs = GuardSet(fresh.device)
    N = sum(sizes)
    gen = torch.Generator().manual_seed(1)
    x0, x1c = gs.inp('x0', torch.randn(N, 3, generator=gen)), gs.inp('x1c', torch.randn(N, 3, generator=gen))
    moved, out = gs.out('moved', (N, 3)), gs.out('out', (2, 4))
    assert call(fresh, x0, x1c, moved, out) == -1
    msg = fresh.lib.fm_last_error(fresh._ctx)
    assert b'molecule 1' in msg and b'257' in msg, msg
    fresh.synchronize()
    assert gs.check() == [] and sorted(gs.unwritten()) == ['moved', 'out']
    with pytest.raises(ValueError, match='257'):
        fresh.ot_align(x0, x1c)
    st = {'x_t': x1c}
    with pytest.raises(ValueError, match='257'):
        fresh.conditional_path(st, [1.0] * 4, seed=1, coupling='ot')
    fresh.bind(torch.tensor([_lib.FM_OT_MAX_ATOMS]))          # the cap itself is served
    x0, x1c = torch.randn(256, 3, generator=gen), torch.randn(256, 3, generator=gen) * 1.5
    moved, res, perm = fresh.ot_align(x0, x1c, perm=True)
    fresh.synchronize()
    assert torch.equal(perm.cpu().long(), ou.assignment(x0, x1c)[0]) and float(res[0, 0]) == 256
    fresh.close()
    # the public interface refuses before any bind
    mdl = mu.model('dev', lib, device)
    big = ru.given(mdl.cfg, [257])
    for fn in (lambda: mdl.resample(big, 1, n_timesteps=3, seed=1, coupling='ot'), lambda: mdl.denoising_loss(big, 0.5, seed=1, coupling='ot'),
               lambda: mdl.conformers(big, n_timesteps=3, seed=1, start_step=1, coupling='ot'),
               lambda: mdl.sampling_queue(seed=1).submit_from(big, 1, 3, coupling='ot')):
        with pytest.raises(ValueError, match='257'):
            fn()
    small = ru.given(mdl.cfg, [3])
    for fn in (lambda: mdl.resample(small, 1, n_timesteps=3, seed=1, coupling='hungarian'), lambda: mdl.inpaint(small, [[True, False, False]], n_timesteps=3, seed=1, coupling=None),
               lambda: mdl.sampling_queue(seed=1).submit_from(small, 1, 3, coupling='x')):
        with pytest.raises(ValueError, match='coupling'):
            fn()
    with pytest.raises(NotImplementedError):
        mu.model('endpoint_small', lib, device).resample(small, 1, n_timesteps=3, seed=1, coupling='ot')


def test_size_cap_and_unbound_context_on_emulation(emu_lib):
    _check_size_cap_and_state(emu_lib, 'cpu')


@pytest.mark.gpu
def test_size_cap_and_unbound_context_on_gpu():
    _check_size_cap_and_state(None, 'cuda:0')
