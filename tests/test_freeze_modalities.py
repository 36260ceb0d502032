"""Frozen rows per modality (ABI 13): fm_ctmc_step_freeze / fm_integrate_freeze, Engine.freeze_spec / ctmc_step_freeze / integrate_freeze /
IntegrationRun(inpaint=freeze spec), FlowMol.resample(keep={...}) / inpaint / conformers, SamplingQueue.submit_from(keep={...}).

The contract.  A step is exactly the plain step on ALL rows; then every row whose OWN modality's flag is set -- keep_x, keep_a, keep_c per atom, keep_e per
unordered pair, four independent arrays -- is set, inside the step kernel, to the conditional path of the given molecule at the step's new time point.  A NULL
keep array leaves its modality free and its path inputs unread.  Everything compares bit for bit (torch.equal) against the plain step and a host torch.where per
modality, or against the ABI-12 calls; the one tolerance is the oracle replay's, that of test_resample.py's own replay.

(1) one step without a network evaluation, four independent masks, both workgroup sizes, campbell and gat, both noise modes, both purity branches, last_step;
(2) equivalence with ABI 12: the derived masks give fm_ctmc_step_inpaint's and fm_integrate_inpaint's bits;
(3) one modality at a time, the others NULL; all-zero flags and all-NULL pointers are the plain step;
(4) integrations against the step-by-step composition, the cases of test_inpaint.py: (T, k) = (6, 2) with and without a sink, (5, 0) with its bootstrap, three
    distinct (T, k) with k > 0; on the GPU also flowmol3;
(5) the API: dict keep = plain keep, batch = alone in shuffled order, conformers, the queue (a batch that mixes both keep forms included);
(6) cpu_ref.OracleVF replayed with the noise tapes and the same per-modality overwrite; (7) guarded raw-ABI calls and every refusal.

Shapes as in test_inpaint.py.  Every check runs on the CPU emulation of the kernel sources and, marked gpu, on the device."""
import ctypes as C

import pytest
import torch

from flowmol_amd import _lib
from flowmol_amd.engine import IntegrationRun, fm_dst, fm_state, fm_step_scalars
from hygiene_util import cpu

import freeze_util as fu
import hygiene_util as hu
import inpaint_util as iu
import mixed_util as mu
import resample_util as ru

SEED = 2024
TRAJ_SIZES = iu.TRAJ_SIZES
TRAJ_IDS = [4, 1, 8, 6]
MIXED_PAIRS = [(6, 2), (5, 1), (4, 2), (6, 2)]          # test_inpaint.py's: three distinct (T, k), every k > 0
MASK = lambda cfg: {'a': cfg.n_atom_types, 'c': cfg.n_charges, 'e': cfg.n_bond_types}


# ---------------------------------------------------------------------------------------------------------------- 1. one step
def _check_step_conditions(case):
    """What keeps the one-step comparison from passing vacuously, as far as it depends on the inputs alone."""
    cfg, m, path, sizes = case['cfg'], case['masks'], case['path'], case['sizes']
    for f in 'ace':          # per modality the frozen rows hold masked and unmasked tokens under alpha_next
        masked = path[f'{f}_t'][m[f]] == MASK(cfg)[f]
        assert bool(masked.any()) and bool((~masked).any()), f
    pa = fu.pair_atoms(sizes)
    ai, aj, xi, xj = m['a'][pa[:, 0]], m['a'][pa[:, 1]], m['x'][pa[:, 0]], m['x'][pa[:, 1]]
    assert bool((m['e'] & ~ai & ~aj).any())          # a frozen bond between two atoms whose types are free
    assert bool((m['e'] & (xi ^ xj)).any())          # a frozen bond with exactly one atom whose position is kept
    assert bool(((m['a'] != m['c']) & (m['c'] != m['x'])).any())          # an atom with keep_a != keep_c != keep_x
    assert all(bool(m[f].any()) and bool((~m[f]).any()) for f in 'xace')


def _check_step(lib, device, threads, dfm_type):
    case = fu.step_case(lib, device, threads)
    _check_step_conditions(case)
    m, path = case['masks'], case['path']
    combos = [(philox, hc, last) for philox in (True, False) for hc in (0.0, 0.9) for last in (0, 1)]
    if dfm_type == 'gat':          # the gat step reads neither hc_thresh nor last_step
        combos = [(True, 0.0, 0), (False, 0.0, 0)]
    for philox, hc, last in combos:
        tag = (threads, dfm_type, philox, hc, last)
        plain, smp_p = fu.plain_step(case, dfm_type, philox, hc, last)
        got, smp_g = fu.freeze_step(case, case['fspec'], dfm_type, philox, hc, last)
        assert mu.first_difference(smp_p, smp_g) is None, tag          # the sampled endpoint tokens are the plain step's
        assert not bool((smp_g['a1'] == -7).any()) and not bool((smp_g['e1'] == -7).any())
        want = fu.composed(plain, path, m)
        for f in 'xace':
            key = f'{f}_t'
            assert torch.equal(got[key], want[key]), (tag, f)
            assert torch.equal(got[key][~m[f]], plain[key][~m[f]]), (tag, f)          # no free row differs from the plain step
            assert not torch.equal(got[key][m[f]], plain[key][m[f]]), (tag, f)          # and the overwrite did something in every modality
        assert not torch.equal(plain['a_t'], cpu(case['state'])['a_t']), tag          # the plain step did something


def test_one_step_is_the_plain_step_then_the_overwrite_per_modality_on_emulation(emu_lib):
    for threads in (256, 1024):
        for dfm_type in ('campbell', 'gat'):
            _check_step(emu_lib, 'cpu', threads, dfm_type)


@pytest.mark.gpu
@pytest.mark.parametrize('threads', [256, 1024])
@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
def test_one_step_is_the_plain_step_then_the_overwrite_per_modality_on_gpu(threads, dfm_type):
    _check_step(None, 'cuda:0', threads, dfm_type)


# ---------------------------------------------------------------------------------------------------------------- 2. equivalence with ABI 12
def _check_abi12_step(lib, device):
    for threads in (256, 1024):
        case = fu.step_case(lib, device, threads)
        eng = fu.rebind(case)
        derived = iu.frozen_masks(case['sizes'], case['keep'])          # x = a = c = keep_atom, e = both atoms kept, written out on the host
        spec = eng.freeze_spec(case['x1'], derived, case['seed'])
        for dfm_type, philox, hc, last in (('campbell', True, 0.9, 0), ('campbell', False, 0.0, 1), ('gat', True, 0.0, 0), ('gat', False, 0.0, 0)):
            got, smp_g = fu.freeze_step(case, spec, dfm_type, philox, hc, last)
            want, smp_w = fu.freeze_step(case, case['spec'], dfm_type, philox, hc, last)          # fm_ctmc_step_inpaint
            plain, _ = fu.plain_step(case, dfm_type, philox, hc, last)
            assert mu.first_difference(got, want) is None and mu.first_difference(smp_g, smp_w) is None, (threads, dfm_type, philox)
            assert mu.first_difference(got, plain) is not None


def _check_abi12_integrate(lib, device, T=5, k=1):
    mdl = mu.model('dev', lib, device)
    eng, x1, keep, spec12, frozen = iu.traj_setup(mdl, TRAJ_SIZES, TRAJ_IDS, SEED)
    spec13 = eng.freeze_spec(x1, frozen, SEED)
    plan = mu.philox_plans(mdl, [T], SEED)[0]
    res = []
    for spec in (spec12, spec13, None):
        state = eng.conditional_path(x1, iu.alpha_table(eng, plan)[k], seed=SEED)
        run = IntegrationRun(eng, state, plan, None, inpaint=spec)
        run.run(k, T - 1)
        eng.synchronize()
        res.append({**cpu(state), **{f'dst.{f}': v.cpu().clone() for f, v in run.last_dst().items()}})
    assert mu.first_difference(res[0], res[1]) is None
    assert mu.first_difference(res[0], res[2]) is not None


def test_derived_masks_give_the_bits_of_abi_12_on_emulation(emu_lib):
    _check_abi12_step(emu_lib, 'cpu')
    _check_abi12_integrate(emu_lib, 'cpu')


@pytest.mark.gpu
@pytest.mark.parametrize('part', ['step', 'integrate'])
def test_derived_masks_give_the_bits_of_abi_12_on_gpu(part):
    {'step': _check_abi12_step, 'integrate': _check_abi12_integrate}[part](None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 3. one modality at a time
def _check_one_modality(lib, device):
    case = fu.step_case(lib, device, 256)
    eng, m, path = fu.rebind(case), case['masks'], case['path']
    for dfm_type, philox in (('campbell', True), ('gat', False)):
        plain, smp_p = fu.plain_step(case, dfm_type, philox, 0.9, 0)
        for f in 'xace':
            spec = eng.freeze_spec(case['x1'], {f: m[f]}, case['seed'])
            own = {'x': ('keep_x', 'x0', 'x1c')}.get(f, (f'keep_{f}', f'{f}1', f'u_{f}'))
            assert sorted(k for k, v in spec.items() if v is not None) == sorted(own), f          # the other keep arrays and path inputs travel as NULL
            got, smp_g = fu.freeze_step(case, spec, dfm_type, philox, 0.9, 0)
            assert mu.first_difference(got, fu.composed(plain, path, {f: m[f]})) is None, (dfm_type, f)
            assert mu.first_difference(smp_g, smp_p) is None
            assert not torch.equal(got[f'{f}_t'], plain[f'{f}_t']), (dfm_type, f)
        zeros = eng.freeze_spec(case['x1'], {f: torch.zeros_like(m[f]) for f in 'xace'}, case['seed'])          # every flag zero
        assert all(v is not None for v in zeros.values())
        assert mu.first_difference(fu.freeze_step(case, zeros, dfm_type, philox, 0.9, 0)[0], plain) is None, dfm_type
        nothing = eng.freeze_spec(case['x1'], {}, case['seed'])          # every pointer NULL
        assert all(v is None for v in nothing.values())
        assert mu.first_difference(fu.freeze_step(case, nothing, dfm_type, philox, 0.9, 0)[0], plain) is None, dfm_type


def test_one_modality_at_a_time_on_emulation(emu_lib):
    _check_one_modality(emu_lib, 'cpu')


@pytest.mark.gpu
def test_one_modality_at_a_time_on_gpu():
    _check_one_modality(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 4. integration = composition
def _check_single(preset, lib, device, sizes, ids, T, k, with_traj):
    mdl = mu.model(preset, lib, device)
    masks = fu.traj_masks(sizes)
    with fu.modal_compositions(masks):
        got, want, frozen = iu.single_runs(mdl, sizes, ids, T, k, SEED, with_traj)
    assert mu.first_difference(got, want) is None, (preset, T, k, with_traj)
    eng = mdl.engine
    given = ru.given(mdl.cfg, sizes)[0]
    x1c = eng.remove_com(ru.as_state(eng, ru.given(mdl.cfg, sizes))['x_t'].clone()).cpu()
    assert torch.equal(got['x_t'][frozen['x']], x1c[frozen['x']])          # alpha(1) = 1: frozen positions are the centred input rows
    assert not torch.equal(got['x_t'][~frozen['x']], x1c[~frozen['x']])
    for f in 'ace':
        assert torch.equal(got[f'{f}_t'][frozen[f]].long(), given[f][frozen[f]].long()), f
    if with_traj:          # the frames of the sink show the overwritten rows: compared frame by frame inside first_difference; none is left unwritten
        assert not bool((got['traj.a'] == -3).any()) and not bool((got['traj.e1'] == -3).any())
        assert torch.equal(got['traj.x'][-1], got['x_t']) and torch.equal(got['traj.e'][-1], got['e_t'])


def _check_mixed(preset, lib, device, sizes, ids, pairs):
    mdl = mu.model(preset, lib, device)
    masks = fu.traj_masks(sizes)
    with fu.modal_compositions(masks):
        got, want, frozen = iu.mixed_runs(mdl, sizes, ids, pairs, SEED)
    assert mu.first_difference(got, want) is None, (preset, pairs)
    given = ru.given(mdl.cfg, sizes)[0]
    for f in 'ace':
        assert torch.equal(got[f'{f}_t'][frozen[f]].long(), given[f][frozen[f]].long()), f


def test_integration_is_the_step_by_step_composition_on_emulation(emu_lib):
    _check_single('dev', emu_lib, 'cpu', TRAJ_SIZES, TRAJ_IDS, 6, 2, False)
    _check_single('dev', emu_lib, 'cpu', TRAJ_SIZES, TRAJ_IDS, 6, 2, True)
    _check_single('dev', emu_lib, 'cpu', TRAJ_SIZES, TRAJ_IDS, 5, 0, False)          # k = 0: the bootstrap evaluation runs
    _check_mixed('dev', emu_lib, 'cpu', TRAJ_SIZES, TRAJ_IDS, MIXED_PAIRS)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['single', 'traj', 'boot', 'mixed', 'flowmol3'])
def test_integration_is_the_step_by_step_composition_on_gpu(case):
    if case == 'flowmol3':
        _check_single('flowmol3', None, 'cuda:0', [5, 9], [2, 7], 5, 2, True)
        _check_mixed('flowmol3', None, 'cuda:0', [5, 9], [2, 7], [(5, 2), (4, 1)])
    elif case == 'mixed':
        _check_mixed('dev', None, 'cuda:0', TRAJ_SIZES, TRAJ_IDS, MIXED_PAIRS)
    else:
        T, k = (5, 0) if case == 'boot' else (6, 2)
        _check_single('dev', None, 'cuda:0', TRAJ_SIZES, TRAJ_IDS, T, k, case == 'traj')


# ---------------------------------------------------------------------------------------------------------------- 5. the API
API_PAIRS = [(6, 2), (6, 0), (5, 1), (4, 3)]          # test_inpaint.py's: one from the prior (an engine call of its own), one that only gets corrupted


def _check_api_forms(lib, device, T=4):
    mdl = mu.model('dev', lib, device)
    mols, ids = ru.given(mdl.cfg, TRAJ_SIZES), TRAJ_IDS
    keep = iu.traj_keep(TRAJ_SIZES)
    derived = iu.frozen_masks(TRAJ_SIZES, iu.flat(keep))
    plain_keep = iu.resample_tensors(mdl, mols, 1, T, SEED, ids, keep)
    assert mu.molecule_differences(fu.resample_tensors(mdl, mols, 1, T, SEED, ids, derived), plain_keep) == []          # tensors over the concatenated rows
    assert mu.molecule_differences(fu.resample_tensors(mdl, mols, 1, T, SEED, ids, fu.per_molecule(derived, TRAJ_SIZES)), plain_keep) == []          # one sequence per molecule
    a = mdl.inpaint(mols, derived, n_timesteps=T, seed=SEED, mol_ids=ids, return_tensors=True)[0]
    b = mdl.inpaint(mols, keep, n_timesteps=T, seed=SEED, mol_ids=ids, return_tensors=True)[0]
    assert mu.first_difference({f: a[f].cpu() for f in 'xace'}, {f: b[f].cpu() for f in 'xace'}) is None
    # an all-False dict, and a dict without keys, are the call without keep
    free = ru.resample_tensors(mdl, mols, 1, T, SEED, ids)
    N, U = fu.rows_of(TRAJ_SIZES)
    nothing = {f: torch.zeros(U if f == 'e' else N, dtype=torch.bool) for f in 'xace'}
    assert mu.molecule_differences(fu.resample_tensors(mdl, mols, 1, T, SEED, ids, nothing), free) == []
    assert mu.molecule_differences(fu.resample_tensors(mdl, mols, 1, T, SEED, ids, {}), free) == []
    assert mu.molecule_differences(plain_keep, free) != []


def _check_api_composition(lib, device):
    """Molecule i of a batch call = the molecule run alone with its id, in shuffled order; independent masks, one (T, k) per molecule."""
    mdl = mu.model('dev', lib, device)
    mols, ids = ru.given(mdl.cfg, TRAJ_SIZES), [3, 5, 7, 9]
    masks = fu.traj_masks(TRAJ_SIZES)
    Ts, ks = [T for T, _ in API_PAIRS], [k for _, k in API_PAIRS]
    want = [fu.resample_tensors(mdl, ru.take(mols, [i]), ks[i], Ts[i], SEED, [ids[i]], fu.take_masks(masks, TRAJ_SIZES, [i]))[0] for i in range(len(TRAJ_SIZES))]
    got = fu.resample_tensors(mdl, mols, ks, Ts, SEED, ids, masks)
    assert mu.molecule_differences(got, want) == []
    order = [2, 0, 3, 1]
    back = fu.resample_tensors(mdl, ru.take(mols, order), [ks[i] for i in order], [Ts[i] for i in order], SEED, [ids[i] for i in order], fu.take_masks(masks, TRAJ_SIZES, order))
    assert mu.molecule_differences(back, [want[i] for i in order]) == []
    assert mu.molecule_differences(got, ru.resample_tensors(mdl, mols, ks, Ts, SEED, ids)) != []
    centred = ru.centred(mdl.engine, mols)
    for i, (g, c) in enumerate(zip(got, centred)):          # alpha(1) = 1: the frozen rows of every modality are the (centred) input's
        mi = fu.take_masks(masks, TRAJ_SIZES, [i])
        for f in 'xace':
            assert torch.equal(g[f][mi[f]].to(c[f].dtype), c[f][mi[f]]), (i, f)


def _check_conformers(lib, device, T=5, K=3):
    mdl = mu.model('dev', lib, device)
    sizes = [5, 3]
    mols = ru.given(mdl.cfg, sizes)
    ids = [21, 4, 9, 30, 2, 17]
    out = mdl.conformers(mols, n_conformers=K, n_timesteps=T, seed=SEED, mol_ids=ids, return_tensors=True)[0]
    rep = fu.repeat(mols, K)
    rsizes = rep[1].tolist()
    assert rsizes == [5, 5, 5, 3, 3, 3]          # molecule-major
    got = mu.split_molecules(out, rsizes)
    centred = ru.centred(mdl.engine, rep)
    for g, c in zip(got, centred):          # every result's a, c, e are the input's; its positions are not
        assert all(torch.equal(g[f].long(), c[f].long()) for f in 'ace')
        assert not torch.equal(g['x'], c['x'])
    assert not torch.equal(got[0]['x'], got[1]['x']) and not torch.equal(got[3]['x'], got[5]['x'])          # two conformers of one molecule differ
    # it is the explicit resample(keep={...}) call, and conformer j is the single-molecule call with its id
    N, U = fu.rows_of(rsizes)
    keep = {'a': torch.ones(N, dtype=torch.bool), 'c': torch.ones(N, dtype=torch.bool), 'e': torch.ones(U, dtype=torch.bool)}
    assert mu.molecule_differences(got, fu.resample_tensors(mdl, rep, 0, T, SEED, ids, keep)) == []
    for j in (1, 4):
        one = mdl.conformers(ru.take(mols, [j // K]), n_conformers=1, n_timesteps=T, seed=SEED, mol_ids=[ids[j]], return_tensors=True)[0]
        assert mu.molecule_differences([got[j]], mu.split_molecules(one, [rsizes[j]])) == [], j
    later = mdl.conformers(mols, n_conformers=K, n_timesteps=T, seed=SEED, mol_ids=ids, start_step=3, return_tensors=True)[0]
    assert mu.molecule_differences(mu.split_molecules(later, rsizes), fu.resample_tensors(mdl, rep, 3, T, SEED, ids, keep)) == []
    assert len(mdl.conformers(mols, n_conformers=2, n_timesteps=3, seed=SEED)) == 4          # defaults: ids 0 .. B K - 1, a flat list of molecules
    with pytest.raises(ValueError, match='n_conformers'):
        mdl.conformers(mols, n_conformers=0, seed=SEED)
    with pytest.raises(ValueError, match='mol_ids'):
        mdl.conformers(mols, n_conformers=K, n_timesteps=T, seed=SEED, mol_ids=[1, 2])


def test_api_on_emulation(emu_lib):
    _check_api_forms(emu_lib, 'cpu')
    _check_api_composition(emu_lib, 'cpu')
    _check_conformers(emu_lib, 'cpu')


@pytest.mark.gpu
@pytest.mark.parametrize('part', ['forms', 'composition', 'conformers'])
def test_api_on_gpu(part):
    {'forms': _check_api_forms, 'composition': _check_api_composition, 'conformers': _check_conformers}[part](None, 'cuda:0')


def _check_queue(lib, device):
    """Tickets submitted with a dict keep -- and, next to them, one with a plain keep -- into a running batch equal their runs alone."""
    mdl = mu.model('dev', lib, device)
    mol, mol2 = ru.given(mdl.cfg, [12]), ru.given(mdl.cfg, [7], seed=18)
    masks = fu.traj_masks([12], seed=23)
    keep2 = [[i % 2 == 0 for i in range(7)]]
    want = fu.resample_tensors(mdl, mol, 2, 6, SEED, [7], masks)[0]
    want_conf = fu.resample_tensors(mdl, mol, 2, 6, SEED, [8], {f: torch.ones_like(masks[f]) for f in 'ace'})[0]
    want2 = iu.resample_tensors(mdl, mol2, 1, 6, SEED, [11], keep2)[0]
    others = mu.alone_runs('dev', lib, device, [9, 5], [8, 8], SEED)
    q = mdl.sampling_queue(seed=SEED)
    t9, t5 = q.submit([9, 5], n_timesteps=8, mol_ids=[0, 1])
    assert q.run(max_steps=3) == 3 and q.pop_finished() == {}
    (tm,) = q.submit_from(mol, start_step=2, n_timesteps=6, mol_ids=[7], keep=fu.per_molecule(masks, [12]))
    (tc,) = q.submit_from(mol, start_step=2, n_timesteps=6, mol_ids=[8], keep={f: torch.ones_like(masks[f]) for f in 'ace'})          # conformer-style: no 'x'
    (t2,) = q.submit_from(mol2, start_step=1, n_timesteps=6, mol_ids=[11], keep=keep2)          # the plain form, in the same batch
    done, calls = {}, 0
    while not q.idle:
        assert q.run(max_steps=2) > 0 and calls < 8
        calls += 1
        done.update(q.pop_finished())
    res = lambda t: {'x': done[t].x_1, 'a': done[t].a_1, 'c': done[t].c_1, 'e': done[t].e_1}
    assert mu.molecule_differences([res(tm), res(tc), res(t2)], [want, want_conf, want2]) == []
    assert mu.molecule_differences([res(t9), res(t5)], others) == []
    assert mu.molecule_differences([res(tm)], [ru.resample_alone(mdl, mol, 0, 2, 6, SEED, 7)]) != []
    given = mu.split_molecules(mol[0], [12])[0]
    assert all(torch.equal(res(tc)[f].long(), given[f].long()) for f in 'ace')


def test_queue_admits_per_modality_requests_on_emulation(emu_lib):
    _check_queue(emu_lib, 'cpu')


@pytest.mark.gpu
def test_queue_admits_per_modality_requests_on_gpu():
    _check_queue(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 6. anchored to the oracle
def _check_oracle(preset, lib, device, sizes, pairs):
    """Every molecule alone: tokens identical; coordinates within 1e-5 of the largest coordinate, the tolerance of test_resample.py's oracle replay."""
    mdl = mu.model(preset, lib, device)
    mols = ru.given(mdl.cfg, sizes)
    masks = fu.traj_masks(sizes)
    for i, (n, (T, k)) in enumerate(zip(sizes, pairs)):
        one, mi = ru.take(mols, [i]), fu.take_masks(masks, sizes, [i])
        with fu.modal_compositions(mi):
            want = iu.oracle_inpaint(mdl, [n], [i], one, [[False] * n], k, T, SEED)
        got = fu.resample_tensors(mdl, one, k, T, SEED, [i], mi)[0]
        for f in 'ace':
            assert torch.equal(got[f].int(), want[f]), (i, f)
        err = float((got['x'] - want['x']).abs().max() / want['x'].abs().max())
        assert err < 1e-5, (i, err)
        free = ~mi['x']
        assert not bool(free.any()) or not torch.equal(got['x'][free], ru.centred(mdl.engine, one)[0]['x'][free])


def test_per_modality_freezing_replayed_by_the_oracle_on_emulation(emu_lib):
    _check_oracle('dev', emu_lib, 'cpu', [5, 3, 2], [(6, 2), (5, 1), (4, 2)])


@pytest.mark.gpu
@pytest.mark.parametrize('preset', ['dev', 'flowmol3'])
def test_per_modality_freezing_replayed_by_the_oracle_on_gpu(preset):
    if preset == 'dev':
        _check_oracle('dev', None, 'cuda:0', [5, 3, 2], [(6, 2), (5, 1), (4, 2)])
    else:
        _check_oracle('flowmol3', None, 'cuda:0', [5, 9], [(5, 2), (4, 1)])


# ---------------------------------------------------------------------------------------------------------------- 7. hygiene and refusals
def _three_fills(eng, sizes, run):
    """``run(ws)`` -> (results, GuardSet) in an arena pre-filled with zeros, with another batch's run, and then with NaNs: arena, guard bands and inputs intact,
    every output written, the results identical.  -> the 'zero' results."""
    results = {}
    for fill in ('zero', 'history', 'ones'):
        ws, intact = hu.arena(eng, [sizes] + [list(s_) for s_ in hu.HISTORY_PREDECESSORS], fill, hu.sample_history)
        res, gs = run(ws)
        assert intact(eng.workspace_bytes), fill
        assert gs.check() == [] and gs.unwritten() == [], (fill, gs.check(), gs.unwritten())
        assert hu.non_finite(res) == [], (fill, hu.non_finite(res))
        results[fill] = res
        if fill != 'zero':
            assert mu.first_difference(results['zero'], res) is None, (fill, mu.first_difference(results['zero'], res))
    return results['zero']


def _check_guarded_calls(lib, device):
    eng, _, _ = mu.engine('qm9', lib, device)
    sizes, ids = list(iu.KERNEL_SIZES), list(iu.KERNEL_IDS)
    case = fu.step_case(lib, device, 256)
    res = _three_fills(eng, sizes, lambda ws: fu.guarded_step(eng, ws, sizes, ids, case['masks'], 91))
    want, _ = fu.freeze_step(case, case['fspec'], 'campbell', True, 0.9, 0)
    assert all(torch.equal(res[f], want[f]) for f in ('x_t', 'a_t', 'c_t', 'e_t'))
    only_e = {'e': case['masks']['e']}          # the position and atom members NULL
    res = _three_fills(eng, sizes, lambda ws: fu.guarded_step(eng, ws, sizes, ids, only_e, 91))
    want, _ = fu.freeze_step(case, fu.rebind(case).freeze_spec(case['x1'], only_e, 91), 'campbell', True, 0.9, 0)
    assert all(torch.equal(res[f], want[f]) for f in ('x_t', 'a_t', 'c_t', 'e_t'))
    mdl = mu.model('dev', lib, device)
    masks = fu.traj_masks(TRAJ_SIZES)
    res = _three_fills(mdl.engine, TRAJ_SIZES, lambda ws: fu.guarded_integrate(mdl, ws, TRAJ_SIZES, TRAJ_IDS, MIXED_PAIRS, masks, SEED))
    with fu.modal_compositions(masks):
        got, _, _ = iu.mixed_runs(mdl, TRAJ_SIZES, TRAJ_IDS, MIXED_PAIRS, SEED)
    assert all(torch.equal(res[f], got[f]) for f in ('x_t', 'a_t', 'c_t', 'e_t'))


def test_freeze_calls_between_guard_bands_on_emulation(emu_lib):
    _check_guarded_calls(emu_lib, 'cpu')


@pytest.mark.gpu
def test_freeze_calls_between_guard_bands_on_gpu():
    _check_guarded_calls(None, 'cuda:0')


def _check_c_refusals(lib, device):
    eng, cfg, _ = mu.engine('qm9', lib, device)
    sizes = [3, 2]
    eng.bind(torch.tensor(sizes))
    eng.set_molecule_ids(None)
    x1 = ru.as_state(eng, ru.given(cfg, sizes))
    masks = {'x': torch.tensor([True, False, True, True, False]), 'a': torch.tensor([False, True, True, False, False]),
             'c': torch.tensor([True, True, False, False, True]), 'e': torch.tensor([True, False, True, True])}
    spec = eng.freeze_spec(x1, masks, 1)
    state = eng.conditional_path(x1, [0.5] * 4, seed=1)
    before = cpu(state)
    dst, dst_b = iu.softmax_dst(eng), iu.softmax_dst(eng, 6)
    plan = iu.make_step_plan(4, 1.0, 0.9, cfg.cat_temperature, philox_seed=1, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)
    gat = iu.make_step_plan(4, 1.0, 0.9, cfg.cat_temperature, dfm_type='gat', philox_seed=1, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)
    tensors = iu.make_step_plan(4, 1.0, 0.9, cfg.cat_temperature, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)
    sc, al = plan.scalars[1], (C.c_float * 4)(0.6, 0.6, 0.6, 0.6)
    temb = torch.zeros(2, cfg.time_embedding_dim, device=device)
    traj = eng.new_traj(1)
    smp = iu.sampled_buffers(eng)
    err = lambda e=eng: e.lib.fm_last_error(e._ctx)

    def step(sp, st=state, d=dst, e=eng, sampled=None):
        s_, d_, fz = e._state_struct(st) if st is not None else fm_state(), e._dst_struct(d) if d is not None else fm_dst(), e._freeze_struct(sp)
        sm = None
        if sampled is not None:
            sm = iu.fm_sampled()
            sm.a1, sm.c1, sm.e1 = mu._ptr(sampled['a1']), mu._ptr(sampled['c1']), mu._ptr(sampled['e1'])
        return e.lib.fm_ctmc_step_freeze(e._ctx, e._stream(), C.byref(s_), C.byref(d_), None, C.byref(sc), C.byref(sm) if sm is not None else None, C.byref(fz), al)

    def integ(sp, G=1, st=state, sink=None, e=eng, scalars=None):
        s_, fz = e._state_struct(st) if st is not None else fm_state(), e._freeze_struct(sp)
        da, db = (e._dst_struct(dst), e._dst_struct(dst_b)) if st is not None else (fm_dst(), fm_dst())
        n = max(G, 1)
        each = list(scalars) if scalars is not None else [sc] * n
        scal, act = (fm_step_scalars * n)(*each), (C.c_int32 * n)(*([1] * n))
        dummy = torch.zeros(n * 256, dtype=torch.uint8, device=device)
        sk = None
        if sink is not None:
            sk = _lib.fm_traj_sink()
            for name, v in sink.items():
                setattr(sk, name, mu._ptr(v))
        al_h = (C.c_float * (4 * n))(*([0.6] * (4 * n)))
        return e.lib.fm_integrate_freeze(e._ctx, e._stream(), C.byref(s_), 1, G, scal, mu._ptr(dummy), act, mu._ptr(dummy), mu._ptr(dummy), mu._ptr(temb), None,
                                         None, C.byref(da), C.byref(db), C.byref(sk) if sk is not None else None, None, C.byref(fz), al_h, mu._ptr(dummy))

    for call in (step, integ):
        # a modality whose keep pointer is given while one of its path inputs is NULL
        for name, owner in (('x0', 'keep_x'), ('x1c', 'keep_x'), ('a1', 'keep_a'), ('u_a', 'keep_a'), ('c1', 'keep_c'), ('u_c', 'keep_c'), ('e1', 'keep_e'), ('u_e', 'keep_e')):
            assert call({**spec, name: None}) == -1 and b'NULL' in err() and name.encode() in err() and owner.encode() in err(), (call.__name__, name)
        # a member equal to a pointer of the call's own buffers
        for name, other in (('keep_x', dst['x']), ('x0', state['x_t']), ('x1c', dst['x']), ('a1', state['a_t']), ('c1', state['c_t']), ('e1', state['e_t']),
                            ('u_a', dst['a']), ('u_e', dst['e']), ('keep_e', state['e_t'])):
            assert call({**spec, name: other}) == -1 and b'alias' in err() and name.encode() in err(), (call.__name__, name)
    assert step({**spec, 'a1': smp['a1']}, sampled=smp) == -1 and b'alias' in err()
    assert integ({**spec, 'u_c': dst_b['c']}) == -1 and b'alias' in err()
    assert integ({**spec, 'x0': traj['x']}, sink={'x': traj['x']}) == -1 and b'alias' in err()
    assert integ({**spec, 'e1': traj['e1']}, sink={'e1': traj['e1']}) == -1 and b'alias' in err()
    for G in (0, -1, 33):
        assert integ(spec, G=G) == -1 and b'n_groups' in err(), G
    # n_groups > 1 keeps fm_integrate_mixed's refusals: a sink, gat, tensor noise, a NULL previous endpoint with only some groups at t = 0
    assert integ(spec, G=2, sink={'x': traj['x']}) == -1 and b'sink' in err()
    assert integ(spec, G=2, scalars=[sc, gat.scalars[1]]) == -1 and b'gat' in err()
    assert integ(spec, G=2, scalars=[sc, tensors.scalars[1]]) == -1 and b'FM_NOISE_TENSORS' in err()
    assert integ(spec, G=2, scalars=[plan.scalars[0], sc]) == -1 and b't = 0' in err()
    eng.synchronize()
    assert mu.first_difference(before, cpu(state)) is None          # a refused call enqueues nothing
    # a free modality's path inputs may be NULL, given or not: the conformer case passes no x0 and no x1c
    conf = {**spec, 'keep_x': None, 'x0': None, 'x1c': None}
    assert step(conf) == 0          # the context stays usable
    eng.synchronize()
    after = cpu(state)
    assert mu.first_difference(before, after) is not None
    end = mu.model('endpoint_small', lib, device).engine
    end.bind(torch.tensor(sizes))
    assert step(spec, None, None, end) == -1 and b'endpoint' in err(end)
    assert integ(spec, 1, None, None, end) == -1 and b'endpoint' in err(end)
    single = mu.engine('qm9', lib, device)[0]          # a batch without pairs: the pair members may be NULL whatever keep_e says
    single.bind(torch.tensor([1, 1]))
    s1 = ru.as_state(single, ru.given(cfg, [1, 1]))
    sp1 = single.freeze_spec(s1, {'x': torch.tensor([True, False]), 'a': torch.tensor([False, True]), 'e': torch.zeros(0, dtype=torch.bool)}, 1)
    st1 = single.conditional_path(s1, [0.5] * 4, seed=1)
    assert step(sp1, st1, iu.softmax_dst(single), single) == 0
    single.synchronize()


def _check_python_refusals(lib, device):
    mdl = mu.model('dev', lib, device)
    mols = ru.given(mdl.cfg, [3, 2])
    rng_state = torch.get_rng_state()
    ok = dict(seed=SEED, n_timesteps=3)
    atoms, pairs = [[True, False, True], [False, True]], [[True, False, True], [False]]
    good = {'a': atoms, 'e': pairs}
    queue = lambda: mdl.sampling_queue(seed=SEED)
    for bad in ({'b': atoms}, {'a': atoms, 'keep_e': pairs}, {0: atoms}):          # an unknown key
        with pytest.raises(ValueError, match='unknown'):
            mdl.resample(mols, 1, keep=bad, **ok)
        with pytest.raises(ValueError, match='unknown'):
            queue().submit_from(mols, 1, n_timesteps=3, keep=bad)
    for bad in ({'a': [[True, False], [False, True]]}, {'c': [[True, False, True]]}, {'x': torch.ones(4, dtype=torch.bool)}, {'e': atoms}, {'e': torch.ones(5, dtype=torch.bool)},
                {'a': atoms, 'e': [[True, False, True], []]}):          # a wrong length
        with pytest.raises(ValueError, match='keep'):
            mdl.resample(mols, 1, keep=bad, **ok)
        with pytest.raises(ValueError, match='keep'):
            queue().submit_from(mols, 1, n_timesteps=3, keep=bad)
    for bad in ({'a': torch.ones(5)}, {'x': torch.ones(5, dtype=torch.int64)}, {'c': [[1, 0, 1], [0, 1]]}, {'e': [[1.0, 0.0, 1.0], [0.0]]}, {'e': torch.ones(4, dtype=torch.uint8)}):
        with pytest.raises(ValueError, match='bool'):          # a dtype other than bool
            mdl.resample(mols, 1, keep=bad, **ok)
        with pytest.raises(ValueError, match='bool'):
            queue().submit_from(mols, 1, n_timesteps=3, keep=bad)
    with pytest.raises(NotImplementedError, match='endpoint'):
        mu.model('endpoint_small', lib, device).resample(mols, 1, keep=good, **ok)
    with pytest.raises(NotImplementedError, match='endpoint'):
        mu.model('endpoint_small', lib, device).conformers(mols, **ok)
    with pytest.raises(NotImplementedError, match='tspan'):
        mdl.resample(mols, 1, keep=good, tspan=torch.linspace(0, 1, 3), **ok)
    with pytest.raises(NotImplementedError, match='gat'):
        mdl.resample(mols, [1, 1], keep=good, dfm_type='gat', **ok)
    with pytest.raises(NotImplementedError, match='xt_traj / ep_traj'):
        mdl.resample(mols, [1, 2], n_timesteps=4, seed=SEED, keep=good, xt_traj=True)
    with pytest.raises(ValueError, match='seed'):
        mdl.conformers(mols, n_timesteps=3)
    eng = mdl.engine
    eng.bind(mols[1])
    x1 = ru.as_state(eng, mols)
    with pytest.raises(ValueError, match='unknown'):
        eng.freeze_spec(x1, {'q': torch.ones(5, dtype=torch.bool)}, SEED)
    with pytest.raises(ValueError, match='pairs'):
        eng.freeze_spec(x1, {'e': torch.ones(5, dtype=torch.bool)}, SEED)
    with pytest.raises(ValueError, match='freeze_spec'):
        eng.ctmc_step_freeze(None, None, None, None, eng.inpaint_spec(x1, torch.ones(5, dtype=torch.bool), SEED), [1.0] * 4)
    assert torch.equal(torch.get_rng_state(), rng_state)
    gat = fu.resample_tensors(mdl, mols, 1, 4, SEED, [0, 1], good, dfm_type='gat')          # gat with one (T, k): the single-schedule kernels take it
    given = mu.split_molecules(mols[0], [3, 2])
    for i, g in enumerate(gat):
        assert torch.equal(g['a'][torch.tensor(atoms[i])].long(), given[i]['a'][torch.tensor(atoms[i])].long())
        assert torch.equal(g['e'][torch.tensor(pairs[i])].long(), given[i]['e'][torch.tensor(pairs[i])].long())


def test_freeze_refusals_on_emulation(emu_lib):
    _check_c_refusals(emu_lib, 'cpu')
    _check_python_refusals(emu_lib, 'cpu')


@pytest.mark.gpu
def test_freeze_refusals_on_gpu():
    _check_c_refusals(None, 'cuda:0')
    _check_python_refusals(None, 'cuda:0')
