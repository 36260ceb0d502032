"""Resampling given molecules from a chosen step: the conditional path p(g_t | g_0, g_1) of the reference (CTMCVectorField.sample_conditional_path,
ctmc_vector_field.py:97-143) drawn inside one kernel from the per-molecule Philox streams (fm_conditional_path, Engine.conditional_path), then steps
k .. T-2 of the unchanged sampler (FlowMol.resample, SamplingQueue.submit_from).

What is checked.  (1) positions bit-exact against the reference's formula on the existing, pinned prior_philox and remove_com; (2) the uniforms against an
independently written numpy Philox (itself first checked against a stream the library already pins) and the tokens against the reference's rule;
(3) the limits alpha = 0 / 1 and what they mean through the API (start_step 0 is sample(), start_step T-1 the centred input); (4) a batch of mixed
(T, k) bit-identical to every molecule resampled alone, in any order; (5) runs replayed by the oracle from the corrupted state and the noise tapes;
(6) trajectory frames; (7) the queue; (8) a guarded call and the refusals.  All comparisons are torch.equal unless a tolerance is named.

Shapes.  Kernel-only checks (no network evaluation): the qm9 preset bound to 1, 2, 5, 24, 47 atoms -- 0 pairs, 1 pair, rows below, just above and far
above one 256-thread pass (276 and 1081 pairs) with a molecule boundary behind each -- in three time groups.  Trajectories: the narrow, self-conditioned
`dev` model with 5, 3, 2, 1 atoms; on the GPU also flowmol3 with 5 and 9 atoms.  Every check runs on the CPU emulation of the kernel sources and, marked
gpu, on the device."""
import ctypes as C

import pytest
import torch

from flowmol_amd import _lib
from flowmol_amd.engine import fm_state
from hygiene_util import cpu

import mixed_util as mu
import resample_util as ru

SEED = 2024
TRAJ_SIZES = ru.TRAJ_SIZES
MASK = lambda cfg: {'a': cfg.n_atom_types, 'c': cfg.n_charges, 'e': cfg.n_bond_types}


# ---------------------------------------------------------------------------------------------------------------- 1. positions
def _check_positions(lib, device):
    case = ru.kernel_case('qm9', lib, device)
    eng = ru.rebind(case)
    x0 = eng.prior_philox(case['seed']).cpu()
    x1c = eng.remove_com(case['x1']['x_t'].to(eng.device).clone()).cpu()
    assert torch.equal(case['tape']['x0'], x0)
    al = ru.node_alpha(case['sizes'], case['groups'], case['alphas'], 0).unsqueeze(-1)
    want = (1 - al) * x0 + al * x1c            # reference line 112, torch float32: three separately rounded operations
    assert torch.equal(case['out']['x_t'], want)
    assert torch.equal(case['out']['x_t'][0], torch.zeros(3))          # the 1-atom molecule: exact zeros
    assert float((want - x0).abs().max()) > 0.1 and float((want - x1c).abs().max()) > 0.1


def test_conditional_path_positions_are_the_reference_formula_on_emulation(emu_lib):
    _check_positions(emu_lib, 'cpu')


@pytest.mark.gpu
def test_conditional_path_positions_are_the_reference_formula_on_gpu():
    _check_positions(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 2. tokens
def _check_numpy_philox(lib, device):
    """The numpy Philox against a stream today's library pins: u1 of a campbell step = fm_u01(word 0 of block 4) of (gid, row, step * 4 + job)."""
    mdl = mu.model('qm9', lib, device)
    eng = mdl.engine
    sizes, ids, step = [5, 2, 24], [9, 70000, 4], 3
    eng.bind(torch.tensor(sizes))
    eng.set_molecule_ids(torch.tensor(ids))
    nz = eng.philox_tape(mu.philox_plans(mdl, [6], SEED)[0], step)
    for job, tag in enumerate('ace'):
        assert torch.equal(getattr(nz, f'u1_{tag}').cpu(), ru.row_uniforms(sizes, ids, job, SEED, step * 4 + job, 4)), tag
        assert torch.equal(getattr(nz, f'u2_{tag}').cpu(), ru.row_uniforms(sizes, ids, job, SEED, step * 4 + job, 4, word=1)), tag


def _check_tokens(lib, device):
    _check_numpy_philox(lib, device)
    case = ru.kernel_case('qm9', lib, device)
    cfg = case['cfg']
    for job, tag in enumerate('ace'):
        u = ru.row_uniforms(case['sizes'], case['ids'], job, case['seed'], 0xFFFFFFFE - job, 8)          # the new stream entry
        assert torch.equal(case['tape'][f'u_{tag}'], u), tag
        al = ru.node_alpha(case['sizes'], case['groups'], case['alphas'], 1 + job)
        tok1 = case['x1'][f'{tag}_t']
        want = torch.where(u < 1 - al, torch.full_like(tok1, MASK(cfg)[tag]), tok1)          # reference lines 126 / 134
        assert torch.equal(case['out'][f'{tag}_t'], want), tag
        assert 0 < int((want == MASK(cfg)[tag]).sum()) < want.numel()


def _check_uniform_mean(lib, device):
    eng, cfg, _ = mu.engine('qm9', lib, device)
    sizes = [50] * 40
    eng.bind(torch.tensor(sizes))
    eng.set_molecule_ids(None)
    _, tape = eng.conditional_path(ru.as_state(eng, ru.given(cfg, sizes)), [0.5] * 4, seed=SEED, tape=True)
    u = tape['u_e'].cpu()
    assert u.numel() == 49000 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert abs(float(u.double().mean()) - 0.5) < 0.01          # 7 standard errors of the mean of 49,000 uniforms


def test_conditional_path_tokens_follow_the_reference_rule_on_emulation(emu_lib):
    _check_tokens(emu_lib, 'cpu')
    _check_uniform_mean(emu_lib, 'cpu')


@pytest.mark.gpu
def test_conditional_path_tokens_follow_the_reference_rule_on_gpu():
    _check_tokens(None, 'cuda:0')
    _check_uniform_mean(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 3. limits
def _check_limits(lib, device):
    case = ru.kernel_case('qm9', lib, device)
    cfg, eng = case['cfg'], ru.rebind(case)
    x0 = eng.prior_philox(case['seed']).cpu()
    x1c = eng.remove_com(case['x1']['x_t'].to(eng.device).clone()).cpu()
    n, al = torch.tensor(case['sizes']), torch.tensor(case['alphas'])
    grp = torch.tensor(case['groups'])
    node_g, pair_g = grp.repeat_interleave(n), grp.repeat_interleave(n * (n - 1) // 2)
    for col, tag in enumerate('xace'):
        rows_g = pair_g if tag == 'e' else node_g
        zero, one = (al[rows_g, col] == 0.0), (al[rows_g, col] == 1.0)
        assert bool(zero.any()) and bool(one.any())
        got = case['out'][f'{tag}_t']
        if tag == 'x':
            assert torch.equal(got[zero], x0[zero]) and torch.equal(got[one], x1c[one])
        else:
            assert bool((got[zero] == MASK(cfg)[tag]).all()) and torch.equal(got[one], case['x1'][f'{tag}_t'][one])


def _check_api_limits(lib, device, preset='dev', T=4):
    mdl = mu.model(preset, lib, device)
    mols, ids = ru.given(mdl.cfg, TRAJ_SIZES), [5, 0, 9, 2]
    first = ru.resample_tensors(mdl, mols, 0, T, SEED, ids)
    out = mdl.sample(mols[1], n_timesteps=T, rng='philox', seed=SEED, mol_ids=ids, return_tensors=True)[0]
    assert mu.molecule_differences(first, mu.split_molecules(out, TRAJ_SIZES)) == []
    assert mu.moved_from_prior(first, mdl.cfg)
    last = ru.resample_tensors(mdl, mols, T - 1, T, SEED, ids)
    assert mu.molecule_differences(last, ru.centred(mdl.engine, mols)) == []


def test_conditional_path_limits_on_emulation(emu_lib):
    _check_limits(emu_lib, 'cpu')
    _check_api_limits(emu_lib, 'cpu')


@pytest.mark.gpu
def test_conditional_path_limits_on_gpu():
    _check_limits(None, 'cuda:0')
    _check_api_limits(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 4. composition independence
PAIRS_A = [(12, 0), (12, 5), (9, 5), (4, 3)]          # (T, k) per molecule: one at step 0 (an engine call of its own), one that only gets corrupted
PAIRS_B = [(6, 2), (4, 3), (12, 0), (9, 5)]


def _check_composition(preset, lib, device, sizes, pairs, tuning=None, tag='traj'):
    mdl = mu.model(preset, lib, device, **(tuning or {}))
    mols, ids = ru.given(mdl.cfg, sizes), [3 + 2 * i for i in range(len(sizes))]
    Ts, ks = [T for T, _ in pairs], [k for _, k in pairs]
    want = ru.alone_runs(preset, lib, device, mols, ks, Ts, SEED, ids, tag)
    got = ru.resample_tensors(mdl, mols, ks, Ts, SEED, ids)
    assert mu.molecule_differences(got, want) == []
    order = list(range(len(sizes)))[::-1]
    back = ru.resample_tensors(mdl, ru.take(mols, order), [ks[i] for i in order], [Ts[i] for i in order], SEED, [ids[i] for i in order])
    assert mu.molecule_differences(back, [want[i] for i in order]) == []
    given = mu.split_molecules(mols[0], sizes)
    assert any(not torch.equal(g[f].long(), w[f].long()) for g, w in zip(got, given) for f in 'ace')          # some token moved from the input


def test_resample_batch_equals_every_molecule_alone_on_emulation(emu_lib):
    _check_composition('dev', emu_lib, 'cpu', TRAJ_SIZES, PAIRS_A)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['pairs_a', 'pairs_b', 'threads256', 'threads1024', 'flowmol3'])
def test_resample_batch_equals_every_molecule_alone_on_gpu(case):
    if case == 'flowmol3':
        _check_composition('flowmol3', None, 'cuda:0', [5, 9], [(5, 2), (4, 0)], tag='fm3')
    else:
        tuning = {'threads256': {'ctmc_threads': 256}, 'threads1024': {'ctmc_threads': 1024}}.get(case)
        _check_composition('dev', None, 'cuda:0', TRAJ_SIZES, PAIRS_B if case == 'pairs_b' else PAIRS_A, tuning=tuning)


# ---------------------------------------------------------------------------------------------------------------- 5. anchored to the oracle
def _check_oracle(preset, lib, device, sizes, pairs):
    """Every molecule alone: the oracle integrates the conditional-path state over linspace(0, 1, T)[k:] with the molecule's noise tapes; resample must give
    its tokens, and its coordinates within 1e-5 of the largest coordinate (the tolerance of test_mixed_time's oracle-anchored trajectory)."""
    mdl = mu.model(preset, lib, device)
    assert mdl.cfg.self_conditioning and any(k > 0 for _, k in pairs)      # the first evaluation runs without a previous endpoint on both sides
    mols = ru.given(mdl.cfg, sizes)
    for i, (n, (T, k)) in enumerate(zip(sizes, pairs)):
        one = ru.take(mols, [i])
        _, want, _ = ru.oracle_from_state(mdl, [n], [i], one, k, T, SEED)
        got = ru.resample_tensors(mdl, one, k, T, SEED, [i])[0]
        for f in 'ace':
            assert torch.equal(got[f].int(), want[f]), (i, f)
        err = float((got['x'] - want['x']).abs().max() / want['x'].abs().max())
        assert err < 1e-5, (i, err)


def test_resample_replayed_by_the_oracle_on_emulation(emu_lib):
    _check_oracle('dev', emu_lib, 'cpu', [5, 3, 2], [(6, 2), (5, 1), (4, 2)])


@pytest.mark.gpu
@pytest.mark.parametrize('preset', ['dev', 'flowmol3'])
def test_resample_replayed_by_the_oracle_on_gpu(preset):
    if preset == 'dev':
        _check_oracle('dev', None, 'cuda:0', [5, 3, 2], [(6, 2), (5, 1), (4, 2)])
    else:
        _check_oracle('flowmol3', None, 'cuda:0', [5, 9], [(5, 2), (4, 1)])


# ---------------------------------------------------------------------------------------------------------------- 6. trajectories
def _check_frames(lib, device, T=6, k=2):
    mdl = mu.model('dev', lib, device)
    mols, ids = ru.given(mdl.cfg, TRAJ_SIZES), [4, 1, 8, 6]
    state, want, ref = ru.oracle_from_state(mdl, TRAJ_SIZES, ids, mols, k, T, SEED, visualize=True)
    got = mdl.resample(mols, k, n_timesteps=T, seed=SEED, mol_ids=ids, xt_traj=True, ep_traj=True)
    plain = ru.resample_tensors(mdl, mols, k, T, SEED, ids)
    frames = {f: torch.cat([m.traj_frames[f] for m in got], dim=1) for f in 'xace'}
    for f in 'xace':
        assert frames[f].shape[0] == T - k, f
        assert torch.equal(frames[f][0], state[f'{f}_t'].to(frames[f].dtype)), f          # frame 0: the corrupted state
        assert torch.equal(frames[f][-1], torch.cat([p[f] for p in plain]).to(frames[f].dtype)), f          # last frame: the result
    for f in 'ace':
        assert torch.equal(frames[f].long(), ref[f].long()), f
        assert torch.equal(frames[f][-1].int(), want[f]), f
        assert got[0].traj_frames[f'{f}_1_pred'].shape[0] == T - k - 1
    assert float((frames['x'] - ref['x']).abs().max() / ref['x'].abs().max()) < 1e-5
    for m, p in zip(got, plain):
        assert torch.equal(m.x_1, p['x']) and torch.equal(m.e_1, p['e'].long())
    only = mdl.resample(mols, T - 1, n_timesteps=T, seed=SEED, mol_ids=ids, xt_traj=True)          # nothing to integrate: one frame
    assert only[0].traj_frames['x'].shape[0] == 1


def test_resample_trajectory_frames_on_emulation(emu_lib):
    _check_frames(emu_lib, 'cpu')


@pytest.mark.gpu
def test_resample_trajectory_frames_on_gpu():
    _check_frames(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 7. queue
def _queue_run(mdl, mol, order):
    """[9, 5] at T = 8 (ids 0, 1), three steps, then the given molecule from step 2 of T = 5 (id 7), until idle."""
    q = mdl.sampling_queue(seed=SEED)
    if order == 'a':
        t9, t5 = q.submit([9, 5], n_timesteps=8, mol_ids=[0, 1])
    else:
        (t5,) = q.submit([5], n_timesteps=8, mol_ids=[1])
        (t9,) = q.submit([9], n_timesteps=8, mol_ids=[0])
    assert q.run(max_steps=3) == 3 and q.pop_finished() == {}
    (tm,) = q.submit_from(mol, start_step=2, n_timesteps=5, mol_ids=[7])
    done, calls = {}, 0
    while not q.idle:
        assert q.run() > 0 and calls < 8
        calls += 1
        done.update(q.pop_finished())
    assert sorted(done) == sorted([t9, t5, tm]) and q.pop_finished() == {}
    return [{'x': done[t].x_1, 'a': done[t].a_1, 'c': done[t].c_1, 'e': done[t].e_1} for t in (t9, t5, tm)]


def _check_queue(lib, device):
    mdl = mu.model('dev', lib, device)
    mol = ru.given(mdl.cfg, [12])
    want = mu.alone_runs('dev', lib, device, [9, 5], [8, 8], SEED) + [ru.resample_alone(mdl, mol, 0, 2, 5, SEED, 7)]
    first = _queue_run(mdl, mol, 'a')
    assert mu.molecule_differences(first, want) == []
    assert mu.molecule_differences(_queue_run(mdl, mol, 'b'), first) == []
    q = mdl.sampling_queue(seed=SEED)          # start_step = T - 1 retires at once with the corrupted (= centred) molecule
    (t,) = q.submit_from(mol, start_step=4, n_timesteps=5, mol_ids=[7])
    assert q.run() == 0 and q.idle
    m = q.pop_finished()[t]
    assert mu.molecule_differences([{'x': m.x_1, 'a': m.a_1, 'c': m.c_1, 'e': m.e_1}], ru.centred(mdl.engine, mol)) == []


def test_queue_admits_given_molecules_on_emulation(emu_lib):
    _check_queue(emu_lib, 'cpu')


@pytest.mark.gpu
def test_queue_admits_given_molecules_on_gpu():
    _check_queue(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 8. hygiene and refusals
def _check_guarded_call(lib, device):
    eng, _, _ = mu.engine('qm9', lib, device)
    case = ru.kernel_case('qm9', lib, device)
    args = (case['sizes'], case['groups'], case['alphas'], case['seed'])
    zero, bad, intact, unwritten = ru.guarded_conditional_path(eng, *args, 'zero', case['ids'])
    assert bad == [] and intact and unwritten == []
    ones, bad, intact, unwritten = ru.guarded_conditional_path(eng, *args, 'ones', case['ids'])          # every f32 of the arena a NaN
    assert bad == [] and intact and unwritten == []
    assert mu.first_difference(zero, ones) is None
    assert mu.first_difference(zero, {**case['out'], **case['tape']}) is None


def _check_c_refusals(lib, device):
    eng, cfg, _ = mu.engine('qm9', lib, device)
    eng.bind(torch.tensor([3, 2]))
    x1 = ru.as_state(eng, ru.given(cfg, [3, 2]))
    out = {k: torch.empty_like(v) for k, v in x1.items()}
    al = torch.full((2, 4), 0.5, device=device)
    group = torch.zeros(2, dtype=torch.int32, device=device)
    err = lambda e=eng: e.lib.fm_last_error(e._ctx)
    call = lambda s1, so, G, grp, e=eng: e.lib.fm_conditional_path(e._ctx, e._stream(), C.c_uint64(1), C.byref(s1), G, mu._ptr(grp), mu._ptr(al), C.byref(so), None)
    s1, so = eng._state_struct(x1), eng._state_struct(out)
    assert call(s1, so, 0, group) == -1 and b'n_groups' in err()
    assert call(s1, so, 2, None) == -1 and b'mol_group' in err()
    for f in ('x_t', 'a_t', 'c_t', 'e_t'):
        assert call(s1, eng._state_struct({**out, f: x1[f]}), 1, None) == -1 and b'alias' in err() and f.encode() in err(), f
    assert call(s1, so, 1, None) == 0          # the context stays usable
    eng.synchronize()
    end = mu.model('endpoint_small', lib, device).engine
    end.bind(torch.tensor([3, 2]))
    assert call(fm_state(), fm_state(), 1, None, end) == -1 and b'endpoint' in err(end)


def _check_python_refusals(lib, device):
    mdl = mu.model('dev', lib, device)
    cfg = mdl.cfg
    mols = ru.given(cfg, [3, 2])
    rng_state = torch.get_rng_state()
    ok = dict(seed=SEED)
    with pytest.raises(NotImplementedError, match='endpoint'):
        mu.model('endpoint_small', lib, device).resample(mols, 1, n_timesteps=3, **ok)
    with pytest.raises(NotImplementedError, match='gat'):
        mdl.resample(mols, [1, 1], n_timesteps=3, dfm_type='gat', **ok)
    with pytest.raises(NotImplementedError, match='gat'):
        mdl.resample(mols, 1, n_timesteps=[3, 3], dfm_type='gat', **ok)
    with pytest.raises(NotImplementedError, match='tspan'):
        mdl.resample(mols, 1, n_timesteps=3, tspan=torch.linspace(0, 1, 3), **ok)
    with pytest.raises(NotImplementedError, match='xt_traj / ep_traj'):
        mdl.resample(mols, [1, 2], n_timesteps=4, xt_traj=True, **ok)
    with pytest.raises(NotImplementedError, match='xt_traj / ep_traj'):
        mdl.resample(mols, 1, n_timesteps=[3, 4], ep_traj=True, **ok)
    many = ru.given(cfg, [2] * 33)
    with pytest.raises(NotImplementedError, match='distinct'):
        mdl.resample(many, 1, n_timesteps=list(range(3, 36)), **ok)
    with pytest.raises(TypeError, match='rng'):
        mdl.resample(mols, 1, n_timesteps=3, rng='philox', **ok)
    with pytest.raises(TypeError, match='bogus'):
        mdl.resample(mols, 1, n_timesteps=3, bogus=1, **ok)
    with pytest.raises(ValueError, match='seed'):
        mdl.resample(mols, 1, n_timesteps=3)
    for k, T in ((-1, 3), (3, 3), ([0, 4], [3, 4])):
        with pytest.raises(ValueError, match='start_step'):
            mdl.resample(mols, k, n_timesteps=T, **ok)
    with pytest.raises(ValueError, match='one entry per molecule'):
        mdl.resample(mols, [1, 1, 1], n_timesteps=3, **ok)
    for f, K in (('a', cfg.n_atom_types), ('c', cfg.n_charges), ('e', cfg.n_bond_types)):
        for bad_tok in (K, K + 3, -1):          # the mask token, out of range
            t = {k: v.clone() for k, v in mols[0].items()}
            t[f][0] = bad_tok
            with pytest.raises(ValueError, match='real categories'):
                mdl.resample((t, mols[1]), 1, n_timesteps=3, **ok)
            with pytest.raises(ValueError, match='real categories'):
                mdl.sampling_queue(seed=SEED).submit_from((t, mols[1]), 1, n_timesteps=3)
    assert torch.equal(torch.get_rng_state(), rng_state)


def test_conditional_path_call_between_guard_bands_on_emulation(emu_lib):
    _check_guarded_call(emu_lib, 'cpu')


@pytest.mark.gpu
def test_conditional_path_call_between_guard_bands_on_gpu():
    _check_guarded_call(None, 'cuda:0')


def test_resample_refusals_on_emulation(emu_lib):
    _check_c_refusals(emu_lib, 'cpu')
    _check_python_refusals(emu_lib, 'cpu')


@pytest.mark.gpu
def test_resample_refusals_on_gpu():
    _check_c_refusals(None, 'cuda:0')
    _check_python_refusals(None, 'cuda:0')
