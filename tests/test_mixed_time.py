"""Per-molecule time: one batch whose molecules sit at different times (fm_forward_mixed), follow schedules of different lengths (fm_integrate_mixed,
FlowMol.sample with one step count per molecule) and join while it runs (SamplingQueue).

What is checked.  (1) a mixed-time evaluation against the oracle's forward with the reference's (B,) time, under the gates of the parity tests;
(2) every molecule of it bit-identical to the molecule evaluated alone through the existing forward; (3) mixed trajectories bit-identical to every
molecule sampled alone; (4) one mixed trajectory replayed by the oracle from the molecules' noise tapes; (5) the queue; (6) refusals and a guarded call.
All comparisons are torch.equal unless a gate is named.

Shapes.  Forward: molecules of 5, 9, 12, 3, 2 atoms (one 4-row node tile holds rows of up to three molecules, i.e. three table slots) at five distinct times;
on the GPU also 24 x 47 atoms (N = 1128: the regular 16-row MLP tiles instead of the 4-row ones) at three times under both edge tile heights.
Trajectories: the narrow `dev` model, 5, 3, 2, 1 atoms with 12, 4, 9, 2 time points: four time groups, i.e. 8 steps per table launch and a launch boundary
inside the 11 steps, a molecule without edges, one whose step 0 is its last, and three that finish early and wait.  GPU only: molecules of 47, 5, 70
atoms (more pair rows than a 1024-thread workgroup) and 33 molecules in 8 groups (4 steps per table launch).

Every check runs on the CPU emulation of the kernel sources and, marked gpu, on the device.  An emulated evaluation costs 0.6 .. 2 s whatever the
molecule, so the emulation runs a selection: the forward checks, the base trajectory case (its alone runs are shared), the oracle-anchored trajectory, the
queue and the guarded call; the remaining trajectory cases (other stochasticity, the uniform-unmasking branch, the second workgroup size, flowmol3) run
on the GPU, where they take a fraction of a second."""
import ctypes as C

import pytest
import torch

from flowmol_amd import _lib
from flowmol_amd.engine import fm_dst, fm_state, fm_step_scalars
from oracle import cpu_ref
from parity_util import OUT_TOL, STAGE_TOL, out_of_tolerance

import mixed_util as mu

SEED = 2024
TRAJ_SIZES, TRAJ_T = [5, 3, 2, 1], [12, 4, 9, 2]


# ---------------------------------------------------------------------------------------------------------------- 1. forward against the oracle
def _check_forward_oracle(preset, lib, device):
    case = mu.forward_case(preset, lib, device)
    bad = out_of_tolerance(mu.oracle_errors(case, dx=False), None, STAGE_TOL, OUT_TOL)
    assert not bad, bad
    vis = mu.forward_case(preset, lib, device, visible=True)
    gates = mu.dx_gates_t(vis['cfg'], vis['sd'], vis['inp'], vis['t'])
    errs = mu.oracle_errors(vis, dx=True)
    assert any(k.startswith('upd') and k.endswith('.dx') for k in errs) and 'out.dx' in errs
    bad = out_of_tolerance(errs, gates, STAGE_TOL, OUT_TOL)
    assert not bad, (bad, gates)


@pytest.mark.parametrize('preset', ['flowmol3', 'geom_ctmc'])
def test_mixed_forward_matches_oracle_on_emulation(emu_lib, preset):
    _check_forward_oracle(preset, emu_lib, 'cpu')


@pytest.mark.gpu
@pytest.mark.parametrize('preset', ['flowmol3', 'geom_ctmc'])
def test_mixed_forward_matches_oracle_on_gpu(preset):
    _check_forward_oracle(preset, None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 2. forward, bit identity
@pytest.mark.parametrize('preset', ['flowmol3', 'geom_ctmc'])
def test_mixed_forward_equals_every_molecule_alone_on_emulation(emu_lib, preset):
    assert mu.alone_differences(mu.forward_case(preset, emu_lib, 'cpu')) == []


@pytest.mark.gpu
@pytest.mark.parametrize('preset', ['flowmol3', 'geom_ctmc'])
def test_mixed_forward_equals_every_molecule_alone_on_gpu(preset):
    assert mu.alone_differences(mu.forward_case(preset, None, 'cuda:0')) == []


@pytest.mark.gpu
@pytest.mark.parametrize('tile_edge', [16, 32])
def test_mixed_forward_equals_every_molecule_alone_on_regular_tiles_on_gpu(tile_edge):
    case = mu.forward_case('flowmol3', None, 'cuda:0', sizes=[47] * 24, times=[0.2, 0.55, 0.85] * 8, tile_edge=tile_edge)
    assert mu.alone_differences(case) == []


# ---------------------------------------------------------------------------------------------------------------- 3. trajectories
def _check_trajectories(preset, lib, device, sizes, Ts, tuning=None, **kw):
    mdl = mu.model(preset, lib, device, **(tuning or {}))
    out = mdl.sample(torch.tensor(sizes), n_timesteps=Ts, rng='philox', seed=SEED, return_tensors=True, **kw)[0]
    got = mu.split_molecules(out, sizes)
    want = mu.alone_runs(preset, lib, device, sizes, Ts, SEED, **kw)
    assert mu.molecule_differences(got, want) == []
    assert mu.moved_from_prior(got, mdl.cfg)


def test_mixed_trajectories_equal_alone_on_emulation(emu_lib):
    """The mixed run on the 256-thread instance of the fused CTMC kernel, the alone runs on the automatic choice (1024 threads for a few molecules)."""
    _check_trajectories('dev', emu_lib, 'cpu', TRAJ_SIZES, TRAJ_T, tuning={'ctmc_threads': 256})


GPU_TRAJ_CASES = {
    'base': ('dev', TRAJ_SIZES, TRAJ_T, {}, {}),
    'remasking': ('dev', TRAJ_SIZES, TRAJ_T, {}, {'stochasticity': 45.0}),        # stochasticity > 0: re-masking with every molecule's own dt
    'uniform_unmasking': ('dev', TRAJ_SIZES, TRAJ_T, {}, {'high_confidence_threshold': 0.0}),
    'threads256': ('dev', TRAJ_SIZES, TRAJ_T, {'ctmc_threads': 256}, {}),
    'threads1024': ('dev', TRAJ_SIZES, TRAJ_T, {'ctmc_threads': 1024}, {}),
    'flowmol3': ('flowmol3', [5, 9], [3, 5], {}, {}),
    'flowmol3_large': ('flowmol3', [47, 5, 70], [12, 33, 20], {}, {}),
    'eight_groups': ('flowmol3', [3] * 33, [(2, 3, 5, 6, 7, 9, 11, 13)[(i * 5) % 8] for i in range(33)], {}, {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(GPU_TRAJ_CASES))
def test_mixed_trajectories_equal_alone_on_gpu(case):
    preset, sizes, Ts, tuning, kw = GPU_TRAJ_CASES[case]
    _check_trajectories(preset, None, 'cuda:0', sizes, Ts, tuning=tuning, **kw)


# ---------------------------------------------------------------------------------------------------------------- 4. oracle-anchored trajectory
def _check_oracle_trajectory(lib, device, sizes=(5, 3, 2), Ts=(6, 4, 9)):
    """Every molecule's noise tape, written with the molecule bound alone, drives the oracle's integrate on a batch of one; the mixed run must give its
    tokens, and its coordinates within 1e-5 of the largest coordinate."""
    mdl = mu.model('dev', lib, device)
    eng, cfg = mdl.engine, mdl.cfg
    orc = cpu_ref.OracleVF(cfg, mdl._sd, prefix=mdl._prefix)
    want = []
    for i, (n, T) in enumerate(zip(sizes, Ts)):
        eng.bind(torch.tensor([n]))
        eng.set_molecule_ids(torch.tensor([i]))
        x0 = eng.prior_philox(SEED).cpu()
        plan = mu.philox_plans(mdl, [T], SEED)[0]
        tape = []
        for s in range(T - 1):
            nz = eng.philox_tape(plan, s)
            for tag in 'ace':
                tape += [getattr(nz, f'{f}_{tag}').cpu() for f in ('q', 'u1', 'u2') if getattr(nz, f'{f}_{tag}') is not None]
        batch = cpu_ref.build_batch(torch.tensor([n]))
        prior = {'x_0': x0, 'a_0': cpu_ref.ctmc_masked_prior(batch.N, cfg.n_atom_types), 'c_0': cpu_ref.ctmc_masked_prior(batch.N, cfg.n_charges),
                 'e_0': cpu_ref.edge_prior(batch.upper_edge_mask, cfg.n_bond_types)}
        noise = cpu_ref.TapeNoise(tape)
        with torch.no_grad():
            ref = orc.integrate(batch, prior, T, noise=noise)
        assert noise.pos == len(tape)
        m = batch.upper_edge_mask
        want.append({'x': ref['x_1'], 'a': ref['a_1'].argmax(-1).int(), 'c': ref['c_1'].argmax(-1).int(), 'e': ref['e_1'][m].argmax(-1).int()})
    out = mdl.sample(torch.tensor(sizes), n_timesteps=list(Ts), rng='philox', seed=SEED, return_tensors=True)[0]
    for i, (g, w) in enumerate(zip(mu.split_molecules(out, sizes), want)):
        for k in 'ace':
            assert torch.equal(g[k].int(), w[k]), (i, k)
        err = float((g['x'] - w['x']).abs().max() / w['x'].abs().max())
        assert err < 1e-5, (i, err)


def test_mixed_trajectory_replayed_by_the_oracle_on_emulation(emu_lib):
    _check_oracle_trajectory(emu_lib, 'cpu')


@pytest.mark.gpu
def test_mixed_trajectory_replayed_by_the_oracle_on_gpu():
    _check_oracle_trajectory(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 5. queue
def _queue_run(mdl, order):
    """[9, 5] at T = 8 (ids 0, 1), three steps, then [12] at T = 5 (id 2), until idle.  order 'b': the first submission as two calls, swapped."""
    q = mdl.sampling_queue(seed=SEED)
    if order == 'a':
        t9, t5 = q.submit([9, 5], n_timesteps=8, mol_ids=[0, 1])
    else:
        (t5,) = q.submit([5], n_timesteps=8, mol_ids=[1])
        (t9,) = q.submit([9], n_timesteps=8, mol_ids=[0])
    assert q.run(max_steps=3) == 3 and q.pop_finished() == {}
    (t12,) = q.submit([12], n_timesteps=5, mol_ids=[2])
    done, calls = {}, 0
    while not q.idle:
        assert q.run() > 0 and calls < 8
        calls += 1
        done.update(q.pop_finished())
    assert sorted(done) == sorted([t9, t5, t12]) and q.pop_finished() == {}
    return [{'x': done[t].x_1, 'a': done[t].a_1, 'c': done[t].c_1, 'e': done[t].e_1} for t in (t9, t5, t12)]


def _check_queue(lib, device):
    mdl = mu.model('dev', lib, device)
    want = mu.alone_runs('dev', lib, device, [9, 5, 12], [8, 8, 5], SEED)
    first = _queue_run(mdl, 'a')
    assert mu.molecule_differences(first, want) == []
    assert mu.molecule_differences(_queue_run(mdl, 'b'), first) == []
    assert mu.moved_from_prior(first, mdl.cfg)


def test_queue_admits_into_a_running_batch_on_emulation(emu_lib):
    _check_queue(emu_lib, 'cpu')


@pytest.mark.gpu
def test_queue_admits_into_a_running_batch_on_gpu():
    _check_queue(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 6. refusals and hygiene
def _check_c_refusals(lib, device):
    mdl = mu.model('dev', lib, device)
    eng = mdl.engine
    eng.bind(torch.tensor([3, 2]))
    state = eng.prior_state(torch.zeros(eng.N, 3))
    st, d0, d1 = eng._state_struct(state), eng._dst_struct(eng.new_dst()), eng._dst_struct(eng.new_dst())
    G = _lib.FM_TAB_SLOTS + 1
    temb = torch.zeros(G, eng.cfg.time_embedding_dim, device=device)
    group = torch.zeros(eng.B, dtype=torch.int32, device=device)
    rc = eng.lib.fm_forward_mixed(eng._ctx, eng._stream(), C.byref(st), mu._ptr(temb), G, mu._ptr(group), None, 0, 1, C.byref(d0))
    assert rc == -1 and b'n_groups' in eng.lib.fm_last_error(eng._ctx)           # FM_ERR_INVALID
    scal, act = (fm_step_scalars * G)(), (C.c_int32 * G)()
    dev_bytes = torch.zeros(C.sizeof(scal), dtype=torch.uint8, device=device)
    args = lambda n_groups, sc, sink=None: (eng._ctx, eng._stream(), C.byref(st), 1, n_groups, sc, mu._ptr(dev_bytes), act, mu._ptr(dev_bytes), mu._ptr(group),
                                             mu._ptr(temb), None, C.byref(d0), C.byref(d1), sink, None)
    assert eng.lib.fm_integrate_mixed(*args(G, scal)) == -1 and b'n_groups' in eng.lib.fm_last_error(eng._ctx)
    from flowmol_amd.engine import fm_traj_sink
    assert eng.lib.fm_integrate_mixed(*args(1, scal, C.byref(fm_traj_sink()))) == -1 and b'sink' in eng.lib.fm_last_error(eng._ctx)
    act[0] = 1
    scal[0].dfm_type, scal[0].noise_mode = _lib.FM_DFM_GAT, _lib.FM_NOISE_PHILOX
    assert eng.lib.fm_integrate_mixed(*args(1, scal)) == -1 and b'gat' in eng.lib.fm_last_error(eng._ctx)
    scal[0].dfm_type, scal[0].noise_mode = _lib.FM_DFM_CAMPBELL, _lib.FM_NOISE_TENSORS
    assert eng.lib.fm_integrate_mixed(*args(1, scal)) == -1 and b'FM_NOISE_TENSORS' in eng.lib.fm_last_error(eng._ctx)
    # prev0 == NULL with one active group at t = 0 and one later
    act[1] = 1
    for k, t in ((0, 0.0), (1, 0.5)):
        scal[k].dfm_type, scal[k].noise_mode, scal[k].t = _lib.FM_DFM_CAMPBELL, _lib.FM_NOISE_PHILOX, t
    assert eng.lib.fm_integrate_mixed(*args(2, scal)) == -1 and b't = 0' in eng.lib.fm_last_error(eng._ctx)
    eng.synchronize()
    # endpoint models
    end = mu.model('endpoint_small', lib, device).engine
    end.bind(torch.tensor([3, 2]))
    temb1 = torch.zeros(1, end.cfg.time_embedding_dim, device=device)
    rc = end.lib.fm_forward_mixed(end._ctx, end._stream(), C.byref(fm_state()), mu._ptr(temb1), 1, mu._ptr(group), None, 0, 1, C.byref(fm_dst()))
    assert rc == -1 and b'endpoint' in end.lib.fm_last_error(end._ctx)


def _check_python_refusals(lib, device):
    mdl = mu.model('dev', lib, device)
    sizes, Ts = torch.tensor([3, 2]), [3, 2]
    ok = dict(rng='philox', seed=SEED)
    with pytest.raises(NotImplementedError, match="rng='torch'"):
        mdl.sample(sizes, n_timesteps=Ts)
    with pytest.raises(NotImplementedError, match='gat'):
        mdl.sample(sizes, n_timesteps=Ts, dfm_type='gat', **ok)
    with pytest.raises(NotImplementedError, match='xt_traj / ep_traj'):
        mdl.sample(sizes, n_timesteps=Ts, xt_traj=True, **ok)
    with pytest.raises(NotImplementedError, match='xt_traj / ep_traj'):
        mdl.sample(sizes, n_timesteps=Ts, ep_traj=True, **ok)
    with pytest.raises(NotImplementedError, match='distinct step counts'):
        mdl.sample(torch.tensor([2] * 33), n_timesteps=list(range(2, 35)), **ok)
    with pytest.raises(NotImplementedError, match='sample_distributed with a sequence'):
        mdl.sample_distributed(sizes, n_timesteps=Ts, noise='philox')
    with pytest.raises(NotImplementedError, match='endpoint'):
        mu.model('endpoint_small', lib, device).sample(sizes, n_timesteps=Ts, **ok)
    with pytest.raises(NotImplementedError, match='endpoint'):
        mu.model('endpoint_small', lib, device).sampling_queue(seed=SEED)


def test_mixed_refusals_on_emulation(emu_lib):
    _check_c_refusals(emu_lib, 'cpu')
    _check_python_refusals(emu_lib, 'cpu')


@pytest.mark.gpu
def test_mixed_refusals_on_gpu():
    _check_c_refusals(None, 'cuda:0')
    _check_python_refusals(None, 'cuda:0')


def _check_guarded_call(lib, device, sizes=(4, 3, 2), Ts=(4, 2, 3)):
    mdl = mu.model('dev', lib, device)
    zero, bad, intact = mu.guarded_mixed_run(mdl, list(sizes), list(Ts), SEED, 'zero')
    assert bad == [] and intact
    ones, bad, intact = mu.guarded_mixed_run(mdl, list(sizes), list(Ts), SEED, 'ones')        # every f32 of the arena a NaN
    assert bad == [] and intact
    assert mu.first_difference(zero, ones) is None
    got = mu.split_molecules(zero, sizes)
    assert mu.molecule_differences(got, mu.alone_runs('dev', lib, device, list(sizes), list(Ts), SEED)) == []


def test_mixed_call_between_guard_bands_on_emulation(emu_lib):
    _check_guarded_call(emu_lib, 'cpu')


@pytest.mark.gpu
def test_mixed_call_between_guard_bands_on_gpu():
    _check_guarded_call(None, 'cuda:0')
