"""Per-molecule Philox noise for every sampler: gat CTMC steps (fm_k_ctmc_gat_fused), the priors of endpoint-parameterised models
(fm_prior_philox_dense) and the noise tape (fm_philox_tape) that ties the in-kernel draws, bit for bit, to the tensor-noise path the reference
fixtures pin.  Every check runs on the CPU emulation of the kernel sources (``emu_lib``) and, marked gpu, on the device.

Shapes.  Emulation: molecules of 4, 6, 3, 5 atoms at both workgroup sizes of the fused CTMC kernels (fm_config.ctmc_threads 256 | 1024).  GPU: 3, 5, 24, 47, 70
atoms = 3 / 10 / 276 / 1081 / 2415 pair rows: rows below one wave, molecule boundaries inside what a flat 256-row block would hold, and more rows than a
1024-thread workgroup (its stride loop runs 2-3 rounds; the 256-thread instance up to 10).  Category counts cover partial draw blocks (flowmol3 a 12+1, c 7+1,
e 5+1 classes in a gat row; qm9's narrower atom map)."""
import multiprocessing as mp
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch

import flowmol_amd as flowmol
from flowmol_amd import _lib, presets, weights
from flowmol_amd.engine import Engine, cat_temp_schedule, forward_weight_schedule, make_step_plan
from flowmol_amd.model import simplex_projection

EMU_SIZES = [4, 6, 3, 5]
GPU_SIZES = [3, 5, 24, 47, 70]


# ---------------------------------------------------------------------------------------------------------------- helpers
def _model(preset, lib=None, device='cpu', ctmc_threads=0, canonical=True):
    kw = {'_engine_lib': lib} if lib is not None else {}
    model = flowmol.FlowMol.from_preset(preset, canonical=canonical, **kw).to(device)
    if ctmc_threads:          # force one instance of the fused CTMC kernels (the automatic choice follows the batch)
        model._engine = Engine(model.cfg, model._sd, device=model.device, prefix=model._prefix, lib=lib, tuning={'ctmc_threads': ctmc_threads})
    return model


def _philox_plan(cfg, T, seed, dfm_type):
    return make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cat_temp_schedule(cfg), dfm_type=dfm_type,
                          forward_weight_func=forward_weight_schedule(cfg), philox_seed=seed, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)


def _masked_prior(model, x0):
    """Reference-format prior dict of a CTMC model: given positions, every categorical row on the mask token."""
    cfg, eng = model.cfg, model.engine
    one_hot = torch.nn.functional.one_hot
    return {'x_0': x0, 'fake_atoms': model.fake_atoms,
            'a_0': one_hot(torch.full((eng.N,), cfg.n_atom_types), cfg.n_atom_types + 1).float(),
            'c_0': one_hot(torch.full((eng.N,), cfg.n_charges), cfg.n_charges + 1).float(),
            'e_0': one_hot(torch.full((eng.U,), cfg.n_bond_types), cfg.n_bond_types + 1).float()}


def _tape_replay(model, sizes, T, seed, dfm_type, **kw):
    """The tensor-noise path (sample(_noise_for_step=...)) fed with Engine.philox_tape's draws, from the same Philox position prior."""
    eng = model.engine
    eng.bind(sizes)
    prior = _masked_prior(model, eng.prior_philox(seed))
    plan = _philox_plan(model.cfg, T, seed, dfm_type)
    return model.sample(sizes, n_timesteps=T, prior=prior, dfm_type=dfm_type, _noise_for_step=lambda i, last: eng.philox_tape(plan, i), **kw)


def _check_tape_equals_in_kernel(model, sizes, T, seed, dfm_type):
    sizes = torch.tensor(sizes)
    kw = dict(return_tensors='device', xt_traj=True, _frames=True)
    out_p, _, fr_p = model.sample(sizes, n_timesteps=T, rng='philox', seed=seed, dfm_type=dfm_type, **kw)
    out_p, fr_p = {k: v.clone() for k, v in out_p.items()}, {k: v.clone() for k, v in fr_p.items()}
    out_t, _, fr_t = _tape_replay(model, sizes, T, seed, dfm_type, **kw)
    for k in 'xace':
        assert torch.equal(out_p[k], out_t[k]), (dfm_type, 'final', k)
    assert set(fr_p) == set(fr_t) and fr_p['x'].shape[0] == T and fr_p['x_1_pred'].shape[0] == T - 1
    for k in fr_p:
        assert torch.equal(fr_p[k], fr_t[k]), (dfm_type, 'frames', k)
    mask = {'a': model.cfg.n_atom_types, 'c': model.cfg.n_charges, 'e': model.cfg.n_bond_types}
    assert any(bool((out_p[k] != mask[k]).any()) for k in 'ace')       # the run did unmask something: the comparison is not of two untouched priors


def _check_composition(model, sizes, T, dfm_type, exact=True, **extra):
    """Full batch vs molecules [3, 1] alone with their ids; same seed twice; another seed."""
    sizes = torch.tensor(sizes)
    run = lambda s, **kw: model.sample(s, n_timesteps=T, return_tensors=True, rng='philox', dfm_type=dfm_type, **extra, **kw)[0]
    full, again, other = run(sizes, seed=1234), run(sizes, seed=1234), run(sizes, seed=99)
    for k in 'xace':
        assert torch.equal(full[k], again[k])
    assert not torch.equal(full['x'], other['x'])
    noff, pairs = torch.cumsum(sizes, 0) - sizes, sizes * (sizes - 1) // 2
    poff = torch.cumsum(pairs, 0) - pairs
    ids = [3, 1]
    sub = run(sizes[ids], seed=1234, mol_ids=ids)
    o_n = o_p = 0
    for i in ids:
        n, u = int(sizes[i]), int(pairs[i])
        for k in 'ac':
            assert torch.equal(sub[k][o_n:o_n + n], full[k][noff[i]:noff[i] + n]), (k, i)
        assert torch.equal(sub['e'][o_p:o_p + u], full['e'][poff[i]:poff[i] + u]), ('e', i)
        if exact:
            assert torch.equal(sub['x'][o_n:o_n + n], full['x'][noff[i]:noff[i] + n]), ('x', i)
        else:
            torch.testing.assert_close(sub['x'][o_n:o_n + n], full['x'][noff[i]:noff[i] + n], rtol=1e-5, atol=1e-5)
        o_n += n; o_p += u


def _check_gat_sink(model, sizes, T, seed):
    """xt_traj / ep_traj of a Philox gat run = the tape-replayed tensor run, in the reference's frame format; one 'ctmc' launch per step, none of the flat
    gat kernels (whose frames are copy nodes)."""
    sizes = torch.tensor(sizes)
    eng = model.engine
    eng.profile(True)
    mols_p = model.sample(sizes, n_timesteps=T, rng='philox', seed=seed, dfm_type='gat', xt_traj=True, ep_traj=True)
    launches = {k: eng.profile_get(k)[1] for k in ('ctmc', 'ctmc_gat', 'x_step')}
    eng.profile(False)
    assert launches == {'ctmc': T - 1, 'ctmc_gat': 0, 'x_step': 0}, launches
    mols_t = _tape_replay(model, sizes, T, seed, 'gat', xt_traj=True, ep_traj=True)
    assert len(mols_p) == len(mols_t) == len(sizes)
    for mp_, mt in zip(mols_p, mols_t):
        fp, ft = mp_.traj_frames_reference(), mt.traj_frames_reference()
        assert set(fp) == set(ft)
        for k in fp:
            assert fp[k].shape == ft[k].shape and torch.equal(fp[k], ft[k]), k


# ---------------------------------------------------------------------------------------------------------------- 1. tape == in-kernel
@pytest.mark.parametrize('nt', [256, 1024])
@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
def test_tape_replay_equals_in_kernel_noise_on_emulation(emu_lib, dfm_type, nt):
    """Engine.philox_tape fed through the tensor-noise path reproduces the rng='philox' run bit for bit -- final state and every frame -- for both
    integrators and both workgroup sizes.  For gat this also checks the fused kernel against the flat gat kernels the reference fixtures pin."""
    _check_tape_equals_in_kernel(_model('qm9', emu_lib, ctmc_threads=nt), EMU_SIZES, 5, 31, dfm_type)


def test_tape_replay_equals_in_kernel_noise_flowmol3_on_emulation(emu_lib):
    """flowmol3's category counts (12 / 7 / 5 + mask: partial draw blocks in every modality)."""
    _check_tape_equals_in_kernel(_model('flowmol3', emu_lib), EMU_SIZES, 3, 8, 'gat')


@pytest.mark.gpu
@pytest.mark.parametrize('preset', ['qm9', 'flowmol3'])
@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
def test_tape_replay_equals_in_kernel_noise_on_gpu(dfm_type, preset):
    _check_tape_equals_in_kernel(_model(preset, device='cuda:0'), GPU_SIZES, 6, 31, dfm_type)


@pytest.mark.gpu
@pytest.mark.parametrize('nt', [256, 1024])
def test_tape_replay_equals_in_kernel_noise_both_workgroup_sizes_on_gpu(nt):
    _check_tape_equals_in_kernel(_model('qm9', device='cuda:0', ctmc_threads=nt), GPU_SIZES, 4, 5, 'gat')


# ---------------------------------------------------------------------------------------------------------------- 2. gat composition independence
@pytest.mark.parametrize('nt', [256, 1024])
def test_gat_philox_is_composition_independent_on_emulation(emu_lib, nt):
    _check_composition(_model('qm9', emu_lib, ctmc_threads=nt), EMU_SIZES, 4, 'gat')


def test_gat_philox_from_the_config_and_non_canonical_on_emulation(emu_lib):
    """gat through cfg.dfm_type instead of the keyword; canonical=False keeps tokens identical and coordinates to rtol 1e-5."""
    import dataclasses
    model = _model('qm9', emu_lib, canonical=False)
    model.cfg = dataclasses.replace(model.cfg, dfm_type='gat')
    _check_composition(model, EMU_SIZES, 4, None, exact=False)


@pytest.mark.gpu
def test_gat_philox_is_composition_independent_on_gpu():
    _check_composition(_model('flowmol3', device='cuda:0'), GPU_SIZES, 6, 'gat')


@pytest.mark.gpu
def test_gat_philox_non_canonical_on_gpu():
    _check_composition(_model('qm9', device='cuda:0', canonical=False), GPU_SIZES, 6, 'gat', exact=False)


def test_philox_still_refuses_row_slicing_and_noise_callbacks(emu_lib):
    model = _model('qm9', emu_lib)
    with pytest.raises(NotImplementedError, match='_noise_for_step'):
        model.sample(torch.tensor([3, 4]), n_timesteps=3, rng='philox', seed=1, _noise_for_step=lambda i, last: None)
    with pytest.raises(NotImplementedError, match='_rows'):
        model.sample(torch.tensor([3, 4]), n_timesteps=3, rng='philox', seed=1, _rows=(7, 9, torch.arange(7), torch.arange(9)))


# ---------------------------------------------------------------------------------------------------------------- 3. gat trajectory sink
def test_gat_trajectory_sink_on_emulation(emu_lib):
    _check_gat_sink(_model('qm9', emu_lib), EMU_SIZES, 4, 17)


@pytest.mark.gpu
def test_gat_trajectory_sink_on_gpu():
    _check_gat_sink(_model('flowmol3', device='cuda:0'), GPU_SIZES, 5, 17)


# ---------------------------------------------------------------------------------------------------------------- 4. endpoint priors
ROWS_E = 2 * (64 * 63 // 2)      # 4032 pair rows of 2 x 64 atoms: the modality of the frequency checks
P_E = torch.tensor([0.1, 0.2, 0.3, 0.4])
P_A = torch.tensor([0.5, 0.0, 0.5, 0.0, 0.0])
P_CA = torch.tensor([[0.7, 0.2, 0.1, 0.0, 0.0, 0.0], [1 / 6] * 6, [0.1, 0.1, 0.0, 0.8, 0.0, 0.0], [1 / 6] * 6, [1 / 6] * 6])


def _check_endpoint_priors(lib, device):
    cfg = presets.endpoint_small()
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device=device, lib=lib)
    eng.bind(torch.tensor([64, 64]))
    assert eng.U == ROWS_E and eng.N == 128 and (cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types) == (5, 6, 4)
    seed = 20
    cpu = lambda st: {k: v.cpu() for k, v in st.items()}
    same = lambda kind, **kw: ({t: kind for t in 'ace'}, {t: dict(kw) for t in 'ace'})
    # the kernel's own normals: the gaussian kind with std = 1
    g = cpu(eng.prior_philox_dense(seed, *same('gaussian', std=1.0)))
    assert torch.equal(g['x_t'], eng.prior_philox(seed).cpu())
    for t in 'ace':          # 4032 x 4 (e) / 128 x 5 | 6 normals: mean 0 and variance 1 within 5 standard errors (SE of the mean 1/sqrt(n), of the variance sqrt(2/n))
        n = g[f'{t}_t'].numel()
        assert abs(float(g[f'{t}_t'].mean())) < 5 / n ** 0.5 and abs(float(g[f'{t}_t'].var()) - 1) < 5 * (2 / n) ** 0.5, t
    sc = cpu(eng.prior_philox_dense(seed, *same('gaussian', std=0.5, simplex_center=True)))
    for t in 'ace':
        assert torch.allclose(sc[f'{t}_t'], g[f'{t}_t'] * 0.5 + 1 / g[f'{t}_t'].shape[1], atol=1e-6)
    # barycenter: exactly 1/d; blurred: the host simplex projection of 1/d + blur g
    bc = cpu(eng.prior_philox_dense(seed, *same('barycenter')))
    bl = cpu(eng.prior_philox_dense(seed, *same('barycenter', blur=0.3)))
    bs = cpu(eng.prior_philox_dense(seed, *same('biased-simplex', vertex_prob=0.75, std=0.2, vertex_idx=1)))
    for t in 'ace':
        gt = g[f'{t}_t']
        d = gt.shape[1]
        assert torch.equal(bc[f'{t}_t'], torch.ones_like(gt) / d)
        assert float((bl[f'{t}_t'] - simplex_projection(1 / d + 0.3 * gt)).abs().max()) <= 1e-6, t
        assert float((bl[f'{t}_t'].sum(1) - 1).abs().max()) <= 1e-6 and float(bl[f'{t}_t'].min()) >= 0
        mu = torch.full((d,), 0.25 / (d - 1))
        mu[1] = 0.75
        assert float((bs[f'{t}_t'] - torch.softmax((mu + 0.2 * gt) * d, dim=1)).abs().max()) <= 1e-6, t
    # uniform simplex on the 4032 pair rows: a flat Dirichlet, component mean 1/d, variance (d-1)/(d^2 (d+1)) -> 5 SE = 5 sqrt(var / 4032) = 0.0152 for d = 4
    us = cpu(eng.prior_philox_dense(seed, *same('uniform-simplex')))['e_t']
    d = us.shape[1]
    assert float(us.min()) >= 0 and float((us.sum(1) - 1).abs().max()) <= 1e-6
    tol = 5 * ((d - 1) / (d * d * (d + 1)) / ROWS_E) ** 0.5
    assert float((us.mean(0) - 1 / d).abs().max()) < tol, (us.mean(0), tol)
    # marginal: frequencies over the 4032 pair rows = p within 5 SE = 5 sqrt(p (1 - p) / 4032) (0.024 .. 0.039); c-given-a on the 128 node rows, conditioned on
    # the sampled atom type (two types of ~64 rows each: 5 SE = 5 sqrt(p (1 - p) / n_a), about 0.29 at p = 0.7 -- enough to tell the two rows of p_c_given_a apart)
    types = {'a': 'marginal', 'c': 'c-given-a', 'e': 'marginal'}
    kws = {'a': {'p': P_A}, 'c': {'p_c_given_a': P_CA}, 'e': {'p': P_E}}
    mg = cpu(eng.prior_philox_dense(seed, types, kws))
    for t in 'ace':
        assert torch.equal(mg[f'{t}_t'].sum(1), torch.ones(mg[f'{t}_t'].shape[0])) and set(mg[f'{t}_t'].unique().tolist()) == {0.0, 1.0}      # one-hot rows
    freq = mg['e_t'].mean(0)
    assert bool(((freq - P_E).abs() < 5 * (P_E * (1 - P_E) / ROWS_E).sqrt()).all()), freq
    a_idx = mg['a_t'].argmax(1)
    assert set(a_idx.tolist()) == {0, 2}
    for a in (0, 2):
        rows = mg['c_t'][a_idx == a]
        n_a = rows.shape[0]
        assert n_a > 30
        assert bool(((rows.mean(0) - P_CA[a]).abs() <= 5 * (P_CA[a] * (1 - P_CA[a]) / n_a).sqrt()).all()), (a, rows.mean(0))
    # blurred marginal: softmax((one_hot(idx) + blur g) d), idx read back from the run without blur (same seed, same Exp race)
    # (the charge draw is conditioned on argmax(a_0): a_0 stays un-blurred in the run that checks c, and is checked in a run of its own)
    kwb = {'a': {'p': P_A}, 'c': {'p_c_given_a': P_CA, 'blur': 0.25}, 'e': {'p': P_E, 'blur': 0.25}}
    mb = cpu(eng.prior_philox_dense(seed, types, kwb))
    mb['a_t'] = cpu(eng.prior_philox_dense(seed, types, {**kwb, 'a': {'p': P_A, 'blur': 0.25}}))['a_t']
    for t in 'ace':
        gt = g[f'{t}_t']
        d = gt.shape[1]
        assert float((mb[f'{t}_t'] - torch.softmax((mg[f'{t}_t'] + 0.25 * gt) * d, dim=1)).abs().max()) <= 1e-6, t
    # another seed, another draw; ids move the streams with the molecules
    assert not torch.equal(cpu(eng.prior_philox_dense(seed + 1, *same('gaussian', std=1.0)))['e_t'], g['e_t'])
    eng.bind(torch.tensor([64]))
    eng.set_molecule_ids(torch.tensor([1]))
    one = cpu(eng.prior_philox_dense(seed, types, kws))
    assert torch.equal(one['e_t'], mg['e_t'][ROWS_E // 2:]) and torch.equal(one['c_t'], mg['c_t'][64:]) and torch.equal(one['x_t'], g['x_t'][64:])


def test_endpoint_priors_match_torch_formulas_on_emulation(emu_lib):
    _check_endpoint_priors(emu_lib, 'cpu')


@pytest.mark.gpu
def test_endpoint_priors_match_torch_formulas_on_gpu():
    _check_endpoint_priors(None, 'cuda:0')


def test_prior_philox_dense_refusals(emu_lib):
    cfg = presets.endpoint_small()
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device='cpu', lib=emu_lib)
    eng.bind(torch.tensor([3, 4]))
    with pytest.raises(ValueError, match="needs kwargs"):
        eng.prior_philox_dense(1, {'a': 'marginal', 'c': 'gaussian', 'e': 'gaussian'}, {})
    with pytest.raises(_lib.FlowMolHipError, match='modality c'):
        eng.prior_philox_dense(1, {'a': 'gaussian', 'c': 'gaussian', 'e': 'c-given-a'}, {'e': {'p_c_given_a': torch.full((5, 4), 0.25)}})
    ctmc = presets.qm9()
    eng2 = Engine(ctmc, weights.synth_state_dict(ctmc, 0), device='cpu', lib=emu_lib)
    eng2.bind(torch.tensor([3, 4]))
    with pytest.raises(_lib.FlowMolHipError, match='CTMC model'):
        eng2.prior_philox_dense(1, {t: 'gaussian' for t in 'ace'}, {})


# ---------------------------------------------------------------------------------------------------------------- 5. endpoint models end to end
def _check_endpoint_end_to_end(lib, device, sizes, T):
    model = _model('endpoint_small', lib, device)
    sizes = torch.tensor(sizes)
    seed = 77
    full, _ = model.sample(sizes, n_timesteps=T, rng='philox', seed=seed, return_tensors='dense')
    full = {k: v.clone() for k, v in full.items()}
    eng = model.engine
    eng.bind(sizes)
    p0 = eng.prior_philox_dense(seed)
    via_prior, _ = model.sample(sizes, n_timesteps=T, return_tensors='dense', prior={'x_0': p0['x_t'], 'a_0': p0['a_t'], 'c_0': p0['c_t'], 'e_0': p0['e_t']})
    for k in 'xace':
        assert torch.equal(full[k], via_prior[k]), k
    other, _ = model.sample(sizes, n_timesteps=T, rng='philox', seed=seed + 1, return_tensors='dense')
    assert not torch.equal(other['x'], full['x'])
    ids = [3, 1]
    sub, _ = model.sample(sizes[ids], n_timesteps=T, rng='philox', seed=seed, mol_ids=ids, return_tensors='dense')
    noff, pairs = torch.cumsum(sizes, 0) - sizes, sizes * (sizes - 1) // 2
    poff = torch.cumsum(pairs, 0) - pairs
    o_n = o_p = 0
    for i in ids:
        n, u = int(sizes[i]), int(pairs[i])
        for k in 'xac':
            assert torch.equal(sub[k][o_n:o_n + n], full[k][noff[i]:noff[i] + n]), (k, i)
        assert torch.equal(sub['e'][o_p:o_p + u], full['e'][poff[i]:poff[i] + u]), ('e', i)
        o_n += n; o_p += u


def test_endpoint_philox_end_to_end_on_emulation(emu_lib):
    _check_endpoint_end_to_end(emu_lib, 'cpu', EMU_SIZES, 3)


@pytest.mark.gpu
def test_endpoint_philox_end_to_end_on_gpu():
    _check_endpoint_end_to_end(None, 'cuda:0', GPU_SIZES, 4)


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _endpoint_philox_worker(rank, world, port, sizes, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    emu = _lib.load(Path(__file__).resolve().parent / 'emu' / 'libflowmol_emu.so')
    model = flowmol.FlowMol.from_preset('endpoint_small', _engine_lib=emu).to('cpu')
    torch.manual_seed(55 + rank)           # different per-rank RNG state on purpose: only rank 0's broadcast seed matters
    full, n = model.sample_distributed(torch.tensor(sizes), n_timesteps=3, return_tensors=True, noise='philox')
    q.put((rank, {k: v.numpy().copy() for k, v in full.items()}))
    dist.destroy_process_group()


def test_endpoint_sample_distributed_philox_equals_single_process(emu_lib_path):
    """An endpoint-parameterised model on two gloo ranks with noise='philox': what one process samples with rank 0's seed, bit for bit."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_endpoint_philox_worker, args=(r, 2, port, EMU_SIZES, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: {k: torch.from_numpy(v) for k, v in d.items()} for r, d in (q.get(timeout=300) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
    for k in 'xace':
        assert torch.equal(res[0][k], res[1][k])
    model = flowmol.FlowMol.from_preset('endpoint_small', _engine_lib=_lib.load(emu_lib_path)).to('cpu')
    torch.manual_seed(55)                  # rank 0's generator state -> the same broadcast seed
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    single, _ = model.sample(torch.tensor(EMU_SIZES), n_timesteps=3, return_tensors=True, rng='philox', seed=seed)
    for k in 'ace':
        assert torch.equal(res[0][k], single[k].to(res[0][k].dtype))
    assert torch.equal(res[0]['x'], single['x'])


# ---------------------------------------------------------------------------------------------------------------- 6. existing streams did not move
def test_existing_philox_streams_did_not_move(emu_lib, golden_dir):
    """tests/golden/philox_streams_v7.npz: prior_philox(7) of 40 x 50 atoms and the campbell Philox run of test_philox_noise_is_sharding_independent...'s sizes
    and seed, recorded through the (deterministic) emulation on the commit before the gat / endpoint / tape streams were added."""
    g = np.load(golden_dir / 'philox_streams_v7.npz')
    model = _model('qm9', emu_lib)
    full, _ = model.sample(torch.from_numpy(g['run_sizes']), n_timesteps=int(g['run_n_timesteps']), return_tensors=True, rng='philox', _philox=int(g['run_seed']))
    for k in 'xace':
        assert torch.equal(full[k], torch.from_numpy(g['run_' + k])), k
    eng = Engine(model.cfg, weights.synth_state_dict(model.cfg, 0), device='cpu', lib=emu_lib)
    eng.bind(torch.from_numpy(g['prior_sizes']))
    assert torch.equal(eng.prior_philox(int(g['prior_seed'])), torch.from_numpy(g['prior_x0']))


# ---------------------------------------------------------------------------------------------------------------- 7. CLI
def test_cli_rng_philox_is_reproducible_on_emulation(tmp_path, emu_lib):
    """--rng philox --seed 5 twice: identical SDF text, also when the same molecules are sampled in batches of another size (a molecule owns stream i of the
    run); another seed gives other molecules."""
    from flowmol_amd import cli

    def run(name, seed, batch):
        out = tmp_path / name
        cli.run(cli.parse_args(['--preset', 'qm9', '--n_mols', '4', '--n_atoms_per_mol', '5', '--n_timesteps', '3', '--max_batch_size', str(batch), '--rng', 'philox',
                                '--seed', str(seed), '--device', 'cpu', '--output_file', str(out)]), engine_lib=emu_lib)
        return out.read_text()
    a, b, c, d = run('a.sdf', 5, 4), run('b.sdf', 5, 4), run('c.sdf', 5, 3), run('d.sdf', 6, 4)
    assert a.count('$$$$') == 4 and a == b and a == c and a != d
