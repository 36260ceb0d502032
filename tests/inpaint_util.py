"""Helpers of tests/test_inpaint.py: frozen atoms (fm_ctmc_step_inpaint / fm_integrate_inpaint, Engine.ctmc_step_inpaint / integrate_inpaint,
FlowMol.resample(keep=...) / inpaint, SamplingQueue.submit_from(keep=...)).  A plain module like resample_util.py, whose given molecules, cached models
and per-molecule comparisons it reuses.

The reference of every check is a COMPOSITION of calls the library already has and tests: the plain step (fm_ctmc_step, one-step fm_integrate /
fm_integrate_mixed with the previous endpoint carried), then a host torch.where that puts the frozen rows onto Engine.conditional_path at the next
time point.  All comparisons are torch.equal."""
from __future__ import annotations

import copy
import ctypes as C

import torch
import torch.nn.functional as F

from flowmol_amd.engine import IntegrationRun, StepNoise, _ptr, fm_sampled, make_step_plan, mixed_step_arrays
from hygiene_util import GuardSet, cpu, dst_shapes
from oracle import cpu_ref
from parity_util import onehots

import mixed_util as mu
import resample_util as ru

KERNEL_SIZES = ru.KERNEL_SIZES          # 1, 2, 5, 24, 47 atoms: 0 pairs, 1 pair, 10, 276 and 1081 pairs
KERNEL_IDS = (11, 3, 40, 7, 1000003)
TRAJ_SIZES = ru.TRAJ_SIZES              # 5, 3, 2, 1


def kernel_keep(sizes=KERNEL_SIZES):
    """The keep pattern of the one-step checks: the 1-atom molecule kept; one of the 2 atoms (its only pair is free); atoms {0, 3} of the 5 (exactly one
    frozen pair); all 24; every third atom of the 47."""
    assert list(sizes) == [1, 2, 5, 24, 47]
    rows = [[True], [False, True], [True, False, False, True, False], [True] * 24, [i % 3 == 0 for i in range(47)]]
    return torch.tensor([v for r in rows for v in r])


def traj_keep(sizes):
    """Trajectory checks: atoms {0, 3, 4} of a 5-atom molecule (three frozen pairs), the middle atom of 3, both of 2, the single atom of 1; for any other
    size every other atom."""
    pat = {5: [True, False, False, True, True], 3: [False, True, False], 2: [True, True], 1: [True]}
    return [list(pat.get(n, [i % 2 == 0 for i in range(n)])) for n in sizes]


def flat(keep):
    return torch.tensor([v for r in keep for v in r])


def frozen_masks(sizes, keep_atom):
    """Bool masks of the frozen rows, written out independently of the library: {'x', 'a', 'c'}: (N,), 'e': (U,) -- a pair (i < j, upper-triangle order
    per molecule) is frozen iff both its atoms are kept."""
    pair = []
    for blk in torch.split(keep_atom, list(sizes)):
        n = blk.shape[0]
        pair += [bool(blk[i]) and bool(blk[j]) for i in range(n) for j in range(i + 1, n)]
    e = torch.tensor(pair, dtype=torch.bool)
    return {'x': keep_atom, 'a': keep_atom, 'c': keep_atom, 'e': e}


def overwrite(state, path, frozen):
    """where(frozen, path rows, state rows) in place on a state dict ('x_t', ...) or a frame dict ('x', ...); tensors on any device."""
    for f in 'xace':
        key = f'{f}_t' if f'{f}_t' in state else f
        m = frozen[f].to(state[key].device)
        state[key][m] = path[f'{f}_t'].to(state[key].device, state[key].dtype)[m]
    return state


def clone(state):
    return {k: v.clone() for k, v in state.items()}


def softmax_dst(eng, seed=5):
    """Seeded endpoint prediction of the bound batch: softmax rows and positions."""
    gen = torch.Generator().manual_seed(seed)
    sh = dst_shapes(eng)
    d = {'x': torch.randn(*sh['x'], generator=gen)}
    for k in 'ace':
        d[k] = torch.softmax(torch.randn(*sh[k], generator=gen) * 2.0, dim=-1)
    return {k: v.to(eng.device).contiguous() for k, v in d.items()}


def tensor_noise(eng, last, dfm_type, seed=23):
    cfg = eng.cfg
    nz = StepNoise.draw(eng.N, eng.U, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types, last, 'cpu', torch.Generator().manual_seed(seed), dfm_type)
    return StepNoise(**{k: (None if getattr(nz, k) is None else getattr(nz, k).to(eng.device).contiguous()) for k in StepNoise.__slots__})


def sampled_buffers(eng):
    i32 = dict(dtype=torch.int32, device=eng.device)
    return {'a1': torch.full((eng.N,), -7, **i32), 'c1': torch.full((eng.N,), -7, **i32), 'e1': torch.full((eng.U,), -7, **i32)}


def step_case(lib, device, threads, T=6, i=2, seed=91):
    """The shared inputs of the one-step checks on the qm9 preset (cached per engine): the given molecules, the spec, the state on the conditional
    path at time point i, the path at time point i + 1 (= alpha_next), a seeded endpoint prediction.  No network evaluation runs."""
    def make():
        eng, cfg, _ = mu.engine('qm9', lib, device, ctmc_threads=threads)
        sizes = list(KERNEL_SIZES)
        eng.bind(torch.tensor(sizes))
        eng.set_molecule_ids(torch.tensor(list(KERNEL_IDS)))
        x1 = ru.as_state(eng, ru.given(cfg, sizes))
        keep = kernel_keep(sizes)
        spec = eng.inpaint_spec(x1, keep, seed)
        al, al_next = ru.alpha_row(cfg, T, i), ru.alpha_row(cfg, T, i + 1)
        state = eng.conditional_path(x1, al, seed=seed)
        path = cpu(eng.conditional_path(x1, al_next, seed=seed))
        eng.synchronize()
        return {'eng': eng, 'cfg': cfg, 'sizes': sizes, 'x1': x1, 'keep': keep, 'spec': spec, 'state': state, 'path': path, 'alpha_next': al_next,
                'dst': softmax_dst(eng), 'frozen': frozen_masks(sizes, keep), 'T': T, 'i': i, 'seed': seed}
    return mu.cached(('inpaint-step', id(lib), str(device), threads, T, i, seed), make)


def step_scalars(case, dfm_type, philox, hc, last, eta=2.0):
    cfg = case['cfg']
    plan = make_step_plan(case['T'], eta, hc, cfg.cat_temperature, dfm_type=dfm_type, philox_seed=case['seed'] if philox else None,
                          schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)
    sc = copy.copy(plan.scalars[case['i']])
    sc.last_step = int(last)
    return sc


def one_step(case, dfm_type, philox, hc, last):
    """(plain step, inpaint step, sampled tokens of each) on clones of the case's state, on the cpu."""
    eng = case['eng']
    eng.bind(torch.tensor(case['sizes']))
    eng.set_molecule_ids(torch.tensor(list(KERNEL_IDS)))
    sc = step_scalars(case, dfm_type, philox, hc, last)
    nz = StepNoise() if philox else tensor_noise(eng, bool(last), dfm_type)
    plain, smp_p = clone(case['state']), sampled_buffers(eng)
    eng.ctmc_step(plain, case['dst'], nz, sc, smp_p)
    got, smp_g = clone(case['state']), sampled_buffers(eng)
    eng.ctmc_step_inpaint(got, case['dst'], nz, sc, case['spec'], case['alpha_next'], smp_g)
    eng.synchronize()
    return cpu(plain), cpu(got), cpu(smp_p), cpu(smp_g)


# ------------------------------------------------------------------------------------------------------------------ integration
def alpha_table(eng, plan):
    return eng.plan_alphas(plan)


def traj_setup(mdl, sizes, ids, seed):
    eng = mdl.engine
    eng.bind(torch.tensor(sizes))
    eng.set_molecule_ids(torch.tensor(ids))
    x1 = ru.as_state(eng, ru.given(mdl.cfg, sizes))
    keep = flat(traj_keep(sizes))
    return eng, x1, keep, eng.inpaint_spec(x1, keep, seed), frozen_masks(sizes, keep)


def single_runs(mdl, sizes, ids, T, k, seed, with_traj):
    """(got, want): the final state, the last endpoint prediction and the frames of steps k .. T-2 -- got: ONE fm_integrate_inpaint run
    (IntegrationRun with the spec); want: per step a one-step fm_integrate with the previous endpoint carried, then the host overwrite of the state
    and of the new state's sink frame from Engine.conditional_path at the next time point."""
    eng, x1, keep, spec, frozen = traj_setup(mdl, sizes, ids, seed)
    plan = mu.philox_plans(mdl, [T], seed)[0]
    alphas = alpha_table(eng, plan)
    res = []
    for composed in (False, True):
        state = eng.conditional_path(x1, alphas[k], seed=seed)
        traj = eng.new_traj(T - 1) if with_traj else None
        if traj is not None:
            for v in traj.values():
                v.fill_(-3)
        run = IntegrationRun(eng, state, plan, None, traj=traj, inpaint=None if composed else spec)
        if composed:
            for i in range(k, T - 1):
                run.run(i, i + 1)
                eng.synchronize()
                path = eng.conditional_path(x1, alphas[i + 1], seed=seed)
                overwrite(state, path, frozen)
                if traj is not None:
                    overwrite({f: traj[f][i] for f in 'xace'}, path, frozen)
        else:
            run.run(k, T - 1)
        eng.synchronize()
        out = {**cpu(state), **{f'dst.{f}': v.cpu().clone() for f, v in run.last_dst().items()}}
        if traj is not None:
            out.update({f'traj.{f}': v[k:].cpu().clone() for f, v in traj.items()})
        res.append(out)
    return res[0], res[1], frozen


def mixed_runs(mdl, sizes, ids, pairs, seed):
    """(got, want) of a batch with one (T, k) per molecule: got: ONE Engine.integrate_inpaint call; want: per call-step a one-step
    Engine.integrate_mixed with the previous endpoint carried, then the host overwrite of the rows of the molecules whose group took the step."""
    eng, x1, keep, spec, frozen = traj_setup(mdl, sizes, ids, seed)
    keys = sorted(set(pairs))
    group = [keys.index(p) for p in pairs]
    plans = mu.philox_plans(mdl, [T for T, _ in keys], seed)
    tabs = [alpha_table(eng, p) for p in plans]
    start = [k for _, k in keys]
    n = max(T - 1 - k for T, k in keys)
    al0 = torch.stack([tabs[g][start[g]] for g in range(len(keys))])
    n_t = torch.tensor(sizes)
    g_t = torch.tensor(group)
    node_g, pair_g = g_t.repeat_interleave(n_t), g_t.repeat_interleave(n_t * (n_t - 1) // 2)
    got = eng.conditional_path(x1, al0, group, seed=seed)
    dst_g = eng.integrate_inpaint(got, plans, group, spec, start=start)
    # the returned endpoint prediction is defined for the molecules that took the call's last step (a finished group's rows are not carried)
    last = torch.tensor([T - 1 - k_ == n for T, k_ in keys])
    rows = lambda f: last[pair_g if f == 'e' else node_g]
    got = {**cpu(got), **{f'dst.{f}': v.cpu()[rows(f)].clone() for f, v in dst_g.items()}}
    want = eng.conditional_path(x1, al0, group, seed=seed)
    prev = None
    for j in range(n):
        at = [s + j for s in start]
        active = torch.tensor([at[g] < len(plans[g].scalars) for g in range(len(keys))])
        prev = eng.integrate_mixed(want, plans, group, start=[min(a, len(p.scalars)) for a, p in zip(at, plans)], n_steps=1, prev=prev)
        nxt = torch.stack([tabs[g][min(at[g] + 1, tabs[g].shape[0] - 1)] for g in range(len(keys))])
        path = eng.conditional_path(x1, nxt, group, seed=seed)
        fz = {f: frozen[f] & active[pair_g if f == 'e' else node_g] for f in 'xace'}
        overwrite(want, path, fz)
    eng.synchronize()
    want = {**cpu(want), **{f'dst.{f}': v.cpu()[rows(f)].clone() for f, v in prev.items()}}
    return got, want, frozen


# ------------------------------------------------------------------------------------------------------------------ the API
def resample_tensors(mdl, mols, k, T, seed, ids, keep, **kw):
    out = mdl.resample(mols, k, n_timesteps=T, seed=seed, mol_ids=ids, return_tensors=True, keep=keep, **kw)[0]
    return mu.split_molecules(out, mols[1].tolist())


def frozen_rows_equal(got, want, keep):
    """[(molecule, field)] whose frozen rows of ``got`` are not bit-identical to those of ``want`` (per-molecule result dicts; keep: per-molecule lists)."""
    bad = []
    for i, (g, w, kp) in enumerate(zip(got, want, keep)):
        fz = frozen_masks([len(kp)], torch.tensor(kp))
        for f in 'xace':
            if not torch.equal(g[f][fz[f]].to(w[f].dtype), w[f][fz[f]]):
                bad.append((i, f))
    return bad


# ------------------------------------------------------------------------------------------------------------------ the oracle
def oracle_inpaint(mdl, sizes, ids, mols, keep, k, T, seed):
    """cpu_ref.OracleVF integrates the conditional-path state over linspace(0, 1, T)[k:] with the noise tapes of steps k .. T-2 (resample_util's
    oracle_from_state) and, after every step, the same overwrite on the host: the frozen rows take the conditional path at the step's new time point,
    computed here with torch from the call's tape (x0, u), the centred positions and the given tokens."""
    eng, cfg = mdl.engine, mdl.cfg
    orc = cpu_ref.OracleVF(cfg, mdl._sd, prefix=mdl._prefix)
    n = torch.tensor(sizes)
    eng.bind(n)
    eng.set_molecule_ids(torch.tensor(ids))
    x1 = ru.as_state(eng, mols)
    plan = mu.philox_plans(mdl, [T], seed)[0]
    alphas = alpha_table(eng, plan)
    state, cond = eng.conditional_path(x1, alphas[k], seed=seed, tape=True)
    state, cond = cpu(state), cpu(cond)
    x1c = eng.remove_com(x1['x_t'].clone()).cpu()
    tok1 = {f: x1[f'{f}_t'].cpu().long() for f in 'ace'}
    mask = {'a': cfg.n_atom_types, 'c': cfg.n_charges, 'e': cfg.n_bond_types}
    frozen = frozen_masks(sizes, flat(keep))
    tape = []
    for s in range(k, T - 1):
        nz = eng.philox_tape(plan, s)
        for tag in 'ace':
            tape += [getattr(nz, f'{f}_{tag}').cpu() for f in ('q', 'u1', 'u2') if getattr(nz, f'{f}_{tag}') is not None]
    batch = cpu_ref.build_batch(n)
    m = batch.upper_edge_mask
    a0, c0, e0 = onehots(cfg, batch, state['a_t'].long(), state['c_t'].long(), state['e_t'].long())

    def hook(s_idx, new, dst):
        al = alphas[k + s_idx]
        fx = frozen['x']
        new['x_t'][fx] = ((1 - al[0]) * cond['x0'] + al[0] * x1c)[fx]
        for col, f in enumerate('ace', 1):
            tok = torch.where(cond[f'u_{f}'] < 1 - al[col], torch.full_like(tok1[f], mask[f]), tok1[f])
            oh = F.one_hot(tok, mask[f] + 1).float()
            if f == 'e':
                upper = new['e_t'][m].clone()
                upper[frozen['e']] = oh[frozen['e']]
                new['e_t'][m] = upper
                new['e_t'][~m] = upper
            else:
                new[f'{f}_t'][frozen[f]] = oh[frozen[f]]
    noise = cpu_ref.TapeNoise(tape)
    with torch.no_grad():
        ref = orc.integrate(batch, {'x_0': state['x_t'], 'a_0': a0, 'c_0': c0, 'e_0': e0}, T, noise=noise, tspan=torch.linspace(0, 1, T)[k:], step_hook=hook)
    assert noise.pos == len(tape)
    return {'x': ref['x_1'], 'a': ref['a_1'].argmax(-1).int(), 'c': ref['c_1'].argmax(-1).int(), 'e': ref['e_1'][m].argmax(-1).int()}


# ------------------------------------------------------------------------------------------------------------------ the raw ABI, guarded
def _guarded_spec(gs, eng, x1, keep, seed):
    """The fm_inpaint struct with every member between guard bands: the inputs as guarded inputs, keep_pair as a guarded output."""
    spec = eng.inpaint_spec(x1, keep, seed)
    eng.synchronize()
    g = {k: gs.inp(f'inp.{k}', v.cpu()) for k, v in spec.items() if k != 'keep_pair'}
    g['keep_pair'] = gs.out('inp.keep_pair', (eng.U,), torch.uint8)
    return g


def guarded_step(eng, ws, sizes, ids, seed, T=6, i=2):
    """One fm_ctmc_step_inpaint call (campbell, Philox) through ctypes with every pointer of the call between 4096-byte 0xA5 bands and the batch bound in
    the arena ``ws`` (hygiene_util.arena) -> (results on the cpu, the GuardSet)."""
    cfg, dev = eng.cfg, eng.device
    eng.bind(torch.tensor(sizes), workspace=ws)
    eng.set_molecule_ids(torch.tensor(ids))
    x1 = ru.as_state(eng, ru.given(cfg, sizes))
    gs, i32 = GuardSet(dev), torch.int32
    spec = _guarded_spec(gs, eng, x1, kernel_keep(sizes), seed)
    st0 = eng.conditional_path(x1, ru.alpha_row(cfg, T, i), seed=seed)
    state = {f: gs.out(f'state.{f}', tuple(v.shape), v.dtype, init=v) for f, v in st0.items()}
    dst = gs.inp_dict('dst', softmax_dst(eng))
    smp = {'a1': gs.out('smp.a1', (eng.N,), i32), 'c1': gs.out('smp.c1', (eng.N,), i32), 'e1': gs.out('smp.e1', (eng.U,), i32)}
    plan = make_step_plan(T, 2.0, 0.9, cfg.cat_temperature, philox_seed=seed, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)
    sc = plan.scalars[i]
    st, d, ip, sm = eng._state_struct(state), eng._dst_struct(dst), eng._inpaint_struct(spec), fm_sampled()
    sm.a1, sm.c1, sm.e1 = _ptr(smp['a1']), _ptr(smp['c1']), _ptr(smp['e1'])
    al = (C.c_float * 4)(*ru.alpha_row(cfg, T, i + 1).tolist())
    rc = eng.lib.fm_ctmc_step_inpaint(eng._ctx, eng._stream(), C.byref(st), C.byref(d), None, C.byref(sc), C.byref(sm), C.byref(ip), al)
    eng._check(rc, 'fm_ctmc_step_inpaint')
    eng.synchronize()
    return cpu({**state, **smp, 'keep_pair': spec['keep_pair']}), gs


def guarded_integrate(mdl, ws, sizes, ids, pairs, seed):
    """One fm_integrate_inpaint call with one (T, k) per molecule, every pointer guarded, the batch bound in the arena ``ws``."""
    eng, cfg = mdl.engine, mdl.cfg
    dev = eng.device
    eng.bind(torch.tensor(sizes), workspace=ws)
    eng.set_molecule_ids(torch.tensor(ids))
    x1 = ru.as_state(eng, ru.given(cfg, sizes))
    keys = sorted(set(pairs))
    grp = [keys.index(p) for p in pairs]
    plans = mu.philox_plans(mdl, [T for T, _ in keys], seed)
    tabs = [alpha_table(eng, p) for p in plans]
    start = [k for _, k in keys]
    n, G = max(T - 1 - k for T, k in keys), len(keys)
    scal, act, temb = mixed_step_arrays(plans, start, n, cfg.time_embedding_dim)
    al = torch.zeros(n, G, 4)
    for j in range(n):
        for g in range(G):
            al[j, g] = tabs[g][min(start[g] + j + 1, tabs[g].shape[0] - 1)]
    gs, i32 = GuardSet(dev), torch.int32
    spec = _guarded_spec(gs, eng, x1, flat(traj_keep(sizes)), seed)
    st0 = eng.conditional_path(x1, torch.stack([tabs[g][start[g]] for g in range(G)]), grp if G > 1 else None, seed=seed)
    state = {f: gs.out(f'state.{f}', tuple(v.shape), v.dtype, init=v) for f, v in st0.items()}
    dst = [gs.out_dict(f'dst{i}', dst_shapes(eng)) for i in (0, 1)]
    scal_dev = gs.inp('steps', torch.frombuffer(bytearray(bytes(scal)), dtype=torch.uint8))
    act_dev = gs.inp('active', torch.tensor(list(act), dtype=i32))
    group = gs.inp('mol_group', torch.tensor(grp, dtype=i32))
    temb_dev = gs.inp('temb', temb)
    al_dev = gs.inp('alpha_next', al)
    al_host = al.contiguous()
    st, ds, ip = eng._state_struct(state), [eng._dst_struct(d) for d in dst], eng._inpaint_struct(spec)
    final = C.c_int(-1)
    rc = eng.lib.fm_integrate_inpaint(eng._ctx, eng._stream(), C.byref(st), n, G, scal, _ptr(scal_dev), act, _ptr(act_dev), _ptr(group), _ptr(temb_dev), None,
                                      None, C.byref(ds[0]), C.byref(ds[1]), None, C.byref(final), C.byref(ip),
                                      C.cast(C.c_void_p(al_host.data_ptr()), C.POINTER(C.c_float)), _ptr(al_dev))
    eng._check(rc, 'fm_integrate_inpaint')
    eng.synchronize()
    assert final.value in (0, 1)
    return cpu({**state, 'keep_pair': spec['keep_pair'], **{f'dst{i}.{k}': v for i in (0, 1) for k, v in dst[i].items()}}), gs
