"""Helpers of tests/test_freeze_modalities.py: frozen rows per modality (fm_ctmc_step_freeze / fm_integrate_freeze, Engine.freeze_spec / ctmc_step_freeze /
integrate_freeze, FlowMol.resample(keep={...}) / conformers, SamplingQueue.submit_from(keep={...})).  A plain module like inpaint_util.py, whose cases, cached
engines and compositions it reuses: the reference of every check is the plain step (or the ABI-12 call) and a host torch.where per modality."""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from flowmol_amd.engine import StepNoise, _ptr, fm_sampled, make_step_plan, mixed_step_arrays
from hygiene_util import GuardSet, cpu, dst_shapes

import inpaint_util as iu
import mixed_util as mu
import resample_util as ru

MODS = 'xace'


def rows_of(sizes):
    n = torch.tensor(list(sizes))
    return int(n.sum()), int((n * (n - 1) // 2).sum())


def random_masks(sizes, seed=7, p=0.5):
    """Four INDEPENDENT masks from a fixed generator: {'x', 'a', 'c': (N,), 'e': (U,)} bool."""
    gen = torch.Generator().manual_seed(seed)
    N, U = rows_of(sizes)
    return {f: torch.rand(U if f == 'e' else N, generator=gen) < p for f in MODS}


def pair_atoms(sizes):
    """(U, 2) the two atoms (indices into the concatenated atoms) of every unordered pair, upper-triangle order per molecule."""
    out, off = [], 0
    for n in sizes:
        out += [(off + i, off + j) for i in range(n) for j in range(i + 1, n)]
        off += n
    return torch.tensor(out, dtype=torch.long).reshape(-1, 2)


def per_molecule(masks, sizes):
    """The masks as the API's per-molecule form: {modality: [one bool list per molecule]}."""
    pairs = [n * (n - 1) // 2 for n in sizes]
    return {f: [[bool(v) for v in blk] for blk in torch.split(m, pairs if f == 'e' else list(sizes))] for f, m in masks.items()}


def take_masks(masks, sizes, idx):
    """The masks of the molecules ``idx`` (a list), in that order."""
    pairs = [n * (n - 1) // 2 for n in sizes]
    cols = {f: torch.split(m, pairs if f == 'e' else list(sizes)) for f, m in masks.items()}
    return {f: torch.cat([cols[f][i] for i in idx]) for f in masks}


def full_masks(masks, sizes):
    """Every modality present: a missing one is all-False (the host overwrite then leaves it alone)."""
    N, U = rows_of(sizes)
    return {f: masks[f] if f in masks else torch.zeros(U if f == 'e' else N, dtype=torch.bool) for f in MODS}


def step_case(lib, device, threads):
    """inpaint_util.step_case (the qm9 preset bound to 1, 2, 5, 24, 47 atoms; state, path, alpha_next, endpoint prediction) with four independent masks and
    their freeze_spec."""
    case = iu.step_case(lib, device, threads)

    def make():
        eng = rebind(case)
        masks = random_masks(case['sizes'])
        return {**case, 'masks': masks, 'fspec': eng.freeze_spec(case['x1'], masks, case['seed'])}
    return mu.cached(('freeze-step', id(lib), str(device), threads), make)


def rebind(case):
    eng = case['eng']
    eng.bind(torch.tensor(case['sizes']))
    eng.set_molecule_ids(torch.tensor(list(iu.KERNEL_IDS)))
    return eng


def plain_step(case, dfm_type, philox, hc, last):
    """The plain step of the case (fm_ctmc_step) and its sampled tokens, on the cpu: computed once per configuration and shared, never modified."""
    def make():
        eng = rebind(case)
        sc = iu.step_scalars(case, dfm_type, philox, hc, last)
        nz = StepNoise() if philox else iu.tensor_noise(eng, bool(last), dfm_type)
        plain, smp = iu.clone(case['state']), iu.sampled_buffers(eng)
        eng.ctmc_step(plain, case['dst'], nz, sc, smp)
        eng.synchronize()
        return cpu(plain), cpu(smp)
    return mu.cached(('freeze-plain', id(case['eng']), dfm_type, philox, hc, last), make)


def freeze_step(case, spec, dfm_type, philox, hc, last):
    """One Engine.ctmc_step_freeze (or, for an inpaint_spec, ctmc_step_inpaint) on a clone of the case's state -> (state, sampled tokens) on the cpu."""
    eng = rebind(case)
    sc = iu.step_scalars(case, dfm_type, philox, hc, last)
    nz = StepNoise() if philox else iu.tensor_noise(eng, bool(last), dfm_type)
    got, smp = iu.clone(case['state']), iu.sampled_buffers(eng)
    (eng.ctmc_step_inpaint if 'keep_atom' in spec else eng.ctmc_step_freeze)(got, case['dst'], nz, sc, spec, case['alpha_next'], smp)
    eng.synchronize()
    return cpu(got), cpu(smp)


def composed(plain, path, masks):
    """where(flag_f, conditional_path(alpha_next) rows, plain rows) per modality, on a copy."""
    want = {k: v.clone() for k, v in plain.items()}
    for f, m in masks.items():
        want[f'{f}_t'][m] = path[f'{f}_t'][m]
    return want


# ------------------------------------------------------------------------------------------------------------------ integration: inpaint_util's compositions
def traj_masks(sizes, seed=19):
    """Independent masks for the trajectory checks (5, 3, 2, 1 atoms; any sizes): drawn at p = 0.5, then every modality is given one frozen and one free row."""
    masks = random_masks(sizes, seed)
    for f in MODS:
        if masks[f].numel() > 1:
            masks[f][0], masks[f][-1] = True, False
    return masks


@contextlib.contextmanager
def modal_compositions(masks):
    """inpaint_util.single_runs / mixed_runs / oracle_inpaint with the per-modality spec and masks in place of the whole-atom ones: those functions take their spec and
    their frozen rows from traj_setup / frozen_masks, which are swapped here for the length of the block -- the compositions themselves (one-step calls with the
    previous endpoint carried, host overwrite from Engine.conditional_path) run unchanged, through fm_integrate_freeze."""
    def traj_setup(mdl, sizes, ids, seed):
        eng = mdl.engine
        eng.bind(torch.tensor(sizes))
        eng.set_molecule_ids(torch.tensor(ids))
        x1 = ru.as_state(eng, ru.given(mdl.cfg, sizes))
        return eng, x1, None, eng.freeze_spec(x1, masks, seed), full_masks(masks, sizes)
    saved = iu.traj_setup, iu.frozen_masks
    iu.traj_setup, iu.frozen_masks = traj_setup, (lambda sizes, keep_atom: full_masks(masks, sizes))
    try:
        yield
    finally:
        iu.traj_setup, iu.frozen_masks = saved


# ------------------------------------------------------------------------------------------------------------------ the API
def resample_tensors(mdl, mols, k, T, seed, ids, keep, **kw):
    return iu.resample_tensors(mdl, mols, k, T, seed, ids, keep, **kw)


def repeat(mols, K):
    """The (tensors, n_atoms) pair with every molecule repeated K times, molecule-major."""
    return ru.take(mols, [i for i in range(int(mols[1].numel())) for _ in range(K)])


# ------------------------------------------------------------------------------------------------------------------ the raw ABI, guarded
def guarded_spec(gs, eng, x1, masks, seed):
    """The fm_freeze members between guard bands, all of them inputs."""
    spec = eng.freeze_spec(x1, masks, seed)
    eng.synchronize()
    return {k: (gs.inp(f'fz.{k}', v.cpu()) if v is not None else None) for k, v in spec.items()}


def guarded_step(eng, ws, sizes, ids, masks, seed, T=6, i=2):
    """One fm_ctmc_step_freeze call (campbell, Philox) through ctypes, every pointer between 4096-byte bands, the batch bound in the arena ``ws``."""
    cfg, dev = eng.cfg, eng.device
    eng.bind(torch.tensor(sizes), workspace=ws)
    eng.set_molecule_ids(torch.tensor(ids))
    x1 = ru.as_state(eng, ru.given(cfg, sizes))
    gs, i32 = GuardSet(dev), torch.int32
    spec = guarded_spec(gs, eng, x1, masks, seed)
    st0 = eng.conditional_path(x1, ru.alpha_row(cfg, T, i), seed=seed)
    state = {f: gs.out(f'state.{f}', tuple(v.shape), v.dtype, init=v) for f, v in st0.items()}
    dst = gs.inp_dict('dst', iu.softmax_dst(eng))
    smp = {'a1': gs.out('smp.a1', (eng.N,), i32), 'c1': gs.out('smp.c1', (eng.N,), i32), 'e1': gs.out('smp.e1', (eng.U,), i32)}
    plan = make_step_plan(T, 2.0, 0.9, cfg.cat_temperature, philox_seed=seed, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)
    sc = plan.scalars[i]
    st, d, fz, sm = eng._state_struct(state), eng._dst_struct(dst), eng._freeze_struct(spec), fm_sampled()
    sm.a1, sm.c1, sm.e1 = _ptr(smp['a1']), _ptr(smp['c1']), _ptr(smp['e1'])
    al = (C.c_float * 4)(*ru.alpha_row(cfg, T, i + 1).tolist())
    rc = eng.lib.fm_ctmc_step_freeze(eng._ctx, eng._stream(), C.byref(st), C.byref(d), None, C.byref(sc), C.byref(sm), C.byref(fz), al)
    eng._check(rc, 'fm_ctmc_step_freeze')
    eng.synchronize()
    return cpu({**state, **smp}), gs


def guarded_integrate(mdl, ws, sizes, ids, pairs, masks, seed):
    """One fm_integrate_freeze call with one (T, k) per molecule, every pointer guarded, the batch bound in the arena ``ws``."""
    eng, cfg = mdl.engine, mdl.cfg
    dev = eng.device
    eng.bind(torch.tensor(sizes), workspace=ws)
    eng.set_molecule_ids(torch.tensor(ids))
    x1 = ru.as_state(eng, ru.given(cfg, sizes))
    keys = sorted(set(pairs))
    grp = [keys.index(p) for p in pairs]
    plans = mu.philox_plans(mdl, [T for T, _ in keys], seed)
    tabs = [iu.alpha_table(eng, p) for p in plans]
    start = [k for _, k in keys]
    n, G = max(T - 1 - k for T, k in keys), len(keys)
    scal, act, temb = mixed_step_arrays(plans, start, n, cfg.time_embedding_dim)
    al = torch.zeros(n, G, 4)
    for j in range(n):
        for g in range(G):
            al[j, g] = tabs[g][min(start[g] + j + 1, tabs[g].shape[0] - 1)]
    gs, i32 = GuardSet(dev), torch.int32
    spec = guarded_spec(gs, eng, x1, masks, seed)
    st0 = eng.conditional_path(x1, torch.stack([tabs[g][start[g]] for g in range(G)]), grp if G > 1 else None, seed=seed)
    state = {f: gs.out(f'state.{f}', tuple(v.shape), v.dtype, init=v) for f, v in st0.items()}
    dst = [gs.out_dict(f'dst{i}', dst_shapes(eng)) for i in (0, 1)]
    scal_dev = gs.inp('steps', torch.frombuffer(bytearray(bytes(scal)), dtype=torch.uint8))
    act_dev = gs.inp('active', torch.tensor(list(act), dtype=i32))
    group = gs.inp('mol_group', torch.tensor(grp, dtype=i32))
    temb_dev = gs.inp('temb', temb)
    al_dev = gs.inp('alpha_next', al)
    al_host = al.contiguous()
    st, ds, fz = eng._state_struct(state), [eng._dst_struct(d) for d in dst], eng._freeze_struct(spec)
    final = C.c_int(-1)
    rc = eng.lib.fm_integrate_freeze(eng._ctx, eng._stream(), C.byref(st), n, G, scal, _ptr(scal_dev), act, _ptr(act_dev), _ptr(group), _ptr(temb_dev), None,
                                     None, C.byref(ds[0]), C.byref(ds[1]), None, C.byref(final), C.byref(fz),
                                     C.cast(C.c_void_p(al_host.data_ptr()), C.POINTER(C.c_float)), _ptr(al_dev))
    eng._check(rc, 'fm_integrate_freeze')
    eng.synchronize()
    assert final.value in (0, 1)
    return cpu({**state, **{f'dst{i}.{k}': v for i in (0, 1) for k, v in dst[i].items()}}), gs
