"""Helpers of tests/test_mixed_time.py: per-molecule time (fm_forward_mixed / fm_integrate_mixed, FlowMol.sample with one step count per molecule,
SamplingQueue).  A plain module like parity_util.py, from which it takes the scoring; what it restates are the two helpers that take ONE time for the
whole batch (oracle_run, engine_stages), here with the reference's (B,) time tensor."""
from __future__ import annotations

import ctypes as C

import torch

import flowmol_amd as flowmol
from flowmol_amd import presets, weights
from flowmol_amd.engine import Engine, _ptr, mixed_step_arrays
from hygiene_util import GuardSet, arena, cpu, dst_shapes, first_difference, tap_shapes
from oracle import cpu_ref
from parity_util import _dx_gates_from, add_dx_stages, edge_perm, onehots, oracle_stage_tensors, parity_stages, seeded_inputs, slice_molecule, stage_errors, visible_weights

FORWARD_SIZES = [5, 9, 12, 3, 2]
FORWARD_T = [0.15, 0.4, 0.65, 0.9, 0.3]          # one time per molecule, none 0 (no bootstrap), in no order

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def model(preset, lib, device, **tuning):
    """A FlowMol of the preset with weights-by-name (cached); ``tuning``: fm_config overrides of its engine (ctmc_threads, tile_edge, ...)."""
    def make():
        kw = {'_engine_lib': lib} if lib is not None else {}
        m = flowmol.FlowMol.from_preset(preset, **kw).to(device)
        if tuning:
            m._engine = Engine(m.cfg, m._sd, device=m.device, prefix=m._prefix, lib=lib, tuning=tuning)
        return m
    return cached(('model', preset, id(lib), str(device), tuple(sorted(tuning.items()))), make)


def engine(preset, lib, device, visible=False, **tuning):
    """(engine, cfg, state dict), weights-by-name as drawn or under parity_util.visible_weights (cached)."""
    def make():
        cfg = presets.PRESETS[preset]()
        sd = weights.synth_state_dict(cfg, 0)
        if visible:
            sd = visible_weights(preset, sd)
        return Engine(cfg, sd, device=device, lib=lib, tuning=tuning or None), cfg, sd
    return cached(('engine', preset, id(lib), str(device), visible, tuple(sorted(tuning.items()))), make)


# ------------------------------------------------------------------------------------------------------------------ forward
def forward_stages(eng, cfg, inp, t):
    """One instrumented evaluation of ``inp`` (seeded_inputs; bound here) at time ``t`` -- a number, or a (B,) tensor -> ({stage: tensor on the cpu}
    with the taps of parity_stages() and the outputs 'out.x|a|c|e', the stages).  The last EdgeUpdate's rows are not tapped (asking would select the
    unfused edge head): `out.e` checks them."""
    dev = eng.device
    eng.bind(inp['batch'].n_atoms)
    state = eng.make_state(inp['x'], inp['a'], inp['c'], inp['eu'])
    prev = None if inp['prev'] is None else {k: v.to(dev).contiguous() for k, v in inp['prev'].items()}
    stages = parity_stages(cfg, 1.0, prev is not None, skip_last_ef=True)         # 1.0: not a bootstrap evaluation
    bufs = {k: torch.zeros(*s, device=dev) for k, s in tap_shapes(eng, stages).items()}
    out = eng.forward(state, t, prev=prev, bootstrap=False, remove_com=True, taps=bufs)
    eng.synchronize()
    got = {k: v.cpu() for k, v in bufs.items()}
    got.update({'out.' + k: out[k].cpu() for k in 'xace'})
    return got, stages


def oracle_run_t(orc, cfg, inp, t, dtype=torch.float32):
    """parity_util.oracle_run with the reference's per-graph time: ``t`` of shape (B,)."""
    batch, prev = inp['batch'], inp['prev']
    a1h, c1h, e1h = onehots(cfg, batch, inp['a'], inp['c'], inp['eu'])
    orc.taps = {}
    try:
        torch.set_default_dtype(dtype)
        with torch.no_grad():
            ref = orc.forward(batch, inp['x'].to(dtype), a1h.to(dtype), c1h.to(dtype), e1h.to(dtype), t.to(dtype),
                              prev=None if prev is None else {k: v.to(dtype) for k, v in prev.items()}, apply_softmax=True, remove_com=True)
    finally:
        torch.set_default_dtype(torch.float32)
    taps_o, orc.taps = orc.taps, None
    return taps_o, ref


def dx_gates_t(cfg, sd, inp, t):
    """parity_util.dx_gates for a (B,) time: the oracle in float32 against the oracle in float64 on the same inputs."""
    res = {}
    for dt in (torch.float32, torch.float64):
        try:
            torch.set_default_dtype(dt)
            orc = cpu_ref.OracleVF(cfg, sd)
        finally:
            torch.set_default_dtype(torch.float32)
        orc.p = {k: v.to(dt) for k, v in orc.p.items()}
        taps_o, out = oracle_run_t(orc, cfg, inp, t, dt)
        res[dt] = dict(taps_o)
        res[dt].update({f'out.{k}': v for k, v in out.items()})
        add_dx_stages(res[dt], cfg, inp)
    return _dx_gates_from(res[torch.float32], res[torch.float64])[0]


def forward_case(preset, lib, device, sizes=FORWARD_SIZES, times=FORWARD_T, visible=False, **tuning):
    """The mixed-time evaluation of the seeded inputs (with ``prev`` where the model is self-conditioned), computed once per configuration and shared:
    {'inp', 't', 'got', 'stages', 'eng', 'cfg', 'sd'}."""
    def make():
        eng, cfg, sd = engine(preset, lib, device, visible, **tuning)
        inp = seeded_inputs(cfg, torch.tensor(sizes), True)
        t = torch.tensor(times, dtype=torch.float32)
        got, stages = forward_stages(eng, cfg, inp, t)
        return {'inp': inp, 't': t, 'got': got, 'stages': stages, 'eng': eng, 'cfg': cfg, 'sd': sd}
    return cached(('forward', preset, id(lib), str(device), tuple(sizes), tuple(times), visible, tuple(sorted(tuning.items()))), make)


def oracle_errors(case, dx):
    """{stage: relative error} of a forward_case against cpu_ref.forward(t = the (B,) tensor); dx: with the displacement stages."""
    eng, cfg, inp = case['eng'], case['cfg'], case['inp']
    taps_o, ref = oracle_run_t(cpu_ref.OracleVF(cfg, case['sd']), cfg, inp, case['t'])
    eng.bind(inp['batch'].n_atoms)
    want = oracle_stage_tensors(taps_o, ref, case['stages'], edge_perm(eng, inp['batch']))
    got = dict(case['got'])
    if dx:
        add_dx_stages(got, cfg, inp)
        add_dx_stages(want, cfg, inp)
    return stage_errors(got, want)


def molecule_rows(sizes, m, stage):
    """Rows of molecule ``m`` in a stage tensor of the batch: node rows, directed-edge rows (internal order: a molecule's n (n - 1) rows are contiguous)
    or, for `out.e`, unordered pairs."""
    n = [int(v) for v in sizes]
    if stage == 'out.e':
        per = [k * (k - 1) // 2 for k in n]
    elif '.msg.' in stage or stage.endswith('.ef'):
        per = [k * (k - 1) for k in n]
    else:
        per = n
    return slice(sum(per[:m]), sum(per[:m + 1]))


def alone_differences(case):
    """Every molecule of a forward_case evaluated alone at its own time through the existing forward (a float t) -> [(molecule, stage)] that are not
    bit-identical to the molecule's rows in the mixed-time evaluation."""
    eng, cfg, inp, sizes = case['eng'], case['cfg'], case['inp'], case['inp']['batch'].n_atoms.tolist()
    bad = []
    for m in range(len(sizes)):
        got, _ = forward_stages(eng, cfg, slice_molecule(inp, m), float(case['t'][m]))
        for k, v in got.items():
            if not torch.equal(v, case['got'][k][molecule_rows(sizes, m, k)]):
                bad.append((m, k))
    return bad


# ------------------------------------------------------------------------------------------------------------------ trajectories
def split_molecules(out, sizes):
    """A batch's result dict {'x','a','c','e'} as one dict per molecule."""
    sizes = [int(v) for v in sizes]
    pairs = [n * (n - 1) // 2 for n in sizes]
    cols = {k: torch.split(out[k].cpu(), pairs if k == 'e' else sizes) for k in 'xace'}
    return [{k: cols[k][i].clone() for k in 'xace'} for i in range(len(sizes))]


def sample_alone(mdl, n, T, seed, mol_id, **kw):
    """Molecule ``mol_id`` on its own through the existing path: sample([n], n_timesteps=T, rng='philox', seed, mol_ids=[mol_id])."""
    out = mdl.sample(torch.tensor([n]), n_timesteps=int(T), rng='philox', seed=seed, mol_ids=[mol_id], return_tensors=True, **kw)[0]
    return {k: out[k].clone() for k in 'xace'}


def alone_runs(preset, lib, device, sizes, Ts, seed, **kw):
    """The alone runs of a case, computed once and shared between the tests that compare against them (launch tuning does not change their bits)."""
    return cached(('alone', preset, id(lib), str(device), tuple(sizes), tuple(Ts), seed, tuple(sorted(kw.items()))),
                  lambda: [sample_alone(model(preset, lib, device), n, T, seed, i, **kw) for i, (n, T) in enumerate(zip(sizes, Ts))])


def molecule_differences(got, want):
    """[(molecule, field)] of two per-molecule result lists that are not bit-identical."""
    same = lambda k, g, w: torch.equal(g, w) if k == 'x' else torch.equal(g.long(), w.long())        # tokens travel as int32, bytes or int64
    return [(i, k) for i, (g, w) in enumerate(zip(got, want)) for k in 'xace' if not same(k, g[k], w[k])]


def moved_from_prior(mols, cfg):
    """The runs did unmask something: the comparison is not of untouched priors."""
    mask = {'a': cfg.n_atom_types, 'c': cfg.n_charges, 'e': cfg.n_bond_types}
    return any(bool((m[k] != mask[k]).any()) for m in mols for k in 'ace')


# ------------------------------------------------------------------------------------------------------------------ the raw ABI, guarded
def philox_plans(mdl, Ts, seed):
    from flowmol_amd.engine import make_step_plan
    args, kw = mdl._mixed_plan_args(None, None, {})
    return [make_step_plan(T, *args, philox_seed=seed, **kw) for T in Ts]


def guarded_mixed_run(mdl, sizes, Ts, seed, fill):
    """One fm_integrate_mixed call through ctypes with EVERY pointer of the call -- state, the two endpoint buffers, the per-(step, group) scalars and
    active flags, mol_group, the time embeddings -- between 4096-byte 0xA5 bands and the batch bound in an arena filled with ``fill``.
    -> (final state on the cpu, guard failures, arena intact)."""
    eng, cfg = mdl.engine, mdl.cfg
    dev = eng.device
    ws, intact = arena(eng, [sizes], fill)
    eng.bind(torch.tensor(sizes), workspace=ws)
    eng.set_molecule_ids(None)
    distinct = sorted(set(Ts))
    plans = philox_plans(mdl, distinct, seed)
    n = max(len(p.scalars) for p in plans)
    scal, act, temb = mixed_step_arrays(plans, [0] * len(plans), n, cfg.time_embedding_dim)
    gs = GuardSet(dev)
    x0 = eng.prior_philox(seed)
    i32 = torch.int32
    state = {'x_t': gs.out('state.x_t', (eng.N, 3), init=x0),
             'a_t': gs.out('state.a_t', (eng.N,), i32, init=torch.full((eng.N,), cfg.n_atom_types)),
             'c_t': gs.out('state.c_t', (eng.N,), i32, init=torch.full((eng.N,), cfg.n_charges)),
             'e_t': gs.out('state.e_t', (eng.U,), i32, init=torch.full((eng.U,), cfg.n_bond_types))}
    dst = [gs.out_dict(f'dst{i}', dst_shapes(eng)) for i in (0, 1)]
    scal_dev = gs.inp('steps', torch.frombuffer(bytearray(bytes(scal)), dtype=torch.uint8))
    act_dev = gs.inp('active', torch.tensor(list(act), dtype=i32))
    group = gs.inp('mol_group', torch.tensor([distinct.index(T) for T in Ts], dtype=i32))
    temb_dev = gs.inp('temb', temb)
    st, ds = eng._state_struct(state), [eng._dst_struct(d) for d in dst]
    final = C.c_int(-1)
    rc = eng.lib.fm_integrate_mixed(eng._ctx, eng._stream(), C.byref(st), n, len(plans), scal, _ptr(scal_dev), act, _ptr(act_dev), _ptr(group), _ptr(temb_dev),
                                    None, C.byref(ds[0]), C.byref(ds[1]), None, C.byref(final))
    eng._check(rc, 'fm_integrate_mixed')
    eng.synchronize()
    assert final.value in (0, 1)
    res = cpu({k[:1]: v for k, v in state.items()})
    return res, gs.check(), intact(eng.workspace_bytes)
