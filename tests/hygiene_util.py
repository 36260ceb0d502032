"""Helpers of tests/test_state_hygiene.py: caller-owned arenas with chosen previous contents, guard bands around every buffer that crosses the ABI, and
the runs whose results are compared bit for bit between them.  A plain module like parity_util.py.

ORDERING RULE (obeyed by every helper and test):
  * Memory is filled BEFORE fm_batch_bind and never between a bind and the calls that use it: the index tables live in the arena, and a kernel that
    follows a poisoned index is a fault the test would have caused.  (Filling an arena that a LATER bind will lay out anew is fine: that is 'history'.)
  * 'ones' (every f32 a NaN) runs after 'zero' and 'history' have passed for the same case in the same test.
  * A run that meets a GPU fault, abort or timeout stops there; nothing is retried.

GUARD BANDS.  BAND = 4096 bytes on either side is a condition, not a measurement: a write further out than 4096 bytes from a buffer is not seen.
The bytes between a payload's end and the next 256-byte boundary belong to the rear band, so a store one row past the end is seen."""
from __future__ import annotations

import ctypes as C

import torch

from flowmol_amd import _lib, presets, weights
from flowmol_amd.engine import (Engine, IntegrationRun, StepNoise, cat_temp_schedule, forward_weight_schedule, fm_prior_spec, make_step_plan, _ptr)
from oracle import cpu_ref
from parity_util import edge_perm, oracle_run, oracle_stage_tensors, out_of_tolerance, parity_stages, seeded_inputs, stage_errors

BAND = 4096
SENTINEL = 0xA5
FILL_BYTE = {'zero': 0x00, 'ones': 0xFF, 'history': 0x00}
HISTORY_PREDECESSORS = ([40, 3, 7], [3, 2])        # more pieces and more rows than any small case, then fewer: the second bind shifts every region


# ------------------------------------------------------------------------------------------------------------------ engines
_ENGINES = {}


def engine(preset, lib, device, tuning=None, precision=None, fresh=False):
    """(engine, cfg, state dict) of a preset with weights-by-name; cached per configuration unless ``fresh``."""
    key = (preset, id(lib), str(device), tuple(sorted((tuning or {}).items())), precision)
    if fresh or key not in _ENGINES:
        cfg = presets.PRESETS[preset]()
        sd = weights.synth_state_dict(cfg, 0)
        got = (Engine(cfg, sd, device=device, lib=lib, tuning=tuning, precision=precision), cfg, sd)
        if fresh:
            return got
        _ENGINES[key] = got
    return _ENGINES[key]


def model(preset, lib, device, ctmc_threads=0):
    """A FlowMol of the preset whose engine is built here (so that its workspace can be chosen)."""
    import flowmol_amd as flowmol
    kw = {'_engine_lib': lib} if lib is not None else {}
    m = flowmol.FlowMol.from_preset(preset, **kw).to(device)
    if ctmc_threads:
        m._engine = Engine(m.cfg, m._sd, device=m.device, prefix=m._prefix, lib=lib, tuning={'ctmc_threads': ctmc_threads})
    return m


# ------------------------------------------------------------------------------------------------------------------ arenas
def arena(eng, sizes_list, fill, history=None):
    """One uint8 tensor large enough for the largest fm_workspace_bytes of ``sizes_list`` plus BAND bytes in front and behind, WHOLLY filled with
    ``fill`` ('zero' | 'ones' = every byte 0xFF | 'history' = zero, then exactly what ``history(eng, ws)`` -- binds plus runs of other batches on the same
    engine -- left in it).  -> (the 256-aligned interior view, guards_intact()).  guards_intact(used=None): both bands still hold the fill byte, and
    (for the constant fills, given the bound batch's byte count) so does the interior beyond ``used``, which the bind did not hand to the library."""
    need = max(eng.workspace_need(torch.tensor(s)) for s in sizes_list)
    byte = FILL_BYTE[fill]
    raw = torch.full((BAND + 256 + need + BAND,), byte, dtype=torch.uint8, device=eng.device)
    off = BAND + (-(raw.data_ptr() + BAND)) % 256
    ws = raw[off:off + need]
    assert ws.data_ptr() % 256 == 0
    if fill == 'history':
        key = (need, getattr(history, '__name__', None))
        cache = eng.__dict__.setdefault('_hygiene_history', {})
        if key not in cache:
            history(eng, ws)
            eng.synchronize()
            cache[key] = ws.clone()
        else:
            ws.copy_(cache[key])

    def guards_intact(used=None):
        ok = bool((raw[:off] == byte).all()) and bool((raw[off + need:] == byte).all())
        if used is not None and fill != 'history':
            ok = ok and bool((ws[used:] == byte).all())
        return ok
    return ws, guards_intact


def forward_history(eng, ws):
    """Predecessors of the forward cases: a batch with more pieces and more rows, then one with fewer, each bound in ``ws`` and evaluated."""
    cfg = eng.cfg
    for sizes in HISTORY_PREDECESSORS:
        n = torch.tensor(sizes)
        eng.bind(n, workspace=ws)
        if cfg.has_mask:
            inp = seeded_inputs(cfg, n, True, seed=11)
            prev = None if inp['prev'] is None else {k: v.to(eng.device).contiguous() for k, v in inp['prev'].items()}
            eng.forward(eng.make_state(inp['x'], inp['a'], inp['c'], inp['eu']), 0.3, prev=prev)
        else:
            eng.forward_dense(dense_inputs(eng, 11), 0.3)
        eng.synchronize()


def sample_history(eng, ws):
    """Predecessors of the sampling cases: two Philox steps (tables, boot.*, CTMC scratch) of each predecessor batch."""
    cfg = eng.cfg
    for sizes in HISTORY_PREDECESSORS:
        eng.bind(torch.tensor(sizes), workspace=ws)
        if cfg.has_mask:
            eng.integrate(eng.prior_state(eng.prior_philox(3)), philox_plan(cfg, 3, 3, 'campbell'), None)
        else:
            eng.forward_dense(dense_inputs(eng, 11), 0.3)
        eng.synchronize()


# ------------------------------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """See guarded()."""

    def __init__(self, shape, dtype, device, init=None, is_input=False, name=''):
        self.name, self.is_input = name, is_input
        numel = 1
        for s in shape:
            numel *= int(s)
        self.nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        if self.nbytes == 0:          # zero rows: what the engine passes today (an empty tensor, a null pointer), no invented pointer and nothing to guard
            self.raw, self.t = None, torch.empty(*shape, dtype=dtype, device=device)
            return
        padded = (self.nbytes + 255) // 256 * 256
        self.raw = torch.full((BAND + padded + BAND,), SENTINEL, dtype=torch.uint8, device=device)
        self.t = self.raw[BAND:BAND + self.nbytes].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init.to(device=device, dtype=dtype).reshape(*shape))
        self.before = self.raw[BAND:BAND + self.nbytes].clone() if is_input else None
        self.had_init = init is not None

    def bands_intact(self):
        return self.raw is None or (bool((self.raw[:BAND] == SENTINEL).all()) and bool((self.raw[BAND + self.nbytes:] == SENTINEL).all()))

    def payload_unchanged(self):
        return self.raw is None or torch.equal(self.raw[BAND:BAND + self.nbytes], self.before)

    def unwritten(self):
        return self.raw is not None and bool((self.raw[BAND:BAND + self.nbytes] == SENTINEL).all())


def guarded(shape, dtype, device, init=None):
    """A tensor view with BAND = 4096 bytes of 0xA5 on either side inside ONE allocation; the payload is padded to 256 bytes (the padding counts as rear
    band), so its alignment is what torch gives the allocation.  Without ``init`` the payload starts as 0xA5 too.  Writes further than 4096 bytes away from
    the payload are not seen.  -> Guarded (``.t`` is the view)."""
    return Guarded(shape, dtype, device, init)


class GuardSet:
    """The guarded buffers of one run.  check() -> names of the buffers whose bands changed, and of the INPUTS whose payload changed;
    unwritten() -> names of the outputs (allocated without initial contents) that still hold nothing but 0xA5."""

    def __init__(self, device):
        self.device, self.items = device, []

    def _add(self, name, shape, dtype, init, is_input):
        g = Guarded(tuple(shape), dtype, self.device, init, is_input, name)
        self.items.append(g)
        return g.t

    def out(self, name, shape, dtype=torch.float32, init=None):
        return self._add(name, shape, dtype, init, False)

    def inp(self, name, tensor, dtype=None):
        return self._add(name, tensor.shape, dtype or tensor.dtype, tensor, True)

    def out_dict(self, prefix, shapes, dtype=torch.float32):
        return {k: self.out(f'{prefix}.{k}', s, dtype) for k, s in shapes.items()}

    def inp_dict(self, prefix, tensors, dtype=None):
        return None if tensors is None else {k: self.inp(f'{prefix}.{k}', v, dtype) for k, v in tensors.items()}

    def check(self):
        bad = [g.name + ':band' for g in self.items if not g.bands_intact()]
        return bad + [g.name + ':input' for g in self.items if g.is_input and not g.payload_unchanged()]

    def unwritten(self):
        return [g.name for g in self.items if not g.is_input and g.raw is not None and not g.had_init and g.unwritten()]


def cpu(d):
    return {k: v.detach().cpu().clone() for k, v in d.items() if v is not None}


def first_difference(a, b):
    """Name of the first tensor of two result dicts that is not bit-identical (NaN payloads included), or None."""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        if x.shape != y.shape or x.dtype != y.dtype or not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
            return k
    return None


def non_finite(res):
    return [k for k, v in res.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]


# ------------------------------------------------------------------------------------------------------------------ A / C: forward
def dst_shapes(eng):
    c = eng.cfg
    return {'x': (eng.N, 3), 'a': (eng.N, c.n_atom_types), 'c': (eng.N, c.n_charges), 'e': (eng.U, c.n_bond_types)}


def tap_shapes(eng, stages):
    V, out = eng.cfg.n_vec_channels, {}
    for k in stages:
        rows = eng.E if ('.msg.' in k or k.endswith('.ef')) else eng.N
        out[k] = (rows,) + ((3,) if k.endswith('.x') else (3, V) if k.endswith('.v') else (128,) if k.endswith('.ef') else (256,))
    return out


def forward_inputs(cfg, sizes, with_prev):
    return seeded_inputs(cfg, torch.tensor(sizes), with_prev)


def forward_run(eng, inp, t_val, ws, sizes):
    """Bind ``sizes`` in the arena ``ws`` and evaluate the seeded inputs twice with every buffer guarded: as the product does (no taps; the fused kernels),
    then with every tap of parity_util.parity_stages.  -> (results on the CPU: 'plain.x|a|c|e', 'out.x|a|c|e', the taps; the GuardSet; the stages)."""
    cfg, dev = eng.cfg, eng.device
    eng.bind(torch.tensor(sizes), workspace=ws)
    gs = GuardSet(dev)
    i32 = torch.int32
    state = {'x_t': gs.inp('state.x', inp['x']), 'a_t': gs.inp('state.a', inp['a'], i32), 'c_t': gs.inp('state.c', inp['c'], i32),
             'e_t': gs.inp('state.e', inp['eu'], i32)}
    prev = gs.inp_dict('prev', inp['prev'])
    bootstrap = (t_val == 0) and prev is None
    eng.profile(True)
    plain = eng.forward(state, t_val, prev=prev, bootstrap=bootstrap, out=gs.out_dict('plain', dst_shapes(eng)))
    eng.synchronize()
    fused_head = eng.profile_get('edge_update_head')[1] > 0
    eng.profile(False)
    stages = parity_stages(cfg, t_val, prev is not None, skip_last_ef=fused_head)
    taps = gs.out_dict('tap', tap_shapes(eng, stages))
    out = eng.forward(state, t_val, prev=prev, bootstrap=bootstrap, out=gs.out_dict('out', dst_shapes(eng)), taps=taps)
    eng.synchronize()
    res = {**{f'plain.{k}': v for k, v in plain.items()}, **{f'out.{k}': v for k, v in out.items()}, **taps}
    return cpu(res), gs, stages


def oracle_failures(eng, sd, inp, t_val, res, stages, stage_tol, out_tol):
    """The stages and outputs of a forward_run (engine still bound to that batch) that miss the parity tests' oracle gate (forward_compare's scoring)."""
    cfg = eng.cfg
    taps_o, ref = oracle_run(cpu_ref.OracleVF(cfg, sd), cfg, inp, t_val)
    want = oracle_stage_tensors(taps_o, ref, stages, edge_perm(eng, inp['batch']))
    got = {k: v for k, v in res.items() if not k.startswith('plain.') and v.numel() > 0}
    bad = out_of_tolerance(stage_errors(got, want), None, stage_tol, out_tol)
    plain = {'out.' + k[6:]: v for k, v in res.items() if k.startswith('plain.') and v.numel() > 0}
    bad.update({'plain.' + k[4:]: v for k, v in out_of_tolerance(stage_errors(plain, want), None, stage_tol, out_tol).items()})
    return bad


# ------------------------------------------------------------------------------------------------------------------ B / C: the other entry points
def philox_plan(cfg, T, seed, dfm_type, tspan=None):
    return make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cat_temp_schedule(cfg), dfm_type=dfm_type, tspan=tspan,
                          forward_weight_func=forward_weight_schedule(cfg), philox_seed=seed, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)


def tensor_plan(cfg, T, dfm_type):
    return make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cat_temp_schedule(cfg), dfm_type=dfm_type,
                          forward_weight_func=forward_weight_schedule(cfg), schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)


def sample_run(mdl, sizes, dfm_type, T=4, seed=31, mol_ids=None):
    """model.sample(rng='philox') with xt_traj / ep_traj frames -> final state and every frame, on the CPU."""
    kw = {} if mol_ids is None else {'mol_ids': mol_ids}
    out, _, frames = mdl.sample(torch.tensor(sizes), n_timesteps=T, rng='philox', seed=seed, dfm_type=dfm_type, return_tensors='device', xt_traj=True,
                                ep_traj=True, _frames=True, **kw)
    return cpu({**{f'final.{k}': v for k, v in out.items()}, **{f'frame.{k}': v for k, v in frames.items()}})


def noise_tape(cfg, N, U, plan, dfm_type, seed=5):
    """The tensor noise of every step of ``plan`` from one seeded CPU generator, drawn once and shared by the runs that are compared."""
    gen = torch.Generator().manual_seed(seed)
    return [StepNoise.draw(N, U, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types, bool(sc.last_step), 'cpu', generator=gen, dfm_type=dfm_type)
            for sc in plan.scalars]


def guarded_noise(gs, nz, tag):
    return StepNoise(**{k: (None if getattr(nz, k) is None else gs.inp(f'{tag}.{k}', getattr(nz, k))) for k in nz.__slots__})


def sink_shapes(eng, n_steps):
    N, U = eng.N, eng.U
    return ({'x': (n_steps, N, 3), 'x1': (n_steps, N, 3)},
            {'a': (n_steps, N), 'c': (n_steps, N), 'e': (n_steps, U), 'a1': (n_steps, N), 'c1': (n_steps, N), 'e1': (n_steps, U)})


def guarded_integration(eng, gs, state, plan, noise_for_step, n_steps):
    """An IntegrationRun whose two endpoint buffers, time embeddings and eight sinks are guarded."""
    f32, i32 = sink_shapes(eng, n_steps)
    traj = {**gs.out_dict('sink', f32), **gs.out_dict('sink', i32, torch.int32)}
    run = IntegrationRun(eng, state, plan, noise_for_step, traj=traj)
    run.dst = [gs.out_dict('dst0', dst_shapes(eng)), gs.out_dict('dst1', dst_shapes(eng))]
    run._dsts = [eng._dst_struct(run.dst[0]), eng._dst_struct(run.dst[1])]
    run.temb_all = gs.inp('temb', run.temb_all)
    return run, traj


def prior_x0(N, seed=9):
    return torch.randn(N, 3, generator=torch.Generator().manual_seed(seed))


def guarded_prior_state(eng, gs, x0):
    """The masked CTMC prior around x0; updated in place by fm_integrate / fm_ctmc_step by contract, so registered as an output."""
    st = eng.prior_state(x0)
    return {k: gs.out(f'state.{k}', v.shape, v.dtype, init=v) for k, v in st.items()}


def integrate_run(eng, sizes, dfm_type, ws, T=6):
    """Tensor-noise Engine.integrate of T - 1 steps with all eight sinks, everything guarded -> (results, GuardSet)."""
    cfg = eng.cfg
    eng.bind(torch.tensor(sizes), workspace=ws)
    gs = GuardSet(eng.device)
    plan = tensor_plan(cfg, T, dfm_type)
    tape = noise_tape(cfg, eng.N, eng.U, plan, dfm_type)
    noises = [guarded_noise(gs, nz, f'noise{i}') for i, nz in enumerate(tape)]
    state = guarded_prior_state(eng, gs, prior_x0(eng.N))
    run, traj = guarded_integration(eng, gs, state, plan, lambda i, last: noises[i], T - 1)
    run.run(0, T - 1)
    eng.synchronize()
    res = {**{f'state.{k}': v for k, v in state.items()}, **{f'sink.{k}': v for k, v in traj.items()}, **{f'last.{k}': v for k, v in run.last_dst().items()}}
    return cpu(res), gs


def seeded_dst(cfg, N, U, seed=13):
    gen = torch.Generator().manual_seed(seed)
    return {'x': torch.randn(N, 3, generator=gen), 'a': torch.softmax(2 * torch.randn(N, cfg.n_atom_types, generator=gen), -1),
            'c': torch.softmax(2 * torch.randn(N, cfg.n_charges, generator=gen), -1), 'e': torch.softmax(2 * torch.randn(U, cfg.n_bond_types, generator=gen), -1)}


def ctmc_step_run(eng, sizes, dfm_type, ws):
    """One fm_ctmc_step (step 1 of a 4-point plan: neither first nor last) on a half-masked state with ``sampled`` -> (results, GuardSet)."""
    cfg = eng.cfg
    eng.bind(torch.tensor(sizes), workspace=ws)
    gs = GuardSet(eng.device)
    plan = tensor_plan(cfg, 4, dfm_type)
    nz = guarded_noise(gs, noise_tape(cfg, eng.N, eng.U, plan, dfm_type)[1], 'noise')
    inp = seeded_inputs(cfg, torch.tensor(sizes), False, seed=17, frac_masked=0.5)
    st = eng.make_state(inp['x'], inp['a'], inp['c'], inp['eu'])
    state = {k: gs.out(f'state.{k}', v.shape, v.dtype, init=v) for k, v in st.items()}
    dst = gs.inp_dict('dst', seeded_dst(cfg, eng.N, eng.U))
    smp = gs.out_dict('sampled', {'a1': (eng.N,), 'c1': (eng.N,), 'e1': (eng.U,)}, torch.int32)
    eng.ctmc_step(state, dst, nz, plan.scalars[1], smp)
    eng.synchronize()
    return cpu({**{f'state.{k}': v for k, v in state.items()}, **{f'sampled.{k}': v for k, v in smp.items()}}), gs


def small_calls_run(eng, sizes, ws):
    """prior_philox, philox_tape (a campbell and a gat step), stability and every batch query, straight through the ABI into guarded buffers
    (the Engine methods of these calls allocate their own results) -> (results, GuardSet)."""
    cfg, lib, ctx = eng.cfg, eng.lib, eng._ctx
    eng.bind(torch.tensor(sizes), workspace=ws)
    gs = GuardSet(eng.device)
    N, U, E, B = eng.N, eng.U, eng.E, eng.B
    res = {}
    with eng._dev():
        x0 = gs.out('x0', (N, 3))
        eng._check(lib.fm_prior_philox(ctx, eng._stream(), C.c_uint64(21), _ptr(x0)), 'fm_prior_philox')
        res['x0'] = x0
        for dfm_type, step in (('campbell', 1), ('gat', 0)):
            sc = philox_plan(cfg, 4, 21, dfm_type).scalars[step]
            gat, out = dfm_type == 'gat', {}
            for tag, rows, k in (('a', N, cfg.n_atom_types), ('c', N, cfg.n_charges), ('e', U, cfg.n_bond_types)):
                out[f'q_{tag}'] = gs.out(f'tape.{dfm_type}.q_{tag}', (rows, k + 1 if gat else k))
                if not gat:
                    out[f'u1_{tag}'] = gs.out(f'tape.{dfm_type}.u1_{tag}', (rows,))
                    out[f'u2_{tag}'] = gs.out(f'tape.{dfm_type}.u2_{tag}', (rows,))
            cs = StepNoise(**out).c_struct()
            eng._check(lib.fm_philox_tape(ctx, eng._stream(), C.byref(sc), C.byref(cs)), 'fm_philox_tape')
            res.update({f'tape.{dfm_type}.{k}': v for k, v in out.items()})
        inp = seeded_inputs(cfg, torch.tensor(sizes), False, seed=19, frac_masked=0.1)
        state = {'x_t': gs.inp('stab.x', inp['x']), 'a_t': gs.inp('stab.a', inp['a'], torch.int32), 'c_t': gs.inp('stab.c', inp['c'], torch.int32),
                 'e_t': gs.inp('stab.e', inp['eu'], torch.int32)}
        table = gs.inp('stab.table', torch.randint(0, 256, (cfg.n_atom_types, cfg.n_charges), generator=torch.Generator().manual_seed(23)), torch.int32)
        stab = gs.out('stability', (B, 4), torch.int32)
        st = eng._state_struct(state)
        eng._check(lib.fm_stability(ctx, eng._stream(), C.byref(st), _ptr(table), cfg.n_atom_types, -1, 0, _ptr(stab)), 'fm_stability')
        res['stability'] = stab
        for name, cnt in (('e_src', E), ('e_dst', E), ('e_pair', E), ('p_e0', U), ('p_e1', U), ('node_mol', N), ('pair_mol', U)):
            q = gs.out(f'query.{name}', (cnt,), torch.int32)
            if cnt:
                eng._check(lib.fm_batch_query(ctx, eng._stream(), name.encode(), _ptr(q)), 'fm_batch_query')
            res[f'query.{name}'] = q
    eng.synchronize()
    return cpu(res), gs


def dense_inputs(eng, seed):
    cfg, gen = eng.cfg, torch.Generator().manual_seed(seed)
    return eng.make_dense_state(torch.randn(eng.N, 3, generator=gen), torch.softmax(torch.randn(eng.N, cfg.n_atom_types, generator=gen), -1),
                                torch.softmax(torch.randn(eng.N, cfg.n_charges, generator=gen), -1), torch.softmax(torch.randn(eng.U, cfg.n_bond_types, generator=gen), -1))


def endpoint_run(eng, sizes, ws):
    """An endpoint-parameterised model: prior_philox_dense (through the ABI, guarded outputs) -> forward_dense -> endpoint_step -> (results, GuardSet)."""
    cfg = eng.cfg
    eng.bind(torch.tensor(sizes), workspace=ws)
    gs = GuardSet(eng.device)
    shapes = {f'{k}_t': s for k, s in dst_shapes(eng).items()}
    prior = gs.out_dict('prior', shapes)
    spec = fm_prior_spec()
    for i, tag in enumerate('ace'):
        kind, kw = cfg.prior_types[tag], cfg.prior_kwargs.get(tag, {}) or {}
        if kind in ('marginal', 'c-given-a'):          # these read a distribution tensor: the gaussian kind exercises the same stores without one
            kind, kw = 'gaussian', {}
        m = spec.mod[i]
        m.kind, m.std = _lib.FM_PRIOR_KINDS[kind], float(kw.get('std', 0.2 if kind == 'biased-simplex' else 1.0))
        m.simplex_center, m.has_blur, m.blur = int(bool(kw.get('simplex_center', False))), int(kw.get('blur') is not None), float(kw.get('blur') or 0.0)
        m.vertex_prob, m.vertex_idx = float(kw.get('vertex_prob', 0.75)), int(kw.get('vertex_idx', 0))
    ds = eng._dense_struct(prior)
    with eng._dev():
        eng._check(eng.lib.fm_prior_philox_dense(eng._ctx, eng._stream(), C.c_uint64(77), C.byref(spec), C.byref(ds)), 'fm_prior_philox_dense')
    eng.synchronize()
    res = {f'prior.{k}': v.detach().cpu().clone() for k, v in prior.items()}
    state = {k: gs.inp(f'state.{k}', v) for k, v in prior.items()}
    out = eng.forward_dense(state, 0.25, out=gs.out_dict('out', dst_shapes(eng)))
    eng.synchronize()
    bad = gs.check()                                  # forward_dense must not touch its state: checked before endpoint_step updates a copy of it
    stepped = {k: gs.out(f'stepped.{k}', v.shape, v.dtype, init=v) for k, v in state.items()}
    dst = gs.inp_dict('dst', out)
    eng.endpoint_step(stepped, dst, 0.25, [1.3, 1.1, 0.9, 0.7], 1.2)
    eng.synchronize()
    res.update(cpu({**{f'out.{k}': v for k, v in out.items()}, **{f'stepped.{k}': v for k, v in stepped.items()}}))
    return res, gs, bad


# ------------------------------------------------------------------------------------------------------------------ D: call patterns
def chunked_run(eng, sizes, dfm_type, T, chunk, ws, seed=41, profile=False):
    """A Philox trajectory of T - 1 steps with all sinks, cut into fm_integrate calls of ``chunk`` steps
    -> (final state, last endpoint prediction and every frame on the CPU; GuardSet; embed_table launches when profiled)."""
    cfg = eng.cfg
    eng.bind(torch.tensor(sizes), workspace=ws)
    gs = GuardSet(eng.device)
    plan = philox_plan(cfg, T, seed, dfm_type)
    state = guarded_prior_state(eng, gs, eng.prior_philox(seed))
    run, traj = guarded_integration(eng, gs, state, plan, None, T - 1)
    if profile:
        eng.profile(True)
    run.run(0, T - 1, chunk=chunk)
    eng.synchronize()
    launches = None
    if profile:
        launches = eng.profile_get('embed_table')[1]
        eng.profile(False)
    res = {**{f'state.{k}': v for k, v in state.items()}, **{f'sink.{k}': v for k, v in traj.items()}, **{f'last.{k}': v for k, v in run.last_dst().items()}}
    return cpu(res), gs, launches
