"""``SamplingQueue``: requests join a batch that is already integrating (no reference counterpart: the reference's ``sample`` starts and ends a
batch together).  One molecule costs about as much per step as eight, so a stream of small requests is served by admitting each newcomer into the
running batch instead of running them back to back.

Built on per-molecule time (``Engine.integrate_mixed``) and the per-molecule Philox streams: every molecule is, bit for bit, the molecule
``model.sample([n], n_timesteps=T, rng='philox', seed=seed, mol_ids=[id])`` run alone, whenever it was admitted and whoever it shared the batch with.
``submit_from`` admits GIVEN molecules the same way: corrupted to a chosen step of their schedule (``FlowMol.resample``), they join from there.
Synchronous and single-stream: ``run`` returns when its steps have run; admission happens at the start of a ``run`` call."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _lib
from .engine import IntegrationRun, alpha_tables, make_step_plan
from .model import _check_coupling, _keep_rows, _pairs_of_atoms


class _Request:
    __slots__ = ('ticket', 'n', 'T', 'mol_id', 'pos', 'state', 'prev', 'given', 'keep', 'spec', 'coupling')

    def __init__(self, ticket, n, T, mol_id, start=0, given=None, keep=None, coupling='independent'):
        self.ticket, self.n, self.T, self.mol_id = ticket, n, T, mol_id
        self.pos = start      # the step it takes next: steps taken, or where a given molecule (submit_from) enters its schedule
        self.given = given    # submit_from: the molecule to corrupt {'x_t', 'a_t', 'c_t', 'e_t'} (CPU); None: start from the prior
        self.keep = keep      # submit_from(keep=...): (n,) bool, the atoms that stay as given, or {modality: its rows' bools}; None: nothing frozen
        self.coupling = coupling      # submit_from(coupling=...): how the position prior is paired with the given molecule (Engine.conditional_path)
        self.spec = None      # its rows of Engine.inpaint_spec / freeze_spec, on the device, from admission on
        self.state = None     # {'x_t', 'a_t', 'c_t', 'e_t'}: this molecule's rows, on the device
        self.prev = None      # {'x', 'a', 'c', 'e'}: its previous endpoint prediction


class SamplingQueue:
    def __init__(self, model, seed: int, stochasticity=None, high_confidence_threshold=None, **kwargs):
        """``model``: a CTMC ``FlowMol`` on its device; ``seed``: the Philox seed of every request.  ``kwargs``: cat_temp_func / forward_weight_func /
        inv_temp_func of ``FlowMol.sample``."""
        model._check_mixed({'rng': 'philox', **kwargs})
        self.model, self.seed = model, int(seed)
        self._plan_args, self._plan_kw = model._plan_args(stochasticity, high_confidence_threshold, kwargs)
        self._plans: Dict[int, object] = {}
        self._pending: List[_Request] = []
        self._running: List[_Request] = []
        self._finished: Dict[int, object] = {}
        self._next_ticket = 0

    # ------------------------------------------------------------------ requests
    def submit(self, n_atoms, n_timesteps=None, mol_ids=None) -> List[int]:
        """Queue molecules of the given sizes; returns one ticket per molecule.  ``n_timesteps``: an int for all of them (default: the model's) or one per
        molecule; ``mol_ids``: their Philox stream ids (default: the ticket numbers).  They are admitted by the next ``run``."""
        sizes = [int(v) for v in torch.as_tensor(n_atoms).reshape(-1).tolist()]
        if n_timesteps is None:
            n_timesteps = self.model.default_n_timesteps
        Ts = [int(n_timesteps)] * len(sizes) if isinstance(n_timesteps, int) else [int(v) for v in n_timesteps]
        ids = None if mol_ids is None else [int(v) for v in torch.as_tensor(mol_ids).reshape(-1).tolist()]
        if len(Ts) != len(sizes) or (ids is not None and len(ids) != len(sizes)):
            raise ValueError('n_timesteps / mol_ids must give one entry per molecule')
        if any(n < 1 for n in sizes) or any(T < 1 for T in Ts):
            raise ValueError('n_atoms and n_timesteps must be >= 1')
        tickets = []
        for i, (n, T) in enumerate(zip(sizes, Ts)):
            t = self._next_ticket
            self._next_ticket += 1
            self._pending.append(_Request(t, n, T, t if ids is None else ids[i]))
            tickets.append(t)
        return tickets

    def submit_from(self, molecules, start_step, n_timesteps=None, mol_ids=None, keep=None, coupling='independent') -> List[int]:
        """Queue given molecules for resampling (``FlowMol.resample``): molecule *i* is corrupted to time point ``start_step[i]`` of its
        ``n_timesteps[i]``-point schedule at admission and joins the running batch from there; ``start_step >= n_timesteps - 1`` retires at once with the
        corrupted state.  ``molecules`` / ``start_step`` / ``n_timesteps`` / ``mol_ids`` as in ``resample`` (ids default to the ticket numbers).  Every
        molecule is, bit for bit, ``model.resample([mol], start_step, n_timesteps, seed, mol_ids=[id])``.  ``keep``: the atoms that stay as given, as in
        ``resample`` -- such molecules are admitted into the running batch like any other and are, bit for bit, their ``resample(..., keep=...)`` run alone.
        Both forms of ``keep`` are taken; a batch that holds requests of both is served in the per-modality form, of which the whole-atom form is a case.
        ``coupling`` ('independent' | 'ot') as in ``resample``: requests of either kind share the running batch, a coupling only decides the prior a
        molecule's path starts from."""
        x1, n_atoms = self.model._given_molecules(molecules)
        _check_coupling(coupling, n_atoms, 'submit_from')
        sizes = n_atoms.tolist()
        B = len(sizes)
        n_pairs = [n * (n - 1) // 2 for n in sizes]
        keep = _keep_rows(keep, n_atoms)
        if isinstance(keep, dict):          # per modality: every molecule gets the modalities in which it has a frozen row
            cols = {f: torch.split(v, n_pairs if f == 'e' else sizes) for f, v in keep.items()}
            kept = [{f: c[i] for f, c in cols.items() if bool(c[i].any())} or None for i in range(B)]
        else:
            kept = list(torch.split(keep, sizes)) if keep is not None else [None] * B
            kept = [k if k is not None and bool(k.any()) else None for k in kept]
        per = lambda v, default: ([int(default if v is None else v)] * B if v is None or isinstance(v, int) or (torch.is_tensor(v) and v.dim() == 0)
                                  else [int(x) for x in v])
        ks, Ts = per(start_step, 0), per(n_timesteps, self.model.default_n_timesteps)
        ids = None if mol_ids is None else [int(v) for v in torch.as_tensor(mol_ids).reshape(-1).tolist()]
        if len(ks) != B or len(Ts) != B or (ids is not None and len(ids) != B):
            raise ValueError('start_step / n_timesteps / mol_ids must give one entry per molecule')
        if any(T < 1 or k < 0 or k > T - 1 for k, T in zip(ks, Ts)):
            raise ValueError('start_step must lie in 0 .. n_timesteps - 1 (and n_timesteps >= 1)')
        cols = {f: torch.split(v, n_pairs if f == 'e_t' else sizes) for f, v in x1.items()}
        tickets = []
        for i in range(B):
            t = self._next_ticket
            self._next_ticket += 1
            self._pending.append(_Request(t, sizes[i], Ts[i], t if ids is None else ids[i], ks[i], {f: cols[f][i] for f in x1}, kept[i], coupling))
            tickets.append(t)
        return tickets

    @property
    def idle(self) -> bool:
        return not self._pending and not self._running

    def pop_finished(self) -> Dict[int, object]:
        """{ticket: SampledMolecule} of the molecules that have finished since the last call."""
        out, self._finished = self._finished, {}
        return out

    # ------------------------------------------------------------------ the batch
    def _plan(self, T: int):
        if T not in self._plans:
            self._plans[T] = make_step_plan(T, *self._plan_args, philox_seed=self.seed, **self._plan_kw)
        return self._plans[T]

    @staticmethod
    def _split(d, sizes, pair_key):
        pairs = [n * (n - 1) // 2 for n in sizes]
        cols = {k: torch.split(v, pairs if k == pair_key else sizes) for k, v in d.items()}
        return [{k: cols[k][i] for k in d} for i in range(len(sizes))]

    @staticmethod
    def _split_spec(spec, sizes):
        """The per-molecule rows of an ``Engine.inpaint_spec`` / ``freeze_spec`` dict (views; a modality the spec leaves out stays None)."""
        pairs = [n * (n - 1) // 2 for n in sizes]
        cols = {k: torch.split(v, pairs if k in ('keep_pair', 'keep_e', 'e1', 'u_e') else sizes) for k, v in spec.items() if v is not None}
        return [{k: (cols[k][i] if k in cols else None) for k in spec} for i in range(len(sizes))]

    @staticmethod
    def _modal(keep):
        """A request's ``keep`` in the per-modality form: the whole-atom form freezes x, a, c of its atoms and the pairs between two of them."""
        return keep if isinstance(keep, dict) else {'x': keep, 'a': keep, 'c': keep, 'e': _pairs_of_atoms(keep)}

    _SPEC_ROWS = {'x0': (torch.float32, lambda n, u: (n, 3)), 'x1c': (torch.float32, lambda n, u: (n, 3)), 'a1': (torch.int32, lambda n, u: (n,)),
                  'c1': (torch.int32, lambda n, u: (n,)), 'e1': (torch.int32, lambda n, u: (u,)), 'u_a': (torch.float32, lambda n, u: (n,)),
                  'u_c': (torch.float32, lambda n, u: (n,)), 'u_e': (torch.float32, lambda n, u: (u,))}
    _OWNER = {'x0': 'x', 'x1c': 'x', 'a1': 'a', 'c1': 'c', 'e1': 'e', 'u_a': 'a', 'u_c': 'c', 'u_e': 'e'}

    def _batch_spec(self, run):
        """The running batch's spec from its molecules' rows; a molecule without frozen rows contributes zero flags (its other rows are never read).
        Whole-atom requests alone give an ``inpaint_spec``; as soon as one request is per modality the batch is a ``freeze_spec``, in which a whole-atom
        request's rows stand as x = a = c = its atoms, e = the pairs between two of them, and a modality nobody freezes stays None."""
        if all(r.spec is None for r in run):
            return None
        dev = self.model.engine.device
        zeros = lambda r, dt, shp: torch.zeros(shp(r.n, r.n * (r.n - 1) // 2), dtype=dt, device=dev)
        u8 = torch.uint8
        if all('keep_atom' in r.spec for r in run if r.spec is not None):
            shapes = {'keep_atom': (u8, lambda n, u: (n,)), 'keep_pair': (u8, lambda n, u: (u,)), **self._SPEC_ROWS}
            return {k: torch.cat([r.spec[k] if r.spec is not None else zeros(r, dt, shp) for r in run]).contiguous() for k, (dt, shp) in shapes.items()}
        flags = {r.ticket: {f: v.to(u8).to(dev) for f, v in self._modal(r.keep).items()} for r in run if r.spec is not None}
        live = {f for fl in flags.values() for f in fl}
        spec = {name: None for name, _ in _lib.fm_freeze._fields_}
        for f in live:
            shp = (lambda n, u: (u,)) if f == 'e' else (lambda n, u: (n,))
            spec[f'keep_{f}'] = torch.cat([flags[r.ticket][f] if r.spec is not None and f in flags[r.ticket] else zeros(r, u8, shp) for r in run]).contiguous()
        for k, (dt, shp) in self._SPEC_ROWS.items():
            if self._OWNER[k] in live:
                spec[k] = torch.cat([r.spec[k] if r.spec is not None and r.spec.get(k) is not None else zeros(r, dt, shp) for r in run]).contiguous()
        return spec

    def _admit(self):
        """Newcomers, grouped by schedule and entry step, take their first step through fm_integrate on a bind of their own -- from the prior (step 0:
        bootstrap evaluation, first step) or, for given molecules, from their conditional path (step k, no previous endpoint) -- then they join the
        running list, as long as the batch keeps to the 32 time groups a bind has embedding tables for."""
        eng, cfg = self.model.engine, self.model.cfg
        groups = {(r.T, r.pos) for r in self._running}         # a time group = same schedule, same step
        by_key: Dict[tuple, List[_Request]] = {}
        keep = []
        for r in self._pending:
            joins = r.pos + 1 < r.T - 1                        # otherwise the first step is the rest of the trajectory
            if joins and (r.T, r.pos + 1) not in groups and len(groups) >= _lib.FM_TAB_SLOTS:
                keep.append(r)                                 # waits for a group to finish
                continue
            if joins:
                groups.add((r.T, r.pos + 1))
            by_key.setdefault((r.T, r.pos, r.given is not None, r.coupling), []).append(r)
        self._pending = keep
        for (T, k, given, coupling), reqs in by_key.items():
            sizes, spec = [r.n for r in reqs], None
            eng.bind(torch.tensor(sizes))
            eng.set_molecule_ids(torch.tensor([r.mol_id for r in reqs]))
            if given:
                x1 = {f: torch.cat([r.given[f] for r in reqs]) for f in ('x_t', 'a_t', 'c_t', 'e_t')}
                alpha = alpha_tables(torch.linspace(0, 1, T), cfg.schedule_type, cfg.cosine_params)[0][k]
                st1 = eng.make_state(x1['x_t'], x1['a_t'], x1['c_t'], x1['e_t'])
                state = eng.conditional_path(st1, alpha, seed=self.seed, coupling=coupling)
                if any(isinstance(r.keep, dict) for r in reqs):          # one per-modality request: the group's first step runs in that form
                    none = lambda r, f: torch.zeros(r.n * (r.n - 1) // 2 if f == 'e' else r.n, dtype=torch.bool)
                    modal = [self._modal(r.keep) if r.keep is not None else {} for r in reqs]
                    live = [f for f in 'xace' if any(f in m for m in modal)]
                    spec = eng.freeze_spec(st1, {f: torch.cat([m[f] if f in m else none(r, f) for r, m in zip(reqs, modal)]) for f in live}, self.seed, coupling=coupling)
                elif any(r.keep is not None for r in reqs):
                    spec = eng.inpaint_spec(st1, torch.cat([r.keep if r.keep is not None else torch.zeros(r.n, dtype=torch.bool) for r in reqs]), self.seed, coupling=coupling)
            else:
                state = eng.prior_state(eng.prior_philox(self.seed))
            prev = None
            if k < T - 1:
                run = IntegrationRun(eng, state, self._plan(T), None, inpaint=spec)
                run.run(k, k + 1)
                prev = run.last_dst()
            eng.synchronize()
            st, pv = self._split(state, sizes, 'e_t'), (self._split(prev, sizes, 'e') if prev is not None else [None] * len(reqs))
            sp = self._split_spec(spec, sizes) if spec is not None else [None] * len(reqs)
            for r, s_, p_, q_ in zip(reqs, st, pv, sp):
                r.state, r.prev, r.pos, r.given, r.spec = s_, p_, min(k + 1, T - 1), None, (q_ if r.keep is not None else None)
                (self._running if r.pos < T - 1 else self._done).append(r)

    def _retire(self, reqs):
        for r in reqs:
            out = {k: r.state[f'{k}_t'].cpu() for k in 'xace'}
            self._finished[r.ticket] = self.model._package(out, torch.tensor([r.n]), None, False, False)[0]

    def run(self, max_steps: Optional[int] = None) -> int:
        """Admit the pending requests, then advance the running batch by up to ``max_steps`` steps (default: until every running molecule has
        finished).  Returns the number of steps taken; molecules that finish inside the call wait, untouched, until it returns."""
        self._done: List[_Request] = []
        if self._pending:
            self._admit()
        k = self._advance(max_steps) if self._running else 0
        self._retire(self._done)
        return k

    def _advance(self, max_steps) -> int:
        run = self._running
        left = max(r.T - 1 - r.pos for r in run)
        k = left if max_steps is None else min(int(max_steps), left)
        if k <= 0:
            return 0
        eng = self.model.engine
        sizes = [r.n for r in run]
        eng.bind(torch.tensor(sizes))
        eng.set_molecule_ids(torch.tensor([r.mol_id for r in run]))
        keys = sorted({(r.T, r.pos) for r in run})
        state = {f: torch.cat([r.state[f] for r in run]).contiguous() for f in ('x_t', 'a_t', 'c_t', 'e_t')}
        prev = {f: torch.cat([r.prev[f] for r in run]).contiguous() for f in 'xace'}
        spec = self._batch_spec(run)
        plans, group, start = [self._plan(T) for T, _ in keys], [keys.index((r.T, r.pos)) for r in run], [pos for _, pos in keys]
        if spec is not None:
            dst = eng.integrate_inpaint(state, plans, group, spec, start=start, n_steps=k, prev=prev)
        else:
            dst = eng.integrate_mixed(state, plans, group, start=start, n_steps=k, prev=prev)
        still = []
        for r, s_, p_ in zip(run, self._split(state, sizes, 'e_t'), self._split(dst, sizes, 'e')):
            r.state, r.prev, r.pos = s_, p_, min(r.pos + k, r.T - 1)
            (still if r.pos < r.T - 1 else self._done).append(r)
        self._running = still
        return k
