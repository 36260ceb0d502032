"""``FlowMol``: the sampling-side drop-in for the reference's LightningModule
(reference flowmol/models/flowmol.py: ``sample_random_sizes`` 473-486, ``sample`` 489-589,
``sample_n_atoms`` 468-471, ``build_n_atoms_dist`` 461-466) backed by the HIP engine.

    import flowmol_amd as flowmol
    model = flowmol.load_pretrained('flowmol3').cuda().eval()
    mols = model.sample_random_sizes(n_molecules=10, n_timesteps=250)

``denoising_loss`` is the reference's ``forward`` (297-415, what ``validation_step`` logs).  Training, optimizers and the chemistry metrics are
out of scope.
"""
from __future__ import annotations

import json
import os
import pickle
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import _lib, presets, shard
from .config import VFConfig, from_reference_hparams
from .engine import Engine, IntegrationRun, StepNoise, alpha_tables, cat_temp_schedule, forward_weight_schedule, make_step_plan
from .molecule import SampledMolecule
from .priors import (adapt_prior, categorical_prior, default_marginals, draw_categorical_priors,          # noqa: F401  (re-exported)
                     load_marginal_dists, simplex_projection)
from .stereo import stereo_elements
from .symmetry import automorphisms
from .weights import synth_state_dict

PKG = Path(__file__).resolve().parent


def load_n_atoms_hist(name: str):
    data = json.loads((PKG / 'data' / 'n_atoms_hist.json').read_text())
    if name not in data:
        raise KeyError(f'no size histogram named {name!r}; have {sorted(data)}')
    return torch.tensor(data[name]['n_atoms'], dtype=torch.int64), torch.tensor(data[name]['counts'], dtype=torch.int64)


class _Lenient(pickle.Unpickler):
    """Unpickler for Lightning checkpoints without Lightning installed: unknown classes
    (pytorch_lightning AttributeDict & co.) become plain dict / object stand-ins."""
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except Exception:
            if 'AttributeDict' in name or name.endswith('Dict'):
                return dict
            return type(name, (), {'__setstate__': lambda self, st: self.__dict__.update(st if isinstance(st, dict) else {})})


class _LenientPickle:
    Unpickler = _Lenient
    __name__ = 'lenient_pickle'

    @staticmethod
    def load(f, **kw):
        return _Lenient(f, **kw).load()


def read_checkpoint(path):
    """Lightning-free reader of ``<model_dir>/checkpoints/last.ckpt``: returns (hyper_parameters, state_dict)
    (reference flowmol/__init__.py:54-55 -> FlowMol.load_from_checkpoint)."""
    ck = torch.load(str(path), map_location='cpu', weights_only=False, pickle_module=_LenientPickle)
    if 'state_dict' not in ck or 'hyper_parameters' not in ck:
        raise ValueError(f'{path}: not a Lightning checkpoint (need state_dict and hyper_parameters)')
    return dict(ck['hyper_parameters']), ck['state_dict']


SUPPORTED_PARAMETERIZATIONS = ('ctmc', 'endpoint')
SUPPORTED_SCHEDULES = ('linear', 'cosine')


ENDPOINT_PRIORS = ('gaussian', 'uniform-simplex', 'barycenter', 'biased-simplex', 'marginal', 'c-given-a')     # priors.py:253-262 minus x / ctmc


def check_reference_hparams(hp: dict) -> None:
    """Reject -- loudly, before any weight is touched -- every checkpoint configuration the HIP path does not reproduce, so that
    no model is ever integrated with the wrong schedule or prior.  Missing keys take the REFERENCE's defaults
    (FlowMol.__init__ flowmol.py:29-55: parameterization='endpoint'; InterpolantScheduler interpolant_scheduler.py:9:
    schedule_type='cosine'), so a checkpoint that relies on an unimplemented default is rejected too."""
    par = hp.get('parameterization', 'endpoint')
    if par not in SUPPORTED_PARAMETERIZATIONS:
        raise NotImplementedError(f"parameterization={par!r}: implemented: {SUPPORTED_PARAMETERIZATIONS}")
    isc = hp.get('interpolant_scheduler_config', {}) or {}
    st = isc.get('schedule_type', 'cosine')
    types = [st.get(f, 'cosine') for f in 'xace'] if isinstance(st, dict) else [st]
    bad = sorted({t for t in types if t not in SUPPORTED_SCHEDULES})
    if bad:
        raise NotImplementedError(f'interpolant schedule_type {bad}: implemented: {SUPPORTED_SCHEDULES} '
                                  '(any other schedule would be integrated with the wrong x and unmasking coefficients)')
    pc = hp.get('prior_config', {}) or {}
    xt = (pc.get('x', {}) or {}).get('type', 'centered-normal')
    if xt != 'centered-normal':
        raise NotImplementedError(f"position prior {xt!r}: only 'centered-normal' is implemented (a 'gaussian' prior would be centred silently)")
    for mod in ('a', 'c', 'e'):
        mt = (pc.get(mod, {}) or {}).get('type')
        if par == 'ctmc' and (mt or 'ctmc') != 'ctmc':
            raise NotImplementedError('only ctmc masked priors are supported for CTMC models (as in the reference, flowmol.py:189-193)')
        if par == 'endpoint' and mt not in ENDPOINT_PRIORS:
            raise NotImplementedError(f"categorical prior {mt!r} of an endpoint model: implemented: {ENDPOINT_PRIORS}")
        if par == 'endpoint' and mt == 'c-given-a' and mod != 'c':
            raise ValueError("the 'c-given-a' prior is the charge prior (flowmol.py:437-438)")
    if hp.get('exclude_charges', False):
        raise NotImplementedError('exclude_charges=True is not implemented (no shipped v3 model uses it)')


class FlowMol:
    canonical_feat_order = ['x', 'a', 'c', 'e']

    def __init__(self, cfg: VFConfig, state_dict: Dict[str, torch.Tensor], prefix: str = 'vector_field.',
                 n_atoms_hist: Optional[str] = None, _engine_lib=None, precision: Optional[str] = None, canonical: bool = True):
        self.cfg = cfg.validate()
        # canonical arithmetic (fm_config.canonical, default on): a molecule's coordinates and tokens are bit-for-bit independent of the batch it is sampled in
        # (size, position, sharding over GPUs) -- the reference's semantics, where every reduction is per molecule.  canonical=False: the one launch
        # choice that selects another summation order (the pair slab) follows the batch size too; differently composed batches then agree to f32 summation
        # order only.  (Up to round 5 this was a "latency mode"; since the small-batch kernels keep the canonical order it gains ~1 %: 0.55 vs 0.56 ms per step.)
        self.canonical = bool(canonical)
        self.precision = precision or 'f32'  # 'f16x3' / 'bf16x3' / 'bf16x6' = opt-in split precision (Engine); explicit argument only, recorded in last_timing
        self._sd = state_dict
        self._prefix = prefix
        self._lib = _engine_lib
        self.atom_type_map = list(cfg.atom_type_map)
        self.n_atom_types = cfg.n_atom_types
        self.n_atom_charges = cfg.n_charges
        self.n_bond_types = cfg.n_bond_types
        self.fake_atoms = cfg.fake_atoms
        self.explicit_aromaticity = cfg.explicit_aromaticity
        self.default_n_timesteps = cfg.default_n_timesteps
        self.parameterization = cfg.parameterization
        self.device = torch.device('cpu')
        self._engine: Optional[Engine] = None
        self.last_timing: Dict[str, object] = {}
        self.loss_hparams: Dict[str, object] = {}      # the checkpoint's loss settings (load_from_checkpoint); presets have none: denoising_loss defaults to off
        self.build_n_atoms_dist(n_atoms_hist or cfg.n_atoms_hist)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_preset(cls, name: str = 'flowmol3', seed: int = 0, **kw) -> "FlowMol":
        """Architecture ``name`` with deterministic weights-by-name (no checkpoint ships with the reference)."""
        cfg = presets.PRESETS[name]()
        sd = {'vector_field.' + k: v for k, v in synth_state_dict(cfg, seed).items()}
        return cls(cfg, sd, **kw)

    @classmethod
    def load_from_checkpoint(cls, ckpt_path, **kw) -> "FlowMol":
        hp, sd = read_checkpoint(ckpt_path)
        check_reference_hparams(hp)
        model = cls(from_reference_hparams(hp), sd, **kw)
        # what FlowMol.forward reads besides the network (flowmol.py:29-55, the reference's defaults for missing keys): the defaults of denoising_loss
        defaults = {'time_scaled_loss': True, 'weight_ae': False, 'target_blur': 0.0, 'distort_p': 0.0, 'distort_t': 0.5, 'total_loss_weights': None}
        model.loss_hparams = {k: hp.get(k, v) for k, v in defaults.items()}
        # the dataset pairs x_1 with an OT-aligned prior when prior_config.x.align is set (priors.py:267-303): the default coupling of denoising_loss
        model.loss_hparams['prior_align_x'] = bool(((hp.get('prior_config') or {}).get('x') or {}).get('align', False))
        return model

    # nn.Module-ish conveniences of the documented usage (readme.md:44-49)
    def to(self, device) -> "FlowMol":
        device = torch.device(device)
        if device != self.device or self._engine is None:
            if self._engine is not None:
                self._engine.close()
                self._engine = None
            self.device = device
        if device.type == 'cuda':
            self.engine          # like nn.Module.to(): the weights are repacked and uploaded NOW (fm_create), not inside the first sample() call
        return self

    def cuda(self, device=None) -> "FlowMol":
        return self.to('cuda:0' if device is None else (f'cuda:{device}' if isinstance(device, int) else device))

    def eval(self) -> "FlowMol":
        return self

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            if self.device.type != 'cuda' and self._lib is None:
                raise RuntimeError('flowmol_amd runs on MI355X only: move the model to a GPU with .cuda() '
                                   '(there is no CPU implementation of the sampling path)')
            self._engine = Engine(self.cfg, self._sd, device=self.device, prefix=self._prefix, lib=self._lib, precision=self.precision,
                                  tuning=None if self.canonical else {'canonical': -1})
        return self._engine

    # ------------------------------------------------------------------ sizes
    def build_n_atoms_dist(self, n_atoms_hist):
        """flowmol.py:461-466."""
        if isinstance(n_atoms_hist, (str, Path)) and str(n_atoms_hist).endswith('.pt'):
            n_atoms, counts = torch.load(str(n_atoms_hist))
        else:
            n_atoms, counts = load_n_atoms_hist(str(n_atoms_hist))
        self.n_atoms_dist = torch.distributions.Categorical(probs=counts / counts.sum())
        self.n_atoms_map = n_atoms

    def sample_n_atoms(self, n_molecules: int, **kwargs):
        """flowmol.py:468-471 (draws on the CPU generator like the reference)."""
        return self.n_atoms_map[self.n_atoms_dist.sample((n_molecules,), **kwargs)]

    _categorical_prior = staticmethod(categorical_prior)

    # ------------------------------------------------------------------ sampling
    # One call runs five stages, each one function: _request (arguments) -> bind -> _initial_state (prior) -> _plan_args + the engine's
    # integrator -> _finish (to host, package).  sample_distributed and SamplingQueue enter the same stages.
    def sample_random_sizes(self, n_molecules: int, device=None, stochasticity=None, high_confidence_threshold=None,
                            xt_traj=False, ep_traj=False, **kwargs) -> List[SampledMolecule]:
        atoms_per_molecule = self.sample_n_atoms(n_molecules)
        return self.sample(atoms_per_molecule, device=device, stochasticity=stochasticity,
                           high_confidence_threshold=high_confidence_threshold, xt_traj=xt_traj, ep_traj=ep_traj, **kwargs)

    @torch.no_grad()
    def sample_distributed(self, n_atoms: torch.Tensor, n_timesteps: int = None, group=None, return_tensors=False,
                           noise: str = 'per_rank', **kwargs):
        """Multi-GPU sampling (no reference counterpart): every rank of ``group`` calls this with the
        SAME ``n_atoms``; the molecules are dealt to the ranks by cost (``shard.partition_lpt``), each rank integrates its
        shard on its own GPU with no communication, and ONE all-gather of the packed results (``shard.gather_results``,
        RCCL over xGMI with backend "nccl") gives every rank the full batch in the caller's order.

        ``noise='per_rank'``: each rank draws only its shard's noise from its own torch RNG stream (seed it per rank);
        results depend on the world size.  ``noise='replicated'`` (parity mode): every rank, seeded identically, draws the
        full batch's prior and per-step noise and keeps its molecules' rows, so the result reproduces the single-GPU
        ``sample(n_atoms)`` with that seed (to float summation order), at world_size times the (cheap) RNG work.
        ``noise='philox'`` (performance mode): prior and CTMC noise are drawn INSIDE the kernels from per-molecule Philox4x32-10
        streams keyed by (seed, original molecule index, step, modality): no noise tensors at all, and every molecule's
        trajectory is the same for any world size or batch composition -- bit for bit with canonical arithmetic (the default).
        It covers every model family: campbell and gat CTMC steps, and the priors of endpoint-parameterised models.

        Everything one ``sample()`` call of the reference takes (flowmol.py:489-493) shards too: ``prior`` (a reference-format prior dict of the WHOLE
        batch: every rank keeps its molecules' rows, flowmol.py:534-545) and ``xt_traj`` / ``ep_traj`` (flowmol.py:564-589, test.py:212-257): each rank
        records its shard's frames in HBM in the compact token format and a SECOND all-gather (``shard.gather_frames``; only when trajectories
        are asked for) gives every rank the full batch's frames in the caller's order."""
        req = self._request(n_atoms, n_timesteps, kwargs, noise=noise)       # every refusal before the first collective
        n_atoms = req.n_atoms
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        parts = shard.partition_lpt(n_atoms, world)
        dev = self.engine.device
        xt_traj, ep_traj = bool(kwargs.pop('xt_traj', False)), bool(kwargs.pop('ep_traj', False))
        visualize = xt_traj or ep_traj
        if kwargs.get('prior') is not None:
            kwargs['prior'] = shard.slice_prior(kwargs['prior'], n_atoms, parts[rank])
        if noise == 'replicated':
            pairs = n_atoms * (n_atoms - 1) // 2
            mine = parts[rank]
            node_rows = shard._ranges((torch.cumsum(n_atoms, 0) - n_atoms)[mine], n_atoms[mine]).to(dev)
            pair_rows = shard._ranges((torch.cumsum(pairs, 0) - pairs)[mine], pairs[mine]).to(dev)
            kwargs['_rows'] = (int(n_atoms.sum()), int(pairs.sum()), node_rows, pair_rows)
        if noise == 'philox':
            # performance mode of SURVEY.md section 8e: per-molecule counter-based streams keyed by (seed, ORIGINAL molecule index, step,
            # modality); rank 0's seed is broadcast; nothing but the shard's own noise is generated, and it is generated in-kernel
            # ``seed=`` / ``mol_ids=`` (the same on every rank; ids of the WHOLE batch, default 0..B-1) fix the streams from outside
            if kwargs.get('seed') is None:
                seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
                sd = seed.to(dev if dist.get_backend(group) == 'nccl' else 'cpu')
                dist.broadcast(sd, src=0, group=group)
                kwargs['seed'] = int(sd.item())
            ids = kwargs.get('mol_ids')
            kwargs.update(rng='philox', mol_ids=parts[rank] if ids is None else torch.as_tensor(ids)[parts[rank]])
        local_frames = None
        if len(parts[rank]):
            got = self.sample(n_atoms[parts[rank]], n_timesteps=n_timesteps, return_tensors='device', xt_traj=visualize, _frames=visualize, **kwargs)   # stays in HBM
            local, local_frames = got[0], (got[2] if visualize else None)
        else:
            i32 = dict(dtype=torch.int32, device=dev)
            local = {'x': torch.zeros(0, 3, device=dev), 'a': torch.zeros(0, **i32), 'c': torch.zeros(0, **i32), 'e': torch.zeros(0, **i32)}
        full_dev = shard.gather_results(local, n_atoms, parts, group=group)
        frames_dev = shard.gather_frames(local_frames, n_atoms, parts, req.n_points, dev, group=group) if visualize else None
        return self._finish({f'{k}_t': v for k, v in full_dev.items()}, n_atoms, frames_dev, return_tensors, visualize, xt_traj, ep_traj)

    @torch.no_grad()
    def sample(self, n_atoms: torch.Tensor, n_timesteps: int = None, device=None, stochasticity=None,
               high_confidence_threshold=None, xt_traj=False, ep_traj=False, prior=None, return_tensors=False,
               **kwargs):
        """Sample molecules with the given numbers of atoms (flowmol.py:489-589).

        RNG use mirrors the reference: ``randn(N,3)`` on the device for the position prior, then per step
        and per modality (a, c, e) ``Exp(1)`` of shape (rows, K), ``rand(rows)``, ``rand(rows)`` (the last
        one skipped on the final step).  Endpoint-parameterised models (EndpointVectorField.integrate, vector_field.py:388-499: the categorical
        modalities are continuous vectors integrated with the same Euler step as the positions; the sampled molecule takes their argmax) draw
        ``randn(N,3)`` on the device, then the a, c, e priors on the CPU generator, and nothing per step.

        ``rng='philox'`` instead draws the prior and every step's noise inside the kernels from per-molecule counter-based streams
        (campbell and gat steps, and the priors of endpoint-parameterised models): no noise tensors, and a molecule's result depends only on
        ``seed=`` (default: one draw from torch's CPU generator) and on its id in ``mol_ids=`` (default 0..B-1), not on its batch.  So
        ``model.sample(n_atoms[i:i+1], rng='philox', seed=s, mol_ids=[i])`` regenerates molecule *i* of an earlier
        ``model.sample(n_atoms, rng='philox', seed=s)`` on its own, bit for bit with canonical arithmetic (the default).

        ``n_timesteps`` may be a sequence of B ints, one per molecule (``rng='philox'``, campbell CTMC models): molecules with equal counts form a
        time group, the groups advance together in one batch (one bind, one fm_integrate_mixed call) and a finished molecule waits until the call
        ends; ``n_timesteps[i] == 1`` returns molecule *i*'s prior.  Molecule *i* is, bit for bit,
        ``model.sample(n_atoms[i:i+1], n_timesteps=n_timesteps[i], rng='philox', seed=s, mol_ids=[i])``.
        Raises NotImplementedError for more than 32 distinct counts, rng='torch', dfm_type 'gat', endpoint models, xt_traj / ep_traj and tspan.

        ``return_tensors``: False -> a list of SampledMolecule; True -> (host tensors {'x','a','c','e'}, n_atoms); 'device' -> the same on the
        device, unsynchronised with the host copy left out; 'dense' (endpoint models) -> the continuous final state instead of its argmax."""
        if device is not None and torch.device(device) != self.device:
            self.to(device)
        req = self._request(n_atoms, n_timesteps, kwargs, xt_traj, ep_traj)
        eng, cfg, kw = self.engine, self.cfg, req.kw
        eng.bind(req.n_atoms)
        state, seed = self._initial_state(req, prior)
        visualize = bool(xt_traj or ep_traj)
        traj = init = None
        if visualize:        # frames as tokens (the molecule of an endpoint model's frame is its argmax, molecule_builder.py:231-247) + fp32 coordinates
            traj, init = eng.new_traj(req.n_points - 1), _tokens(state, copy=True)
        if req.path == 'endpoint':
            integrate = lambda: eng.integrate_endpoint(state, req.n_timesteps, inv_temp_func=kw.get('inv_temp_func'), tspan=kw.get('tspan'), traj=traj)
        else:
            args, plan_kw = self._plan_args(stochasticity, high_confidence_threshold, kw, req.dfm_type)
            if req.path == 'mixed':
                distinct = sorted(set(req.counts))
                plans = [make_step_plan(T, *args, philox_seed=seed, **plan_kw) for T in distinct]
                integrate = lambda: eng.integrate_mixed(state, plans, [distinct.index(T) for T in req.counts])
            else:
                plan = make_step_plan(req.n_timesteps, *args, philox_seed=seed, **plan_kw)
                rows = kw.get('_rows')     # sample_distributed(noise='replicated'): (N_full, U_full, node rows, pair rows): draw the full batch's noise, keep this shard's
                nN, nU = (eng.N, eng.U) if rows is None else rows[:2]

                def noise_for_step(i, last):
                    nz = StepNoise.draw(nN, nU, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types, last, eng.device, dfm_type=req.dfm_type)
                    return nz if rows is None else nz.take_rows(rows[2], rows[3])
                # _noise_for_step(i, last) -> StepNoise: recorded draws instead of torch's generator (parity tests drive the public API with
                # the oracle's RNG tape); never set by the product itself.  A Philox plan draws inside the kernels: no callback
                noise = None if seed is not None else (kw.get('_noise_for_step') or noise_for_step)
                integrate = lambda: eng.integrate(state, plan, noise, traj=traj)
        t0 = time.perf_counter()
        integrate()          # every integrator synchronises at its end
        t_integrate = time.perf_counter() - t0
        frames_in_tuple = bool(kw.get('_frames')) and return_tensors == 'device'      # sample_distributed: this shard's frames stay in HBM for the second gather
        frames = _frames_of(init, traj) if visualize and (frames_in_tuple or not return_tensors) else None
        return self._finish(state, req.n_atoms, frames, return_tensors, frames_in_tuple, xt_traj, ep_traj, t_integrate)

    # ------------------------------------------------------------------ resampling given molecules
    @torch.no_grad()
    def resample(self, molecules, start_step, n_timesteps=None, seed=None, mol_ids=None, stochasticity=None, high_confidence_threshold=None,
                 return_tensors=False, xt_traj=False, ep_traj=False, keep=None, coupling='independent', **kwargs):
        """Variations of given molecules (no reference entry point; its parts are the reference's): molecule *i* is noised back to time point
        ``k = start_step[i]`` of its ``T = n_timesteps[i]``-point schedule, ``t = linspace(0, 1, T)[k]``, with the model's own corruption process
        (CTMCVectorField.sample_conditional_path, ctmc_vector_field.py:97-143: the distribution the network was trained on), and then takes steps
        ``k .. T-2`` of the unchanged Philox plan of a full ``T``-point run -- the step indices, and so the draws, of ``sample``.  ``start_step = 0``
        is ``sample`` itself (whatever the molecules hold), ``start_step = T - 1`` returns the centred input; in between, the later the start the
        closer the result stays to the input.

        ``molecules``: a list of SampledMolecule (their raw x_1, a_1, c_1, e_1, fake atoms included) or the ``(tensors, n_atoms)`` pair of
        ``sample(return_tensors=True)``; every token must be a real category.  ``start_step`` / ``n_timesteps``: an int, or one per molecule
        (at most 32 distinct pairs per call).  Noise is Philox only: ``seed`` is required, ``mol_ids`` (default 0..B-1) name the streams.  Molecule *i*
        is, bit for bit, ``resample([mol_i], start_step[i], n_timesteps[i], seed, mol_ids=[id_i])``.  ``xt_traj`` / ``ep_traj`` (one (T, k) for all
        molecules only) record T - k frames, frame 0 being the corrupted state.  Raises NotImplementedError for endpoint models, ``tspan``, dfm_type
        'gat' with a per-molecule argument, trajectories with several (T, k) pairs and more than 32 of those; ``return_tensors`` as in ``sample``.

        ``keep`` (frozen atoms, replacement conditioning): a bool tensor over the concatenated atoms, or a list with one bool sequence per molecule,
        marking the atoms -- fake atoms included -- that stay exactly as given while the model regenerates the rest (scaffold decoration, linker design).
        Every step runs on the whole molecule as always; then the kept atoms (position, type, charge) and the bonds between two kept atoms are put back
        onto the given molecule's conditional path at the new time, inside the step kernel, so the network always sees the kept part at the noise level it
        was trained on.  On models with alpha(1) = 1 the kept rows of the result are the CENTRED input rows bit for bit; the result is not re-centred:
        its frame is that of the given molecule.  A bond with one free atom is free.  ``None`` or all-False is the call without ``keep``.  Sharding
        across ranks and the command line do not take ``keep``.

        ``keep`` per modality: a dict with any of the keys 'x', 'a', 'c' (positions, atom types, charges: given like the whole-atom form) and 'e'
        (bonds: a bool tensor over the concatenated unordered pairs, or one sequence of n (n - 1) / 2 entries per molecule in upper-triangle order, the
        order of ``e``).  The four are independent -- every type, charge and bond frozen with the positions free gives conformers of the given graph
        (``conformers``), 'x' alone fixes a pose and lets the chemistry run, a bond may be frozen between two free atoms -- and a missing key leaves
        that modality free.  {'x': k, 'a': k, 'c': k, 'e': both atoms in k} is ``keep=k`` bit for bit; an all-False dict is the call without ``keep``.

        ``coupling``: 'independent' (default) corrupts with the molecule's own Gaussian draw, and ``resample(mols, 0, T)`` is ``sample`` as stated above.
        'ot' pairs the draw with the molecule the way the reference's datasets do for every shipped config (``prior_config.x.align: True``: optimal
        assignment, then a rigid fit that may reflect; ``Engine.ot_align``, priors.py:109-169), which is the path a checkpoint trained that way saw: the
        start state and, under a ``keep`` that freezes positions, the frozen path use the coupled prior.  Per molecule, so the bit-for-bit single-molecule
        statement holds.  ValueError, before the bind, for any other value and, with 'ot', a molecule above 256 atoms; not sharded, no command line."""
        cfg = self.cfg
        # ---- arguments: every refusal before the bind and before anything is enqueued; no generator is touched
        if cfg.parameterization == 'endpoint':
            raise NotImplementedError('resample: endpoint models are not supported (they have no masked conditional path)')
        unknown = set(kwargs) - RESAMPLE_KWARGS
        if unknown:
            raise TypeError(f'resample() got unexpected keyword arguments {sorted(unknown)}')
        if kwargs.get('tspan') is not None:
            raise NotImplementedError('resample: tspan is not supported (start_step indexes the linspace(0, 1, n_timesteps) schedule)')
        if seed is None:
            raise ValueError('resample draws from the per-molecule Philox streams: seed is required')
        dfm_type = kwargs.get('dfm_type') or cfg.dfm_type
        if dfm_type not in ('campbell', 'gat'):
            raise ValueError(f"Invalid dfm_type: {dfm_type}")
        ks, Ts = _step_counts(start_step), _step_counts(n_timesteps)
        if dfm_type == 'gat' and (ks is not None or Ts is not None):
            raise NotImplementedError("resample with per-molecule start_step / n_timesteps: dfm_type 'gat' is not supported")
        x1, n_atoms = self._given_molecules(molecules)
        _check_coupling(coupling, n_atoms, 'resample')
        B = int(n_atoms.numel())
        keep = _keep_rows(keep, n_atoms)
        ks = [int(start_step)] * B if ks is None else ks
        Ts = [int(self.default_n_timesteps if n_timesteps is None else n_timesteps)] * B if Ts is None else Ts
        if len(ks) != B or len(Ts) != B:
            raise ValueError(f'start_step / n_timesteps must be an int or give one entry per molecule ({B})')
        if any(T < 1 or k < 0 or k > T - 1 for k, T in zip(ks, Ts)):
            raise ValueError('start_step must lie in 0 .. n_timesteps - 1 (and n_timesteps >= 1)')
        ids = list(range(B)) if mol_ids is None else [int(v) for v in torch.as_tensor(mol_ids).reshape(-1).tolist()]
        if len(ids) != B:
            raise ValueError(f'mol_ids has {len(ids)} entries for {B} molecules')
        pairs = sorted(set(zip(Ts, ks)))
        visualize = bool(xt_traj or ep_traj)
        if len(pairs) > 1 and visualize:
            raise NotImplementedError('resample with several (n_timesteps, start_step) pairs: xt_traj / ep_traj are not supported (no trajectory sink)')
        if len(pairs) > _lib.FM_TAB_SLOTS:
            raise NotImplementedError(f'more than {_lib.FM_TAB_SLOTS} distinct (n_timesteps, start_step) pairs in one call ({len(pairs)}): split the call')
        eng = self.engine
        args, plan_kw = self._plan_args(stochasticity, high_confidence_threshold, kwargs, dfm_type)
        plans = {T: make_step_plan(T, *args, philox_seed=int(seed), **plan_kw) for T in sorted({T for T, _ in pairs})}
        alphas = {(T, k): alpha_tables(torch.linspace(0, 1, T), cfg.schedule_type, cfg.cosine_params)[0][k] for T, k in pairs}
        sizes = n_atoms.tolist()
        given = _split_molecules(x1, sizes)
        n_pairs = [n * (n - 1) // 2 for n in sizes]
        if isinstance(keep, dict):          # per modality: {modality: one block of rows per molecule}
            kept = {f: torch.split(v, n_pairs if f == 'e' else sizes) for f, v in keep.items()}
        else:
            kept = torch.split(keep, sizes) if keep is not None else None
        # ---- the library refuses a NULL previous endpoint with only some groups at t = 0: molecules that start at step 0 run in an engine call of their own
        parts = [[i for i in range(B) if ks[i] == 0], [i for i in range(B) if ks[i] > 0]]
        parts = [p for p in parts if p]
        results, frames, t_integrate = [None] * B, None, 0.0
        for part in parts:
            whole = len(part) == B
            st1 = x1 if whole else {f: torch.cat([given[i][f] for i in part]) for f in ('x_t', 'a_t', 'c_t', 'e_t')}
            eng.bind(n_atoms[part])
            eng.set_molecule_ids(torch.tensor([ids[i] for i in part]))
            st1 = eng.make_state(st1['x_t'], st1['a_t'], st1['c_t'], st1['e_t'])
            keys = sorted({(Ts[i], ks[i]) for i in part})
            group = [keys.index((Ts[i], ks[i])) for i in part]
            state = eng.conditional_path(st1, torch.stack([alphas[key] for key in keys]), group if len(keys) > 1 else None, seed=int(seed), coupling=coupling)
            spec = None
            if isinstance(kept, dict):
                spec = eng.freeze_spec(st1, {f: torch.cat([blocks[i] for i in part]) for f, blocks in kept.items()}, int(seed), coupling=coupling)
            elif kept is not None:
                spec = eng.inpaint_spec(st1, torch.cat([kept[i] for i in part]), int(seed), coupling=coupling)
            t0 = time.perf_counter()
            if len(keys) == 1:
                (T, k), traj, init = keys[0], None, None
                if visualize:
                    traj, init = eng.new_traj(T - 1), _tokens(state, copy=True)
                IntegrationRun(eng, state, plans[T], None, traj=traj, inpaint=spec).run(k, T - 1)
                eng.synchronize()
                if visualize:
                    frames = _frames_of(init, {f: v[k:] for f, v in traj.items()})
            elif spec is not None:
                eng.integrate_inpaint(state, [plans[T] for T, _ in keys], group, spec, start=[k for _, k in keys])
            else:
                eng.integrate_mixed(state, [plans[T] for T, _ in keys], group, start=[k for _, k in keys])
                eng.synchronize()
            t_integrate += time.perf_counter() - t0
            if whole:
                final = state
            else:
                for i, s_ in zip(part, _split_molecules(state, [sizes[i] for i in part])):
                    results[i] = s_
        if len(parts) > 1:
            final = {f: torch.cat([results[i][f] for i in range(B)]).contiguous() for f in ('x_t', 'a_t', 'c_t', 'e_t')}
        return self._finish(final, n_atoms, frames if not return_tensors else None, return_tensors, False, xt_traj, ep_traj, t_integrate)

    def inpaint(self, molecules, keep, n_timesteps=None, seed=None, mol_ids=None, **kwargs):
        """Generate the free atoms of ``molecules`` from the prior around the kept ones: ``resample(molecules, 0, n_timesteps, keep=keep, ...)``;
        ``coupling='ot'`` (a keyword of ``resample``) lets the kept positions follow the coupled path."""
        return self.resample(molecules, 0, n_timesteps, seed=seed, mol_ids=mol_ids, keep=keep, **kwargs)

    def conformers(self, molecules, n_conformers=1, n_timesteps=None, seed=None, mol_ids=None, start_step=0, **kwargs):
        """3D conformers of given molecular graphs: every molecule is repeated ``n_conformers`` times, molecule-major, every atom's type and charge and
        every pair's bond order are frozen and the positions are left free -- ``resample(repeated molecules, start_step, n_timesteps, seed=seed,
        mol_ids=mol_ids, keep={'a': all, 'c': all, 'e': all})``, whose other arguments and refusals it takes.  ``mol_ids`` (B * n_conformers entries,
        default 0 .. B * n_conformers - 1) name the Philox streams: two conformers of a molecule differ because their streams do.  Returns the flat list of
        B * n_conformers molecules (``return_tensors`` as in ``resample``); on models with alpha(1) = 1 the tokens of every result are the input's.
        ``coupling`` (a keyword of ``resample``, default 'independent'): with ``start_step > 0`` and 'ot' the conformers start from the coupled path."""
        if self.cfg.parameterization == 'endpoint':          # resample's refusal, before the molecules are read as tokens of a CTMC model
            raise NotImplementedError('conformers: endpoint models are not supported (they have no masked conditional path)')
        K = int(n_conformers)
        if K < 1:
            raise ValueError('n_conformers must be >= 1')
        x1, n_atoms = self._given_molecules(molecules)
        sizes = n_atoms.tolist()
        given = _split_molecules(x1, sizes)
        rep = [i for i in range(len(sizes)) for _ in range(K)]
        tensors = {k: torch.cat([given[i][f'{k}_t'] for i in rep]) for k in 'xace'}
        n_rep = n_atoms[rep]
        N, U = int(n_rep.sum()), int((n_rep * (n_rep - 1) // 2).sum())
        keep = {'a': torch.ones(N, dtype=torch.bool), 'c': torch.ones(N, dtype=torch.bool), 'e': torch.ones(U, dtype=torch.bool)}
        return self.resample((tensors, n_rep), start_step, n_timesteps, seed=seed, mol_ids=mol_ids, keep=keep, **kwargs)

    @torch.no_grad()
    def rmsd(self, molecules_a, molecules_b, select=None, heavy=False) -> torch.Tensor:
        """Aligned RMSD of ``molecules_a`` onto ``molecules_b``, molecule by molecule, in one launch on the device (``Engine.align_rmsd``): a (B,) float32
        tensor on the CPU, the rmsd after centring and the optimal proper rotation (no reflection) over the selected atoms.  ``molecules_*`` as in
        ``resample``; the sizes must match molecule by molecule (ValueError).  ``select``: a bool tensor over the concatenated atoms or one bool sequence
        per molecule (None = all atoms); ``heavy``: only atoms whose type in ``molecules_b`` is neither 'H' nor the fake-atom token.  A molecule
        without a selected atom gives 0.  With ``conformers``: ``model.rmsd(confs, [m for m in mols for _ in range(K)], heavy=True)``."""
        xa, na = self._given_molecules(molecules_a)
        xb, nb = self._given_molecules(molecules_b)
        if na.tolist() != nb.tolist():
            raise ValueError(f'rmsd: the molecules must match in size one by one, got {na.tolist()} and {nb.tolist()}')
        sel = self._selection(xb['a_t'], nb.tolist(), select, heavy)
        eng = self.engine
        eng.bind(nb)
        out = eng.align_rmsd(xa['x_t'], xb['x_t'], sel)
        eng.synchronize()
        return out[:, 2].cpu()

    def _selection(self, a_tok: torch.Tensor, sizes, select, heavy: bool) -> Optional[torch.Tensor]:
        """``select`` / ``heavy`` of ``rmsd`` and ``rmsd_matrix`` as one bool tensor over the concatenated atoms, or None for all atoms: ``select`` a bool
        tensor over the atoms or one bool sequence per molecule; ``heavy`` drops the atoms whose type in ``a_tok`` is 'H' or the fake-atom token."""
        if select is None and not heavy:
            return None
        sel = torch.ones(int(sum(sizes)), dtype=torch.bool) if select is None else _keep_flat(select, list(sizes), 'select', 'atoms')
        if heavy:
            amap = list(self.cfg.atom_type_map)
            light = [i for i, sym in enumerate(amap) if sym == 'H'] + [len(amap)]          # the fake atom's token follows the real types
            sel = sel & ~torch.isin(a_tok, torch.tensor(light))
        return sel

    # ------------------------------------------------------------------ conformer ensembles
    def _conformer_groups(self, n_mols: int, n_conformers, groups) -> List[int]:
        if groups is not None:
            sizes = [int(g) for g in groups]
            if any(g < 0 for g in sizes) or sum(sizes) != n_mols:
                raise ValueError(f'groups must hold non-negative sizes that add up to the {n_mols} molecules given, got {sizes}')
            return sizes
        if n_conformers is None:
            raise ValueError('give n_conformers (the K of conformers()) or groups=[sizes]')
        K = int(n_conformers)
        if K < 1 or n_mols % K:
            raise ValueError(f'{n_mols} molecules are not a whole number of groups of n_conformers = {K}')
        return [K] * (n_mols // K)

    def _rmsd_triangles(self, x, tok, n_atoms, group_sizes, select, heavy, symmetry, max_perms):
        """The strict upper triangles (row-major, i < j) of every group's RMSD matrix, concatenated, as one float32 tensor on the engine's device: one
        bind, one ``Engine.pair_rmsd`` launch.  ``x`` (N,3) on any device; ``tok`` {'a_t', 'c_t', 'e_t'} on the CPU; ``n_atoms`` (M,) the molecules' sizes."""
        sizes = [int(v) for v in n_atoms.tolist()]
        n_pairs = [n * (n - 1) // 2 for n in sizes]
        sel = self._selection(tok['a_t'], sizes, select, heavy)
        a_m, c_m, e_m = torch.split(tok['a_t'], sizes), torch.split(tok['c_t'], sizes), torch.split(tok['e_t'], n_pairs)
        s_m = torch.split(sel, sizes) if sel is not None else None
        pairs, perm_set, rows, m0 = [], [-1] * len(sizes), [], 0
        for g, K in enumerate(group_sizes):
            for k in range(1, K):
                if sizes[m0 + k] != sizes[m0]:
                    raise ValueError(f'group {g}: the conformers differ in size ({sizes[m0]} and {sizes[m0 + k]} atoms)')
                if s_m is not None and not torch.equal(s_m[m0 + k], s_m[m0]):
                    raise ValueError(f'group {g}: select / heavy flag different atoms in its conformers')
                if symmetry and not (torch.equal(a_m[m0 + k], a_m[m0]) and torch.equal(c_m[m0 + k], c_m[m0]) and torch.equal(e_m[m0 + k], e_m[m0])):
                    raise ValueError(f'group {g}: symmetry=True needs conformers of ONE graph, conformer {k} differs from conformer 0 in a token')
            if symmetry and K > 1:
                rows.append(automorphisms(a_m[m0], c_m[m0], e_m[m0], None if s_m is None else s_m[m0], max_perms=max_perms, mask_token=self.cfg.n_bond_types))
                perm_set[m0:m0 + K] = [len(rows) - 1] * K
            pairs += [(m0 + i, m0 + j) for i in range(K) for j in range(i + 1, K)]
            m0 += K
        eng = self.engine
        eng.bind(n_atoms)
        if not pairs:
            return torch.zeros(0, device=eng.device)
        out = eng.pair_rmsd(x, torch.tensor(pairs, dtype=torch.int32), sel, (torch.tensor(perm_set, dtype=torch.int32), rows) if rows else None)
        return out[:, 1].contiguous()

    @torch.no_grad()
    def rmsd_matrix(self, molecules, n_conformers=None, select=None, heavy=False, symmetry=False, max_perms=256, groups=None) -> List[torch.Tensor]:
        """The aligned-RMSD matrix of every group of conformers, in one bind and one launch on the device (``Engine.pair_rmsd``): a list of symmetric
        (K, K) float32 CPU tensors with a zero diagonal -- the upper triangle is computed and mirrored.  ``molecules``: the flat, molecule-major list that
        ``conformers`` returns (or its ``(tensors, n_atoms)`` pair), cut into groups of ``n_conformers``, or into ``groups=[sizes]``.  ``select`` and
        ``heavy`` as in ``rmsd``.  ``symmetry``: the rmsd of a pair is the smallest over the automorphisms of the group's first conformer
        (``symmetry.automorphisms`` of its selected atoms, computed once per group and shared by its members; more than ``max_perms`` is its ValueError),
        so a flipped phenyl or a rotated methyl is the same conformer; the identity is among them, hence never larger than without.  ValueError when the
        conformers of a group differ in size, in their selected atoms or, with ``symmetry``, in any token."""
        x1, n_atoms = self._given_molecules(molecules)
        gs = self._conformer_groups(int(n_atoms.numel()), n_conformers, groups)
        tri = self._rmsd_triangles(x1['x_t'], x1, n_atoms, gs, select, heavy, symmetry, max_perms)
        self.engine.synchronize()
        mats = []
        for K, t in zip(gs, torch.split(tri.cpu(), [K * (K - 1) // 2 for K in gs])):
            m = torch.zeros(K, K)
            i, j = torch.triu_indices(K, K, 1)
            m[i, j] = t
            mats.append(m + m.T)
        return mats

    @torch.no_grad()
    def prune_conformers(self, molecules, n_conformers=None, threshold=0.5, heavy=True, symmetry=True, select=None, max_perms=256, groups=None):
        """Greedy RMSD-threshold pruning of conformer groups, on the device (``rmsd_matrix``'s launch, then ``Engine.prune_rmsd``): in every group, for
        i = 0, 1, ... conformer i is dropped when the nearest KEPT earlier conformer (ties: the first) is closer than ``threshold`` -- the rule of RDKit's
        pruneRmsThresh.  Returns ``(kept, keep, rep)``: ``kept`` one list per group with its kept molecules (the objects given; for the
        ``(tensors, n_atoms)`` form their indices in the flat list), ``keep`` (M,) bool and ``rep`` (M,) int64 over the flat list -- rep[i] = i for a
        kept conformer, else the index of the kept one it was dropped for, so cluster populations are ``torch.bincount(rep)``.  Arguments and refusals of
        ``rmsd_matrix``; the molecules are never altered."""
        x1, n_atoms = self._given_molecules(molecules)
        gs = self._conformer_groups(int(n_atoms.numel()), n_conformers, groups)
        tri = self._rmsd_triangles(x1['x_t'], x1, n_atoms, gs, select, heavy, symmetry, max_perms)
        keep, rep = self.engine.prune_rmsd(tri, gs, threshold)
        self.engine.synchronize()
        keep, rep = keep.cpu(), rep.cpu()
        items = list(range(int(n_atoms.numel()))) if isinstance(molecules[0], dict) else list(molecules)
        return _grouped([m for m, k in zip(items, keep.tolist()) if k], [int(k.sum()) for k in torch.split(keep, gs)]), keep, rep

    @torch.no_grad()
    def conformer_ensembles(self, molecules, n_conformers=1, n_timesteps=None, seed=None, prune_rmsd=None, heavy=True, symmetry=True, max_perms=256,
                            stereo=None, flat_tol=0.05, **conformers_kwargs):
        """Conformer ensembles of given molecular graphs: ``conformers(molecules, n_conformers, n_timesteps, seed, ...)``, then, with ``prune_rmsd`` a
        threshold, the symmetry-aware RMSD matrices and the greedy pruning of ``prune_conformers`` on the device, the coordinates going from the sampler
        to the RMSD launch as one device tensor.  Returns one list of molecules per input molecule; ``prune_rmsd=None`` returns all ``n_conformers``.
        Pruning selects and never alters: the kept molecules are bit for bit those ``conformers`` returns.  ``return_tensors`` together with
        ``prune_rmsd`` is a ValueError.

        ``stereo`` (None | 'match' | 'mirror'; ``flat_tol`` as in ``match_stereo``): the frozen tokens carry no stereo information, so a conformer may
        come back with a stereocentre inverted or a double bond flipped -- a different compound.  'match' drops, before any pruning, every conformer
        whose stereo state (``match_stereo`` against the input's own coordinates, one launch on the device between the sampler and the RMSD launch) is
        not the input's; 'mirror' first point-inverts the exact mirror images (their coordinates become exactly the negative of what ``conformers``
        gives) and then drops what still mismatches.  The lists then have between 0 and ``n_conformers`` members; nothing is sampled again to fill them
        up.  None is the call without the argument.  ``stereo`` together with ``return_tensors`` or trajectories, any other value, and a conformer
        whose tokens are not the input's (a model with alpha(1) < 1) are a ValueError.
        ``coupling`` goes to ``conformers`` with the other keywords; the coordinates stay on the device with either value.
        Not covered: sharding across ranks, the command line."""
        K = int(n_conformers)
        if stereo not in (None, 'match', 'mirror'):
            raise ValueError(f"conformer_ensembles: stereo must be None, 'match' or 'mirror', got {stereo!r}")
        if stereo is not None and conformers_kwargs.get('return_tensors'):
            raise ValueError('conformer_ensembles: return_tensors together with stereo is not supported (the stereo filter returns lists of molecules)')
        if prune_rmsd is None and stereo is None:
            out = self.conformers(molecules, K, n_timesteps, seed=seed, **conformers_kwargs)
            if conformers_kwargs.get('return_tensors'):
                return out
            return _grouped(out, [K] * (len(out) // K))
        if conformers_kwargs.get('return_tensors'):
            raise ValueError('conformer_ensembles: return_tensors together with prune_rmsd is not supported (pruning returns lists of molecules)')
        if conformers_kwargs.get('xt_traj') or conformers_kwargs.get('ep_traj'):
            raise ValueError('conformer_ensembles: trajectories together with prune_rmsd or stereo are not supported')
        dev_out, n_atoms = self.conformers(molecules, K, n_timesteps, seed=seed, return_tensors='device', **conformers_kwargs)
        gs = [K] * (int(n_atoms.numel()) // K)
        tok = {f'{k}_t': dev_out[k].to('cpu', torch.int64) for k in 'ace'}
        if stereo is not None:
            ref, n_ref = self._given_molecules(molecules)
            rep = [i for i in range(int(n_ref.numel())) for _ in range(K)]
            given = _split_molecules(ref, n_ref.tolist())
            ref = {k: torch.cat([given[i][k] for i in rep]) for k in ('x_t', 'a_t', 'c_t', 'e_t')}
            ok, _, x_fixed = self._stereo_launch(dev_out['x'], tok, n_atoms, ref, n_ref[rep], stereo == 'mirror', flat_tol)
            atom_keep = torch.repeat_interleave(ok, n_atoms)
            pair_keep = torch.repeat_interleave(ok, n_atoms * (n_atoms - 1) // 2)
            gs = [int(k.sum()) for k in torch.split(ok, gs)]
            n_atoms = n_atoms[ok]
            if not sum(gs):
                return [[] for _ in gs]
            dev = dev_out['x'].device
            ak, pk = atom_keep.to(dev), pair_keep.to(dev)
            dev_out = {'x': (x_fixed if x_fixed is not None else dev_out['x'])[ak].contiguous(), 'a': dev_out['a'][ak].contiguous(),
                       'c': dev_out['c'][ak].contiguous(), 'e': dev_out['e'][pk].contiguous()}
            tok = {'a_t': tok['a_t'][atom_keep], 'c_t': tok['c_t'][atom_keep], 'e_t': tok['e_t'][pair_keep]}
        if prune_rmsd is None:
            return _grouped(self._package(_to_host(dev_out), n_atoms, None, False, False), gs)
        tri = self._rmsd_triangles(dev_out['x'], tok, n_atoms, gs, None, heavy, symmetry, max_perms)
        keep, _ = self.engine.prune_rmsd(tri, gs, prune_rmsd)
        keep = keep.cpu()
        mols = self._package(_to_host(dev_out), n_atoms, None, False, False)
        return _grouped([m for m, k in zip(mols, keep.tolist()) if k], [int(k.sum()) for k in torch.split(keep, gs)])

    # ------------------------------------------------------------------ stereo check
    def _stereo_launch(self, x, tok, n_atoms, ref, n_ref, mirror: bool, flat_tol):
        """One bind and one ``Engine.stereo`` launch of the coordinates ``x`` ((N,3), any device) with the CPU tokens ``tok`` against the CPU reference state
        ``ref`` {'x_t', 'a_t', 'c_t', 'e_t'}: -> (match (B,) bool with the mirror images counted in when ``mirror``, table (B,8) int32, both on the CPU, and
        with ``mirror`` the (N,3) coordinates on the engine's device with the mirror images inverted, else None).  The stereo elements come from the
        reference's tokens, once per run of consecutive identical graphs.  ValueError when a molecule and its reference differ in size or in a token."""
        if n_atoms.tolist() != n_ref.tolist():
            raise ValueError(f'stereo: a molecule and its reference must match in size one by one, got {n_atoms.tolist()} and {n_ref.tolist()}')
        for f, what in (('a_t', 'an atom type'), ('c_t', 'a charge'), ('e_t', 'a bond order')):
            if not torch.equal(tok[f], ref[f]):
                raise ValueError(f'stereo: a molecule differs from its reference in {what} token: the stereo state is compared between arrangements of ONE graph')
        sizes = n_atoms.tolist()
        a_m, c_m = torch.split(ref['a_t'], sizes), torch.split(ref['c_t'], sizes)
        e_m = torch.split(ref['e_t'], [n * (n - 1) // 2 for n in sizes])
        elem_set, rows = [], []
        for m in range(len(sizes)):
            if not (m and sizes[m] == sizes[m - 1] and torch.equal(a_m[m], a_m[m - 1]) and torch.equal(c_m[m], c_m[m - 1]) and torch.equal(e_m[m], e_m[m - 1])):
                rows.append(stereo_elements(a_m[m], c_m[m], e_m[m], mask_token=self.cfg.n_bond_types,
                                            fake_token=len(self.cfg.atom_type_map) if self.fake_atoms else None))
            elem_set.append(len(rows) - 1)
        eng = self.engine
        eng.bind(n_atoms)
        res = eng.stereo(x, ref['x_t'], (torch.tensor(elem_set, dtype=torch.int32), rows), flat_tol, fixed=mirror)
        table, x_fixed = res if mirror else (res, None)
        eng.synchronize()
        table = table.cpu()
        ok = table[:, 6] != 0
        if mirror:
            ok = ok | (table[:, 7] != 0)
        return ok, table, x_fixed

    @torch.no_grad()
    def match_stereo(self, molecules, references, mirror=False, flat_tol=0.05):
        """Do ``molecules`` have the stereo state of ``references``?  Molecule i is compared with reference i, an arrangement in space of the same graph
        (``molecules_*`` as in ``resample``; ValueError when the two differ in size or in any token).  The stereo elements -- tetrahedral centres and
        double bonds as ``stereo.stereo_elements`` defines them, which also says what that leaves out -- are perceived on the reference's tokens, once per
        run of consecutive identical graphs, and compared in one bind and one launch on the device (``Engine.stereo``, whose ``flat_tol`` this is: an
        element flatter than that in either arrangement is undefined, and a molecule with an undefined element does not match).
        Returns ``(molecules_out, match, table)``: ``match`` (B,) bool, ``table`` (B,8) int32 on the CPU = {centres, defined in both, mismatches, double
        bonds, defined in both, mismatches, match, mirror} per molecule, ``molecules_out`` the full list, unfiltered, in the form given.  With
        ``mirror`` the molecules flagged as exact mirror images (every centre inverted, every double bond as in the reference) come back point-inverted:
        their coordinates are exactly the negative of the input's, their tokens unchanged (new objects without trajectory frames; the others are the
        objects given), and they count as matching.  ``mirror=False`` alters nothing."""
        x1, n_atoms = self._given_molecules(molecules)
        ref, n_ref = self._given_molecules(references)
        ok, table, x_fixed = self._stereo_launch(x1['x_t'], x1, n_atoms, ref, n_ref, bool(mirror), flat_tol)
        tensor_form = isinstance(molecules[0], dict)
        if not mirror:
            return (molecules if tensor_form else list(molecules)), ok, table
        x_fixed = x_fixed.cpu()
        if tensor_form:
            return ({'x': x_fixed, **{k: x1[f'{k}_t'] for k in 'ace'}}, n_atoms), ok, table
        out = list(molecules)
        flipped = (table[:, 7] != 0).tolist()
        xs = torch.split(x_fixed, n_atoms.tolist())
        for i, m in enumerate(out):
            if flipped[i]:
                out[i] = self._package({'x': xs[i].clone(), 'a': m.a_1, 'c': m.c_1, 'e': m.e_1}, n_atoms[i:i + 1], None, False, False)[0]
        return out, ok, table

    def denoising_loss(self, molecules, t, seed=None, mol_ids=None, distort=None, time_scaled=None, total_loss_weights=None, coupling=None):
        """The denoising losses of given molecules: the reference's ``FlowMol.forward(g)`` (flowmol.py:297-415, what its ``validation_step`` logs) --
        corrupt every molecule to its time ``t``, evaluate the network once, and compare its logits and positions with the molecule.  The standard check
        of a ported checkpoint: compare ``losses`` on a few hundred dataset molecules with what training logged.

        ``molecules``: as in ``resample``.  ``t`` is required: a float, or one value in [0, 1) per molecule -- ``torch.rand(B)`` is the reference's
        protocol (:328).  Noise is Philox only: ``seed`` is required, ``mol_ids`` (default 0..B-1) name the streams.  ``distort``: ``(distort_p, distort_t)``
        of the geometry distortion (:333-337), ``False`` for none; ``time_scaled``: the reference's ``time_scaled_loss``.  Both default to the checkpoint's
        hparams (``self.loss_hparams``; presets: off).  Per call: centre, ``Engine.conditional_path``, optional ``Engine.distort``,
        ``Engine.denoising_loss``; more than 32 distinct ``t`` are served by sorting on ``t`` and binding several batches, which canonical arithmetic makes
        invisible: molecule *i* of any call is, bit for bit, ``denoising_loss([mol_i], t[i], seed=s, mol_ids=[id_i])``.

        ``coupling`` ('independent' | 'ot' | None): how x_0 is paired with x_1.  The reference's loaders hand ``forward`` an x_0 that was OT-aligned to the
        molecule whenever ``prior_config.x.align`` is set (priors.py:267-303; every shipped config), so the logged position loss is that of 'ot'.  None
        follows the checkpoint (``loss_hparams['prior_align_x']``); presets and an empty ``loss_hparams`` give 'independent'.  Per molecule, so the
        bit-for-bit statement above holds for both.  ValueError for another value and, with 'ot', a molecule above 256 atoms.

        Returns ``per_molecule`` (B,8) = {se_x, 3 n_atoms, nll_a, cnt_a, nll_c, cnt_c, nll_e, cnt_e} and ``rows`` {'x', 'a', 'c' (N), 'e' (U)} (CPU), and
        ``losses`` {'x', 'a', 'c', 'e'}: the reference's four batch values, formed from the table on the host as its code forms them (:388-413).
        Unscaled: x = mean over the 3N elements; a categorical value = sum nll / sum cnt (NaN when nothing is masked, as in torch).  Time-scaled: weights
        ``clamp(alpha / (1 - alpha), 0.05, 1.5)`` per molecule and feature (interpolant_scheduler.py:87-95); x = mean of weight * squared error; a
        categorical value is what the reference's code EVALUATES, not what it presumably meant: ``loss (rows,) * weight (rows, 1)`` broadcasts to a
        (rows, rows) outer product, so the value is mean(loss over all rows, ignored rows as 0) * mean(weight over rows).  ``total`` (:259-267) is returned
        when ``total_loss_weights`` is given (argument or hparams; missing features weigh 1).  One deliberate difference: the evaluation never takes the
        reference's eval-mode bootstrap pass for a batch that is entirely at t = 0, which depends on the batch.  NotImplementedError for ``weight_ae``,
        ``target_blur != 0`` and endpoint models; ValueError, before anything is enqueued, for ``t`` outside [0, 1), a mask token and a missing seed."""
        cfg, hp = self.cfg, getattr(self, 'loss_hparams', None) or {}
        if cfg.parameterization == 'endpoint':
            raise NotImplementedError('denoising_loss: endpoint models are not supported (the loss of the masked CTMC parameterisation only)')
        if hp.get('weight_ae', False):
            raise NotImplementedError('denoising_loss: weight_ae=True (class-weighted cross-entropy) is not implemented')
        if float(hp.get('target_blur', 0.0)) != 0.0:
            raise NotImplementedError(f"denoising_loss: target_blur={hp['target_blur']} != 0 (soft targets) is not implemented")
        if seed is None:
            raise ValueError('denoising_loss draws from the per-molecule Philox streams: seed is required')
        x1, n_atoms = self._given_molecules(molecules)
        if coupling is None:
            coupling = 'ot' if hp.get('prior_align_x', False) else 'independent'
        _check_coupling(coupling, n_atoms, 'denoising_loss')
        B = int(n_atoms.numel())
        tv = torch.as_tensor(t).detach().to('cpu', torch.float32).reshape(-1)
        tv = tv.expand(B).clone() if tv.numel() == 1 else tv
        if tv.numel() != B:
            raise ValueError(f't must be a float or give one value per molecule ({B})')
        if not bool(((tv >= 0) & (tv < 1)).all()):
            raise ValueError('denoising_loss: t must lie in [0, 1)')
        ids = list(range(B)) if mol_ids is None else [int(v) for v in torch.as_tensor(mol_ids).reshape(-1).tolist()]
        if len(ids) != B:
            raise ValueError(f'mol_ids has {len(ids)} entries for {B} molecules')
        if distort is None:
            distort = (float(hp.get('distort_p', 0.0)), float(hp.get('distort_t', 0.5)))
        distort = None if not distort or float(distort[0]) <= 0.0 else (float(distort[0]), float(distort[1]))
        time_scaled = bool(hp.get('time_scaled_loss', False)) if time_scaled is None else bool(time_scaled)
        total_loss_weights = hp.get('total_loss_weights') if total_loss_weights is None else total_loss_weights
        # ---- batches of at most FM_TAB_SLOTS distinct times, molecules sorted on t
        vals = torch.unique(tv).tolist()
        eng, sizes = self.engine, n_atoms.tolist()
        given = _split_molecules(x1, sizes)
        table, rows = [None] * B, [None] * B
        for lo in range(0, len(vals), _lib.FM_TAB_SLOTS):
            chunk = set(vals[lo:lo + _lib.FM_TAB_SLOTS])
            part = [i for i in sorted(range(B), key=lambda i: float(tv[i])) if float(tv[i]) in chunk]
            st1 = {f: torch.cat([given[i][f] for i in part]) for f in ('x_t', 'a_t', 'c_t', 'e_t')}
            eng.bind(n_atoms[part])
            eng.set_molecule_ids(torch.tensor([ids[i] for i in part]))
            raw = eng.make_state(st1['x_t'], st1['a_t'], st1['c_t'], st1['e_t'])
            target = dict(raw, x_t=eng.remove_com(raw['x_t'].clone()))      # x_1 - mean with the arithmetic the conditional path centres with
            tp = tv[part]
            tvals, group = torch.unique(tp, return_inverse=True)
            alphas = alpha_tables(tvals.clone(), cfg.schedule_type, cfg.cosine_params)[0]
            state = eng.conditional_path(raw, alphas, group if tvals.numel() > 1 else None, seed=int(seed), coupling=coupling)
            if distort is not None:
                eng.distort(state['x_t'], distort[0], tp > distort[1], seed=int(seed))
            res = eng.denoising_loss(state, target, tp)
            eng.synchronize()
            mol = res['mol'].cpu()
            per = _split_molecules({f'{k}_t': res['rows'][k].cpu() for k in 'ace'}, [sizes[i] for i in part])
            xs = torch.split(res['rows']['x'].cpu(), [sizes[i] for i in part])
            for j, i in enumerate(part):
                table[i] = mol[j]
                rows[i] = {'x': xs[j], 'a': per[j]['a_t'], 'c': per[j]['c_t'], 'e': per[j]['e_t']}
        table = torch.stack(table)
        out = {'per_molecule': table, 'rows': {k: torch.cat([r[k] for r in rows]) for k in 'xace'},
               'losses': self.batch_losses(table, tv, n_atoms, time_scaled)}
        if total_loss_weights is not None:
            out['total'] = sum(float(total_loss_weights.get(f, 1.0)) * out['losses'][f] for f in 'xace')
        return out

    def batch_losses(self, table: torch.Tensor, t: torch.Tensor, n_atoms: torch.Tensor, time_scaled: bool) -> Dict[str, torch.Tensor]:
        """The reference's four batch values (flowmol.py:388-413) from the per-molecule table of ``denoising_loss``, in float32 on the host; see there."""
        table, losses = table.to('cpu', torch.float32), {}
        n = n_atoms.to(torch.float32)
        n_rows = {'x': n, 'a': n, 'c': n, 'e': n * (n - 1) / 2}
        if time_scaled:
            alpha = alpha_tables(t.detach().to('cpu', torch.float32).clone(), self.cfg.schedule_type, self.cfg.cosine_params)[0]
            w = torch.clamp(alpha / (1 - alpha), min=0.05, max=1.5)      # (B,4), interpolant_scheduler.py:87-95
        for f, name in enumerate('xace'):
            term, cnt = table[:, 2 * f], table[:, 2 * f + 1]
            if not time_scaled:
                losses[name] = term.sum() / cnt.sum()
            elif name == 'x':
                losses[name] = (w[:, f] * term).sum() / cnt.sum()
            else:      # (rows,) * (rows, 1): the mean of an outer product
                R = n_rows[name].sum()
                losses[name] = (term.sum() / R) * ((w[:, f] * n_rows[name]).sum() / R)
        return losses

    def _given_molecules(self, molecules):
        """The molecules of a ``resample`` call as one token state on the CPU ({'x_t' (N,3) float32, 'a_t', 'c_t' (N), 'e_t' (U) int64}) and their
        sizes; ValueError for a token that is not a real category (a mask token, an index out of range) or for shapes that do not fit the sizes."""
        cfg = self.cfg
        if isinstance(molecules, (tuple, list)) and len(molecules) == 2 and isinstance(molecules[0], dict):
            t, n_atoms = molecules
            n_atoms = torch.as_tensor(n_atoms).detach().to('cpu', torch.int64).reshape(-1)
            x1 = {f'{k}_t': torch.as_tensor(t[k]).detach().cpu() for k in 'xace'}
        else:
            mols = list(molecules)
            if not mols or not all(isinstance(m, SampledMolecule) for m in mols):
                raise ValueError('molecules must be a non-empty list of SampledMolecule or the (tensors, n_atoms) pair of sample(return_tensors=True)')
            n_atoms = torch.tensor([int(m.x_1.shape[0]) for m in mols], dtype=torch.int64)
            x1 = {'x_t': torch.cat([m.x_1.detach().cpu() for m in mols]), 'a_t': torch.cat([m.a_1.detach().cpu() for m in mols]),
                  'c_t': torch.cat([m.c_1.detach().cpu() for m in mols]), 'e_t': torch.cat([m.e_1.detach().cpu() for m in mols])}
        if n_atoms.numel() == 0 or int(n_atoms.min()) < 1:
            raise ValueError('resample needs at least one molecule, each with at least one atom')
        N, U = int(n_atoms.sum()), int((n_atoms * (n_atoms - 1) // 2).sum())
        x1['x_t'] = x1['x_t'].to(torch.float32)
        if tuple(x1['x_t'].shape) != (N, 3) or tuple(x1['a_t'].shape) != (N,) or tuple(x1['c_t'].shape) != (N,) or tuple(x1['e_t'].shape) != (U,):
            raise ValueError(f'molecule tensors do not fit the sizes: need x ({N}, 3), a ({N},), c ({N},), e ({U},) per unordered pair')
        for f, K, what in (('a_t', cfg.n_atom_types, 'atom type'), ('c_t', cfg.n_charges, 'charge'), ('e_t', cfg.n_bond_types, 'bond order')):
            tok = x1[f] = x1[f].to(torch.int64)
            if tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= K):
                raise ValueError(f'resample: {what} tokens must be real categories 0 .. {K - 1} (no mask token, nothing out of range); '
                                 f'got {int(tok.min())} .. {int(tok.max())}')
        return x1, n_atoms

    # ---- stage 1: arguments
    def _request(self, n_atoms, n_timesteps, kwargs, xt_traj=False, ep_traj=False, noise=None) -> "_Request":
        """What every entry point does first: name the path, refuse what it does not take -- before the bind and before any draw from a generator --
        and normalise the rest (``n_atoms`` a CPU int64 tensor, the default step count, ``seed`` / ``mol_ids`` and their earlier spellings ``_philox``
        / ``_mol_ids``).  ``noise``: the noise mode of a ``sample_distributed`` call, whose ``kwargs`` still hold sample()'s named arguments."""
        counts = _step_counts(n_timesteps)
        if noise is not None:
            if counts is not None:
                raise NotImplementedError('sample_distributed with a sequence of n_timesteps: a mixed-time batch is not sharded across ranks')
            if noise not in ('per_rank', 'replicated', 'philox'):
                raise ValueError(f"noise must be 'per_rank', 'replicated' or 'philox', got {noise!r}")
            kwargs = {k: v for k, v in kwargs.items() if k not in SAMPLE_NAMED_ARGS}         # as the shard's sample() call will see them
            kwargs.update({'philox': {'rng': 'philox'}, 'replicated': {'_rows': ()}}.get(noise, {}))
        path = 'mixed' if counts is not None else ('endpoint' if self.cfg.parameterization == 'endpoint' else 'ctmc')
        if path == 'mixed':
            self._check_mixed(kwargs, xt_traj, ep_traj)
        rng = kwargs.get('rng', 'torch')
        if rng not in ('torch', 'philox'):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        # integrator variants of CTMCVectorField.integrate/step (ctmc_vector_field.py:145-156,287-315): all optional
        dfm_type = kwargs.get('dfm_type') or self.cfg.dfm_type
        if path != 'endpoint' and dfm_type not in ('campbell', 'gat'):
            raise ValueError(f"Invalid dfm_type: {dfm_type}")
        unknown = set(kwargs) - ALLOWED_KWARGS[path]
        if unknown:
            raise TypeError(f'sample() got unexpected keyword arguments {sorted(unknown)}')
        if rng == 'philox' and (kwargs.get('_rows') is not None or kwargs.get('_noise_for_step') is not None):
            raise NotImplementedError("rng='philox' draws inside the kernels: it does not combine with replicated row slicing (_rows) or a noise callback (_noise_for_step)")
        n_atoms = torch.as_tensor(n_atoms).detach().to('cpu', torch.int64)
        if counts is None:
            n_timesteps = self.default_n_timesteps if n_timesteps is None else n_timesteps
        else:
            if len(counts) != n_atoms.numel():
                raise ValueError(f'n_timesteps has {len(counts)} entries for {n_atoms.numel()} molecules')
            if min(counts) < 1:
                raise ValueError('n_timesteps must be >= 1')
            if len(set(counts)) > _lib.FM_TAB_SLOTS:
                raise NotImplementedError(f'more than {_lib.FM_TAB_SLOTS} distinct step counts in one batch ({len(set(counts))}): split the call')
        seed = kwargs.get('seed') if kwargs.get('seed') is not None else kwargs.get('_philox')
        ids = kwargs.get('mol_ids') if kwargs.get('mol_ids') is not None else kwargs.get('_mol_ids')
        return _Request(path, n_atoms, n_timesteps, counts, rng, dfm_type, None if seed is None else int(seed), ids, kwargs)

    def _check_mixed(self, kwargs, xt_traj=False, ep_traj=False):
        """The combinations per-molecule step counts do not cover, each refused by name."""
        if self.cfg.parameterization == 'endpoint':
            raise NotImplementedError('per-molecule n_timesteps: endpoint models are not supported (time enters their embedding MLP per node)')
        if kwargs.get('rng', 'torch') != 'philox':
            raise NotImplementedError("per-molecule n_timesteps needs rng='philox': with rng='torch' the reference's draw order depends on every molecule's last step")
        if (kwargs.get('dfm_type') or self.cfg.dfm_type) != 'campbell':
            raise NotImplementedError("per-molecule n_timesteps: dfm_type 'gat' is not supported")
        if xt_traj or ep_traj:
            raise NotImplementedError('per-molecule n_timesteps: xt_traj / ep_traj are not supported (no trajectory sink)')
        if kwargs.get('tspan') is not None:
            raise NotImplementedError('per-molecule n_timesteps: tspan is one schedule for the whole batch')

    # ---- stage 2: what make_step_plan takes
    def _plan_args(self, stochasticity, high_confidence_threshold, kwargs, dfm_type='campbell'):
        """(args, kwargs) of ``make_step_plan`` besides the step count and the Philox seed: stochasticity and confidence threshold (default: the
        model's), the temperature and forward-weight schedules (default: the configured ones) and the caller's tspan / inv_temp_func."""
        cfg = self.cfg
        eta = cfg.stochasticity if stochasticity is None else stochasticity
        hc = cfg.high_confidence_threshold if high_confidence_threshold is None else high_confidence_threshold
        return (eta, hc, kwargs.get('cat_temp_func') or cat_temp_schedule(cfg)), dict(
            tspan=kwargs.get('tspan'), dfm_type=dfm_type, forward_weight_func=kwargs.get('forward_weight_func') or forward_weight_schedule(cfg),
            inv_temp_func=kwargs.get('inv_temp_func'), schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)

    def _mixed_plan_args(self, stochasticity, high_confidence_threshold, kwargs):
        return self._plan_args(stochasticity, high_confidence_threshold, kwargs)

    # ---- stage 3: prior
    def _initial_state(self, req: "_Request", prior):
        """The initial state of the bound batch, and the Philox seed of the run (None with rng='torch').  A caller's ``prior`` dict is adapted to the
        model; without one the prior is drawn: inside the kernels from the per-molecule Philox streams, or with torch's generators in the reference's
        order (flowmol.py:417-448 / 534-545).  An endpoint model's own ``x_0`` is centred here; a caller's is taken as it is."""
        eng, cfg = self.engine, self.cfg
        endpoint, rows = req.path == 'endpoint', req.kw.get('_rows')
        seed = None
        if req.rng == 'philox' and not (endpoint and prior is not None):      # an endpoint run is deterministic behind its prior: a given prior needs no seed
            # one 62-bit seed per call from torch's CPU generator (torch.manual_seed controls it), drawn behind the bind
            seed = req.seed if req.seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
            eng.set_molecule_ids(None if req.mol_ids is None else torch.as_tensor(req.mol_ids))
        if prior is not None:
            x0, a0, c0, e0 = adapt_prior(prior, req.n_atoms, cfg, eng.E, only_missing_column=endpoint)
            if not endpoint:
                return eng.make_state(x0, a0.argmax(-1), c0.argmax(-1), e0.argmax(-1)), seed
            N = eng.N
            if a0.shape != (N, cfg.n_atom_types) or c0.shape != (N, cfg.n_charges) or tuple(x0.shape) != (N, 3):
                raise ValueError(f"prior shapes x_0 {tuple(x0.shape)}, a_0 {tuple(a0.shape)}, c_0 {tuple(c0.shape)} do not fit the batch "
                                 f"({N} atoms, {cfg.n_atom_types} atom types, {cfg.n_charges} charges)")
        elif seed is not None and not endpoint:
            return eng.prior_state(eng.prior_philox(seed)), seed
        elif seed is not None:          # the whole prior in one launch (fm_prior_philox_dense)
            p0 = eng.prior_philox_dense(seed, default_p=default_marginals(cfg))
            x0, a0, c0, e0 = p0['x_t'], p0['a_t'], p0['c_t'], p0['e_t']
        else:                           # rows: draw the full batch's prior, keep this shard's
            nN, nU = (eng.N, eng.U) if rows is None else rows[:2]
            x0 = torch.randn(nN, 3, device=eng.device)
            if endpoint:
                a0, c0, e0 = draw_categorical_priors(cfg, nN, nU, default_p=default_marginals(cfg))
            if rows is not None:
                x0 = x0[rows[2]].contiguous()
                if endpoint:
                    a0, c0, e0 = a0[rows[2].cpu()], c0[rows[2].cpu()], e0[rows[3].cpu()]
            eng.remove_com(x0)          # per molecule, so centring after the row selection equals centring the full batch
            if not endpoint:
                return eng.prior_state(x0), seed
        return eng.make_dense_state(x0, a0, c0, e0), seed

    # ---- stage 4: epilogue
    def _finish(self, state, n_atoms, frames, return_tensors, frames_in_tuple, xt_traj, ep_traj, t_integrate=None):
        """The final state on the device (tokens, or an endpoint model's continuous features) -> what the caller asked for with ``return_tensors``
        ('dense' | 'device' | True | False, see ``sample``); ``frames``: the run's frames on the device, where they stay for 'device'; ``frames_in_tuple``:
        the tensor forms return (out, n_atoms, frames).  ``last_timing``: 'integrate' and 'precision' (as set by the shard's sample() when
        ``t_integrate`` is None), 'to_host' when the result was copied and 'package' when molecules were built."""
        if t_integrate is not None:
            self.last_timing = {'integrate': t_integrate, 'precision': self.engine.precision}
        if return_tensors == 'dense' and state['a_t'].dim() == 2:
            return {k: state[f'{k}_t'] for k in 'xace'}, n_atoms
        out, t1 = _tokens(state), time.perf_counter()
        if return_tensors != 'device':
            out = _to_host(out)            # one packed device->host copy of the whole batch (1.7 KB/molecule)
            self.last_timing['to_host'] = time.perf_counter() - t1
            t2 = time.perf_counter()
            if frames is not None and (frames_in_tuple or not return_tensors):
                frames = {k: v.cpu() for k, v in frames.items()}
        if return_tensors:
            return (out, n_atoms, frames) if frames_in_tuple else (out, n_atoms)
        mols = self._package(out, n_atoms, frames, xt_traj, ep_traj)
        self.last_timing['package'] = time.perf_counter() - t2
        return mols

    def _package(self, out, n_atoms, frames, xt_traj, ep_traj) -> List[SampledMolecule]:
        """Host tensors of the whole batch -> one SampledMolecule per molecule, in batch order (flowmol.py:564-589)."""
        sizes = n_atoms.tolist()
        pairs = [n * (n - 1) // 2 for n in sizes]
        xs, as_, cs = torch.split(out['x'], sizes), torch.split(out['a'], sizes), torch.split(out['c'], sizes)
        es = torch.split(out['e'], pairs)
        fr = None
        if frames is not None:
            fr = {k: torch.split(v, pairs if k.startswith('e') else sizes, dim=1) for k, v in frames.items()}
        mols = []
        for i in range(len(sizes)):
            tf = {k: v[i] for k, v in fr.items()} if fr is not None else None
            mols.append(SampledMolecule(xs[i], as_[i], cs[i], es[i], self.atom_type_map, fake_atoms=self.fake_atoms,
                                        ctmc_mol=self.cfg.has_mask, explicit_aromaticity=self.explicit_aromaticity, traj_frames=tf,
                                        build_xt_traj=xt_traj, build_ep_traj=ep_traj, n_charges=self.n_atom_charges))
        return mols

    def sampling_queue(self, seed: int, stochasticity=None, high_confidence_threshold=None, **kwargs) -> "SamplingQueue":
        """A queue that admits requests into a batch that is already running (flowmol_amd.sampling_queue.SamplingQueue)."""
        from .sampling_queue import SamplingQueue
        return SamplingQueue(self, seed, stochasticity=stochasticity, high_confidence_threshold=high_confidence_threshold, **kwargs)


# what sample() names itself; everything else arrives in **kwargs and is checked against the path's table
SAMPLE_NAMED_ARGS = ('device', 'stochasticity', 'high_confidence_threshold', 'xt_traj', 'ep_traj', 'prior')
_PHILOX_KWARGS = {'rng', 'seed', 'mol_ids', '_philox', '_mol_ids'}
ALLOWED_KWARGS = {
    'ctmc': {'dfm_type', 'tspan', 'cat_temp_func', 'forward_weight_func', 'inv_temp_func', '_rows', '_noise_for_step', '_frames'} | _PHILOX_KWARGS,
    'endpoint': {'inv_temp_func', 'tspan', '_rows', '_frames'} | _PHILOX_KWARGS,
    'mixed': {'dfm_type', 'tspan', 'cat_temp_func', 'forward_weight_func', 'inv_temp_func'} | _PHILOX_KWARGS,
}


RESAMPLE_KWARGS = {'dfm_type', 'tspan', 'cat_temp_func', 'forward_weight_func', 'inv_temp_func'}       # resample(): Philox only, so no rng and no noise hooks


def _check_coupling(coupling, n_atoms: torch.Tensor, who: str) -> None:
    """The refusals of a ``coupling`` argument, before any bind: an unknown value; with 'ot', a molecule above the cap of fm_ot_align."""
    if coupling not in ('independent', 'ot'):
        raise ValueError(f"{who}: coupling must be 'independent' or 'ot', got {coupling!r}")
    if coupling == 'ot' and n_atoms.numel() and int(n_atoms.max()) > _lib.FM_OT_MAX_ATOMS:
        m = int(n_atoms.argmax())
        raise ValueError(f"{who}: coupling='ot' takes molecules of at most {_lib.FM_OT_MAX_ATOMS} atoms, molecule {m} has {int(n_atoms[m])}")


def _keep_flat(keep, sizes, name: str, what: str) -> torch.Tensor:
    """One ``keep`` entry as a bool tensor over the concatenated rows: ``keep`` is a bool tensor of sum(sizes) entries or one bool sequence per molecule,
    molecule i's of sizes[i] entries (``what``: 'atoms' or 'pairs').  ValueError for anything else."""
    if torch.is_tensor(keep):
        if keep.dtype != torch.bool:
            raise ValueError(f'{name} must be a bool tensor, got {keep.dtype}')
        flat = keep.detach().cpu().reshape(-1)
    else:
        rows = list(keep)
        if len(rows) != len(sizes):
            raise ValueError(f'{name} has {len(rows)} entries for {len(sizes)} molecules (one bool sequence per molecule)')
        cols = []
        for i, (r, n) in enumerate(zip(rows, sizes)):
            r = r.detach().cpu().reshape(-1) if torch.is_tensor(r) else torch.as_tensor(list(r))
            if r.numel() != n:
                raise ValueError(f'{name}[{i}] has {r.numel()} entries, molecule {i} has {n} {what}')
            if n and r.dtype != torch.bool:
                raise ValueError(f'{name}[{i}] must hold bools, got {r.dtype}')
            cols.append(r.to(torch.bool))
        flat = torch.cat(cols) if cols else torch.zeros(0, dtype=torch.bool)
    if flat.numel() != sum(sizes):
        raise ValueError(f'{name} has {flat.numel()} entries, the molecules have {sum(sizes)} {what}')
    return flat


def _keep_atoms(keep, n_atoms: torch.Tensor) -> Optional[torch.Tensor]:
    """The whole-atom ``keep`` of resample() / submit_from() as one bool tensor over the concatenated atoms, or None when nothing is kept.  ValueError for
    anything but a bool tensor of N entries or one bool sequence per molecule, each of the molecule's length."""
    if keep is None:
        return None
    flat = _keep_flat(keep, n_atoms.tolist(), 'keep', 'atoms')
    return flat if bool(flat.any()) else None


def _keep_rows(keep, n_atoms: torch.Tensor):
    """``keep`` of resample() / submit_from() in either form: None when nothing is kept; a bool tensor over the concatenated atoms (the whole-atom form,
    ``_keep_atoms``); or, for a dict {'x', 'a', 'c': atoms, 'e': unordered pairs}, a dict of bool tensors over the concatenated rows that holds the
    modalities with a frozen row.  ValueError for an unknown key, a wrong length and a dtype other than bool."""
    if not isinstance(keep, dict):
        return _keep_atoms(keep, n_atoms)
    unknown = [k for k in keep if k not in ('x', 'a', 'c', 'e')]
    if unknown:
        raise ValueError(f"keep has unknown keys {sorted(map(str, unknown))}: 'x', 'a', 'c' (per atom) and 'e' (per unordered pair) are the modalities")
    sizes = n_atoms.tolist()
    pairs = [n * (n - 1) // 2 for n in sizes]
    rows = {f: _keep_flat(keep[f], pairs if f == 'e' else sizes, f"keep['{f}']", 'pairs' if f == 'e' else 'atoms') for f in 'xace' if keep.get(f) is not None}
    rows = {f: v for f, v in rows.items() if bool(v.any())}
    return rows or None


def _pairs_of_atoms(keep_atom: torch.Tensor) -> torch.Tensor:
    """One molecule's whole-atom keep as its pair flags, upper-triangle order: a pair is kept iff both its atoms are (the rule of fm_inpaint)."""
    n = int(keep_atom.shape[0])
    i, j = torch.triu_indices(n, n, 1)
    return keep_atom[i] & keep_atom[j]


def _grouped(items: list, counts) -> List[list]:
    """A flat list cut into consecutive lists of ``counts`` items."""
    out, k = [], 0
    for n in counts:
        out.append(items[k:k + n])
        k += n
    return out


def _split_molecules(state: Dict[str, torch.Tensor], sizes) -> List[Dict[str, torch.Tensor]]:
    """A batch's token state {'x_t', 'a_t', 'c_t', 'e_t'} as one dict per molecule (views)."""
    pairs = [n * (n - 1) // 2 for n in sizes]
    cols = {k: torch.split(v, pairs if k == 'e_t' else sizes) for k, v in state.items()}
    return [{k: cols[k][i] for k in state} for i in range(len(sizes))]


@dataclass
class _Request:
    """One sample() call behind the argument stage (``FlowMol._request``)."""
    path: str                       # 'ctmc' | 'endpoint' | 'mixed'
    n_atoms: torch.Tensor           # (B,) int64 on the CPU
    n_timesteps: object             # one count for the batch, as given or the model's default ('ctmc', 'endpoint')
    counts: Optional[List[int]]     # one count per molecule ('mixed')
    rng: str                        # 'torch' | 'philox'
    dfm_type: str
    seed: Optional[int]             # the caller's Philox seed; None: one draw from the CPU generator behind the bind
    mol_ids: object                 # the caller's Philox stream ids; None: 0..B-1
    kw: dict                        # the checked keyword arguments: schedules, tspan, _rows, _noise_for_step, _frames

    @property
    def n_points(self) -> int:
        """Time points of the run = frames of a visualised one."""
        ts = self.kw.get('tspan')
        return int(self.n_timesteps) if ts is None else int(ts.shape[0])


def _step_counts(n_timesteps):
    """A per-molecule sequence of step counts as a list of ints, or None for what sample() has always taken (None, an int, a 0-dim tensor)."""
    if n_timesteps is None or isinstance(n_timesteps, int):
        return None
    if torch.is_tensor(n_timesteps):
        return None if n_timesteps.dim() == 0 else [int(v) for v in n_timesteps.reshape(-1).tolist()]
    if isinstance(n_timesteps, (list, tuple)) or (hasattr(n_timesteps, '__len__') and hasattr(n_timesteps, '__iter__')):
        return [int(v) for v in n_timesteps]
    return None


def _tokens(state: Dict[str, torch.Tensor], copy: bool = False) -> Dict[str, torch.Tensor]:
    """{'x', 'a', 'c', 'e'} of a state on its device: coordinates and int32 tokens -- a CTMC state's own tensors (clones with ``copy``), the argmax
    of an endpoint model's continuous (rows, K) features."""
    out = {}
    for k in 'xace':
        v = state[f'{k}_t']
        out[k] = v.argmax(-1).int() if k != 'x' and v.dim() == 2 else (v.clone() if copy else v)
    return out


def _frames_of(init: Dict[str, torch.Tensor], traj: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Compact frames of a visualised run on the device: 'x', 'a', 'c', 'e' = the prior + the state after every step (T frames), '*_1_pred' = every step's
    endpoint prediction (T - 1 frames) -- the frame set of the reference (ctmc_vector_field.py:188-202,235-283), tokens instead of one-hots."""
    frames = {k: torch.cat([init[k].unsqueeze(0), traj[k]]) for k in 'xace'}
    frames.update({f'{k}_1_pred': traj[f'{k}1'] for k in 'xace'})
    return frames


def _to_host(dev_out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Final state of a batch, device -> host, as ONE packed copy (x fp32 | a, c, e as bytes: 14 B/atom + 1 B/pair)."""
    if dev_out['x'].device.type == 'cpu':
        return {k: v for k, v in dev_out.items()}
    N, U = int(dev_out['x'].shape[0]), int(dev_out['e'].shape[0])
    return shard.unpack_results(shard.pack_results(dev_out['x'], dev_out['a'], dev_out['c'], dev_out['e']).cpu(), N, U)


# names accepted by the reference's load_pretrained (flowmol/__init__.py:5-28)
pretrained_model_names = [
    'flowmol3', 'fm3_nodistort', 'fm3_none', 'fm3_ahigh', 'fm3_alow', 'fm3_chigh', 'fm3_clow', 'fm3_distort_extreme',
    'fm3_distort_highp', 'fm3_distort_hight', 'fm3_distort_lowp', 'fm3_distort_lowt', 'fm3_ehigh', 'fm3_elow',
    'fm3_fa_highp', 'fm3_fa_highstd', 'fm3_fa_lowp', 'fm3_fa_lowstd', 'fm3_scprop_high', 'fm3_scprop_low',
    'fm3_xhigh', 'fm3_xlow',
]


def load_pretrained(model_name: str = 'flowmol3', precision: Optional[str] = None) -> FlowMol:
    """Load ``<models_dir>/<model_name>/checkpoints/last.ckpt`` (reference flowmol/__init__.py:30-56).  ``precision`` (not a reference argument;
    None = 'f32', the reference's arithmetic) selects an opt-in split-precision mode of the engine ('f16x3', 'bf16x3', 'bf16x6').

    ``models_dir`` is ``$FLOWMOL_MODELS_DIR`` or ``flowmol_amd/trained_models``.  The reference downloads
    missing models with wget; there is no network in this environment, so a missing directory is an error
    that says where to put the files (``FlowMol.from_preset`` gives the same architecture with synthetic weights)."""
    if model_name not in pretrained_model_names:
        raise ValueError(f'Model {model_name} not found. Supported models: {pretrained_model_names}')
    root = Path(os.environ.get('FLOWMOL_MODELS_DIR', PKG / 'trained_models'))
    ckpt = root / model_name / 'checkpoints' / 'last.ckpt'
    if not ckpt.exists():
        raise FileNotFoundError(
            f'{ckpt} not found. Download the model directory from https://bits.csb.pitt.edu/files/FlowMol/trained_models_v3.1/'
            f'{model_name}/ into {root} (or set FLOWMOL_MODELS_DIR); this build has no network access and does not wget.')
    kw = {}
    if 'qm9' in model_name:
        kw['n_atoms_hist'] = 'qm9'
    if precision is not None:
        kw['precision'] = precision
    return FlowMol.load_from_checkpoint(ckpt, **kw)

