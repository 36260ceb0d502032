"""Python host side of the HIP engine: owns the ``fm_ctx``, the per-batch workspace and the state
tensors, and mirrors the call structure of the reference's ``CTMCVectorField`` for the sampling path
(reference flowmol/models/ctmc_vector_field.py:145-411, flowmol/models/vector_field.py:212-293).

PyTorch is used for device memory, the current stream and (optionally) noise generation only; all
arithmetic of the hot path happens in libflowmol_hip.so.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import _lib
from ._lib import (FM_DFM_CAMPBELL, FM_DFM_GAT, FM_NOISE_PHILOX, FlowMolHipError, fm_dense_state, fm_endpoint_scalars, fm_config, fm_dst, fm_prior_spec, fm_sampled, fm_state, fm_step_noise,
                   fm_step_scalars, fm_tensor_desc, fm_traj_sink)
from .config import VFConfig
from .weights import check_state_dict, state_dict_shapes


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def time_embedding_host(t: float, dim: int) -> torch.Tensor:
    """Sinusoidal time embedding of one scalar t, float32 on the host
    (reference flowmol/utils/embedding.py:5-17; max_positions=1000).  dim == 1 -> raw t."""
    tt = torch.tensor([t], dtype=torch.float32)
    if dim == 1:
        return tt.clone()
    ts = tt * 1000
    half = dim // 2
    emb = math.log(1000) / (half - 1)
    emb = torch.exp(torch.arange(half, dtype=torch.float32) * -emb)
    emb = ts.float()[:, None] * emb[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1)
    if dim % 2 == 1:
        emb = torch.nn.functional.pad(emb, (0, 1))
    return emb[0].contiguous()


@dataclass
class StepPlan:
    """Per-step scalars computed with the reference's float32 tensor arithmetic
    (ctmc_vector_field.py:170-176,205-233,331-334,430-434)."""
    t: torch.Tensor                # (T,) float32 time points
    scalars: List[fm_step_scalars]


def cat_temp_schedule(cfg: VFConfig) -> Callable:
    """CTMCVectorField.build_cat_temp_schedule (ctmc_vector_field.py:71-82) for the configured schedule."""
    sched = cfg.cat_temperature_schedule
    if sched == 'decay':
        mx, a = cfg.cat_temp_decay_max, cfg.cat_temp_decay_a
        return lambda t: mx * torch.pow(1 - t, a)
    val = cfg.cat_temperature if isinstance(sched, str) else sched
    return lambda t: val


def forward_weight_schedule(cfg: VFConfig) -> Callable:
    """CTMCVectorField.build_fw_schedule (ctmc_vector_field.py:84-95)."""
    sched = cfg.forward_weight_schedule
    if sched == 'beta':
        a, b, mx = cfg.fw_beta_a, cfg.fw_beta_b, cfg.fw_beta_max
        return lambda t: 1 + mx * torch.pow(t, a) * torch.pow(1 - t, b)
    return lambda t: sched


def _f32(v) -> float:
    """A Python number or 0-dim tensor as the float32 value a torch op on float32 tensors would use."""
    return float(v.to(torch.float32)) if torch.is_tensor(v) else float(torch.tensor(v, dtype=torch.float32))


def alpha_tables(t: torch.Tensor, schedule_type=None, cosine_params=None):
    """InterpolantScheduler.alpha_t / alpha_t_prime (interpolant_scheduler.py:97-153) for the time points ``t`` (T,), columns in the
    canonical order x, a, c, e, with the reference's float32 tensor arithmetic -- INCLUDING its side effect: the cosine
    derivative clamps ``t`` in place to >= 1e-9 (:140-141), after alpha_t was taken from the unclamped tensor
    (ctmc_vector_field.py:175-176), so a cosine-scheduled trajectory starts at t = 1e-9 and has no bootstrap evaluation."""
    schedule_type = schedule_type or {}
    cosine_params = cosine_params or {}
    nus = {k: torch.tensor(cosine_params[k]).unsqueeze(0) for k in cosine_params}        # interpolant_scheduler.py:53-55
    cols = []
    for k in 'xace':
        if schedule_type.get(k, 'linear') == 'cosine':
            cols.append(1 - torch.cos(torch.pi * 0.5 * torch.pow(t.unsqueeze(-1), nus[k])).square())
        else:
            cols.append(t.unsqueeze(-1))
    alpha = torch.cat(cols, dim=1)
    cols = []
    for k in 'xace':
        if schedule_type.get(k, 'linear') == 'cosine':
            t = torch.clamp_(t, min=1e-9)
            tt = t.unsqueeze(-1)
            cols.append(torch.pi * 0.5 * torch.sin(torch.pi * torch.pow(tt, nus[k])) * nus[k] * torch.pow(tt, nus[k] - 1))
        else:
            cols.append(torch.ones_like(t).unsqueeze(-1))
    return alpha, torch.cat(cols, dim=1)


def euler_steps(n_timesteps: int, tspan: Optional[torch.Tensor] = None, schedule_type=None, cosine_params=None):
    """The time points of an integration (``tspan``, or n_timesteps points on [0, 1]) and, per Euler step, (t_i, dt, alpha(t_i), alpha'(t_i)) with
    the columns of ``alpha_tables``: what the CTMC plan and the endpoint integrator both walk (ctmc_vector_field.py:169-178, vector_field.py:430-434)."""
    t = torch.linspace(0, 1, n_timesteps) if tspan is None else tspan.detach().to('cpu', torch.float32).clone()
    alpha, alpha_p = alpha_tables(t, schedule_type, cosine_params)      # (T,4) each; may clamp t[0] in place (cosine)
    return t, [(t[i - 1], t[i] - t[i - 1], alpha[i - 1], alpha_p[i - 1]) for i in range(1, t.shape[0])]


def make_step_plan(n_timesteps: int, eta: float, hc_thresh: float, cat_temperature,
                   tspan: Optional[torch.Tensor] = None, dfm_type: str = 'campbell', forward_weight_func: Optional[Callable] = None,
                   inv_temp_func: Optional[Callable] = None, philox_seed: Optional[int] = None,
                   schedule_type=None, cosine_params=None) -> StepPlan:
    """Per-step scalars of CTMCVectorField.integrate/step (ctmc_vector_field.py:169-178, 287-340), computed with the
    reference's own float32 tensor arithmetic.  ``cat_temperature`` is a number or a callable of the 0-dim tensor t_i."""
    t, steps = euler_steps(n_timesteps, tspan, schedule_type, cosine_params)
    if dfm_type not in ('campbell', 'gat'):
        raise ValueError(f"Invalid dfm_type: {dfm_type}")
    out = []
    for s_idx, (t_i, dt, a_i, ap_i) in enumerate(steps, 1):      # a_i, ap_i: columns x, a, c, e
        sc = fm_step_scalars()
        sc.t = float(t_i)
        sc.dt = float(dt)
        sc.x_coef = float(ap_i[0] / (1 - a_i[0]))
        mask = torch.clamp(dt * eta, min=0, max=1)
        for k in range(3):
            sc.unmask_prob[k] = float(torch.clamp(dt * (ap_i[k + 1] + eta * a_i[k + 1]) / (1 - a_i[k + 1]), min=0, max=1))
            sc.mask_prob[k] = float(mask)
        sc.hc_thresh = float(torch.tensor(hc_thresh, dtype=torch.float32))
        sc.cat_temperature = _f32(cat_temperature(t_i) if callable(cat_temperature) else cat_temperature)
        sc.last_step = 1 if s_idx == t.shape[0] - 1 else 0
        sc.x_scale = 1.0 if inv_temp_func is None else _f32(inv_temp_func(t_i))
        sc.dfm_type = FM_DFM_GAT if dfm_type == 'gat' else FM_DFM_CAMPBELL
        if dfm_type == 'gat':
            fw = 1.0 if forward_weight_func is None else forward_weight_func(t_i)
            bw = fw - 1                                     # python or tensor arithmetic, as in gat_step
            for k in range(3):
                sc.gat_cf[k] = float(ap_i[k + 1] / (1 - a_i[k + 1]))
                sc.gat_cb[k] = float(ap_i[k + 1] / (a_i[k + 1] + 1e-8))
            sc.gat_fw, sc.gat_bw = _f32(fw), _f32(bw)
        if philox_seed is not None:        # noise drawn inside the CTMC kernel from per-molecule counter-based streams (fm_noise_mode), campbell and gat
            sc.noise_mode = FM_NOISE_PHILOX
            sc.step_index = s_idx - 1
            sc.philox_seed_lo, sc.philox_seed_hi = philox_seed & 0xffffffff, (philox_seed >> 32) & 0xffffffff
        out.append(sc)
    return StepPlan(t, out)


def mixed_step_arrays(plans: Sequence[StepPlan], start: Sequence[int], n_steps: int, time_embedding_dim: int):
    """Host arrays of one fm_integrate_mixed call: (n_steps * G) fm_step_scalars and int32 active flags, row k * G + g = step start[g] + k of
    plans[g] (inactive, zeroed, once the plan has run out), and the (n_steps * G, time_embedding_dim) time embeddings of those steps."""
    G = len(plans)
    scal = (fm_step_scalars * (n_steps * G))()
    act = (C.c_int32 * (n_steps * G))()
    temb = torch.zeros(n_steps * G, time_embedding_dim)
    rows = {}
    for k in range(n_steps):
        for g in range(G):
            if start[g] + k < len(plans[g].scalars):
                sc = plans[g].scalars[start[g] + k]
                scal[k * G + g] = sc
                act[k * G + g] = 1
                if sc.t not in rows:
                    rows[sc.t] = time_embedding_host(sc.t, time_embedding_dim)
                temb[k * G + g] = rows[sc.t]
    return scal, act, temb


def noise_layout(last_step: bool, dfm_type: str = 'campbell', N: int = 0, U: int = 0, na: int = 0, nc: int = 0, ne: int = 0):
    """(field, rows, width) of the noise tensors of one CTMC step in the reference's draw order -- per modality a, c, e: q Exp(1) (rows, K), u1 and
    u2 uniform (rows,) [width None; u2 not drawn on the last step]; 'gat': q (rows, K + 1) only.  The one description every producer iterates."""
    gat = dfm_type == 'gat'
    for tag, rows, k in (('a', N, na), ('c', N, nc), ('e', U, ne)):
        yield f'q_{tag}', rows, k + 1 if gat else k
        if not gat:
            yield f'u1_{tag}', rows, None
            if not last_step:
                yield f'u2_{tag}', rows, None


class StepNoise:
    """The nine noise tensors of one CTMC step, in the reference's draw order (``noise_layout``); a tensor that is not drawn is None."""
    __slots__ = ('q_a', 'u1_a', 'u2_a', 'q_c', 'u1_c', 'u2_c', 'q_e', 'u1_e', 'u2_e')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    @staticmethod
    def draw(N: int, U: int, na: int, nc: int, ne: int, last_step: bool, device, generator=None, dfm_type: str = 'campbell') -> "StepNoise":
        """Draw with torch's generator on ``device`` exactly as the reference's ops would
        (torch.multinomial's Exp(1) draw, then the two torch.rand calls; 'gat': one Exp(1) draw over K+1 classes)."""
        out = {}
        for field, rows, width in noise_layout(last_step, dfm_type, N, U, na, nc, ne):
            if width is None:
                out[field] = torch.rand(rows, device=device, generator=generator)
            else:
                out[field] = torch.empty(rows, width, device=device, dtype=torch.float32).exponential_(1, generator=generator)
        return StepNoise(**out)

    @staticmethod
    def from_tape(tape: Sequence[torch.Tensor], pos: int, last_step: bool, device, dfm_type: str = 'campbell') -> "tuple[StepNoise, int]":
        fields = [f for f, _, _ in noise_layout(last_step, dfm_type)]
        out = {f: tape[pos + i].to(device, torch.float32).contiguous() for i, f in enumerate(fields)}
        return StepNoise(**out), pos + len(fields)

    def take_rows(self, node_rows: torch.Tensor, pair_rows: torch.Tensor) -> "StepNoise":
        """The draws of a subset of the batch's nodes / unordered pairs (sharded runs that replicate the full-batch noise)."""
        out = {}
        for k in self.__slots__:
            t = getattr(self, k)
            out[k] = None if t is None else t[pair_rows if k.endswith('_e') else node_rows].contiguous()
        return StepNoise(**out)

    def c_struct(self) -> fm_step_noise:
        s = fm_step_noise()
        for k in self.__slots__:
            setattr(s, k, _ptr(getattr(self, k)))
        return s


class Engine:
    """One ``fm_ctx`` on one device."""

    def __init__(self, cfg: VFConfig, state_dict: Dict[str, torch.Tensor], device='cuda:0', prefix: str = '', lib=None, precision: Optional[str] = None,
                 tuning: Optional[Dict[str, int]] = None):
        """``precision``: 'f32' (default, also for None; the reference's arithmetic), 'bf16x3' (OPT-IN split precision of the edge-message
        GEMMs on the bf16 matrix cores: faster, ~10x larger per-stage error, never used for parity claims) or 'bf16x6' (OPT-IN three-term split of the
        edge-message GEMMs only: f32-class accuracy on the bf16 matrix cores; round 5's measurement of whether that beats the f32 roof).  It is an explicit argument
        only -- no environment variable changes what an Engine computes -- and is recorded in ``self.precision``.
        ``tuning``: launch-tuning overrides of fm_config (ABI 5 / 6 / 8: tile_edge, tile_node, tile_edge_update, xcd_swizzle, fuse_node, pair_mlps, pair_slab,
        mlp_small_tiles, ctmc_threads; 0 / absent = automatic) for A/B measurements and the parity tests that run every tile size."""
        precision = precision or 'f32'
        if precision not in ('f32', 'bf16x3', 'bf16x6', 'f16x3'):
            raise ValueError(f"precision must be 'f32', 'bf16x3', 'bf16x6' or 'f16x3', got {precision!r}")
        self.precision = precision
        self.tuning = {k: int(v) for k, v in (tuning or {}).items() if int(v) != 0}
        unknown = set(self.tuning) - set(_lib.TUNING_FIELDS)
        if unknown:
            raise ValueError(f'unknown tuning fields {sorted(unknown)}; have {_lib.TUNING_FIELDS}')
        cfg.validate()
        self.cfg = cfg
        self.device = torch.device(device)
        self.lib = lib if lib is not None else _lib.get_lib()
        check_state_dict(cfg, state_dict, prefix)
        shapes = state_dict_shapes(cfg)
        # ---- flat host blob + descriptors, keys named as in the reference state dict
        descs = (fm_tensor_desc * len(shapes))()
        chunks, off = [], 0
        self._names = []
        for i, (key, shape) in enumerate(shapes.items()):
            t = state_dict[prefix + key].detach().to('cpu', torch.float32).contiguous().reshape(-1)
            chunks.append(t)
            nm = key.encode()
            self._names.append(nm)
            descs[i].name = nm
            descs[i].offset = off
            descs[i].ndim = len(shape)
            descs[i].shape[0] = shape[0]
            descs[i].shape[1] = shape[1] if len(shape) > 1 else 0
            off += t.numel()
        blob = torch.cat(chunks) if chunks else torch.zeros(0)
        c = fm_config()
        c.abi_version = _lib.FM_ABI_VERSION
        c.n_atom_types, c.n_charges, c.n_bond_types = cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types
        c.n_vec_channels, c.n_hidden_scalars, c.n_hidden_edge_feats = cfg.n_vec_channels, cfg.n_hidden_scalars, cfg.n_hidden_edge_feats
        c.rbf_dim, c.n_convs, c.n_updaters = cfg.rbf_dim, cfg.n_convs, cfg.n_updaters
        sched = cfg.update_schedule()
        if len(sched) > _lib.FM_MAX_CONVS:
            raise NotImplementedError(f'more than {_lib.FM_MAX_CONVS} convolutions')
        for i in range(_lib.FM_MAX_CONVS):
            c.update_after[i] = sched[i] if i < len(sched) else -1
        c.self_conditioning = int(cfg.self_conditioning)
        c.time_embedding_dim = cfg.time_embedding_dim
        c.a_token_dim, c.c_token_dim, c.e_token_dim = cfg.a_token_dim, cfg.c_token_dim, cfg.e_token_dim
        c.rbf_dmax = float(cfg.rbf_dmax)
        c.msg_z = float(cfg.msg_z)
        c.s_dst_feats, c.v_dst_feats = cfg.s_dst_feats, cfg.v_dst_feats
        c.has_mask = int(cfg.has_mask)
        c.precision = {'f32': _lib.FM_PREC_F32, 'bf16x3': _lib.FM_PREC_BF16X3, 'bf16x6': _lib.FM_PREC_BF16X6, 'f16x3': _lib.FM_PREC_F16X3}[precision]
        c.n_recycles = int(cfg.n_recycles)
        c.edge_update_no_distance = int(not cfg.update_edge_w_distance)
        for k, v in self.tuning.items():
            setattr(c, k, v)
        self._ctx = C.c_void_p()
        with self._dev():
            rc = self.lib.fm_create(C.byref(c), descs, len(shapes), C.c_void_p(blob.data_ptr()), C.byref(self._ctx))
        if rc != 0:
            raise FlowMolHipError(f'fm_create failed ({rc}): {self.lib.fm_last_error(None).decode()}')
        self._keep = []          # tensors referenced by raw pointer inside the library
        self.N = self.E = self.U = self.B = 0
        self._ws = None
        self.n_atoms = None

    # ------------------------------------------------------------------ plumbing
    def _dev(self):
        return torch.cuda.device(self.device) if self.device.type == 'cuda' else contextlib.nullcontext()

    @contextlib.contextmanager
    def _taps(self, taps: Optional[Dict[str, torch.Tensor]]):
        """Taps set for the evaluation inside the block (stale ones cleared first), cleared again behind it."""
        self.lib.fm_clear_taps(self._ctx)
        for k, v in (taps or {}).items():
            self._check(self.lib.fm_set_tap(self._ctx, k.encode(), _ptr(v)), 'fm_set_tap')
        yield
        if taps:
            self.lib.fm_clear_taps(self._ctx)

    def _stream(self):
        if self.device.type == 'cuda':
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def _check(self, rc, what):
        if rc != 0:
            raise FlowMolHipError(f'{what} failed ({rc}): {self.lib.fm_last_error(self._ctx).decode()}')

    def close(self):
        if getattr(self, '_ctx', None) is not None and self._ctx.value:
            if self.device.type == 'cuda':
                torch.cuda.synchronize(self.device)
            self.lib.fm_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ batch
    def workspace_need(self, n_atoms: torch.Tensor) -> int:
        """Bytes of workspace a batch of these molecule sizes needs (fm_workspace_bytes)."""
        n = torch.as_tensor(n_atoms).detach().to('cpu', torch.int32).contiguous()
        if n.dim() != 1 or n.numel() == 0:
            raise ValueError('n_atoms must be a non-empty 1-D tensor')
        need = C.c_size_t()
        self._check(self.lib.fm_workspace_bytes(self._ctx, C.c_void_p(n.data_ptr()), n.numel(), C.byref(need)), 'fm_workspace_bytes')
        return int(need.value)

    def bind(self, n_atoms: torch.Tensor, workspace: Optional[torch.Tensor] = None):
        """Bind a batch of molecules given their sizes (order preserved).  Replaces the reference's
        dgl.graph / dgl.batch / upper-edge-mask / batch-index construction (flowmol.py:509-529).
        ``workspace``: a caller-owned uint8 tensor on the engine's device, 256-byte aligned and of at least ``workspace_need(n_atoms)``
        bytes, used as the batch's arena as it is (what fm_batch_bind takes in C).  The engine keeps a reference and never reallocates it: later
        binds without ``workspace`` stay in it while it is large enough, and move to an allocation of the engine's own when it is not."""
        n = n_atoms.detach().to('cpu', torch.int32).contiguous()
        if n.dim() != 1 or n.numel() == 0:
            raise ValueError('n_atoms must be a non-empty 1-D tensor')
        need = C.c_size_t(self.workspace_need(n))
        if workspace is not None:
            if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
                raise ValueError('workspace must be a contiguous 1-D uint8 tensor')
            if workspace.device != self.device and not (workspace.device.type == self.device.type == 'cuda' and
                                                        workspace.device.index == (self.device.index or 0)):
                raise ValueError(f'workspace must be on {self.device}, got {workspace.device}')
            if workspace.data_ptr() % 256 != 0:
                raise ValueError('workspace must be 256-byte aligned (data_ptr() % 256 == 0)')
            if workspace.numel() < need.value:
                raise ValueError(f'workspace has {workspace.numel()} bytes, the batch needs {need.value}')
            self._ws = workspace
        elif self._ws is None or self._ws.numel() < need.value + (-self._ws.data_ptr()) % 256:
            self._ws = None
            self._ws = torch.empty(need.value + 256, dtype=torch.uint8, device=self.device)
        base = self._ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        with self._dev():
            self._check(self.lib.fm_batch_bind(self._ctx, self._stream(), C.c_void_p(n.data_ptr()), n.numel(),
                                               C.c_void_p(aligned), need.value), 'fm_batch_bind')
        n64 = n.to(torch.int64)
        self.n_atoms = n64
        self.B = int(n.numel())
        self.N = int(n64.sum())
        self.E = int((n64 * (n64 - 1)).sum())
        self.U = self.E // 2
        self.workspace_bytes = int(need.value)
        return self

    def query(self, name: str) -> torch.Tensor:
        cnt = {'e_src': self.E, 'e_dst': self.E, 'e_pair': self.E, 'p_e0': self.U, 'p_e1': self.U,
               'node_mol': self.N, 'pair_mol': self.U}[name]
        out = torch.empty(cnt, dtype=torch.int32, device=self.device)
        if cnt == 0:          # a batch without edges: nothing to copy (and an empty tensor has no pointer to pass)
            return out
        with self._dev():
            self._check(self.lib.fm_batch_query(self._ctx, self._stream(), name.encode(), _ptr(out)), 'fm_batch_query')
        self.synchronize()
        return out

    # ------------------------------------------------------------------ tensors
    def new_dst(self) -> Dict[str, torch.Tensor]:
        d = self.device
        return {'x': torch.empty(self.N, 3, device=d), 'a': torch.empty(self.N, self.cfg.n_atom_types, device=d),
                'c': torch.empty(self.N, self.cfg.n_charges, device=d), 'e': torch.empty(self.U, self.cfg.n_bond_types, device=d)}

    @staticmethod
    def _dst_struct(d) -> fm_dst:
        s = fm_dst()
        s.x, s.a, s.c, s.e = _ptr(d['x']), _ptr(d['a']), _ptr(d['c']), _ptr(d['e'])
        return s

    @staticmethod
    def _state_struct(st, struct=fm_state):
        s = struct()
        s.x_t, s.a_t, s.c_t, s.e_t = _ptr(st['x_t']), _ptr(st['a_t']), _ptr(st['c_t']), _ptr(st['e_t'])
        return s

    @staticmethod
    def _dense_struct(st) -> fm_dense_state:
        return Engine._state_struct(st, fm_dense_state)

    def new_traj(self, n_steps: int) -> Dict[str, torch.Tensor]:
        """The eight per-step frame buffers of a visualised run (fm_traj_sink): state 'x', 'a', 'c', 'e' after every step, endpoint predictions '*1'."""
        f32, i32 = dict(device=self.device), dict(dtype=torch.int32, device=self.device)
        return {'x': torch.empty(n_steps, self.N, 3, **f32), 'a': torch.empty(n_steps, self.N, **i32),
                'c': torch.empty(n_steps, self.N, **i32), 'e': torch.empty(n_steps, self.U, **i32),
                'x1': torch.empty(n_steps, self.N, 3, **f32), 'a1': torch.empty(n_steps, self.N, **i32),
                'c1': torch.empty(n_steps, self.N, **i32), 'e1': torch.empty(n_steps, self.U, **i32)}

    def make_state(self, x_t, a_t, c_t, e_t) -> Dict[str, torch.Tensor]:
        """x_t (N,3) float; a_t, c_t (N) and e_t (U, per unordered pair in reference upper-edge order) int tokens."""
        d = self.device
        st = {'x_t': x_t.detach().to(d, torch.float32).contiguous().clone(),
              'a_t': a_t.detach().to(d, torch.int32).contiguous().clone(),
              'c_t': c_t.detach().to(d, torch.int32).contiguous().clone(),
              'e_t': e_t.detach().to(d, torch.int32).contiguous().clone()}
        assert st['x_t'].shape == (self.N, 3) and st['a_t'].shape == (self.N,) and st['e_t'].shape == (self.U,)
        return st

    def prior_state(self, x_0: torch.Tensor) -> Dict[str, torch.Tensor]:
        """CTMC masked prior for a, c, e (priors.py:101-107,305-316) around given positions."""
        return self.make_state(x_0, torch.full((self.N,), self.cfg.n_atom_types, dtype=torch.int32),
                               torch.full((self.N,), self.cfg.n_charges, dtype=torch.int32),
                               torch.full((self.U,), self.cfg.n_bond_types, dtype=torch.int32))

    def remove_com(self, x: torch.Tensor) -> torch.Tensor:
        """In-place per-molecule centring of an (N,3) tensor on the engine's device."""
        assert x.is_contiguous() and x.dtype == torch.float32 and x.shape == (self.N, 3)
        with self._dev():
            self._check(self.lib.fm_remove_com(self._ctx, self._stream(), _ptr(x)), 'fm_remove_com')
        return x

    def set_molecule_ids(self, ids: Optional[torch.Tensor]):
        """Global ids of the bound batch's molecules for the Philox noise streams (None = 0..B-1): a molecule keeps its id, and
        therefore its draws, however the batch is sharded."""
        if ids is None:
            ptr = None
        else:
            ids = ids.detach().to('cpu', torch.int32).contiguous()
            assert ids.shape == (self.B,)
            ptr = C.c_void_p(ids.data_ptr())
        with self._dev():
            self._check(self.lib.fm_set_molecule_ids(self._ctx, self._stream(), ptr), 'fm_set_molecule_ids')

    def prior_philox(self, seed: int) -> torch.Tensor:
        """Centred Gaussian position prior (priors.py:27-35) from the per-molecule Philox streams."""
        x0 = torch.empty(self.N, 3, device=self.device)
        with self._dev():
            self._check(self.lib.fm_prior_philox(self._ctx, self._stream(), C.c_uint64(seed), _ptr(x0)), 'fm_prior_philox')
        return x0

    def prior_philox_dense(self, seed: int, prior_types: Optional[Dict[str, str]] = None, prior_kwargs: Optional[Dict[str, dict]] = None,
                           default_p: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The whole prior of an endpoint-parameterised model for the bound batch from the per-molecule Philox streams, in one launch
        (fm_prior_philox_dense): a dense state dict x_t (N,3) = ``prior_philox(seed)``'s bits, a_t (N,na), c_t (N,nc), e_t (U,ne) per unordered pair.
        ``prior_types`` / ``prior_kwargs`` (default: the model's config) name the reference's prior functions and their keyword arguments
        (priors.py:8-107); 'marginal' / 'c-given-a' take ``p`` / ``p_c_given_a`` from the kwargs or, when absent, from ``default_p`` (keys 'a', 'c', 'e')."""
        cfg, d = self.cfg, self.device
        types = prior_types if prior_types is not None else cfg.prior_types
        kws = prior_kwargs if prior_kwargs is not None else cfg.prior_kwargs
        spec, keep = fm_prior_spec(), []
        for i, (tag, width) in enumerate((('a', cfg.n_atom_types), ('c', cfg.n_charges), ('e', cfg.n_bond_types))):
            kind, kw, m = types[tag], kws.get(tag, {}) or {}, spec.mod[i]
            if kind not in _lib.FM_PRIOR_KINDS:
                raise NotImplementedError(f'prior type {kind!r}')
            m.kind = _lib.FM_PRIOR_KINDS[kind]
            m.std = float(kw.get('std', 0.2 if kind == 'biased-simplex' else 1.0))
            m.simplex_center = int(bool(kw.get('simplex_center', False)))
            m.has_blur = int(kw.get('blur') is not None)
            m.blur = float(kw.get('blur') or 0.0)
            m.vertex_prob, m.vertex_idx = float(kw.get('vertex_prob', 0.75)), int(kw.get('vertex_idx', 0))
            if kind in ('marginal', 'c-given-a'):
                key = 'p' if kind == 'marginal' else 'p_c_given_a'
                p = kw.get(key, (default_p or {}).get(tag))
                if p is None:
                    raise ValueError(f"prior {kind!r} needs kwargs[{key!r}] (or a dataset whose shipped marginals have {width} categories)")
                p = torch.as_tensor(p, dtype=torch.float32).to(d).contiguous()          # uploaded once per call
                want = (width,) if kind == 'marginal' else (cfg.n_atom_types, width)
                if tuple(p.shape) != want:
                    raise ValueError(f"prior {kind!r}: distribution has shape {tuple(p.shape)}, the model needs {want}")
                keep.append(p)
                m.p = _ptr(p)
        st = {'x_t': torch.empty(self.N, 3, device=d), 'a_t': torch.empty(self.N, cfg.n_atom_types, device=d),
              'c_t': torch.empty(self.N, cfg.n_charges, device=d), 'e_t': torch.empty(self.U, cfg.n_bond_types, device=d)}
        ds = self._dense_struct(st)
        with self._dev():
            self._check(self.lib.fm_prior_philox_dense(self._ctx, self._stream(), C.c_uint64(seed), C.byref(spec), C.byref(ds)), 'fm_prior_philox_dense')
        self._keep = [keep, st]
        return st

    def philox_tape(self, plan: "StepPlan", step: int) -> "StepNoise":
        """The draws the in-kernel noise mode consumes in step ``step`` of a Philox ``plan`` for the bound batch (and its molecule ids), as the tensors
        the reference draws (fm_philox_tape): campbell q_* (rows,K), u1_*, u2_* (u2 absent on the last step, as in ``StepNoise.draw``); gat q_* (rows,K+1).
        Fed back through the tensor-noise path -- or to the reference's integrate in place of its RNG -- it replays the Philox run."""
        sc = plan.scalars[step]
        if sc.noise_mode != FM_NOISE_PHILOX:
            raise ValueError('philox_tape needs a plan made with philox_seed')
        cfg = self.cfg
        layout = noise_layout(bool(sc.last_step), 'gat' if sc.dfm_type == FM_DFM_GAT else 'campbell', self.N, self.U, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types)
        nz = StepNoise(**{f: torch.empty(*((rows,) if width is None else (rows, width)), device=self.device) for f, rows, width in layout})
        cs = nz.c_struct()
        with self._dev():
            self._check(self.lib.fm_philox_tape(self._ctx, self._stream(), C.byref(sc), C.byref(cs)), 'fm_philox_tape')
        return nz

    def _check_ot_sizes(self, what: str):
        """ValueError when a bound molecule is above the cap of fm_ot_align (host-side sizes; nothing is enqueued)."""
        if self.n_atoms is None:          # no batch bound: the library's refusal
            return
        big = (self.n_atoms > _lib.FM_OT_MAX_ATOMS).nonzero().reshape(-1)
        if big.numel():
            m = int(big[0])
            raise ValueError(f"{what}: molecule {m} has {int(self.n_atoms[m])} atoms, the OT coupling takes at most {_lib.FM_OT_MAX_ATOMS}")

    def ot_align(self, x0: torch.Tensor, x1c: torch.Tensor, reflect: bool = True, perm: bool = False):
        """The equivariant-OT coupling of a position prior ``x0`` to the centred given positions ``x1c`` ((N,3) each, the bound batch's atoms, both used as
        given), molecule by molecule on the device (fm_ot_align; the reference's ``align_prior(x_0, x_1, permutation=True, rigid_body=True)``,
        priors.py:109-169): the optimal assignment of prior rows to atoms under the float32 distance, then the rigid fit of the permuted prior onto
        ``x1c``.  ``reflect`` (default: the reference's behaviour) lets the fit be improper, False takes the optimal proper rotation.  Returns
        (x0_aligned (N,3), out (B,4) = {n, assignment cost, rmsd after the permutation only, rmsd after the fit}) and, with ``perm``, the (N,) int32 local
        index of the prior row each atom received.  ValueError, before the call, for a molecule above 256 atoms.  Does not synchronise."""
        d = self.device
        x0, x1c = (v.detach().to(d, torch.float32).contiguous() for v in (x0, x1c))
        if tuple(x0.shape) != (self.N, 3) or tuple(x1c.shape) != (self.N, 3):
            raise ValueError(f'x0 and x1c must be ({self.N}, 3): the atoms of the bound batch')
        self._check_ot_sizes('ot_align')
        moved, out = torch.empty(self.N, 3, device=d), torch.empty(self.B, 4, device=d)
        pm = torch.empty(self.N, dtype=torch.int32, device=d) if perm else None
        with self._dev():
            rc = self.lib.fm_ot_align(self._ctx, self._stream(), _ptr(x0), _ptr(x1c), int(bool(reflect)), _ptr(moved), _ptr(pm), _ptr(out))
        self._check(rc, 'fm_ot_align')
        self._keep = [x0, x1c, moved, pm, out]
        return (moved, out, pm) if perm else (moved, out)

    def conditional_path(self, x1_state, alphas, mol_group=None, seed: int = None, tape: bool = False, coupling: str = 'independent', reflect: bool = True):
        """g_t ~ p(g_t | g_0, g_1) for the bound batch's molecules ``x1_state`` (a token state dict, real categories only; left untouched), the
        reference's CTMCVectorField.sample_conditional_path (ctmc_vector_field.py:97-143) in one launch (fm_conditional_path) with x_0 and the uniforms
        from the per-molecule Philox streams of ``seed``.  ``alphas``: (G, 4) -- or (4,) for one group -- rows of ``alpha_tables(t)[0]``, alpha_t of
        x, a, c, e at each time group's t; ``mol_group`` (B,): every molecule's group (None with one group).  Returns the new state dict; with
        ``tape`` also {'x0', 'u_a', 'u_c', 'u_e'}: the draws the call consumed.

        ``coupling``: 'independent' pairs every molecule with its own Gaussian draw; 'ot' with the draw after the reference's equivariant-OT alignment
        (``ot_align`` with ``reflect``; what a checkpoint trained with ``prior_config.x.align: True`` saw): fm_prior_philox, fm_ot_align and
        fm_conditional_path_x0 back to back on the device.  The tape's 'x0' is then the coupled prior, and the tape also holds 'x0_raw' (the draws before the
        coupling) and 'perm'.  Tokens and uniforms do not depend on ``coupling``."""
        if seed is None:
            raise ValueError('conditional_path draws from the Philox streams: seed is required')
        if coupling not in ('independent', 'ot'):
            raise ValueError(f"coupling must be 'independent' or 'ot', got {coupling!r}")
        if coupling == 'ot':
            self._check_ot_sizes('conditional_path')
        d = self.device
        al = torch.as_tensor(alphas).detach().to('cpu', torch.float32).reshape(-1, 4).contiguous()
        G = int(al.shape[0])
        group = None
        if mol_group is not None:
            group = torch.as_tensor(mol_group).detach().to('cpu', torch.int32).reshape(-1)
            if group.shape[0] != self.B or int(group.min()) < 0 or int(group.max()) >= G:
                raise ValueError(f'mol_group must hold one group index in [0, {G}) per bound molecule')
            group = group.to(d)
        elif G != 1:
            raise ValueError(f'{G} rows of alphas need mol_group')
        al = al.to(d)
        i32 = dict(dtype=torch.int32, device=d)
        out = {'x_t': torch.empty(self.N, 3, device=d), 'a_t': torch.empty(self.N, **i32), 'c_t': torch.empty(self.N, **i32), 'e_t': torch.empty(self.U, **i32)}
        tp = cs = None
        if tape:
            tp = {'x0': torch.empty(self.N, 3, device=d), 'u_a': torch.empty(self.N, device=d), 'u_c': torch.empty(self.N, device=d), 'u_e': torch.empty(self.U, device=d)}
            cs = _lib.fm_cond_tape()
            cs.x0, cs.u_a, cs.u_c, cs.u_e = _ptr(tp['x0']), _ptr(tp['u_a']), _ptr(tp['u_c']), _ptr(tp['u_e'])
        s1, so = self._state_struct(x1_state), self._state_struct(out)
        if coupling == 'ot':
            x0_raw = self.prior_philox(seed)
            x1c = self.remove_com(x1_state['x_t'].detach().to(d, torch.float32).contiguous().clone())
            x0, _, pm = self.ot_align(x0_raw, x1c, reflect=reflect, perm=True)
            with self._dev():
                rc = self.lib.fm_conditional_path_x0(self._ctx, self._stream(), C.c_uint64(seed), C.byref(s1), G, _ptr(group), _ptr(al), C.byref(so),
                                                     C.byref(cs) if cs is not None else None, _ptr(x0))
            self._check(rc, 'fm_conditional_path_x0')
            if tape:
                tp.update(x0_raw=x0_raw, perm=pm)
            self._keep = [x1_state, al, group, out, tp, x0_raw, x1c, x0, pm]
            return (out, tp) if tape else out
        with self._dev():
            rc = self.lib.fm_conditional_path(self._ctx, self._stream(), C.c_uint64(seed), C.byref(s1), G, _ptr(group), _ptr(al), C.byref(so),
                                              C.byref(cs) if cs is not None else None)
        self._check(rc, 'fm_conditional_path')
        self._keep = [x1_state, al, group, out, tp]
        return (out, tp) if tape else out

    def _time_groups(self, t):
        """``t`` (a number, or one value per bound molecule) as (distinct float32 values, device (B,) int32 group of every molecule or None for one group)."""
        if torch.is_tensor(t) and t.dim() > 0:
            tv = t.detach().to('cpu', torch.float32).reshape(-1)
            if tv.shape[0] != self.B:
                raise ValueError(f't has {tv.shape[0]} entries, the bound batch {self.B} molecules')
            vals, group = torch.unique(tv, return_inverse=True)
            return vals, group.to(torch.int32).to(self.device)
        return torch.tensor([_f32(t)], dtype=torch.float32), None

    def denoising_loss(self, xt_state, x1_state, t, rows=None):
        """The denoising-loss terms of the bound batch (fm_denoising_loss; the reference's FlowMol.forward after its sample_conditional_path call,
        flowmol.py:339-413): one evaluation on ``xt_state`` at ``t`` -- a number or a (B,) tensor with at most 32 distinct values -- with the heads' loss
        epilogue (CrossEntropyLoss on logits, vector_field.py:217), then one reduction.  ``x1_state`` holds the targets: real-category tokens and the
        centred positions.  Returns {'mol': (B,8) = se_x, 3 n_atoms, nll_a, cnt_a, nll_c, cnt_c, nll_e, cnt_e per molecule, 'rows': {'x', 'a', 'c' (N),
        'e' (U)}}: squared errors and nll per row, +0.0 on the rows the reference ignores (token of x_t not the mask token).  It never bootstraps.
        ``rows`` (testing the reduction alone): the caller's row terms, four float32 tensors; no evaluation runs, ``t`` is not read and the tokens of
        ``xt_state`` only say which rows count."""
        d = self.device
        if rows is None:
            vals, group = self._time_groups(t)
            temb = torch.stack([time_embedding_host(float(v), self.cfg.time_embedding_dim) for v in vals]).to(d).contiguous()
            rows = {'x': torch.empty(self.N, device=d), 'a': torch.empty(self.N, device=d), 'c': torch.empty(self.N, device=d), 'e': torch.empty(self.U, device=d)}
        else:
            vals, group, temb = [0.0], None, None
            rows = {k: rows[k].detach().to(d, torch.float32).contiguous() for k in 'xace'}
            if [int(rows[k].numel()) for k in 'xace'] != [self.N, self.N, self.N, self.U]:
                raise ValueError('rows must hold N, N, N and U terms')
        mol = torch.empty(self.B, 8, device=d)
        rs = _lib.fm_loss_rows()
        no_pairs = torch.empty(1, device=d) if self.U == 0 else None      # a batch of single atoms: a valid address that is never dereferenced
        rs.x, rs.a, rs.c, rs.e = _ptr(rows['x']), _ptr(rows['a']), _ptr(rows['c']), _ptr(rows['e'] if no_pairs is None else no_pairs)
        st, s1 = self._state_struct(xt_state), self._state_struct(x1_state)
        with self._dev():
            rc = self.lib.fm_denoising_loss(self._ctx, self._stream(), C.byref(st), C.byref(s1), _ptr(temb), len(vals), _ptr(group), C.byref(rs), _ptr(mol))
        self._check(rc, 'fm_denoising_loss')
        self._keep = [xt_state, x1_state, temb, group, rows, mol, no_pairs]
        return {'mol': mol, 'rows': rows}

    def distort(self, x: torch.Tensor, p: float, on, seed: int = None, tape: bool = False):
        """The geometry distortion of the reference's FlowMol.forward (flowmol.py:333-337; fm_distort_philox) in place on ``x`` (N,3): every atom of a
        molecule with ``on`` set -- a bool, or one per bound molecule: the caller's t > distort_t -- gets x += (z * [u < p]) * 0.5 with z, u from the
        per-molecule Philox streams of ``seed``.  Returns x; with ``tape`` also {'z' (N,3), 'u' (N)}: the draws of every atom, switched on or not."""
        if seed is None:
            raise ValueError('distort draws from the Philox streams: seed is required')
        d = self.device
        assert x.is_contiguous() and x.dtype == torch.float32 and tuple(x.shape) == (self.N, 3) and x.device == d
        flags = torch.as_tensor(on).detach().to('cpu').reshape(-1).to(torch.int32)
        if flags.shape[0] == 1:
            group, flags = None, flags.to(d)
        elif flags.shape[0] == self.B:
            group, flags = flags.to(d), torch.tensor([0, 1], dtype=torch.int32, device=d)      # two groups: off, on
        else:
            raise ValueError(f'on must be one flag or one per bound molecule ({self.B})')
        tp = ts = None
        if tape:
            tp = {'z': torch.empty(self.N, 3, device=d), 'u': torch.empty(self.N, device=d)}
            ts = _lib.fm_distort_tape()
            ts.z, ts.u = _ptr(tp['z']), _ptr(tp['u'])
        with self._dev():
            rc = self.lib.fm_distort_philox(self._ctx, self._stream(), C.c_uint64(seed), C.c_float(p), int(flags.shape[0]), _ptr(group), _ptr(flags), _ptr(x),
                                            C.byref(ts) if ts is not None else None)
        self._check(rc, 'fm_distort_philox')
        self._keep = [x, group, flags, tp]
        return (x, tp) if tape else x

    def stability(self, state, table: torch.Tensor, fake_atom_token: int = -1, explicit_aromaticity: bool = False) -> torch.Tensor:
        """Valence stability + connectivity of the bound batch's molecules from their tokens, on the device
        (see fm_stability).  table: (n_types, n_charges) int32 bit masks.  Returns (B,4) int32:
        stable atoms, real atoms, connected components, largest component."""
        tab = table.detach().to(self.device, torch.int32).contiguous()
        assert tab.dim() == 2 and tab.shape[1] == self.cfg.n_charges
        out = torch.empty(self.B, 4, dtype=torch.int32, device=self.device)
        st = self._state_struct(state)
        with self._dev():
            self._check(self.lib.fm_stability(self._ctx, self._stream(), C.byref(st), _ptr(tab), int(tab.shape[0]),
                                              int(fake_atom_token), int(bool(explicit_aromaticity)), _ptr(out)), 'fm_stability')
        return out

    # ------------------------------------------------------------------ hot path
    def forward(self, state, t, prev=None, bootstrap=False, remove_com=True, out=None, taps: Optional[Dict[str, torch.Tensor]] = None):
        """One network evaluation -> dst dict of probabilities (EndpointVectorField.forward with
        apply_softmax=True).  ``t``: a number, or the reference's per-graph time, a (B,) tensor (vector_field.py:212: molecules with equal t share
        an embedding table, fm_forward_mixed; at most 32 distinct values).  A molecule's result is the same bits either way."""
        out = out if out is not None else self.new_dst()
        mixed = torch.is_tensor(t) and t.dim() > 0
        if mixed:
            tv = t.detach().to('cpu', torch.float32).reshape(-1)
            if tv.shape[0] != self.B:
                raise ValueError(f't has {tv.shape[0]} entries, the bound batch {self.B} molecules')
            vals, group = torch.unique(tv, return_inverse=True)
            temb = torch.stack([time_embedding_host(float(v), self.cfg.time_embedding_dim) for v in vals]).to(self.device).contiguous()
            group = group.to(torch.int32).to(self.device)
        else:
            temb = time_embedding_host(float(t), self.cfg.time_embedding_dim).to(self.device)
        st = self._state_struct(state)
        o = self._dst_struct(out)
        p = self._dst_struct(prev) if prev is not None else None
        with self._taps(taps), self._dev():
            if mixed:
                rc = self.lib.fm_forward_mixed(self._ctx, self._stream(), C.byref(st), _ptr(temb), int(vals.shape[0]), _ptr(group),
                                               C.byref(p) if p is not None else None, int(bool(bootstrap)), int(bool(remove_com)), C.byref(o))
            else:
                rc = self.lib.fm_forward(self._ctx, self._stream(), C.byref(st), _ptr(temb), C.byref(p) if p is not None else None,
                                         int(bool(bootstrap)), int(bool(remove_com)), C.byref(o))
            self._check(rc, 'fm_forward_mixed' if mixed else 'fm_forward')
        self._keep = [temb, state, out, prev, group if mixed else None]
        return out

    # ------------------------------------------------------------------ endpoint parameterization (EndpointVectorField)
    def make_dense_state(self, x_t, a_t, c_t, e_t) -> Dict[str, torch.Tensor]:
        """x_t (N,3), a_t (N,na), c_t (N,nc), e_t (U,ne): continuous features of an endpoint-parameterised model (copies)."""
        d = self.device
        st = {k: v.detach().to(d, torch.float32).contiguous().clone() for k, v in (('x_t', x_t), ('a_t', a_t), ('c_t', c_t), ('e_t', e_t))}
        assert st['x_t'].shape == (self.N, 3) and st['a_t'].shape == (self.N, self.cfg.n_atom_types)
        assert st['c_t'].shape == (self.N, self.cfg.n_charges) and st['e_t'].shape == (self.U, self.cfg.n_bond_types)
        return st

    def forward_dense(self, state, t: float, remove_com=True, out=None, taps: Optional[Dict[str, torch.Tensor]] = None):
        """EndpointVectorField.forward on continuous categorical features (vector_field.py:212-293, no self-conditioning)."""
        out = out if out is not None else self.new_dst()
        temb = time_embedding_host(float(t), self.cfg.time_embedding_dim).to(self.device)
        st, o = self._dense_struct(state), self._dst_struct(out)
        with self._taps(taps), self._dev():
            self._check(self.lib.fm_forward_dense(self._ctx, self._stream(), C.byref(st), _ptr(temb), int(bool(remove_com)), C.byref(o)), 'fm_forward_dense')
        self._keep = [temb, state, out]
        return out

    def endpoint_step(self, state, dst, dt: float, coef, scale: float = 1.0):
        """x_s = x_t + ((coef (x_1 - x_t)) scale) dt for x, a, c, e in place (EndpointVectorField.step, vector_field.py:528-543)."""
        sc = fm_endpoint_scalars()
        sc.dt, sc.scale = float(dt), float(scale)
        for k in range(4):
            sc.coef[k] = float(coef[k])
        st, d = self._dense_struct(state), self._dst_struct(dst)
        with self._dev():
            rc = self.lib.fm_endpoint_step(self._ctx, self._stream(), C.byref(st), C.byref(d), C.byref(sc))
        self._check(rc, 'fm_endpoint_step')
        return state

    def integrate_endpoint(self, state, n_timesteps: int, inv_temp_func=None, tspan=None, traj: Optional[Dict[str, torch.Tensor]] = None):
        """EndpointVectorField.integrate (vector_field.py:388-499): Euler steps of all four modalities; the per-step scalars are computed
        with the reference's float32 tensor arithmetic on the host, the steps are enqueued back to back (no host synchronisation).
        ``traj`` (optional, vector_field.py:412-466 `visualize`): preallocated per-step frames -- 'x' (steps,N,3) and the argmax categories
        'a','c' (steps,N), 'e' (steps,U) of the state after each step, 'x1','a1','c1','e1' of the step's endpoint prediction."""
        cfg = self.cfg
        t, steps = euler_steps(n_timesteps, tspan, cfg.schedule_type, cfg.cosine_params)
        if inv_temp_func is None:
            if cfg.continuous_inv_temp_schedule == 'linear':
                mx = cfg.continuous_inv_temp_max
                inv_temp_func = lambda tt: mx * (1 - tt)                     # vector_field.py:203-204
            else:
                inv_temp_func = lambda tt: 1.0
        dst = [self.new_dst(), self.new_dst()]
        for s_idx, (t_i, dt, a_i, ap_i) in enumerate(steps, 1):
            out = dst[s_idx & 1]
            self.forward_dense(state, float(t_i), remove_com=True, out=out)
            self.endpoint_step(state, out, float(dt), [float(ap_i[k] / (1 - a_i[k])) for k in range(4)], _f32(inv_temp_func(t_i)))
            if traj is not None:
                f = s_idx - 1
                traj['x'][f].copy_(state['x_t']); traj['x1'][f].copy_(out['x'])
                for k in 'ace':
                    traj[k][f].copy_(state[f'{k}_t'].argmax(-1)); traj[f'{k}1'][f].copy_(out[k].argmax(-1))
        self.synchronize()
        return dst[(t.shape[0] - 1) & 1] if t.shape[0] > 1 else None

    def ctmc_step(self, state, dst, noise: StepNoise, sc: fm_step_scalars, sampled: Optional[Dict[str, torch.Tensor]] = None):
        st = self._state_struct(state)
        d = self._dst_struct(dst)
        nz = noise.c_struct()
        smp = fm_sampled()
        if sampled is not None:
            smp.a1, smp.c1, smp.e1 = _ptr(sampled['a1']), _ptr(sampled['c1']), _ptr(sampled['e1'])
        with self._dev():
            rc = self.lib.fm_ctmc_step(self._ctx, self._stream(), C.byref(st), C.byref(d), C.byref(nz), C.byref(sc), C.byref(smp))
        self._check(rc, 'fm_ctmc_step')
        self._keep = [state, dst, noise, sampled]
        return state

    def integrate(self, state, plan: StepPlan, noise_for_step, chunk: int = 32, traj: Optional[Dict[str, torch.Tensor]] = None):
        """Run all steps of ``plan`` (CTMCVectorField.integrate).  ``noise_for_step(i, last)`` returns the
        StepNoise of step i; noise is produced ``chunk`` steps ahead and each chunk is one fm_integrate
        call (no host synchronisation in between).  Returns the final endpoint prediction dict."""
        run = IntegrationRun(self, state, plan, noise_for_step, traj=traj)
        run.run(0, len(plan.scalars), chunk=chunk)
        self.synchronize()
        return run.last_dst()

    def integrate_mixed(self, state, plans: Sequence[StepPlan], mol_group, start: Optional[Sequence[int]] = None, n_steps: Optional[int] = None,
                        prev=None):
        """Advance a batch whose molecules follow different schedules (fm_integrate_mixed).  ``plans``: one Philox campbell ``StepPlan`` of the
        unchanged ``make_step_plan`` per group (at most 32); ``mol_group`` (B,): the group of every molecule; ``start[g]``: the step of its plan group
        ``g`` takes first (default 0; > 0 continues a trajectory and needs ``prev``, the endpoint dict the previous call returned).  Runs ``n_steps``
        call-steps (default: until the longest group has finished); a group that runs out of steps waits inactive, its molecules' state untouched.
        Returns the final endpoint prediction dict (None when nothing ran) and synchronises, like ``integrate``."""
        G = len(plans)
        start = [0] * G if start is None else [int(v) for v in start]
        left = [len(pl.scalars) - s0 for pl, s0 in zip(plans, start)]
        if len(start) != G or min(left, default=0) < 0:
            raise ValueError('start must give one step index inside its plan per group')
        n = max(left, default=0) if n_steps is None else int(n_steps)
        group = torch.as_tensor(mol_group).detach().to('cpu', torch.int32).reshape(-1)
        if group.shape[0] != self.B or (G and (int(group.min()) < 0 or int(group.max()) >= G)):
            raise ValueError(f'mol_group must hold one group index in [0, {G}) per bound molecule')
        if n <= 0:
            return None
        scal, act, temb = mixed_step_arrays(plans, start, n, self.cfg.time_embedding_dim)
        d = self.device
        scal_dev = torch.frombuffer(bytearray(bytes(scal)), dtype=torch.uint8).to(d)
        act_dev = torch.tensor(list(act), dtype=torch.int32).to(d)
        temb, group = temb.to(d).contiguous(), group.to(d)
        dst = [self.new_dst(), self.new_dst()]
        ds = [self._dst_struct(dst[0]), self._dst_struct(dst[1])]
        st = self._state_struct(state)
        p = self._dst_struct(prev) if prev is not None else None
        final = C.c_int(0)
        with self._dev():
            rc = self.lib.fm_integrate_mixed(self._ctx, self._stream(), C.byref(st), n, G, scal, _ptr(scal_dev), act, _ptr(act_dev), _ptr(group), _ptr(temb),
                                             C.byref(p) if p is not None else None, C.byref(ds[0]), C.byref(ds[1]), None, C.byref(final))
        self._check(rc, 'fm_integrate_mixed')
        self.synchronize()
        self._keep = [state, prev, dst]
        return dst[final.value]

    # ------------------------------------------------------------------ frozen atoms (replacement conditioning)
    def inpaint_spec(self, x1_state, keep, seed: int, coupling: str = 'independent') -> Dict[str, torch.Tensor]:
        """The tensors of an ``fm_inpaint`` struct for the bound batch (and its molecule ids): ``keep`` (N,) marks the atoms of the given molecules
        ``x1_state`` that stay as given.  'x0' and 'u_a' / 'u_c' / 'u_e' are the tape of ``conditional_path(x1_state, ..., seed, tape=True)`` (they do not
        depend on alpha), 'x1c' the given positions after ``remove_com``, 'a1' / 'c1' / 'e1' copies of the given tokens, 'keep_pair' (U,) scratch that
        every call fills.  ``x1_state`` is left untouched.  ``coupling`` as in ``conditional_path``: with 'ot' the frozen positions follow the coupled path."""
        d = self.device
        k = torch.as_tensor(keep).detach().reshape(-1)
        if k.shape[0] != self.N:
            raise ValueError(f'keep has {k.shape[0]} entries, the bound batch {self.N} atoms')
        _, tape = self.conditional_path(x1_state, [1.0, 1.0, 1.0, 1.0], seed=seed, tape=True, coupling=coupling)
        return {'keep_atom': (k != 0).to(torch.uint8).to(d).contiguous(), 'keep_pair': torch.zeros(self.U, dtype=torch.uint8, device=d),
                'x0': tape['x0'], 'x1c': self.remove_com(x1_state['x_t'].detach().to(d, torch.float32).contiguous().clone()),
                'a1': x1_state['a_t'].detach().to(d, torch.int32).contiguous().clone(), 'c1': x1_state['c_t'].detach().to(d, torch.int32).contiguous().clone(),
                'e1': x1_state['e_t'].detach().to(d, torch.int32).contiguous().clone(), 'u_a': tape['u_a'], 'u_c': tape['u_c'], 'u_e': tape['u_e']}

    @staticmethod
    def _inpaint_struct(spec) -> "_lib.fm_inpaint":
        s = _lib.fm_inpaint()
        for name, _ in _lib.fm_inpaint._fields_:
            setattr(s, name, _ptr(spec[name]) if spec[name].numel() else None)      # a batch without pairs: empty pair tensors travel as NULL
        return s

    def freeze_spec(self, x1_state, keep: Dict[str, torch.Tensor], seed: int, coupling: str = 'independent') -> Dict[str, Optional[torch.Tensor]]:
        """The tensors of an ``fm_freeze`` struct for the bound batch (and its molecule ids): frozen rows per modality.  ``keep``: a dict with any of the
        keys 'x', 'a', 'c' ((N,) bool: positions, atom types, charges) and 'e' ((U,) bool, the pair order of ``e_t``); a missing key -- or None -- leaves
        that modality free: its keep array and its path inputs stay None and travel as NULL.  The other members are those of ``inpaint_spec``, of which
        this is the general form: 'x': k, 'a': k, 'c': k, 'e': both atoms in k gives the bits of ``inpaint_spec(x1_state, k, seed)``.  ``coupling`` as in
        ``conditional_path``: it changes 'x0' alone, so it matters only with an 'x' part."""
        unknown = set(keep) - set('xace')
        if unknown:
            raise ValueError(f"keep has unknown keys {sorted(unknown)}: 'x', 'a', 'c' (atoms) and 'e' (pairs) are the modalities")
        d, flags = self.device, {}
        for f in 'xace':
            k = keep.get(f)
            if k is None:
                continue
            k = torch.as_tensor(k).detach().reshape(-1)
            rows = self.U if f == 'e' else self.N
            if k.shape[0] != rows:
                raise ValueError(f"keep['{f}'] has {k.shape[0]} entries, the bound batch {rows} {'pairs' if f == 'e' else 'atoms'}")
            flags[f] = (k != 0).to(torch.uint8).to(d).contiguous()
        _, tape = self.conditional_path(x1_state, [1.0, 1.0, 1.0, 1.0], seed=seed, tape=True, coupling=coupling)
        spec = {name: None for name, _ in _lib.fm_freeze._fields_}
        if 'x' in flags:
            spec.update(keep_x=flags['x'], x0=tape['x0'], x1c=self.remove_com(x1_state['x_t'].detach().to(d, torch.float32).contiguous().clone()))
        for f in 'ace':
            if f in flags:
                spec.update({f'keep_{f}': flags[f], f'{f}1': x1_state[f'{f}_t'].detach().to(d, torch.int32).contiguous().clone(), f'u_{f}': tape[f'u_{f}']})
        return spec

    @staticmethod
    def _freeze_struct(spec) -> "_lib.fm_freeze":
        s = _lib.fm_freeze()
        for name, _ in _lib.fm_freeze._fields_:
            setattr(s, name, _ptr(spec[name]) if spec[name] is not None and spec[name].numel() else None)
        return s

    def _keep_struct(self, spec):
        """(the C struct, the entry points' suffix) of either kind of spec: ``inpaint_spec`` (fm_*_inpaint) or ``freeze_spec`` (fm_*_freeze)."""
        return (self._inpaint_struct(spec), 'inpaint') if 'keep_atom' in spec else (self._freeze_struct(spec), 'freeze')

    def ctmc_step_inpaint(self, state, dst, noise: Optional[StepNoise], sc: fm_step_scalars, spec, alpha_next, sampled: Optional[Dict[str, torch.Tensor]] = None):
        """``ctmc_step`` with the frozen rows of ``spec`` (``inpaint_spec``) put back onto the given molecule's conditional path at ``alpha_next``
        (4 values: alpha_t of x, a, c, e at the time the step arrives at) inside the step kernel (fm_ctmc_step_inpaint)."""
        (ip, kind), st, d = self._keep_struct(spec), self._state_struct(state), self._dst_struct(dst)
        nz = noise.c_struct() if noise is not None else None
        smp = fm_sampled()
        if sampled is not None:
            smp.a1, smp.c1, smp.e1 = _ptr(sampled['a1']), _ptr(sampled['c1']), _ptr(sampled['e1'])
        al = (C.c_float * 4)(*[float(v) for v in torch.as_tensor(alpha_next, dtype=torch.float32).reshape(-1).tolist()])
        with self._dev():
            rc = getattr(self.lib, f'fm_ctmc_step_{kind}')(self._ctx, self._stream(), C.byref(st), C.byref(d), C.byref(nz) if nz is not None else None, C.byref(sc),
                                                           C.byref(smp), C.byref(ip), al)
        self._check(rc, f'fm_ctmc_step_{kind}')
        self._keep = [state, dst, noise, sampled, spec]
        return state

    def ctmc_step_freeze(self, state, dst, noise: Optional[StepNoise], sc: fm_step_scalars, spec, alpha_next, sampled: Optional[Dict[str, torch.Tensor]] = None):
        """``ctmc_step`` with the rows ``spec`` (``freeze_spec``) flags, modality by modality, put back onto the given molecule's conditional path at
        ``alpha_next`` inside the step kernel (fm_ctmc_step_freeze)."""
        if 'keep_atom' in spec:
            raise ValueError('ctmc_step_freeze takes the spec of freeze_spec')
        return self.ctmc_step_inpaint(state, dst, noise, sc, spec, alpha_next, sampled)

    def plan_alphas(self, plan: StepPlan) -> torch.Tensor:
        """alpha_t (T, 4: x, a, c, e) at the time points of ``plan``: row i + 1 is the ``alpha_next`` of its step i."""
        return alpha_tables(plan.t.clone(), self.cfg.schedule_type, self.cfg.cosine_params)[0]

    def integrate_inpaint(self, state, plans: Sequence[StepPlan], mol_group, spec, start: Optional[Sequence[int]] = None, n_steps: Optional[int] = None,
                          prev=None):
        """``integrate_mixed`` with the frozen rows of ``spec`` (``inpaint_spec``): after every step the kept atoms -- and the pairs between two kept
        atoms -- of every active molecule sit on the given molecule's conditional path at the step's new time point (fm_integrate_inpaint).  Arguments
        and return value as in ``integrate_mixed``; one plan (``mol_group`` may then be None) runs the single-schedule step kernels, so gat plans pass."""
        G = len(plans)
        start = [0] * G if start is None else [int(v) for v in start]
        left = [len(pl.scalars) - s0 for pl, s0 in zip(plans, start)]
        if len(start) != G or min(left, default=0) < 0:
            raise ValueError('start must give one step index inside its plan per group')
        n = max(left, default=0) if n_steps is None else int(n_steps)
        group = torch.zeros(self.B, dtype=torch.int32) if mol_group is None and G == 1 else torch.as_tensor(mol_group).detach().to('cpu', torch.int32).reshape(-1)
        if group.shape[0] != self.B or (G and (int(group.min()) < 0 or int(group.max()) >= G)):
            raise ValueError(f'mol_group must hold one group index in [0, {G}) per bound molecule')
        if n <= 0:
            return None
        scal, act, temb = mixed_step_arrays(plans, start, n, self.cfg.time_embedding_dim)
        tabs = [self.plan_alphas(pl) for pl in plans]
        al = torch.zeros(n, G, 4)
        for k in range(n):
            for g in range(G):
                if start[g] + k + 1 < tabs[g].shape[0]:
                    al[k, g] = tabs[g][start[g] + k + 1]
        al = al.contiguous()
        d = self.device
        scal_dev = torch.frombuffer(bytearray(bytes(scal)), dtype=torch.uint8).to(d)
        act_dev = torch.tensor(list(act), dtype=torch.int32).to(d)
        temb, group, al_dev = temb.to(d).contiguous(), group.to(d), al.to(d)
        dst = [self.new_dst(), self.new_dst()]
        ds = [self._dst_struct(dst[0]), self._dst_struct(dst[1])]
        (ip, kind), st = self._keep_struct(spec), self._state_struct(state)
        p = self._dst_struct(prev) if prev is not None else None
        final = C.c_int(0)
        with self._dev():
            rc = getattr(self.lib, f'fm_integrate_{kind}')(self._ctx, self._stream(), C.byref(st), n, G, scal, _ptr(scal_dev), act, _ptr(act_dev), _ptr(group), _ptr(temb),
                                                           None, C.byref(p) if p is not None else None, C.byref(ds[0]), C.byref(ds[1]), None, C.byref(final), C.byref(ip),
                                                           C.cast(C.c_void_p(al.data_ptr()), C.POINTER(C.c_float)), _ptr(al_dev))
        self._check(rc, f'fm_integrate_{kind}')
        self.synchronize()
        self._keep = [state, prev, dst, spec]
        return dst[final.value]

    def integrate_freeze(self, state, plans: Sequence[StepPlan], mol_group, spec, start: Optional[Sequence[int]] = None, n_steps: Optional[int] = None, prev=None):
        """``integrate_inpaint`` with the per-modality frozen rows of ``spec`` (``freeze_spec``): fm_integrate_freeze, same arguments and return value."""
        if 'keep_atom' in spec:
            raise ValueError('integrate_freeze takes the spec of freeze_spec')
        return self.integrate_inpaint(state, plans, mol_group, spec, start=start, n_steps=n_steps, prev=prev)

    # ------------------------------------------------------------------ aligned RMSD
    def align_rmsd(self, xa: torch.Tensor, xb: torch.Tensor, select=None, aligned: bool = False):
        """RMSD of the coordinate sets ``xa`` and ``xb`` ((N,3) each, the bound batch's atoms) molecule by molecule, on the device (fm_align_rmsd): returns
        (B,4) float32 = {selected atoms, rmsd after centring both on the selected atoms, rmsd after the optimal proper rotation of xa onto xb, 0}.
        ``select`` ((N,) bool, None = all): the atoms the fit and the rmsd run over; a molecule without one gives zeros.  ``aligned``: also return (N,3),
        all atoms of ``xa`` moved by the transform fitted on the selected ones.  Does not synchronise."""
        d = self.device
        xa, xb = (v.detach().to(d, torch.float32).contiguous() for v in (xa, xb))
        if tuple(xa.shape) != (self.N, 3) or tuple(xb.shape) != (self.N, 3):
            raise ValueError(f'xa and xb must be ({self.N}, 3): the atoms of the bound batch')
        sel = None
        if select is not None:
            sel = torch.as_tensor(select).detach().reshape(-1)
            if sel.shape[0] != self.N:
                raise ValueError(f'select has {sel.shape[0]} entries, the bound batch {self.N} atoms')
            sel = (sel != 0).to(torch.uint8).to(d).contiguous()
        out = torch.empty(self.B, 4, device=d)
        moved = torch.empty(self.N, 3, device=d) if aligned else None
        with self._dev():
            rc = self.lib.fm_align_rmsd(self._ctx, self._stream(), _ptr(xa), _ptr(xb), _ptr(sel), _ptr(out), _ptr(moved))
        self._check(rc, 'fm_align_rmsd')
        self._keep = [xa, xb, sel, out, moved]
        return (out, moved) if aligned else out

    # ------------------------------------------------------------------ stereo check
    def stereo(self, x: torch.Tensor, x_ref: torch.Tensor, elem_sets, flat_tol: float = 0.05, values: bool = False, fixed: bool = False):
        """The stereo state of ``x`` against that of ``x_ref`` ((N,3) each, the bound batch's atoms) molecule by molecule, one launch on the device
        (fm_stereo).  ``elem_sets`` = (elem_set (B,) set id per molecule or -1 for none, [rows (Q_s, 5) per set]) or None: a row is ``[kind, i0, i1, i2, i3]``
        with local atom indices as ``stereo.stereo_elements`` gives them -- kind 0 a tetrahedral centre i0 with neighbours i1..i3, valued
        (u1 x u2) . u3 over the unit bond vectors; kind 1 a double bond i1 = i2, valued cos of the dihedral i0-i1-i2-i3.  An element is defined in a
        coordinate set when |value| >= ``flat_tol`` and mismatches when it is defined in both with different signs.  ``flat_tol`` = 0.05 is the
        DEFINITION of a flat element here (a centre within about 3 degrees of planar, a dihedral within 3 degrees of perpendicular), not a measured tolerance.
        Returns (B,8) int32 on the device = {kind-0 elements, defined in both, mismatches, kind-1 elements, defined in both, mismatches, match, mirror}
        (fm_stereo in include/flowmol_hip.h); with ``values`` also (the float32 values of ``x``, concatenated in row order, and their (B+1,) CPU
        offsets); with ``fixed`` also (N,3): ``-x`` for the molecules flagged mirror, ``x`` for the rest.  ValueError, before the call, for what the
        library cannot check: a set whose rows are not (Q,5), a kind outside {0, 1}, an index outside a molecule that names the set, an index repeated
        within a row.  A molecule's results do not depend on the rest of the batch.  Does not synchronise."""
        d = self.device
        x, x_ref = (v.detach().to(d, torch.float32).contiguous() for v in (x, x_ref))
        if tuple(x.shape) != (self.N, 3) or tuple(x_ref.shape) != (self.N, 3):
            raise ValueError(f'x and x_ref must be ({self.N}, 3): the atoms of the bound batch')
        tol = float(flat_tol)
        if not tol >= 0.0:
            raise ValueError(f'flat_tol = {flat_tol} must be a number >= 0')
        sizes = self.n_atoms
        table, n_sets, n_rows = (None, None, None), 0, torch.zeros(self.B, dtype=torch.int64)
        if elem_sets is not None:
            es, rows = elem_sets
            es = torch.as_tensor(es).detach().to('cpu', torch.int32).reshape(-1)
            rows = [torch.as_tensor(r).detach().to('cpu', torch.int64) for r in rows]
            if es.shape[0] != self.B or (self.B and (int(es.min()) < -1 or int(es.max()) >= len(rows))):
                raise ValueError(f'elem_set must hold one set id in -1 .. {len(rows) - 1} per bound molecule')
            for s, r in enumerate(rows):
                if r.dim() != 2 or r.shape[1] != 5:
                    raise ValueError(f'element set {s} must be a (rows, 5) tensor of [kind, i0, i1, i2, i3]')
                if not r.shape[0]:
                    continue
                if bool(((r[:, 0] != 0) & (r[:, 0] != 1)).any()):
                    raise ValueError(f'element set {s}: a kind outside {{0, 1}}')
                if bool((torch.sort(r[:, 1:], dim=1).values.diff(dim=1) == 0).any()):
                    raise ValueError(f'element set {s}: a row names an atom twice')
                mols = (es == s).nonzero().reshape(-1)
                if mols.numel() and (int(r[:, 1:].min()) < 0 or int(r[:, 1:].max()) >= int(sizes[mols].min())):
                    raise ValueError(f'element set {s}: an index outside 0 .. {int(sizes[mols].min()) - 1}, the atoms of the smallest molecule that names the set')
            per_set = torch.tensor([r.shape[0] for r in rows], dtype=torch.int64)
            if int(per_set.sum()):          # with no row at all there is no table, and an empty tensor has no pointer to pass
                n_sets = len(rows)
                set_off = torch.zeros(n_sets + 1, dtype=torch.int32)
                set_off[1:] = torch.cumsum(per_set, 0).to(torch.int32)
                table = (es.to(d).contiguous(), set_off.to(d), torch.cat([r.reshape(-1) for r in rows]).to(torch.int32).to(d).contiguous())
                n_rows = torch.where(es >= 0, per_set[es.long().clamp(min=0)], torch.zeros((), dtype=torch.int64))
        out = torch.empty(self.B, 8, dtype=torch.int32, device=d)
        val_off = torch.zeros(self.B + 1, dtype=torch.int64)
        val_off[1:] = torch.cumsum(n_rows, 0)
        vals = torch.empty(int(val_off[-1]), device=d) if values else None
        voff = val_off.to(torch.int32).to(d) if values and vals.numel() else None
        x_out = torch.empty(self.N, 3, device=d) if fixed else None
        with self._dev():
            rc = self.lib.fm_stereo(self._ctx, self._stream(), _ptr(x), _ptr(x_ref), _ptr(table[0]), _ptr(table[1]), _ptr(table[2]), n_sets, tol, _ptr(out),
                                    _ptr(voff), _ptr(vals) if voff is not None else None, _ptr(x_out))
        self._check(rc, 'fm_stereo')
        self._keep = [x, x_ref, table, out, voff, vals, x_out]
        res = (out,) + (((vals, val_off),) if values else ()) + ((x_out,) if fixed else ())
        return res if len(res) > 1 else out

    # ------------------------------------------------------------------ conformer ensembles: pairwise RMSD, pruning
    def pair_rmsd(self, x: torch.Tensor, pairs, select=None, perm_sets=None, best: bool = False):
        """Symmetry-aware aligned RMSD of pairs of molecules of the bound batch, one launch on the device (fm_pair_rmsd): ``x`` (N,3) the batch's atoms,
        ``pairs`` (P,2) molecule indices, each pair of equal size.  Returns (P,2) float32 on the device = {selected atoms, the smallest rmsd over the
        permutation rows after centring and the optimal proper rotation of a[i] onto b[row[i]]}; with ``best`` also (P,) int32, the lowest row index that
        attains it.  ``select`` ((N,) bool, None = all): the atoms the fit runs over, read at the first molecule of a pair -- both molecules of a pair
        must carry the same flags.  ``perm_sets`` = (perm_set (B,) set id per molecule or -1, [rows (P_s, n) per set]) or None for the identity only: the
        rows of a pair are those of its first molecule's set; a row must be a permutation of 0..n-1 that maps selected atoms onto selected atoms and is
        the identity on the rest.  ValueError, before the call, for anything else.  The two numbers of a pair do not depend on the rest of the batch, on
        the pair's place in ``pairs`` or on the order of the rows; the row index does depend on that order.  Does not synchronise."""
        d = self.device
        x = x.detach().to(d, torch.float32).contiguous()
        if tuple(x.shape) != (self.N, 3):
            raise ValueError(f'x must be ({self.N}, 3): the atoms of the bound batch')
        pr = torch.as_tensor(pairs).detach().to('cpu', torch.int32).reshape(-1, 2).contiguous()
        P = int(pr.shape[0])
        sizes = self.n_atoms
        off = torch.zeros(self.B + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(sizes, 0)
        if P and (int(pr.min()) < 0 or int(pr.max()) >= self.B):
            raise ValueError(f'pairs must name molecules 0 .. {self.B - 1} of the bound batch')
        pa, pb = pr[:, 0].long(), pr[:, 1].long()
        if P and not torch.equal(sizes[pa], sizes[pb]):
            k = int((sizes[pa] != sizes[pb]).nonzero()[0])
            raise ValueError(f'pair {k} = ({int(pa[k])}, {int(pb[k])}): the sizes of a pair differ, {int(sizes[pa[k]])} and {int(sizes[pb[k]])} atoms')
        sel_h = None
        if select is not None:
            sel_h = torch.as_tensor(select).detach().cpu().reshape(-1) != 0
            if sel_h.shape[0] != self.N:
                raise ValueError(f'select has {sel_h.shape[0]} entries, the bound batch {self.N} atoms')
            if P:
                n_p = sizes[pa]
                local = torch.arange(int(n_p.sum())) - torch.repeat_interleave(torch.cumsum(n_p, 0) - n_p, n_p)
                ia, ib = torch.repeat_interleave(off[pa], n_p) + local, torch.repeat_interleave(off[pb], n_p) + local
                if not torch.equal(sel_h[ia], sel_h[ib]):
                    raise ValueError('select must flag the same atoms in both molecules of a pair')
        table = (None, None, None)
        n_sets = 0
        if perm_sets is not None:
            ps, rows = perm_sets
            ps = torch.as_tensor(ps).detach().to('cpu', torch.int32).reshape(-1)
            rows = [torch.as_tensor(r).detach().to('cpu', torch.int64) for r in rows]
            n_sets = len(rows)
            if ps.shape[0] != self.B or (self.B and (int(ps.min()) < -1 or int(ps.max()) >= n_sets)):
                raise ValueError(f'perm_set must hold one set id in -1 .. {n_sets - 1} per bound molecule')
            for s, r in enumerate(rows):
                if r.dim() != 2 or r.shape[0] < 1:
                    raise ValueError(f'permutation set {s} must be a (rows, n) tensor with at least one row')
                n = int(r.shape[1])
                if not torch.equal(torch.sort(r, dim=1).values, torch.arange(n).expand_as(r)):
                    raise ValueError(f'permutation set {s}: a row is not a permutation of 0 .. {n - 1}')
                mols = (ps == s).nonzero().reshape(-1)
                if bool((sizes[mols] != n).any()):
                    m = int(mols[(sizes[mols] != n).nonzero()[0]])
                    raise ValueError(f'permutation set {s} has rows of {n} entries, molecule {m} has {int(sizes[m])} atoms')
                if sel_h is not None and mols.numel():
                    flags = torch.unique(sel_h[off[mols][:, None] + torch.arange(n)], dim=0)          # the distinct selections of the set's molecules
                    for sm in flags:
                        if not bool(sm[r][:, sm].all()) or not torch.equal(r[:, ~sm], torch.arange(n)[~sm].expand(r.shape[0], -1)):
                            raise ValueError(f'permutation set {s}: a row moves a selected atom onto an unselected one, or moves an unselected atom')
            if n_sets:
                set_off = torch.zeros(n_sets + 1, dtype=torch.int32)
                set_off[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0).to(torch.int32)
                table = (ps.to(d).contiguous(), set_off.to(d), torch.cat([r.reshape(-1) for r in rows]).to(torch.int32).to(d).contiguous())
        sel = None if sel_h is None else sel_h.to(torch.uint8).to(d).contiguous()
        pr_dev = pr.to(d)
        out = torch.empty(P, 2, device=d)
        best_perm = torch.empty(P, dtype=torch.int32, device=d) if best else None
        if P == 0:          # nothing to launch, and an empty tensor has no pointer to pass
            return (out, best_perm) if best else out
        with self._dev():
            rc = self.lib.fm_pair_rmsd(self._ctx, self._stream(), _ptr(x), P, _ptr(pr), _ptr(pr_dev), _ptr(sel), _ptr(table[0]),
                                       _ptr(table[1]), _ptr(table[2]), n_sets, _ptr(out), _ptr(best_perm))
        self._check(rc, 'fm_pair_rmsd')
        self._keep = [x, pr, pr_dev, sel, table, out, best_perm]
        return (out, best_perm) if best else out

    def prune_rmsd(self, d: torch.Tensor, group_sizes, threshold: float):
        """Greedy RMSD-threshold pruning of conformer groups on the device (fm_prune_rmsd): ``group_sizes`` the conformers per group, ``d`` the groups'
        strict upper triangles (row-major, i < j), concatenated -- the layout ``pair_rmsd`` gives for the pairs in that order.  In each group, for
        i = 0, 1, ...: the nearest KEPT j < i (ties: the lowest j) drops i when d(j, i) < ``threshold``.  Returns (keep (M,) bool, rep (M,) int64) on the
        device over the concatenated conformers: rep[i] = i for a kept conformer, else the index of the one it was dropped for.  A NaN drops nothing.
        Needs no bound batch; does not synchronise."""
        dev = self.device
        gs = torch.as_tensor(group_sizes).detach().to('cpu', torch.int64).reshape(-1)
        if gs.numel() and int(gs.min()) < 0:
            raise ValueError('group_sizes must not be negative')
        G, M = int(gs.numel()), int(gs.sum())
        tri = gs * (gs - 1) // 2
        if M >= 2 ** 31 or int(tri.sum()) >= 2 ** 31:
            raise ValueError('prune_rmsd: the conformers or the triangles exceed int32 offsets')
        dd = torch.as_tensor(d).detach().to(dev, torch.float32).reshape(-1).contiguous()
        if dd.numel() != int(tri.sum()):
            raise ValueError(f'd has {dd.numel()} values, the groups have {int(tri.sum())} pairs (K (K - 1) / 2 per group)')
        if M == 0:
            return torch.zeros(0, dtype=torch.bool, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
        group_off, tri_off = torch.zeros(G + 1, dtype=torch.int32), torch.zeros(G + 1, dtype=torch.int32)
        group_off[1:], tri_off[1:] = torch.cumsum(gs, 0).to(torch.int32), torch.cumsum(tri, 0).to(torch.int32)
        group_off, tri_off = group_off.to(dev), tri_off.to(dev)
        keep, rep = torch.empty(M, dtype=torch.uint8, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
        with self._dev():
            rc = self.lib.fm_prune_rmsd(self._ctx, self._stream(), G, _ptr(group_off), _ptr(dd) if dd.numel() else None, _ptr(tri_off), float(threshold),
                                        _ptr(keep), _ptr(rep))
        self._check(rc, 'fm_prune_rmsd')
        self._keep = [group_off, tri_off, dd, keep, rep]
        return keep != 0, rep.long()

    # ------------------------------------------------------------------ profiling
    def profile(self, on: bool):
        self._check(self.lib.fm_profile_enable(self._ctx, int(on)), 'fm_profile_enable')

    def profile_get(self, kernel: str):
        ms, n = C.c_double(), C.c_int64()
        self._check(self.lib.fm_profile_get(self._ctx, kernel.encode(), C.byref(ms), C.byref(n)), 'fm_profile_get')
        return ms.value, n.value


class IntegrationRun:
    """A trajectory in progress: owns the two endpoint buffers and remembers which one holds the previous
    step's prediction, so a trajectory can be advanced in several fm_integrate calls (bench.py times a
    window of steps; Engine.integrate runs them all)."""

    def __init__(self, eng: Engine, state, plan: StepPlan, noise_for_step, traj=None, inpaint=None):
        """``inpaint``: the spec of ``Engine.inpaint_spec`` or ``Engine.freeze_spec`` -- every step then freezes its rows (fm_integrate_inpaint /
        fm_integrate_freeze with one group, which keep the trajectory sink and the noise callback); None: fm_integrate."""
        self.eng, self.state, self.plan, self.noise_for_step, self.traj = eng, state, plan, noise_for_step, traj
        self.inpaint = inpaint
        self._ip, self._kind = eng._keep_struct(inpaint) if inpaint is not None else (None, None)
        self._alphas = eng.plan_alphas(plan) if inpaint is not None else None
        tt = eng.cfg.time_embedding_dim
        self.temb_all = (torch.stack([time_embedding_host(sc.t, tt) for sc in plan.scalars]) if plan.scalars
                         else torch.zeros(0, tt)).to(eng.device).contiguous()      # n_timesteps = 1: no step, the prior is the result
        self.dst = [eng.new_dst(), eng.new_dst()]
        self._dsts = [eng._dst_struct(self.dst[0]), eng._dst_struct(self.dst[1])]
        self._st = eng._state_struct(state)
        self.prev_idx = None
        self._keep = []

    def reset(self, state):
        self.state = state
        self._st = self.eng._state_struct(state)
        self.prev_idx = None

    def last_dst(self):
        return None if self.prev_idx is None else self.dst[self.prev_idx]

    NOISE_BYTES_PER_CHUNK = 256 << 20     # torch-generated noise kept alive per fm_integrate call (up to 3 chunks are in flight)

    def run(self, lo: int, hi: int, chunk: int = 32):
        eng = self.eng
        final = C.c_int(0)
        if self.noise_for_step is not None:
            # the reference's draws are tensors: (N, na) + (N, nc) + (U, ne) Exp(1) and two uniforms per row and step.  Bound the
            # transient footprint (30 MB per step at 1024 x 47 atoms) instead of letting it grow with the batch; the in-kernel
            # Philox mode has no noise tensors at all.
            cfg = eng.cfg
            per_step = 4 * (eng.N * (cfg.n_atom_types + cfg.n_charges + 4) + eng.U * (cfg.n_bond_types + 2))
            chunk = max(1, min(chunk, self.NOISE_BYTES_PER_CHUNK // max(per_step, 1)))
        for a in range(lo, hi, chunk):
            b = min(hi, a + chunk)
            k = b - a
            scal = (fm_step_scalars * k)(*self.plan.scalars[a:b])
            if self.noise_for_step is None:        # Philox plan: the kernel draws its own noise
                noises, nzs = None, None
            else:
                noises = [self.noise_for_step(i, bool(self.plan.scalars[i].last_step)) for i in range(a, b)]
                nzs = (fm_step_noise * k)(*[nz.c_struct() for nz in noises])
            sink = None
            if self.traj is not None:
                sink = fm_traj_sink()
                for name in ('x', 'a', 'c', 'e', 'x1', 'a1', 'c1', 'e1'):
                    tsr = self.traj.get(name)
                    setattr(sink, name, _ptr(tsr[a:]) if tsr is not None else None)
            prev = C.byref(self._dsts[self.prev_idx]) if self.prev_idx is not None else None
            with eng._dev():
                if self._ip is None:
                    rc = eng.lib.fm_integrate(eng._ctx, eng._stream(), C.byref(self._st), k, scal, _ptr(self.temb_all[a:]), nzs, prev,
                                              C.byref(self._dsts[0]), C.byref(self._dsts[1]),
                                              C.byref(sink) if sink is not None else None, C.byref(final))
                else:
                    al = (C.c_float * (4 * k))(*self._alphas[a + 1:b + 1].reshape(-1).tolist())
                    rc = getattr(eng.lib, f'fm_integrate_{self._kind}')(eng._ctx, eng._stream(), C.byref(self._st), k, 1, scal, None, None, None, None,
                                                                        _ptr(self.temb_all[a:]), nzs, prev, C.byref(self._dsts[0]), C.byref(self._dsts[1]),
                                                                        C.byref(sink) if sink is not None else None, C.byref(final), C.byref(self._ip), al, None)
            eng._check(rc, 'fm_integrate' if self._ip is None else f'fm_integrate_{self._kind}')
            self.prev_idx = final.value
            # bound the noise kept alive: a chunk's tensors are released once the GPU has passed the event recorded behind it.  The host waits for
            # the chunk BEFORE the previous one only, so two chunks stay enqueued and the device never idles (a device-wide synchronise here
            # drained the queue every third chunk)
            ev = None
            if eng.device.type == 'cuda':
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(eng.device))
            self._keep.append((noises, scal, nzs, ev))
            while len(self._keep) > 2:
                old = self._keep.pop(0)
                if old[3] is not None:
                    old[3].synchronize()
