"""Helpers of tests/test_denoising_loss.py: the denoising loss of given molecules (fm_denoising_loss / fm_distort_philox, Engine.denoising_loss / distort,
FlowMol.denoising_loss).  A plain module like resample_util.py, whose given molecules and numpy Philox it reuses.

What is restated here INDEPENDENTLY of the library: the documented summation order of fm_k_denoise_reduce in numpy float32 (chunk_sum), the reference's
row terms from the oracle's logits with torch's own cross_entropy (oracle_rows), and the reference's batch reduction flowmol.py:388-413 with the tensor
shapes its code has (reference_losses)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from flowmol_amd import _lib, presets, weights
from flowmol_amd.engine import Engine, _ptr, alpha_tables
from hygiene_util import GuardSet, arena, cpu
from oracle import cpu_ref
from parity_util import onehots

import mixed_util as mu
import resample_util as ru

REDUCE_SIZES = ru.KERNEL_SIZES            # 1, 2, 5, 24, 47 atoms: 0 pairs, 1 pair, pair rows below (276) and far above (1081) one 64-chunk pass of the wave
REDUCE_T = [0.2, 0.5, 0.2, 0.8, 0.5]      # three time groups
ROW_SIZES = [5, 3, 2, 1]
ROW_T = [0.3, 0.7, 0.3, 0.55]             # three time groups, none 0 (the oracle would bootstrap a batch that is entirely at t = 0)
GPU_SIZES = [5, 9]
GPU_T = [0.35, 0.6]
SEED = 515
MASKS = lambda cfg: {'a': cfg.n_atom_types, 'c': cfg.n_charges, 'e': cfg.n_bond_types}


def loss_engine(preset, lib, device, head_scale=1.0):
    """(engine, cfg, state dict) of the preset with weights-by-name, the last layers of the categorical heads times ``head_scale`` (cached)."""
    if head_scale == 1.0:
        return mu.engine(preset, lib, device)

    def make():
        cfg = presets.PRESETS[preset]()
        sd = weights.scaled_weights(weights.synth_state_dict(cfg, 0), 1.0, cat_head_scale=head_scale)
        return Engine(cfg, sd, device=device, lib=lib), cfg, sd
    return mu.cached(('loss-engine', preset, id(lib), str(device), head_scale), make)


# ------------------------------------------------------------------------------------------------------------------ the reduction, restated
def chunk_sum(v) -> np.float32:
    """The documented order of fm_k_denoise_reduce in numpy float32: 16-row chunks from the first row, a chunk's rows added in order to +0, the chunk sums
    added in order to +0."""
    v = np.asarray(v, dtype=np.float32)
    total = np.float32(0.0)
    for b in range(0, len(v), 16):
        cs = np.float32(0.0)
        for x in v[b:b + 16]:
            cs = np.float32(cs + x)
        total = np.float32(total + cs)
    return total


def mol_table(rows, tok_t, cfg, sizes):
    """(B,8) {se_x, 3 n, nll_a, cnt_a, nll_c, cnt_c, nll_e, cnt_e} from row terms {'x','a','c','e'} and the tokens of x_t {'a','c','e'} (cpu tensors)."""
    out, n0, p0 = [], 0, 0
    for n in sizes:
        p = n * (n - 1) // 2
        r = [chunk_sum(rows['x'][n0:n0 + n].numpy()), np.float32(3 * n)]
        for k in 'ace':
            sl = slice(p0, p0 + p) if k == 'e' else slice(n0, n0 + n)
            r += [chunk_sum(rows[k][sl].numpy()), np.float32(int((tok_t[k][sl] == MASKS(cfg)[k]).sum()))]
        out.append(r)
        n0, p0 = n0 + n, p0 + p
    return torch.tensor(np.array(out, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ one evaluated batch
def loss_case(preset, lib, device, sizes=ROW_SIZES, times=ROW_T, head_scale=1.0, seed=SEED, ids=None):
    """Given molecules corrupted by Engine.conditional_path at one time per molecule, then Engine.denoising_loss and -- on the same state and t, not
    COM-removed -- Engine.forward; computed once per configuration and shared.  Everything on the cpu: {'x1' the given state, 'target' (x centred),
    'xt', 'mol', 'rows', 'probs'} plus 'eng', 'cfg', 'sd', 'sizes', 't', 'ids'."""
    ids = list(ids) if ids is not None else [7 + 13 * i for i in range(len(sizes))]

    def make():
        eng, cfg, sd = loss_engine(preset, lib, device, head_scale)
        t = torch.tensor(times, dtype=torch.float32)
        eng.bind(torch.tensor(sizes))
        eng.set_molecule_ids(torch.tensor(ids))
        raw = ru.as_state(eng, ru.given(cfg, sizes))
        target = dict(raw, x_t=eng.remove_com(raw['x_t'].clone()))
        tvals, group = torch.unique(t, return_inverse=True)
        xt = eng.conditional_path(raw, alpha_tables(tvals.clone(), cfg.schedule_type, cfg.cosine_params)[0], group if tvals.numel() > 1 else None, seed=seed)
        before = cpu(xt), cpu(target)
        res = eng.denoising_loss(xt, target, t)
        eng.synchronize()
        assert mu.first_difference(before[0], cpu(xt)) is None and mu.first_difference(before[1], cpu(target)) is None          # inputs are only read
        probs = eng.forward(xt, t, remove_com=False)
        eng.synchronize()
        return {'eng': eng, 'cfg': cfg, 'sd': sd, 'sizes': list(sizes), 't': t, 'ids': ids, 'x1': cpu(raw), 'target': before[1], 'xt': before[0],
                'mol': res['mol'].cpu(), 'rows': cpu(res['rows']), 'probs': cpu(probs)}
    return mu.cached(('loss', preset, id(lib), str(device), tuple(sizes), tuple(times), head_scale, seed, tuple(ids)), make)


def targets(case):
    """The reference's targets (flowmol.py:353-384): the x_1 token, -100 (ignore_index) where the token of x_t is not the mask token."""
    out = {}
    for k in 'ace':
        tgt = case['target'][f'{k}_t'].long().clone()
        tgt[case['xt'][f'{k}_t'].long() != MASKS(case['cfg'])[k]] = -100
        out[k] = tgt
    return out


def oracle_rows(case, dtype=torch.float32):
    """The reference's row terms in ``dtype``: OracleVF.forward(x_t, t of shape (B,), apply_softmax=False, remove_com=False) -> logits and x, then
    F.cross_entropy(reduction='none', ignore_index=-100) on the targets above and the squared errors summed over xyz.  float64: the state dict cast."""
    cfg, xt = case['cfg'], case['xt']
    batch = cpu_ref.build_batch(torch.tensor(case['sizes']))
    a1h, c1h, e1h = onehots(cfg, batch, xt['a_t'].long(), xt['c_t'].long(), xt['e_t'].long())
    try:
        torch.set_default_dtype(dtype)
        orc = cpu_ref.OracleVF(cfg, case['sd'])
        orc.p = {k: v.to(dtype) for k, v in orc.p.items()}
        with torch.no_grad():
            out = orc.forward(batch, xt['x_t'].to(dtype), a1h.to(dtype), c1h.to(dtype), e1h.to(dtype), case['t'].to(dtype), prev=None, apply_softmax=False,
                              remove_com=False)
    finally:
        torch.set_default_dtype(torch.float32)
    tg = targets(case)
    rows = {k: F.cross_entropy(out[k], tg[k], reduction='none', ignore_index=-100) if tg[k].numel() else out[k].new_zeros(0) for k in 'ace'}
    rows['x'] = ((out['x'] - case['target']['x_t'].to(dtype)) ** 2).sum(-1)
    return rows


def rounding_noise(case):
    """{term: max |float32 oracle - float64 oracle| / max |float64 oracle|} on exactly the case's inputs, and the float32 oracle's rows."""
    r32, r64 = oracle_rows(case), oracle_rows(case, torch.float64)
    return {k: float((r32[k].double() - r64[k]).abs().max() / r64[k].abs().max()) if r64[k].numel() else 0.0 for k in 'xace'}, r32


# ------------------------------------------------------------------------------------------------------------------ the batch values, restated
def reference_losses(rows, t, sizes, cfg, time_scaled):
    """flowmol.py:388-413 in torch on row terms: rows['x'] here is (N,3) squared errors, rows['a'|'c'|'e'] the cross-entropy with ignored rows 0 plus
    the ignore flags rows['keep_*'].  time_scaled: `loss (rows,) * weight (rows, 1)` is evaluated as the reference's code evaluates it."""
    n = torch.tensor(sizes)
    node_idx, pair_idx = torch.arange(len(sizes)).repeat_interleave(n), torch.arange(len(sizes)).repeat_interleave(n * (n - 1) // 2)
    losses = {}
    if time_scaled:
        alpha = alpha_tables(t.clone(), cfg.schedule_type, cfg.cosine_params)[0]
        w_all = torch.clamp(alpha / (1 - alpha), min=0.05, max=1.5)
    for f, k in enumerate('xace'):
        if not time_scaled:
            losses[k] = rows['x'].mean() if k == 'x' else rows[k].sum() / rows['keep_' + k].sum()
        else:
            weight = w_all[:, f][pair_idx if k == 'e' else node_idx].unsqueeze(-1)
            losses[k] = (rows[k] * weight).mean()
    return losses


# ------------------------------------------------------------------------------------------------------------------ the raw ABI, guarded
def guarded_denoising_loss(case, fill):
    """One fm_denoising_loss call through ctypes on the case's state with EVERY pointer of the call between 4096-byte 0xA5 bands and the batch bound in an
    arena filled with ``fill`` -> (rows and mol on the cpu, guard failures incl. written inputs, arena intact, unwritten outputs)."""
    eng, sizes = case['eng'], case['sizes']
    dev, i32 = eng.device, torch.int32
    ws, intact = arena(eng, [sizes], fill)
    eng.bind(torch.tensor(sizes), workspace=ws)
    eng.set_molecule_ids(torch.tensor(case['ids']))
    gs = GuardSet(dev)
    st = {tag: {'x_t': gs.inp(f'{tag}.x_t', case[tag]['x_t']), **{f'{k}_t': gs.inp(f'{tag}.{k}_t', case[tag][f'{k}_t'], i32) for k in 'ace'}} for tag in ('xt', 'target')}
    rows = {'x': gs.out('rows.x', (eng.N,)), 'a': gs.out('rows.a', (eng.N,)), 'c': gs.out('rows.c', (eng.N,)), 'e': gs.out('rows.e', (eng.U,))}
    mol = gs.out('mol_out', (eng.B, 8))
    tvals, group = torch.unique(case['t'], return_inverse=True)
    from flowmol_amd.engine import time_embedding_host
    temb = gs.inp('temb', torch.stack([time_embedding_host(float(v), eng.cfg.time_embedding_dim) for v in tvals]))
    grp = gs.inp('mol_group', group, i32)
    rs = _lib.fm_loss_rows()
    rs.x, rs.a, rs.c, rs.e = _ptr(rows['x']), _ptr(rows['a']), _ptr(rows['c']), _ptr(rows['e'])
    s_t, s_1 = eng._state_struct(st['xt']), eng._state_struct(st['target'])
    with eng._dev():
        rc = eng.lib.fm_denoising_loss(eng._ctx, eng._stream(), C.byref(s_t), C.byref(s_1), _ptr(temb), int(tvals.numel()), _ptr(grp), C.byref(rs), _ptr(mol))
    eng._check(rc, 'fm_denoising_loss')
    eng.synchronize()
    return cpu({**rows, 'mol': mol}), gs.check(), intact(eng.workspace_bytes), gs.unwritten()
