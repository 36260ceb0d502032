"""Helpers of tests/test_resample.py: the conditional path of given molecules (fm_conditional_path, Engine.conditional_path), FlowMol.resample and
SamplingQueue.submit_from.  A plain module like mixed_util.py, whose cached models and per-molecule comparisons it reuses.

The uniforms of the new stream entry are derived here INDEPENDENTLY of the library: a numpy Philox4x32-10 (uint64 products, the constants of
csrc/fm_device.h) that test_resample.py first validates against a stream the library already pins (the u1 of a campbell step's noise tape)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from flowmol_amd import _lib
from flowmol_amd.engine import _ptr, alpha_tables
from hygiene_util import GuardSet, arena, cpu
from oracle import cpu_ref
from parity_util import onehots

import mixed_util as mu

KERNEL_SIZES = [1, 2, 5, 24, 47]          # 0 pairs, 1 pair, rows below / just above / far above one 256-thread pass (276 and 1081 pairs)
KERNEL_GROUPS = [0, 1, 0, 2, 1]
KERNEL_ALPHAS = [[0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 0.5, 0.3], [0.4, 0.7, 1.0, 0.0]]      # columns x, a, c, e; every column holds a 0.0, a 1.0 and a value between
TRAJ_SIZES = [5, 3, 2, 1]

_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------ Philox in numpy
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (broadcast against each other) -> the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & _M32, p0 & _M32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def u01(word):
    """fm_u01: the top 24 bits as a float32 in [0, 1)."""
    return (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def row_uniforms(sizes, ids, job, seed, c2, block, word=0):
    """u01(word of block) of counter (global molecule id, row, c2, block) for every row of modality ``job`` (0, 1: atoms, 2: unordered pairs) of the
    batch, molecules concatenated -> float32 tensor."""
    out = []
    for n, gid in zip(sizes, ids):
        rows = n if job < 2 else n * (n - 1) // 2
        w = philox4x32(gid, np.arange(rows), c2, block, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        out.append(u01(w[word]))
    return torch.from_numpy(np.concatenate(out).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ given molecules
def given(cfg, sizes, seed=17):
    """Seeded molecules to resample, as the (tensors, n_atoms) pair of sample(return_tensors=True): real categories only, coordinates not centred."""
    gen = torch.Generator().manual_seed(seed)
    n = torch.tensor(sizes)
    N, U = int(n.sum()), int((n * (n - 1) // 2).sum())
    rnd = lambda rows, K: torch.randint(0, K, (rows,), generator=gen)
    return {'x': torch.randn(N, 3, generator=gen) * 1.5 + 0.7, 'a': rnd(N, cfg.n_atom_types), 'c': rnd(N, cfg.n_charges), 'e': rnd(U, cfg.n_bond_types)}, n


def take(mols, idx):
    """The molecules ``idx`` (a list) of a given() pair, in that order."""
    t, n = mols
    sizes = n.tolist()
    pairs = [k * (k - 1) // 2 for k in sizes]
    cols = {k: torch.split(t[k], pairs if k == 'e' else sizes) for k in 'xace'}
    return {k: torch.cat([cols[k][i] for i in idx]) for k in 'xace'}, n[idx]


def as_state(eng, mols):
    t, _ = mols
    return eng.make_state(t['x'], t['a'], t['c'], t['e'])


def node_alpha(sizes, groups, alphas, col):
    """alphas[group of the row's molecule][col] for every atom (col 0 .. 2) or unordered pair (col 3) -> float32 (rows,)."""
    al = torch.tensor(alphas, dtype=torch.float32)
    rows = [n * (n - 1) // 2 if col == 3 else n for n in sizes]
    return torch.cat([al[g, col].repeat(r) for r, g in zip(rows, groups)])


def alpha_row(cfg, T, k):
    return alpha_tables(torch.linspace(0, 1, T), cfg.schedule_type, cfg.cosine_params)[0][k]


def kernel_case(preset, lib, device, sizes=KERNEL_SIZES, groups=KERNEL_GROUPS, alphas=KERNEL_ALPHAS, seed=91, ids=(11, 3, 40, 7, 1000003)):
    """One conditional_path call with its tape on the kernel-only shapes, computed once per configuration and shared:
    {'eng', 'cfg', 'x1' (cpu state), 'out', 'tape' (cpu), 'sizes', 'groups', 'alphas', 'seed', 'ids'}.  No network evaluation runs."""
    def make():
        eng, cfg, _ = mu.engine(preset, lib, device)
        mols = given(cfg, sizes)
        eng.bind(torch.tensor(sizes))
        eng.set_molecule_ids(torch.tensor(list(ids)))
        x1 = as_state(eng, mols)
        before = cpu(x1)
        out, tape = eng.conditional_path(x1, alphas, groups, seed=seed, tape=True)
        eng.synchronize()
        assert mu.first_difference(before, cpu(x1)) is None          # x1 is only read
        return {'eng': eng, 'cfg': cfg, 'x1': before, 'out': cpu(out), 'tape': cpu(tape), 'sizes': list(sizes), 'groups': list(groups), 'alphas': alphas,
                'seed': seed, 'ids': list(ids)}
    return mu.cached(('cond', preset, id(lib), str(device), tuple(sizes), tuple(groups), str(alphas), seed, tuple(ids)), make)


def rebind(case):
    eng = case['eng']
    eng.bind(torch.tensor(case['sizes']))
    eng.set_molecule_ids(torch.tensor(case['ids']))
    return eng


# ------------------------------------------------------------------------------------------------------------------ the API
def resample_tensors(mdl, mols, k, T, seed, ids, **kw):
    out = mdl.resample(mols, k, n_timesteps=T, seed=seed, mol_ids=ids, return_tensors=True, **kw)[0]
    return mu.split_molecules(out, mols[1].tolist())


def resample_alone(mdl, mols, i, k, T, seed, mol_id, **kw):
    return resample_tensors(mdl, take(mols, [i]), int(k), int(T), seed, [mol_id], **kw)[0]


def alone_runs(preset, lib, device, mols, ks, Ts, seed, ids, tag):
    """Every molecule resampled alone, computed once per (molecule, T, k, id) and shared between the comparisons."""
    mdl = mu.model(preset, lib, device)
    return [mu.cached(('resample-alone', preset, id(lib), str(device), tag, i, int(k), int(T), seed, mid), lambda: resample_alone(mdl, mols, i, k, T, seed, mid))
            for i, (k, T, mid) in enumerate(zip(ks, Ts, ids))]


def centred(eng, mols):
    """The given molecules with remove_com's centring (the engine bound to their sizes here) -> per-molecule result dicts."""
    t, n = mols
    eng.bind(n)
    x = eng.remove_com(t['x'].to(eng.device, torch.float32).contiguous().clone()).cpu()
    return mu.split_molecules({'x': x, 'a': t['a'], 'c': t['c'], 'e': t['e']}, n.tolist())


# ------------------------------------------------------------------------------------------------------------------ the oracle
def oracle_from_state(mdl, sizes, ids, mols, k, T, seed, visualize=False):
    """The bound batch ``sizes`` with ``ids``: its conditional-path state at time point k of T, as one-hots, integrated by cpu_ref.OracleVF over
    tspan = linspace(0, 1, T)[k:] with the noise tapes of steps k .. T-2 -> (the corrupted state on the cpu, the oracle's result, its frames or None)."""
    eng, cfg = mdl.engine, mdl.cfg
    orc = cpu_ref.OracleVF(cfg, mdl._sd, prefix=mdl._prefix)
    n = torch.tensor(sizes)
    eng.bind(n)
    eng.set_molecule_ids(torch.tensor(ids))
    state = cpu(eng.conditional_path(as_state(eng, mols), alpha_row(cfg, T, k), seed=seed))
    plan = mu.philox_plans(mdl, [T], seed)[0]
    tape = []
    for s in range(k, T - 1):
        nz = eng.philox_tape(plan, s)
        for tag in 'ace':
            tape += [getattr(nz, f'{f}_{tag}').cpu() for f in ('q', 'u1', 'u2') if getattr(nz, f'{f}_{tag}') is not None]
    batch = cpu_ref.build_batch(n)
    a0, c0, e0 = onehots(cfg, batch, state['a_t'].long(), state['c_t'].long(), state['e_t'].long())
    noise = cpu_ref.TapeNoise(tape)
    with torch.no_grad():
        ref = orc.integrate(batch, {'x_0': state['x_t'], 'a_0': a0, 'c_0': c0, 'e_0': e0}, T, noise=noise, tspan=torch.linspace(0, 1, T)[k:],
                            visualize=visualize)
    assert noise.pos == len(tape)
    ref, frames = ref if visualize else (ref, None)
    m = batch.upper_edge_mask
    want = {'x': ref['x_1'], 'a': ref['a_1'].argmax(-1).int(), 'c': ref['c_1'].argmax(-1).int(), 'e': ref['e_1'][m].argmax(-1).int()}
    if frames is not None:
        frames = {'x': torch.stack(frames['x']), 'a': torch.stack([f.argmax(-1) for f in frames['a']]), 'c': torch.stack([f.argmax(-1) for f in frames['c']]),
                  'e': torch.stack([f[m].argmax(-1) for f in frames['e']])}
    return state, want, frames


# ------------------------------------------------------------------------------------------------------------------ the raw ABI, guarded
def guarded_conditional_path(eng, sizes, groups, alphas, seed, fill, ids):
    """One fm_conditional_path call through ctypes with EVERY pointer of the call -- x1, out, alpha, mol_group, the tape -- between 4096-byte 0xA5 bands and
    the batch bound in an arena filled with ``fill`` -> (out and tape on the cpu, guard failures incl. written inputs, arena intact, unwritten outputs)."""
    cfg, dev = eng.cfg, eng.device
    ws, intact = arena(eng, [sizes], fill)
    eng.bind(torch.tensor(sizes), workspace=ws)
    eng.set_molecule_ids(torch.tensor(ids))
    t, _ = given(cfg, sizes)
    gs, i32 = GuardSet(dev), torch.int32
    x1 = {'x_t': gs.inp('x1.x_t', t['x']), 'a_t': gs.inp('x1.a_t', t['a'], i32), 'c_t': gs.inp('x1.c_t', t['c'], i32), 'e_t': gs.inp('x1.e_t', t['e'], i32)}
    out = {'x_t': gs.out('out.x_t', (eng.N, 3)), 'a_t': gs.out('out.a_t', (eng.N,), i32), 'c_t': gs.out('out.c_t', (eng.N,), i32), 'e_t': gs.out('out.e_t', (eng.U,), i32)}
    tape = {'x0': gs.out('tape.x0', (eng.N, 3)), 'u_a': gs.out('tape.u_a', (eng.N,)), 'u_c': gs.out('tape.u_c', (eng.N,)), 'u_e': gs.out('tape.u_e', (eng.U,))}
    al = gs.inp('alpha', torch.tensor(alphas, dtype=torch.float32))
    group = gs.inp('mol_group', torch.tensor(groups, dtype=i32))
    cs = _lib.fm_cond_tape()
    cs.x0, cs.u_a, cs.u_c, cs.u_e = _ptr(tape['x0']), _ptr(tape['u_a']), _ptr(tape['u_c']), _ptr(tape['u_e'])
    s1, so = eng._state_struct(x1), eng._state_struct(out)
    with eng._dev():
        rc = eng.lib.fm_conditional_path(eng._ctx, eng._stream(), C.c_uint64(seed), C.byref(s1), len(alphas), _ptr(group), _ptr(al), C.byref(so), C.byref(cs))
    eng._check(rc, 'fm_conditional_path')
    eng.synchronize()
    return cpu({**out, **tape}), gs.check(), intact(eng.workspace_bytes), gs.unwritten()
