"""Time one fm_denoising_loss next to one fm_forward_mixed on the same bound batch, on the GPU.

    python tools/time_denoising_loss.py [--n_mols 1024] [--n_atoms 47] [--groups 8] [--reps 9] [--out file.json]

Both calls are made through the C ABI with every buffer, struct and time embedding prepared beforehand, so the timed window holds the library call alone:
    forward   fm_forward_mixed(prev = NULL, bootstrap = 0, remove_com = 0): table launch, evaluation, heads with softmax, copy of x
    loss      fm_denoising_loss: table launch, the same evaluation with the heads' loss epilogue, fm_k_denoise_reduce
Device events around the call, then a synchronise; the two alternate inside every repetition; min / median / max over the repetitions, and the library's own
per-kernel profile of one loss call (fm_profile_get) to say where the time goes.  The state is a conditional path of seeded molecules at `groups` times.
One JSON object on stdout (and in --out) with the digest of the library sources.  Needs a GPU: there is no CPU fallback for a timing."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from flowmol_amd import _lib, build          # noqa: E402
from flowmol_amd.engine import _ptr, alpha_tables, time_embedding_host          # noqa: E402
from flowmol_amd.model import FlowMol          # noqa: E402

SEED = 11


def summary(v):
    return {'min': min(v), 'median': statistics.median(v), 'max': max(v)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_mols', type=int, default=1024)
    ap.add_argument('--n_atoms', type=int, default=47)
    ap.add_argument('--groups', type=int, default=8)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', type=Path, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('time_denoising_loss.py measures on the GPU; none is visible')
    model = FlowMol.from_preset('flowmol3').to('cuda:0')
    eng, cfg, dev = model.engine, model.cfg, 'cuda:0'
    B, n, G = args.n_mols, args.n_atoms, args.groups
    eng.bind(torch.full((B,), n))
    eng.set_molecule_ids(None)
    gen = torch.Generator().manual_seed(SEED)
    N, U = eng.N, eng.U
    x1 = eng.make_state(torch.randn(N, 3, generator=gen) * 1.5, torch.randint(0, cfg.n_atom_types, (N,), generator=gen),
                        torch.randint(0, cfg.n_charges, (N,), generator=gen), torch.randint(0, cfg.n_bond_types, (U,), generator=gen))
    target = dict(x1, x_t=eng.remove_com(x1['x_t'].clone()))
    tvals = torch.linspace(0.1, 0.9, G)
    group = (torch.arange(B) % G).to(torch.int32)
    xt = eng.conditional_path(x1, alpha_tables(tvals.clone(), cfg.schedule_type, cfg.cosine_params)[0], group if G > 1 else None, seed=SEED)
    temb = torch.stack([time_embedding_host(float(v), cfg.time_embedding_dim) for v in tvals]).to(dev).contiguous()
    group = group.to(dev)
    dst = eng.new_dst()
    rows = {'x': torch.empty(N, device=dev), 'a': torch.empty(N, device=dev), 'c': torch.empty(N, device=dev), 'e': torch.empty(U, device=dev)}
    mol = torch.empty(B, 8, device=dev)
    rs = _lib.fm_loss_rows()
    rs.x, rs.a, rs.c, rs.e = _ptr(rows['x']), _ptr(rows['a']), _ptr(rows['c']), _ptr(rows['e'])
    s_t, s_1, o = eng._state_struct(xt), eng._state_struct(target), eng._dst_struct(dst)
    lib, ctx = eng.lib, eng._ctx

    def forward():
        eng._check(lib.fm_forward_mixed(ctx, eng._stream(), C.byref(s_t), _ptr(temb), G, _ptr(group), None, 0, 0, C.byref(o)), 'fm_forward_mixed')

    def loss():
        eng._check(lib.fm_denoising_loss(ctx, eng._stream(), C.byref(s_t), C.byref(s_1), _ptr(temb), G, _ptr(group), C.byref(rs), _ptr(mol)), 'fm_denoising_loss')

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    calls = {'forward': forward, 'loss': loss}
    for _ in range(args.warmup):
        for fn in calls.values():
            timed(fn)
    samples = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():          # alternate inside every repetition
            samples[k].append(timed(fn))
    eng.profile(True)
    loss()
    torch.cuda.synchronize()
    kernels = {}
    for name in ('embed_table', 'gather_s', 'gather_ef', 'node_proj', 'edge_message', 'node_update', 'edge_update', 'edge_update_head', 'heads', 'node_head',
                 'edge_head', 'denoise_reduce'):
        got = eng.profile_get(name)
        if got and got[1]:
            kernels[name] = {'ms': got[0], 'launches': got[1]}
    eng.profile(False)
    table = mol.cpu()
    res = {'tool': 'time_denoising_loss', 'device': torch.cuda.get_device_name(0), 'library_digest': build._digest(), 'reps': args.reps,
           'n_mols': B, 'n_atoms': n, 'groups': G, 'unit': 'ms per call', 'clock': 'device events', 'timings': {k: summary(v) for k, v in samples.items()},
           'loss_over_forward_median': statistics.median(samples['loss']) / statistics.median(samples['forward']),
           'loss_call_kernels': kernels, 'finite': bool(torch.isfinite(table).all()), 'mean_nll_a': float(table[:, 2].sum() / table[:, 3].sum())}
    line = json.dumps(res)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + '\n')


if __name__ == '__main__':
    main()
