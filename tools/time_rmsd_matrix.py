"""Time the RMSD matrices of a conformer job three ways, on the GPU.

    python tools/time_rmsd_matrix.py [--n_mols 64] [--n_conf 32] [--n_atoms 47] [--reps 7] [--out file.json]

The job: n_mols molecules x n_conf conformers x n_atoms atoms, every group's strict upper triangle (n_mols n_conf (n_conf - 1) / 2 pairs).
    identity   Engine.bind of the n_mols n_conf conformers + Engine.pair_rmsd without a permutation table
    perms12    the same with one 12-row permutation set (the automorphisms of a six-ring on atoms 0..5, the identity elsewhere) shared by all molecules
    gathered   what the library offered before fm_pair_rmsd: both sides of every pair gathered into two (P n_atoms, 3) tensors on the device, a bind of P
               "molecules" and one fm_align_rmsd call -- in chunks of at most --max_bind pairs (default 8192, the largest batch the test suite binds), so
               ceil(P / max_bind) binds and calls
Each window is host wall-clock time from before the bind (for `gathered`: before the gather) to after a device synchronise, so the gather, the bind, the
uploads and the launch are all inside; the pair list is built beforehand.  Warm-up runs first, then --reps repetitions with the three alternating inside every
repetition; min / median / max.  `kernel_ms` is the library's own per-kernel profile (device events) of one more call of each.  One JSON object on stdout (and
in --out) with the device name and the digest of the library sources.  Needs a GPU: there is no CPU fallback for a timing."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from flowmol_amd import build          # noqa: E402
from flowmol_amd.model import FlowMol          # noqa: E402
from flowmol_amd.symmetry import automorphisms          # noqa: E402

SEED = 11


def summary(v):
    return {'min': min(v), 'median': statistics.median(v), 'max': max(v)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_mols', type=int, default=64)
    ap.add_argument('--n_conf', type=int, default=32)
    ap.add_argument('--n_atoms', type=int, default=47)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--max_bind', type=int, default=8192)
    ap.add_argument('--out', type=Path, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('time_rmsd_matrix.py measures on the GPU; none is visible')
    dev = 'cuda:0'
    eng = FlowMol.from_preset('qm9').to(dev).engine
    B, K, n = args.n_mols, args.n_conf, args.n_atoms
    M = B * K
    gen = torch.Generator().manual_seed(SEED)
    x = (torch.randn(M * n, 3, generator=gen) * 1.5).to(dev)
    i, j = torch.triu_indices(K, K, 1)
    pairs = torch.cat([torch.stack([g * K + i, g * K + j], dim=1) for g in range(B)]).to(torch.int32)
    P = int(pairs.shape[0])
    sizes = torch.full((M,), n)
    ring = {(a, (a + 1) % 6) for a in range(6)}
    e = torch.tensor([1 if (a, b) in ring or (b, a) in ring else 0 for a in range(6) for b in range(a + 1, 6)])
    rows = torch.cat([automorphisms(torch.zeros(6), torch.zeros(6), e), torch.arange(6, n).expand(12, -1)], dim=1)
    assert rows.shape == (12, n)
    perm_sets = (torch.zeros(M, dtype=torch.int32), [rows])
    atoms = torch.arange(n)
    res = {}

    def identity():
        eng.bind(sizes)
        res['identity'] = eng.pair_rmsd(x, pairs)[:, 1]

    def perms12():
        eng.bind(sizes)
        res['perms12'] = eng.pair_rmsd(x, pairs, None, perm_sets)[:, 1]

    def gathered():
        out = []
        for p0 in range(0, P, args.max_bind):
            pr = pairs[p0:p0 + args.max_bind].to(dev).long()
            ia = (pr[:, 0, None] * n + atoms.to(dev)).reshape(-1)
            ib = (pr[:, 1, None] * n + atoms.to(dev)).reshape(-1)
            xa, xb = x[ia], x[ib]
            eng.bind(torch.full((int(pr.shape[0]),), n))
            out.append(eng.align_rmsd(xa, xb)[:, 2])
        res['gathered'] = torch.cat(out)

    calls = {'identity': identity, 'perms12': perms12, 'gathered': gathered}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        for fn in calls.values():
            timed(fn)
    samples = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():          # alternate inside every repetition
            samples[k].append(timed(fn))
    kernels = {}
    for k, fn in calls.items():
        eng.profile(True)
        fn()
        torch.cuda.synchronize()
        name = 'align_rmsd' if k == 'gathered' else 'pair_rmsd'
        ms, launches = eng.profile_get(name)
        kernels[k] = {'kernel': name, 'ms': ms, 'launches': launches}
        eng.profile(False)
    same = float((res['identity'] - res['gathered']).abs().max())
    out = {'tool': 'time_rmsd_matrix', 'device': torch.cuda.get_device_name(0), 'library_digest': build._digest(), 'reps': args.reps, 'warmup': args.warmup,
           'n_mols': B, 'n_conf': K, 'n_atoms': n, 'pairs': P, 'max_bind': args.max_bind, 'unit': 'ms per job', 'clock': 'host wall clock around bind + call + synchronise',
           'timings': {k: summary(v) for k, v in samples.items()}, 'kernel_ms': kernels,
           'gathered_over_identity_median': statistics.median(samples['gathered']) / statistics.median(samples['identity']),
           'perms12_over_identity_median': statistics.median(samples['perms12']) / statistics.median(samples['identity']),
           'max_abs_identity_minus_gathered': same, 'perms12_not_above_identity': bool((res['perms12'] <= res['identity']).all())}
    line = json.dumps(out)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + '\n')


if __name__ == '__main__':
    main()
