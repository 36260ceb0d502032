"""Time one gat CTMC step (fm_ctmc_step alone, no network evaluation) and the endpoint prior on the GPU.

    python tools/time_gat_step.py --n_mols 1024 --n_atoms 47 [--variants a,b,c,p_host,p_dev] [--reps 15] [--inner 20] [--out file.json]

Variants, timed with device events around `inner` back-to-back calls, after a warm-up of every variant, ALTERNATING between the variants in every
repetition (so drift of the shared machine hits all of them alike); min / median / max over the repetitions, per call:
  a       tensor-noise gat step INCLUDING torch drawing its (rows, K+1) Exp(1) tensors on the device (what sample() pays per step)
  b       the same step with the noise drawn beforehand (x_step + three flat gat kernels: four launches)
  c       the Philox step: fm_k_ctmc_gat_fused, one launch, no noise tensors
  p_host  endpoint prior as the torch path draws it: CPU generator for the whole batch, then the upload (host clock around a synchronise)
  p_dev   fm_prior_philox_dense: one launch
A tree that predates the Philox gat step runs `--variants a,b,p_host` (the others need ABI 8).  One JSON object on stdout (and in --out) with the digest of the
library sources.  Needs a GPU: there is no CPU fallback for a timing."""
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

from flowmol_amd import build, presets, weights          # noqa: E402
from flowmol_amd.engine import Engine, StepNoise, cat_temp_schedule, make_step_plan          # noqa: E402
from flowmol_amd.priors import draw_categorical_priors          # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_mols', type=int, default=1024)
    ap.add_argument('--n_atoms', type=int, default=47)
    ap.add_argument('--variants', type=str, default='a,b,c,p_host,p_dev')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', type=Path, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('time_gat_step.py measures on the GPU; none is visible')
    dev = 'cuda:0'
    variants = [v for v in args.variants.split(',') if v]
    sizes = torch.full((args.n_mols,), args.n_atoms)
    runs = {}

    # ---- gat step of the flowmol3 model
    step_variants = [v for v in variants if v in 'abc']
    if step_variants:
        cfg = presets.flowmol3()
        eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device=dev)
        eng.bind(sizes)
        N, U = eng.N, eng.U
        g = torch.Generator(device=dev).manual_seed(0)
        dst = {'x': torch.randn(N, 3, device=dev, generator=g),
               'a': torch.softmax(torch.randn(N, cfg.n_atom_types, device=dev, generator=g), 1), 'c': torch.softmax(torch.randn(N, cfg.n_charges, device=dev, generator=g), 1),
               'e': torch.softmax(torch.randn(U, cfg.n_bond_types, device=dev, generator=g), 1)}
        state = eng.prior_state(torch.randn(N, 3, device=dev, generator=g))
        T = 100
        kw = dict(dfm_type='gat', forward_weight_func=lambda t: 1.5)
        sc_t = make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cat_temp_schedule(cfg), **kw).scalars[T // 2]
        draw = lambda: StepNoise.draw(N, U, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types, False, dev, dfm_type='gat')
        fixed = draw()
        empty = StepNoise()
        if 'c' in step_variants:
            sc_p = make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cat_temp_schedule(cfg), philox_seed=11, **kw).scalars[T // 2]
        runs.update({'a': lambda: eng.ctmc_step(state, dst, draw(), sc_t), 'b': lambda: eng.ctmc_step(state, dst, fixed, sc_t)})
        if 'c' in step_variants:
            runs['c'] = lambda: eng.ctmc_step(state, dst, empty, sc_p)

    # ---- endpoint prior (two prior configurations: the preset's, and Gaussian pair rows -- the 1.1 M x 4 normals of a 1024 x 47 batch)
    prior_variants = [v for v in variants if v.startswith('p_')]
    if prior_variants:
        ecfg = presets.endpoint_small()
        eeng = Engine(ecfg, weights.synth_state_dict(ecfg, 0), device=dev)
        eeng.bind(sizes)
        for tag, types in (('', dict(ecfg.prior_types)), ('_gauss_e', {**ecfg.prior_types, 'e': 'gaussian'})):
            kws = {**ecfg.prior_kwargs, 'e': {}}

            def host(types=types, kws=kws):
                x0 = torch.randn(eeng.N, 3, device=dev)
                a0, c0, e0 = draw_categorical_priors(ecfg, eeng.N, eeng.U, types, kws)
                eeng.remove_com(x0)
                return a0.to(dev), c0.to(dev), e0.to(dev)
            if 'p_host' in prior_variants:
                runs['p_host' + tag] = host
            if 'p_dev' in prior_variants:
                runs['p_dev' + tag] = lambda types=types, kws=kws: eeng.prior_philox_dense(5, types, kws)

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / inner, (time.perf_counter() - t0) * 1e3 / inner

    inner = {k: (2 if k.startswith('p_host') else args.inner) for k in runs}
    for k, fn in runs.items():
        for _ in range(args.warmup):
            timed(fn, inner[k])
    samples = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():          # alternate the variants inside every repetition
            ev, wall = timed(fn, inner[k])
            samples[k].append(wall if k.startswith('p_host') else ev)      # host-side work is not inside device events
    res = {'tool': 'time_gat_step', 'n_mols': args.n_mols, 'n_atoms': args.n_atoms, 'reps': args.reps, 'inner': inner, 'unit': 'ms per call',
           'clock': {k: 'host clock around a device synchronise' if k.startswith('p_host') else 'device events' for k in runs},
           'device': torch.cuda.get_device_name(0), 'library_digest': build._digest(),
           'timings': {k: {'min': min(v), 'median': statistics.median(v), 'max': max(v)} for k, v in samples.items()}}
    line = json.dumps(res)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + '\n')


if __name__ == '__main__':
    main()
