"""The f32 edge-message instances of 16 and 32 rows take a row's endpoints from the tile descriptor (the molecule's first edge row, first node, atom count
and the destination of the tile's first row; flowmol_amd/csrc/fm_tile_desc.h) and request their gathers at entry.  Through the engine, on the host
emulation and on the GPU:

  * per-stage parity with the CPU oracle (per-edge messages of the first convolution, every convolution's aggregate and output, the outputs) at the
    tolerances of parity_util;
  * composition invariance, torch.equal: every molecule evaluated alone, and the same molecules in one batch in two different orders with 1-atom
    molecules (which own no tile) in between, give the same bits per molecule in every tap -- a wrong first node, first edge row or first destination
    in a descriptor moves a molecule's rows as soon as something stands in front of it.

Molecule sizes are where the row arithmetic can go wrong: n = 2 (n - 1 = 1: every row a new destination), 3, 9 (72 rows: a ragged 8-row tile with a chunk
boundary inside), 17 (n - 1 = the aggregation chunk), 33 (n - 1 = the tile height), 34 (the destination boundary drifts one row per tile); on the GPU also 47
(the benchmark's molecule) and 92.  flowmol3 has 32 vector channels, geom_ctmc 16, dev destination features.  pair_slab = 1 runs the pair-slab instance on the
convolutions in front of the first molecule update of a self-conditioned evaluation, -1 the full instance everywhere."""
import pytest
import torch

from flowmol_amd import presets, weights
from flowmol_amd.engine import Engine
from oracle import cpu_ref
from parity_util import (edge_perm, engine_stages, oracle_run, oracle_stage_tensors, out_of_tolerance, seeded_inputs, slice_molecule,
                         stage_errors)


def _concat(inp, order):
    """The molecules ``order`` of ``inp`` as one batch, in that order."""
    parts = [slice_molecule(inp, m) for m in order]
    cat = lambda k: torch.cat([p[k] for p in parts])
    prev = None
    if inp['prev'] is not None:
        prev = {k: torch.cat([p['prev'][k] for p in parts]) for k in inp['prev']}
    n_atoms = inp['batch'].n_atoms[torch.tensor(order)]
    return {'batch': cpu_ref.build_batch(n_atoms), 'x': cat('x'), 'a': cat('a'), 'c': cat('c'), 'eu': cat('eu'), 'prev': prev}


def _per_molecule(got, n_atoms):
    """{stage: [rows of molecule 0, rows of molecule 1, ..]}: node rows, directed-edge rows (the engine keeps a molecule's edges together) or pair rows."""
    n = [int(v) for v in n_atoms.tolist()]
    out = {}
    for k, v in got.items():
        per = [a * (a - 1) for a in n] if ('.msg.' in k or k.endswith('.ef')) else [a * (a - 1) // 2 for a in n] if k == 'out.e' else n
        v = v.detach().cpu()
        assert v.shape[0] == sum(per), (k, v.shape, sum(per))
        out[k] = list(torch.split(v, per))
    return out


def _check(lib, device, name, sizes, order_b, prev, tile, pair_slab):
    cfg = presets.PRESETS[name]()
    sd = weights.synth_state_dict(cfg, 0)
    eng = Engine(cfg, sd, device=device, lib=lib, tuning={'tile_edge': tile, 'pair_slab': pair_slab})
    inp = seeded_inputs(cfg, torch.tensor(sizes), prev)
    # parity with the oracle, stage by stage
    got, stages, _ = engine_stages(eng, cfg, inp, 0.5, taps=True)
    got = {k: v.detach().cpu().clone() for k, v in got.items()}
    want_taps = ['conv0.msg.s', 'conv0.msg.v'] + [f'conv{i}.{k}' for i in range(cfg.n_convs) for k in ('agg.s', 'agg.v', 's', 'v')] + ['out.' + k for k in 'xace']
    assert set(want_taps) <= set(got), sorted(set(want_taps) - set(got))
    perm = edge_perm(eng, inp['batch'])
    taps_o, ref = oracle_run(cpu_ref.OracleVF(cfg, sd), cfg, inp, 0.5)
    errs = stage_errors(got, oracle_stage_tensors(taps_o, ref, stages, perm))
    print(name, sizes, 'prev' if prev else 'plain', tile, pair_slab, {k: f'{v:.2e}' for k, v in errs.items()})
    bad = out_of_tolerance(errs)
    assert not bad, bad
    # the same molecules in another order
    a = _per_molecule(got, inp['batch'].n_atoms)
    inp_b = _concat(inp, order_b)
    got_b, _, _ = engine_stages(eng, cfg, inp_b, 0.5, taps=True)
    b = _per_molecule(got_b, inp_b['batch'].n_atoms)
    moved = [(k, m) for k in a for pos, m in enumerate(order_b) if not torch.equal(b[k][pos], a[k][m])]
    assert not moved, moved
    # ... and every size alone
    seen = set()
    for m, n in enumerate(sizes):
        if n in seen or n < 2:
            continue
        seen.add(n)
        got_m, _, _ = engine_stages(eng, cfg, slice_molecule(inp, m), 0.5, taps=True)
        diff = [k for k in a if not torch.equal(got_m[k].detach().cpu(), a[k][m])]
        assert not diff, (n, diff)
    eng.close()


def _reorder(sizes):
    """The batch reversed; every molecule with edges must stand behind a different number of nodes than before."""
    order = list(reversed(range(len(sizes))))
    off = lambda seq: {m: sum(sizes[k] for k in seq[:pos]) for pos, m in enumerate(seq)}
    a, b = off(list(range(len(sizes)))), off(order)
    assert all(a[m] != b[m] for m in order if sizes[m] >= 2), (a, b)
    return order


# (preset, sizes): 1-atom molecules stand between the others in both orders.
# The emulation runs a lane at a time, so its cases are cut by cost, not by what they check: the sizes up to 9 atoms (80 rows) run every preset, tile height,
# instance and evaluation kind; the sizes whose tiles are all full (17, 33, 34 atoms: 2,450 rows, each evaluated alone and in two orders) run once per
# code path -- 32 vector channels on both heights and both instances, 16 channels and destination features on one height each.  The GPU runs every
# combination on every size.
EMU_SMALL = [('flowmol3', [2, 1, 9, 1, 3]), ('geom_ctmc', [3, 1, 9, 2]), ('dev', [3, 1, 9, 2])]
EMU_LARGE = [('flowmol3', [17, 1, 34, 33], True, 1, 32), ('flowmol3', [17, 1, 34, 33], False, -1, 16),
             ('geom_ctmc', [34, 1, 17], True, 1, 32), ('dev', [17, 1, 33], True, -1, 16)]
GPU_CASES = [('flowmol3', [2, 1, 9, 3, 47, 1, 17, 34, 33, 92]), ('geom_ctmc', [9, 1, 2, 17, 3, 34, 1, 33, 47, 92]), ('dev', [3, 1, 9, 2, 17, 33, 1, 34, 47, 92])]
MODES = [(True, 1), (True, -1), (False, 1), (False, -1)]
MODE_IDS = ['selfcond-slab', 'selfcond-full', 'plain-slab', 'plain-full']


# destination-feature models have no pair-slab instance: asking for it changes no launch, so `dev` runs the two pair_slab = -1 kinds
EMU_SMALL_CASES = [pytest.param(name, sizes, prev, ps, tile, id=f'{name}-{mid}-{tile}') for name, sizes in EMU_SMALL
                   for (prev, ps), mid in zip(MODES, MODE_IDS) for tile in (16, 32) if not (name == 'dev' and ps > 0)]


@pytest.mark.parametrize('name,sizes,prev,pair_slab,tile', EMU_SMALL_CASES)
def test_computed_endpoints_parity_and_composition_on_emulation(emu_lib, name, sizes, prev, pair_slab, tile):
    _check(emu_lib, 'cpu', name, sizes, _reorder(sizes), prev, tile, pair_slab)


@pytest.mark.parametrize('name,sizes,prev,pair_slab,tile', EMU_LARGE)
def test_computed_endpoints_on_full_tiles_on_emulation(emu_lib, name, sizes, prev, pair_slab, tile):
    _check(emu_lib, 'cpu', name, sizes, _reorder(sizes), prev, tile, pair_slab)


@pytest.mark.gpu
@pytest.mark.parametrize('tile', [16, 32])
@pytest.mark.parametrize('prev,pair_slab', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('name,sizes', GPU_CASES)
def test_computed_endpoints_parity_and_composition_on_gpu(name, sizes, prev, pair_slab, tile):
    _check(None, 'cuda:0', name, sizes, _reorder(sizes), prev, tile, pair_slab)
