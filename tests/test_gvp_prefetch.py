"""The 32-row f32 tiles of the edge-message and node-update kernels (32 vector channels) request the weight fragments of a GVP's latency phases one
phase ahead and let a wave's two jobs of a phase share them (fm_gvp_core_pf, fm_device.h); the MFMA sequences are those of the plain path.  The 16-row
instances keep the plain path and, under canonical arithmetic, give a row the same bits whatever the tile height -- so they are the in-tree reference
of the new code: every comparison here is torch.equal between an evaluation on 16-row and one on 32-row edge and node tiles, through the engine's
`tuning` argument.

Shapes: n = 2 is a 2-row tile; n = 9 is 72 rows = two full 32-row tiles and a ragged 8-row one with a chunk boundary inside; 47 atoms (68 tiles) is the
benchmark's molecule.  flowmol3 has 32 vector channels (the new path), geom_ctmc 16 (the plain path at both heights).  Self-conditioned evaluations run
the pair-slab instance on the convolutions in front of the first molecule update (`pair_slab` forced on), the others the full instance.  The engine taps
the per-edge messages of the first convolution only (`conv0.msg.*`); every convolution's aggregate and output are compared."""
import pytest
import torch

from flowmol_amd import presets, weights
from flowmol_amd.engine import Engine, cat_temp_schedule, forward_weight_schedule, make_step_plan
from parity_util import engine_stages, seeded_inputs


def _stages_under(lib, device, name, sizes, prev, tile):
    cfg = presets.PRESETS[name]()
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device=device, lib=lib, tuning={'tile_edge': tile, 'tile_node': tile, 'pair_slab': 1})
    inp = seeded_inputs(cfg, torch.tensor(sizes), prev)
    got, stages, _ = engine_stages(eng, cfg, inp, 0.5, taps=True)
    got = {k: v.detach().cpu().clone() for k, v in got.items()}
    eng.close()
    return cfg, got, stages


def _check_tile_heights_agree(lib, device, name, sizes, prev):
    cfg, ref, stages = _stages_under(lib, device, name, sizes, prev, 16)
    _, got, _ = _stages_under(lib, device, name, sizes, prev, 32)
    want = ['conv0.msg.s', 'conv0.msg.v'] + [f'conv{i}.{k}' for i in range(cfg.n_convs) for k in ('agg.s', 'agg.v', 's', 'v')] + ['out.' + k for k in 'xace']
    assert set(want) <= set(got) == set(ref), sorted(set(want) - set(got))
    assert float(ref['conv0.msg.s'].abs().max()) > 0 and float(ref[f'conv{cfg.n_convs - 1}.agg.v'].abs().max()) > 0      # the taps were written
    bad = [k for k in sorted(got) if not torch.equal(got[k], ref[k])]
    assert not bad, {k: float((got[k] - ref[k]).abs().max()) for k in bad}


EMU_CASES = [('flowmol3', [2, 9, 5]), ('geom_ctmc', [3, 9])]
GPU_CASES = [('flowmol3', [2, 9, 47]), ('geom_ctmc', [3, 9, 20])]


@pytest.mark.parametrize('prev', [True, False], ids=['selfcond', 'plain'])
@pytest.mark.parametrize('name,sizes', EMU_CASES)
def test_prefetched_gvp_phases_give_the_16_row_tiles_bits_on_emulation(emu_lib, name, sizes, prev):
    _check_tile_heights_agree(emu_lib, 'cpu', name, sizes, prev)


@pytest.mark.gpu
@pytest.mark.parametrize('prev', [True, False], ids=['selfcond', 'plain'])
@pytest.mark.parametrize('name,sizes', GPU_CASES)
def test_prefetched_gvp_phases_give_the_16_row_tiles_bits_on_gpu(name, sizes, prev):
    _check_tile_heights_agree(None, 'cuda:0', name, sizes, prev)


@pytest.mark.gpu
def test_six_integration_steps_agree_between_tile_heights_on_gpu():
    """fm_integrate, 6 steps of [9, 47] with in-kernel Philox noise: tokens and coordinates equal under both edge-tile heights."""
    cfg = presets.PRESETS['flowmol3']()
    sd = weights.synth_state_dict(cfg, 0)
    sizes = torch.tensor([9, 47])
    outs = {}
    for tile in (16, 32):
        eng = Engine(cfg, sd, device='cuda:0', tuning={'tile_edge': tile})
        eng.bind(sizes)
        x0 = eng.prior_philox(11)
        outs['prior'] = x0.detach().cpu().clone()
        state = eng.prior_state(x0)
        plan = make_step_plan(6, cfg.stochasticity, cfg.high_confidence_threshold, cat_temp_schedule(cfg), forward_weight_func=forward_weight_schedule(cfg),
                              philox_seed=11, schedule_type=cfg.schedule_type, cosine_params=cfg.cosine_params)
        eng.integrate(state, plan, None)
        eng.synchronize()
        outs[tile] = {k: state[k].detach().cpu().clone() for k in ('x_t', 'a_t', 'c_t', 'e_t')}
        eng.close()
    assert not torch.equal(outs[16]['x_t'], outs['prior'])      # the steps moved the molecules
    for k in outs[16]:
        assert torch.equal(outs[16][k], outs[32][k]), k

