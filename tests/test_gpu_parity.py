"""-m gpu: the HIP path (through the C ABI of libflowmol_hip.so) against the CPU oracle on the same seeded
inputs, and against the golden vectors generated from the reference.  Tolerances (BASELINE.json north star):
coordinates within 1e-4 relative end-to-end (per-evaluation gate 1e-5), categorical sampling
indices bit-exact given identical noise."""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from flowmol_amd import presets, weights
from oracle import cpu_ref
from parity_util import add_dx_stages, dx_gates, forward_compare, integrate_golden, mutation_targets, out_of_tolerance, stage_errors, visible_weights

pytestmark = pytest.mark.gpu

STAGE_TOL = 2e-5      # per-stage relative error (max abs diff / max abs ref) inside one network evaluation
OUT_TOL = 1e-5        # per-evaluation gate on the outputs
REPORT = Path(os.environ.get('GRAFT_REPO_ROOT', Path(__file__).resolve().parent.parent)) / 'gpurun_out'


def _report(name, obj):
    try:
        REPORT.mkdir(exist_ok=True)
        with open(REPORT / 'parity_report.jsonl', 'a') as f:
            f.write(json.dumps({'test': name, **obj}) + '\n')
    except Exception:
        pass


_engines = {}


def engine_for(name, tile=0, visible=False):
    """Engine + oracle per preset.  tile = 0: the library chooses the row-tile size per batch (16 rows for batches that
    do not fill the chip, else 32); 16 / 32: forced through fm_config.tile_edge / tile_node.  precision is passed explicitly:
    no environment variable can change what the parity tests verify.  visible: under parity_util.visible_weights(), the regime of the
    displacement stages (cached like the weights as drawn: one engine per preset, tile and regime for the whole session)."""
    from flowmol_amd.engine import Engine
    key = (name, tile, 'visible') if visible else (name, tile)
    if key not in _engines:
        cfg = presets.PRESETS[name]()
        sd = weights.synth_state_dict(cfg, 0)
        if visible:
            sd = visible_weights(name, sd)
        eng = Engine(cfg, sd, device='cuda:0', precision='f32', tuning={'tile_edge': tile, 'tile_node': tile})
        _engines[key] = (cfg, sd, eng, cpu_ref.OracleVF(cfg, sd))
    return _engines[key]


_dx_gates = {}


def dx_gates_for(name, sd, sizes, t, prev):
    """parity_util.dx_gates of one case under visible_weights() (two oracle runs, one in float64), computed once per case: both tile heights and every
    tuning share it."""
    key = (name, tuple(sizes), float(t), bool(prev))
    if key not in _dx_gates:
        _dx_gates[key] = dx_gates(presets.PRESETS[name](), sd, torch.tensor(sizes), t, prev)
    return _dx_gates[key]


def visible_regime_failures(label, name, eng, orc, cfg, sd, sizes, t, prev):
    """The same evaluation under visible_weights() with the displacement stages `upd{i}.dx` / `out.dx` next to every stage and output: what each position
    update ADDS, scored against its own size (the coordinate stages are blind to it: a whole update is as large as their tolerance) and gated by the
    reference arithmetic alone -- max(8 x the oracle's f32-vs-f64 discrepancy of that stage, 4 ulp(max|x|) / max|ref dx|).  Measured yardsticks
    (flowmol3, [5, 9, 12, 3, 2], t = 0.5): f32-vs-f64 1.0e-6 .. 3.5e-6, floor 3.5e-6 .. 1.1e-5 per displacement stage, displacements 3 .. 9 % of max|x|.
    The errors go into the parity report with both yardsticks beside them.  Returns the stages out of tolerance."""
    errs, out, ref = forward_compare(eng, orc, cfg, torch.tensor(sizes), t, prev, dx=True)
    gates, detail = dx_gates_for(name, sd, sizes, t, prev)
    _report(label, {**errs, 'dx_gate': gates, 'dx_oracle_f32_vs_f64': {k: d['f32_vs_f64'] for k, d in detail.items()},
                    'dx_subtraction_floor': {k: d['floor'] for k, d in detail.items()}})
    assert 'out.dx' in errs and any(k.startswith('upd') and k.endswith('.dx') for k in errs)
    return out_of_tolerance(errs, gates, STAGE_TOL, OUT_TOL)


def test_native_library_is_the_hip_build():
    from flowmol_amd import _lib
    lib = _lib.get_lib()
    assert Path(lib._name).name == 'libflowmol_hip.so'
    assert torch.cuda.is_available()


@pytest.mark.parametrize('name,sizes,t,prev', [
    ('flowmol3', [5, 9, 12, 3, 2], 0.5, True),
    ('flowmol3', [5, 9, 12, 3, 2], 0.0, False),        # bootstrap: two evaluations
    ('flowmol3', [70, 2, 47, 130], 0.3, True),         # destinations spanning several edge tiles
    ('flowmol3', [181, 2], 0.6, True),                 # largest GEOM molecule (7 pieces per destination) next to the smallest
    ('flowmol3', [47], 0.2, True),                     # single-molecule batch
    ('geom_ctmc', [2, 2, 2], 0.9, False),
    ('geom_ctmc', [5, 17, 8, 30, 2], 0.5, False),
    ('geom_arom', [5, 17, 8, 30, 2], 0.5, False),      # explicit aromaticity (geom_full_aromatic.yaml / geom_5_aromatic.yaml): 5 bond types + mask
    ('flowmol3_arom', [5, 9, 47, 2], 0.5, True),
    ('flowmol3_arom', [5, 9, 12], 0.0, False),
    ('qm9', [18] * 8, 0.7, True),
    ('dev_narrow', [70, 2, 47], 0.3, True),            # 64 scalars / 64 edge features on zero-padded 256 / 128-column tiles
    ('dev', [5, 9, 12, 3, 2], 0.5, True),              # configs/dev.yml:78-108: narrow dims + use_dst_feats (gvp.py:300-316,472-473,527-537)
    ('dev', [5, 9, 12, 3, 2], 0.0, False),
    ('dev', [47, 1, 30], 0.4, True),
    ('arch_variants', [5, 9, 1, 30, 2], 0.5, True),    # n_recycles=2, message_norm='mean' (1-atom molecule: no in-edges), EdgeUpdate without distances, one shared updater
    ('arch_variants', [47, 3], 0.0, False),
])
@pytest.mark.parametrize('tile', [16, 32])
def test_forward_matches_oracle(name, sizes, t, prev, tile):
    cfg, sd, eng, orc = engine_for(name, tile)
    errs, out, ref = forward_compare(eng, orc, cfg, torch.tensor(sizes), t, prev)
    _report(f'forward[{name},{sizes},{t},tile{tile}]', errs)
    bad = {k: v for k, v in errs.items() if not (v < (OUT_TOL if k.startswith('out.') else STAGE_TOL))}
    assert not bad, f'stages out of tolerance: {bad}\nall: {errs}'
    for k in 'ace':     # probabilities are normalised
        assert torch.allclose(out[k].sum(-1).cpu(), torch.ones(out[k].shape[0]), atol=1e-5)
    cfg, sd, eng, orc = engine_for(name, tile, visible=True)
    bad = visible_regime_failures(f'forward_visible[{name},{sizes},{t},tile{tile}]', name, eng, orc, cfg, sd, sizes, t, prev)
    assert not bad, f'visible weights, stages out of tolerance: {bad}'


@pytest.mark.parametrize('tuning', [{'tile_edge': 64, 'tile_node': 64}, {'tile_edge_update': 64}, {'tile_edge': 64, 'tile_node': 64, 'tile_edge_update': 64, 'pair_slab': -1},
                                    {'pair_slab': -1}, {'pair_slab': 1}, {'pair_slab': 1, 'pair_mlps': -1, 'mlp_small_tiles': -1}, {'xcd_swizzle': -1, 'fuse_node': -1},
                                    {'tile_edge': 64, 'pair_slab': 1}, {'pair_slab': 1, 'pair_mlps': 1, 'mlp_small_tiles': -1},      # the PQ instance on 64-row tiles, the slab in the shared 64-row SC launch
                                    {'tile_node': 4}, {'tile_node': 4, 'tile_edge': 32, 'pair_slab': 1}, {'tile_node': 8}, {'tile_node': 12}, {'tile_node': 20}, {'tile_node': 16},
                                    {'mlp_small_tiles': 2}, {'mlp_small_tiles': 2, 'pair_mlps': -1}, {'mlp_small_tiles': 1}, {'fuse_node': 2}])      # r5: node-side MLPs on 4-row tiles (automatic up to 1024 nodes) forced / off
@pytest.mark.parametrize('name,sizes,t,prev', [('flowmol3', [70, 2, 47, 130], 0.3, True), ('geom_ctmc', [5, 17, 8, 30, 2], 0.5, False), ('flowmol3', [5, 9, 12, 3, 2], 0.0, False)])
def test_forward_matches_oracle_under_every_accepted_tuning(name, sizes, t, prev, tuning):
    """Every launch-tuning value fm_config accepts is parity-tested (VERDICT r3 hygiene #14): 64-row tiles of the GVP kernels and of EdgeUpdate
    (accepted by fm_create, never chosen automatically), the pair-slab hoist switched off / forced on at small sizes (ABI 6; automatic only for
    large batches), the unfused / unswizzled launch sequence, and the 4 / 8 / 12 / 20-node tiles of the node kernel (chosen automatically as the smallest tile
    that fits one per CU) forced on for batches with 130-atom molecules, and the regular 16-row tile forced for small ones."""
    from flowmol_amd.engine import Engine
    cfg = presets.PRESETS[name]()
    sd = weights.synth_state_dict(cfg, 0)
    eng = Engine(cfg, sd, device='cuda:0', precision='f32', tuning=tuning)
    errs, out, ref = forward_compare(eng, cpu_ref.OracleVF(cfg, sd), cfg, torch.tensor(sizes), t, prev)
    _report(f'forward_tuning[{name},{sizes},{t},{tuning}]', errs)
    bad = {k: v for k, v in errs.items() if not (v < (OUT_TOL if k.startswith('out.') else STAGE_TOL))}
    assert not bad, f'stages out of tolerance: {bad}'
    eng.close()
    sd = visible_weights(name, sd)
    eng = Engine(cfg, sd, device='cuda:0', precision='f32', tuning=tuning)
    bad = visible_regime_failures(f'forward_tuning_visible[{name},{sizes},{t},{tuning}]', name, eng, cpu_ref.OracleVF(cfg, sd), cfg, sd, sizes, t, prev)
    assert not bad, f'visible weights, stages out of tolerance: {bad}'
    eng.close()


@pytest.mark.parametrize('name,sizes,t,prev', [('flowmol3', [47, 5, 130, 18], 0.3, True), ('geom_ctmc', [5, 17, 8, 30, 2], 0.5, False)])
def test_every_tile_height_gives_the_same_bits_on_gpu(name, sizes, t, prev):
    """Canonical arithmetic across tile heights ON THE HARDWARE (round 6): the 4 / 8 / 12 / 20-node tiles of the node kernel and the 4-row node MLPs run their GEMMs
    on v_mfma_f32_4x4x1 as ONE fma chain per output element in the k-order of the regular tiles' v_mfma_f32_16x16x4 accumulators (fm_wave_gemm4) -- which
    only gives the regular tiles' bits if the hardware's 16x16x4 instruction IS that chain.  One network evaluation under every node / edge / MLP tile
    height: all outputs bit-identical (64-row tiles and pair_slab = -1 are documented as other orders and are not in the list)."""
    from flowmol_amd.engine import Engine
    cfg = presets.PRESETS[name]()
    sd = weights.synth_state_dict(cfg, 0)
    ref = None
    for tuning in ({'tile_node': 16, 'tile_edge': 16, 'mlp_small_tiles': 1}, {}, {'tile_node': 4}, {'tile_node': 8}, {'tile_node': 12}, {'tile_node': 20}, {'tile_node': 32, 'tile_edge': 32},
                   {'mlp_small_tiles': 2}, {'mlp_small_tiles': 2, 'pair_mlps': -1, 'tile_node': 4}, {'mlp_small_tiles': -1, 'tile_node': 8}):
        eng = Engine(cfg, sd, device='cuda:0', precision='f32', tuning=tuning)
        errs, out, _ = forward_compare(eng, cpu_ref.OracleVF(cfg, sd), cfg, torch.tensor(sizes), t, prev, taps=False)
        got = {k: out[k].detach().cpu().clone() for k in 'xace'}
        ref = ref or got
        for k in 'xace':
            assert torch.equal(got[k], ref[k]), (tuning, k, float((got[k] - ref[k]).abs().max()))
        eng.close()


@pytest.mark.parametrize('fname,name', [('integrate_flowmol3_F7.npz', 'flowmol3'), ('integrate_qm9_C1.npz', 'qm9'),
                                        ('integrate_geom_ctmc_C5s.npz', 'geom_ctmc'),
                                        ('integrate_geom_arom_T16.npz', 'geom_arom'), ('integrate_flowmol3_arom_T12.npz', 'flowmol3_arom')])
def test_integrate_matches_reference_golden(golden_dir, fname, name):
    """Free-running trajectories with the reference's recorded noise: zero categorical flips and
    coordinates within 1e-4 relative of the reference's own output."""
    cfg, sd, eng, orc = engine_for(name)
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / fname).items()}
    res, state = integrate_golden(eng, cfg, g, device='cuda:0')
    _report(f'integrate[{fname}]', res)
    assert res['a_flips'] == 0 and res['c_flips'] == 0 and res['e_flips'] == 0, res
    assert res['traj0_a_flips'] == 0, res
    assert res['x_rel'] < 1e-4 and res['traj0_x_rel'] < 1e-4, res
    assert (state['a_t'] != cfg.n_atom_types).all() and (state['e_t'] != cfg.n_bond_types).all()   # no mask tokens left


@pytest.mark.parametrize('tag,name', [('flowmol3_47x8_T250', 'flowmol3'), ('flowmol3_mixed_T250_w2', 'flowmol3'), ('geom_ctmc_mixed_T500', 'geom_ctmc'),
                                      ('flowmol3_geom64_T250', 'flowmol3'), ('flowmol3_geom16_T250_pos128', 'flowmol3'), ('flowmol3_geom16_T250_heads256', 'flowmol3')])
def test_long_horizon_matches_reference_trajectory(golden_dir, tag, name):
    """The product's DEFAULT protocol against the reference itself: free-running trajectories of the reference's own
    CTMCVectorField.integrate at n_timesteps = 250 (test.py:25, flowmol.py:46; 8 x 47 atoms, and a 5/33/60/90-atom batch with all weight
    matrices x2 so that the endpoint prediction moves every atom by several percent per evaluation) and 500 (BASELINE config C5's
    horizon, geom_ctmc model).  Noise is re-drawn from the stored seed on torch's CPU generator in the reference's order.  Every state
    token and every sampled endpoint token of every step must equal the reference's (0 flips over 250 / 500 tempered CTMC steps), the
    coordinates stay within 1e-4 relative (north star) at the end, at every 10th frame and in every per-step per-molecule norm."""
    from flowmol_amd.engine import Engine
    from parity_util import integrate_long_golden
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(golden_dir / f'long_{tag}.npz').items()}
    cfg = presets.PRESETS[name]()
    scale = float(g['weight_scale']) * (float(g['pos_head_scale']) if 'pos_head_scale' in g else 1.0)
    heads = float(g['cat_head_scale']) if 'cat_head_scale' in g else 1.0
    if scale == 1 and heads == 1:
        eng = engine_for(name)[2]
    else:
        eng = Engine(cfg, weights.long_fixture_weights(cfg, g), device='cuda:0', precision='f32')
    res = integrate_long_golden(eng, cfg, g)
    res['categorical_decisions'] = (int(g['T']) - 1) * int(2 * g['a_1'].numel() + g['e_1_upper'].numel())       # tempered argmax + unmask decisions: rows x steps
    _report(f'long[{tag}]', res)
    # Fixtures of up to ~1 M decisions: every STATE token and every sampled endpoint token of every step equals the reference's -- the trajectory
    # is the reference's trajectory.  The 20-M-decision fixture holds a handful of decisions whose two candidates are equal to f32 summation
    # order (measured over five builds: 0-2 sampled tokens; with contraction off one of them is USED at step 113): which way such a near-tie
    # falls depends on the order of the f32 sums, so there the free-running gate is the final state (tokens identical, coordinates 1e-4) with
    # the divergence CONFINED to the tie's molecule (molecules never interact), and test_teacher_forced_decisions_... audits every one of the
    # 20.2 M decisions under the reference's own state and shows that each differing one is such a tie.
    sample_diffs = res['a1_sample_diffs'] + res['c1_sample_diffs'] + res['e1_sample_diffs']
    big = res['categorical_decisions'] > 10_000_000
    assert res['a_flips'] == res['c_flips'] == res['e_flips'] == 0, res
    if big:
        # numeric ceilings next to the molecule count, and the diverging molecules must be the AUDITED near-tie molecules -- 31 (step 113: a charge
        # row's purity 1.8e-7 above the 0.9 threshold) and 58 (step 79: two sampled charge candidates 2.7e-6 apart), the two events of the teacher-forced
        # audit below -- so that a regression in any other molecule cannot hide behind the allowance.  Measured on this library (profiles/r06b_*):
        # molecule 31 only, 350 state tokens over all steps, 106 sampled tokens.
        assert set(res['molecules_with_state_diffs']) <= {31, 58}, res
        assert res['state_token_diffs_all_steps'] <= 1000 and sample_diffs <= 300, res
    else:
        assert res['state_token_diffs_all_steps'] == 0 and sample_diffs == 0, res
    assert res['x_rel'] < 1e-4 and res['x_frames_rel'] < 1e-4 and res['x_norm_rel'] < 1e-4 and res['x1_norm_rel'] < 1e-4, res
    if scale > 1:
        assert res['mean_rel_move'] > 0.02, res          # all weights x2 / the position heads x128: the coordinates really depend on the network's arithmetic
    if heads > 1:
        # the trained-model regime of the categorical heads: head logit gaps of tens, so most classes of the tempered
        # distribution softmax(log p / 0.05) are EXACTLY 0, rows with p == 1.0, exact zeros (log 0 = -inf) and denormals in p, near-one-hot
        # self-conditioning inputs -- over a free-running 250-step trajectory of the reference (ctmc_vector_field.py:349-357,430-457), every state and
        # sampled token of every step (asserted above: a 4.7-M-decision fixture takes the exact branch)
        # (the regime itself is measured on the device's probabilities in test_teacher_forced_decisions_...[heads256])
        assert res['state_token_diffs_all_steps'] == 0 and sample_diffs == 0, res


def test_long_horizon_64_molecules_without_the_pair_slab(golden_dir):
    """The 20-M-decision reference trajectory with the pair-slab hoist switched OFF (fm_config.pair_slab = -1; canonical arithmetic computes the slab in
    every self-conditioned evaluation, whatever the batch size): same gate as the default path -- the final tokens and coordinates, the diverging
    molecules confined to the audited near-ties -- so the other summation order (one K = 200 chain instead of slab + K = 40) is covered over
    the full horizon, not only per evaluation."""
    from flowmol_amd.engine import Engine
    from parity_util import integrate_long_golden
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(golden_dir / 'long_flowmol3_geom64_T250.npz').items()}
    cfg = presets.flowmol3()
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device='cuda:0', precision='f32', tuning={'pair_slab': -1})
    res = integrate_long_golden(eng, cfg, g)
    res['categorical_decisions'] = (int(g['T']) - 1) * int(2 * g['a_1'].numel() + g['e_1_upper'].numel())
    _report('long[flowmol3_geom64_T250, pair_slab=-1]', res)
    assert res['a_flips'] == res['c_flips'] == res['e_flips'] == 0 and set(res['molecules_with_state_diffs']) <= {31, 58}, res
    assert res['state_token_diffs_all_steps'] <= 1000 and res['a1_sample_diffs'] + res['c1_sample_diffs'] + res['e1_sample_diffs'] <= 300, res
    assert res['x_rel'] < 1e-4 and res['x_frames_rel'] < 1e-4 and res['x_norm_rel'] < 1e-4, res
    eng.close()


@pytest.mark.parametrize('tag,tuning', [('flowmol3_geom64_T250', {}), ('flowmol3_geom64_T250', {'pair_slab': -1}), ('flowmol3_geom16_T250_pos128', {}),
                                        ('flowmol3_geom16_T250_heads256', {})])
def test_teacher_forced_decisions_differ_from_the_reference_only_at_near_ties(golden_dir, tag, tuning):
    """"Bit-exact categorical indices" made checkable over 20.2 M decisions: every step is started from the REFERENCE's token
    state (coordinates and self-conditioning input run free), so each of the fixture's decisions -- sampled endpoint token and new state token of
    every row at every step -- is compared under the reference's own preconditions, not only up to the first divergence.  Every differing decision
    must be EXPLAINED (tests/parity_util.py:audit_long_decisions): a sampled token whose two candidates' (p~ / sum) / q lie within 1e-4 of each
    other, or a molecule with a masked row whose purity lies within 5e-5 of the high-confidence threshold (the count h moves by one and with it
    the molecule's unmasking probabilities) -- decisions that f32 summation order decides; anything else fails.  The events are recorded
    (which step, row, candidates, margin): the measured constant of this library instead of a loose bound."""
    from flowmol_amd.engine import Engine
    from parity_util import audit_long_decisions, integrate_long_teacher_forced
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(golden_dir / f'long_{tag}.npz').items()}
    cfg = presets.flowmol3()
    eng = Engine(cfg, weights.long_fixture_weights(cfg, g), device='cuda:0', precision='f32', tuning=tuning)
    traj, probs = integrate_long_teacher_forced(eng, cfg, g)
    res = audit_long_decisions(cfg, g, traj, probs)
    _report(f'teacher_forced_audit[{tag},{tuning}]', {k: v for k, v in res.items()})
    assert not res['unexplained'], res['unexplained'][:5]
    # the measured constants of this library (profiles/r06b_gpu_parity_report.jsonl; the same two events as round 5's pair-slab path): of the 20,185,683 decisions
    # of the 64-molecule fixture TWO differ on the default (canonical: pair slab in every evaluation) path -- step 113, a charge row of molecule 31 whose purity
    # sits 1.8e-7 (3 ulp) above the 0.9 threshold, and one sampled charge token of molecule 58 at step 79 (margin 2.7e-6) -- at most those two without the slab;
    # none of the 4,733,490 decisions of the position-heads fixture.  The arithmetic is deterministic and, since round 6, independent of the batch a
    # molecule sits in, so these are constants of the LIBRARY, not of (library, batch).
    if 'heads' in tag:
        # what the fixture is for: the device's OWN endpoint probabilities over the whole horizon are in the trained-model regime -- most
        # classes of the tempered distribution softmax(log p / 0.05) exactly 0, rows with p == 1.0, exact zeros (log 0 = -inf in the CTMC kernel) and denormals
        regime = {}
        for k in 'ace':
            p_ = probs[k]
            regime[k] = {'p_zero_frac': float((p_ == 0).float().mean()), 'p_one_rows_frac': float((p_.max(-1).values == 1.0).float().mean()),
                         'p_denormal_frac': float(((p_ > 0) & (p_ < 1.1754944e-38)).float().mean()),
                         'tempered_zero_frac': float((torch.softmax(torch.log(p_) / 0.05, -1) == 0).float().mean())}
        _report(f'head_regime[{tag}]', regime)
        assert all(regime[k]['tempered_zero_frac'] > 0.5 for k in 'ace'), regime
        assert regime['e']['p_one_rows_frac'] > 0.1 and max(regime[k]['p_zero_frac'] for k in 'ace') > 0.01, regime
    assert len(res['events']) <= (0 if 'geom16' in tag else 2), res['events']
    # ... and WHICH near-ties: molecule 31 (the purity 1-3 ulp from the 0.9 threshold) on both paths, plus one sampled token whose two candidates lie 2-3e-6
    # apart -- molecule 58 (step 79) with the pair slab, molecule 28 (step 11) without (profiles/r06c_gpu_parity_report.jsonl)
    assert {ev['molecule'] for ev in res['events']} <= ({31, 28} if tuning else {31, 58}), res['events']
    x = traj['x'][-1].cpu()
    assert float((x - g['x_1']).abs().max() / g['x_1'].abs().max()) < 1e-4
    eng.close()
    del traj, probs
    torch.cuda.empty_cache()


@pytest.mark.parametrize('fname,dfm_type', [('integrate_qm9_gat.npz', 'gat'), ('integrate_qm9_sched.npz', 'campbell')])
def test_integrator_variants_match_reference_golden(golden_dir, fname, dfm_type):
    """SURVEY 8f rank 4 on the GPU: non-uniform tspan, 'decay' temperature schedule, inv_temp_func, and dfm_type
    'gat' with the 'beta' forward weight (ctmc_vector_field.py:71-95, 287-340, 463-510) vs the reference's own run."""
    from parity_util import integrate_variant_golden
    cfg, sd, eng, orc = engine_for('qm9')
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / fname).items()}
    res = integrate_variant_golden(eng, cfg, g, dfm_type, device='cuda:0')
    _report(f'integrate_variant[{fname}]', res)
    assert res['a_flips'] == 0 and res['c_flips'] == 0 and res['e_flips'] == 0, res
    assert res['traj0_a_flips'] == 0 and res['traj0_a1_flips'] == 0, res
    assert res['x_rel'] < 1e-4 and res['traj0_x_rel'] < 1e-4, res


@pytest.mark.parametrize('tag,dataset,arom,fake', [('kek', 'geom_full_kekulized', False, True), ('arom', 'geom_5_aromatic', True, False)])
def test_stability_kernel_matches_reference_verdicts(golden_dir, tag, dataset, arom, fake):
    """device valence-stability / connectivity counts vs the reference's check_stability verdicts."""
    import dataclasses
    from flowmol_amd import _lib
    from flowmol_amd.engine import Engine
    from parity_util import stability_compare
    cfg = presets.flowmol3()
    if arom:
        cfg = dataclasses.replace(cfg, fake_atoms=False, n_bond_types=5, explicit_aromaticity=True)
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / 'stability.npz').items()}
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device='cuda:0', lib=_lib.get_lib())
    assert stability_compare(eng, g, tag, dataset, arom, fake) == []


def test_ctmc_step_teacher_forced_bit_exact():
    """Given the oracle's probabilities and the same noise, the sampled indices are bit-exact
    (incl. purity-sampling edge cases: hc=0 branch, last step)."""
    from flowmol_amd.engine import StepNoise, make_step_plan
    cfg, sd, eng, orc = engine_for('flowmol3')
    n_atoms = torch.tensor([12, 30, 5, 47, 9, 21])
    eng.bind(n_atoms)
    batch = cpu_ref.build_batch(n_atoms)
    gen = torch.Generator().manual_seed(9)
    N, U = eng.N, eng.U
    total = 0
    for case, (hc, last, eta, frac) in enumerate([(0.9, False, 30.0, 0.5), (0.9, True, 30.0, 0.2), (0.0, False, 10.0, 0.5), (0.9, False, 30.0, 1.0)]):
        from parity_util import rand_tokens, onehots
        a = rand_tokens(N, cfg.n_atom_types, frac, gen); c = rand_tokens(N, cfg.n_charges, frac, gen); eu = rand_tokens(U, cfg.n_bond_types, frac, gen)
        x = torch.randn(N, 3, generator=gen)
        sharp = 8.0 if case != 3 else 0.5
        dst = {'x': torch.randn(N, 3, generator=gen), 'a': torch.softmax(torch.randn(N, cfg.n_atom_types, generator=gen) * sharp, -1),
               'c': torch.softmax(torch.randn(N, cfg.n_charges, generator=gen) * sharp, -1),
               'e': torch.softmax(torch.randn(U, cfg.n_bond_types, generator=gen) * sharp, -1)}
        T = 250
        s_idx = T - 1 if last else 100
        plan = make_step_plan(T, eta, hc, cfg.cat_temperature)
        sc = plan.scalars[s_idx - 1]
        assert bool(sc.last_step) == last
        # oracle
        t = plan.t
        al, alp = cpu_ref.alpha_tables(t)
        a1h, c1h, e1h = onehots(cfg, batch, a, c, eu)
        rec = cpu_ref.RecordingNoise()
        torch.manual_seed(100 + case)

        class FixedDst(cpu_ref.OracleVF):
            def forward(self, *a_, **k_):
                return dst
        o2 = FixedDst(cfg, sd)
        new, _ = o2.step(batch, {'x_t': x, 'a_t': a1h, 'c_t': c1h, 'e_t': e1h}, t[s_idx], t[s_idx - 1], al[s_idx - 1], alp[s_idx - 1],
                         prev=None, eta=eta, hc_thresh=hc, last_step=last, noise=rec)
        nz, used = StepNoise.from_tape(rec.tape, 0, last, 'cuda:0')
        assert used == len(rec.tape)
        state = eng.make_state(x, a, c, eu)
        ddev = {k: v.to('cuda:0').contiguous() for k, v in dst.items()}
        smp = {'a1': torch.zeros(N, dtype=torch.int32, device='cuda:0'), 'c1': torch.zeros(N, dtype=torch.int32, device='cuda:0'),
               'e1': torch.zeros(U, dtype=torch.int32, device='cuda:0')}
        eng.ctmc_step(state, ddev, nz, sc, smp)
        eng.synchronize()
        m = batch.upper_edge_mask
        flips = int((state['a_t'].cpu().long() != new['a_t'].argmax(-1)).sum() + (state['c_t'].cpu().long() != new['c_t'].argmax(-1)).sum()
                    + (state['e_t'].cpu().long() != new['e_t'][m].argmax(-1)).sum())
        flips1 = int((smp['a1'].cpu().long() != new['a_1_pred'].argmax(-1)).sum() + (smp['e1'].cpu().long() != new['e_1_pred'][m].argmax(-1)).sum())
        xerr = float((state['x_t'].cpu() - new['x_t']).abs().max())
        _report(f'ctmc_step[{case}]', {'flips': flips, 'flips_x1': flips1, 'x_abs': xerr})
        assert flips == 0 and flips1 == 0, (case, flips, flips1)
        assert xerr == 0.0, xerr        # the Euler step uses the same f32 operations
        total += 1
    assert total == 4


def test_sample_api_and_determinism():
    """flowmol.load_pretrained()/sample_random_sizes()-style API on synthetic weights: shapes, no mask tokens,
    same seed -> same molecules; upper/lower symmetry is structural (edge state is per pair)."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('qm9').cuda().eval()
    torch.manual_seed(5)
    mols = model.sample_random_sizes(6, n_timesteps=6)
    torch.manual_seed(5)
    mols2 = model.sample_random_sizes(6, n_timesteps=6)
    assert len(mols) == 6
    for m1, m2 in zip(mols, mols2):
        assert m1.positions.shape[1] == 3 and torch.isfinite(m1.positions).all()
        assert torch.equal(m1.positions, m2.positions) and m1.atom_types == m2.atom_types
        assert torch.equal(m1.bond_types, m2.bond_types)
        assert 'Se' not in m1.atom_types and 'Sn' not in m1.atom_types       # no mask / fake atoms in the result
        assert (m1.bond_types >= 1).all() and (m1.bond_types <= 3).all()
        assert m1.num_atoms == len(m1.atom_types) == m1.positions.shape[0]
    # trajectories
    torch.manual_seed(5)
    mt = model.sample(torch.tensor([7, 4]), n_timesteps=5, xt_traj=True, ep_traj=True)
    assert mt[0].traj_frames['x'].shape == (5, 7, 3) and mt[0].traj_frames['x_1_pred'].shape == (4, 7, 3)
    assert mt[1].traj_frames['e'].shape == (5, 6)


def test_full_size_properties():
    """BASELINE config C3 shape at reduced molecule count (64 x 47 atoms): finite outputs, normalised
    probabilities, per-molecule zero centre of mass, and batch-composition independence (a molecule's result
    does not depend on its neighbours in the batch, up to summation order)."""
    cfg, sd, eng, orc = engine_for('flowmol3')
    gen = torch.Generator().manual_seed(1)
    n = 47
    B = 64

    def run(order):
        n_atoms = torch.full((len(order),), n)
        eng.bind(n_atoms)
        xs = torch.stack([torch.randn(n, 3, generator=torch.Generator().manual_seed(100 + i)) for i in order]).reshape(-1, 3)
        st = eng.prior_state(xs)
        out = eng.forward(st, 0.0, prev=None, bootstrap=True, remove_com=True)
        eng.synchronize()
        return {k: v.cpu() for k, v in out.items()}
    o1 = run(list(range(B)))
    for k in 'xace':
        assert torch.isfinite(o1[k]).all()
    assert torch.allclose(o1['x'].reshape(B, n, 3).mean(1), torch.zeros(B, 3), atol=2e-6)
    o2 = run([5, 3])
    assert torch.allclose(o2['x'][:n], o1['x'][5 * n:6 * n], rtol=0, atol=1e-5)
    U = n * (n - 1) // 2
    assert torch.allclose(o2['e'][U:], o1['e'][3 * U:4 * U], rtol=0, atol=1e-5)


def test_c5_mixed_sizes_trajectory_matches_oracle():
    """BASELINE config C5 shape (geom_full_kekulized model, mixed 5-60 atoms, trajectory dump) at reduced T:
    free-running trajectory with recorded noise vs the oracle, every frame."""
    from flowmol_amd.engine import StepNoise, make_step_plan
    cfg, sd, eng, orc = engine_for('geom_ctmc')
    g = torch.Generator().manual_seed(0)
    n_atoms = torch.randint(5, 61, (8,), generator=g)
    batch = cpu_ref.build_batch(n_atoms)
    torch.manual_seed(3)
    prior = orc.sample_prior(batch)
    T = 12
    rec = cpu_ref.RecordingNoise()
    with torch.no_grad():
        ref, frames = orc.integrate(batch, prior, T, noise=rec, visualize=True)
    eng.bind(n_atoms)
    plan = make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cfg.cat_temperature)
    state = eng.prior_state(prior['x_0'])
    pos = [0]

    def noise_for_step(i, last):
        nz, pos[0] = StepNoise.from_tape(rec.tape, pos[0], last, 'cuda:0')
        return nz
    traj = {'x': torch.zeros(T - 1, eng.N, 3, device='cuda:0'), 'a': torch.zeros(T - 1, eng.N, dtype=torch.int32, device='cuda:0'),
            'e': torch.zeros(T - 1, eng.U, dtype=torch.int32, device='cuda:0'), 'x1': torch.zeros(T - 1, eng.N, 3, device='cuda:0')}
    eng.integrate(state, plan, noise_for_step, chunk=5, traj=traj)
    m = batch.upper_edge_mask
    ref_x = torch.stack(frames['x'][1:])
    ref_a = torch.stack([f.argmax(-1) for f in frames['a'][1:]])
    ref_e = torch.stack([f[m].argmax(-1) for f in frames['e'][1:]])
    ref_x1 = torch.stack(frames['x_1_pred'])
    res = {'a_flips': int((traj['a'].cpu().long() != ref_a).sum()), 'e_flips': int((traj['e'].cpu().long() != ref_e).sum()),
           'x_rel': float((traj['x'].cpu() - ref_x).abs().max() / ref_x.abs().max()),
           'x1_rel': float((traj['x1'].cpu() - ref_x1).abs().max() / ref_x1.abs().max())}
    _report('c5_traj', res)
    assert res['a_flips'] == 0 and res['e_flips'] == 0 and res['x_rel'] < 1e-4 and res['x1_rel'] < 1e-4, res


def test_cli_on_gpu(tmp_path):
    from flowmol_amd import cli
    args = cli.parse_args(['--preset', 'qm9', '--n_mols', '5', '--n_timesteps', '8', '--max_batch_size', '3', '--seed', '1',
                           '--output_file', str(tmp_path / 'out.sdf')])
    mols, t = cli.run(args)
    assert len(mols) == 5 and (tmp_path / 'out.sdf').read_text().count('$$$$') == 5


def test_c2_full_size_qm9_properties():
    """BASELINE config C2 at full size (QM9 model, 256 molecules, n_timesteps=100): size-independent properties --
    finite coordinates, no mask tokens left, result independent of how the batch is split (same per-molecule noise)."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('qm9').cuda().eval()
    torch.manual_seed(11)
    n_atoms = model.sample_n_atoms(256)
    torch.manual_seed(12)
    out, _ = model.sample(n_atoms, n_timesteps=100, return_tensors=True)
    assert torch.isfinite(out['x']).all()
    assert (out['a'] != model.cfg.n_atom_types).all() and (out['c'] != model.cfg.n_charges).all() and (out['e'] != model.cfg.n_bond_types).all()
    torch.manual_seed(12)
    out2, _ = model.sample(n_atoms, n_timesteps=100, return_tensors=True)
    for k in 'xace':
        assert torch.equal(out[k], out2[k])          # deterministic given the seed


def test_c3_full_size_geom_properties():
    """BASELINE config C3 at full size (flowmol3, 1024 molecules x 47 atoms, n_timesteps=250, ~25 s on one MI355X):
    finite, no mask tokens, zero per-molecule centre of mass of the final coordinates' endpoint prediction."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
    torch.manual_seed(21)
    out, n_atoms = model.sample(torch.full((1024,), 47), n_timesteps=250, return_tensors=True)
    assert torch.isfinite(out['x']).all()
    assert (out['a'] != model.cfg.n_atom_types).all() and (out['e'] != model.cfg.n_bond_types).all()
    # x_1 == last endpoint prediction (Appendix C.10), which is COM-free per molecule
    com = out['x'].reshape(1024, 47, 3).mean(1)
    assert com.abs().max() < 1e-3


@pytest.mark.gpu
def test_shards_with_replicated_noise_equal_the_full_batch():
    """SURVEY.md §8e on one GPU: the three shards of an LPT partition, each integrated alone with the full batch's
    noise rows (what sample_distributed(noise='replicated') does per rank), reproduce the unsharded run BIT FOR BIT --
    tokens and coordinates (canonical arithmetic, fm_config.canonical: the f32 summation order of a molecule is a function
    of the molecule alone, as every reduction of the reference is per molecule: gvp.py:491-492, ctmc_utils.py:11-20,
    vector_field.py:347-350)."""
    import flowmol_amd as flowmol
    from flowmol_amd import shard
    model = flowmol.FlowMol.from_preset('flowmol3').cuda()
    sizes = torch.tensor([12, 30, 5, 47, 9, 21, 33, 2, 16, 40, 7, 25])
    torch.manual_seed(5)
    full, _ = model.sample(sizes, n_timesteps=6, return_tensors=True)
    pairs = sizes * (sizes - 1) // 2
    noff, poff = torch.cumsum(sizes, 0) - sizes, torch.cumsum(pairs, 0) - pairs
    for mine in shard.partition_lpt(sizes, 3):
        rows = (int(sizes.sum()), int(pairs.sum()), shard._ranges(noff[mine], sizes[mine]).cuda(), shard._ranges(poff[mine], pairs[mine]).cuda())
        torch.manual_seed(5)
        part, _ = model.sample(sizes[mine], n_timesteps=6, return_tensors=True, _rows=rows)
        nidx, pidx = rows[2].cpu(), rows[3].cpu()
        assert torch.equal(part['a'], full['a'][nidx]) and torch.equal(part['c'], full['c'][nidx])
        assert torch.equal(part['e'], full['e'][pidx])
        assert torch.equal(part['x'], full['x'][nidx])


def _gloo_rank_on_shared_gpu(rank, world, port, sizes, T, seed, q):
    """One of `world` processes sharing the box's single GPU: its own HIP context, engine and workspace; process group over gloo
    (RCCL refuses two ranks on one device), the data path's one collective on device tensors."""
    import os
    os.environ.update({'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'HSA_ENABLE_IPC_MODE_LEGACY': '0'})
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import flowmol_amd as flowmol
        from flowmol_amd import shard
        model = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
        n_atoms = torch.tensor(sizes)
        out = {}
        for mode in ('replicated', 'philox'):
            torch.manual_seed(seed)
            full, _ = model.sample_distributed(n_atoms, n_timesteps=T, return_tensors=True, noise=mode)
            out[mode] = {k: v.numpy().copy() for k, v in full.items()}
        mine = n_atoms[shard.partition_lpt(n_atoms, world)[rank]]
        q.put((rank, out, int(mine.numel()), int(mine.sum() * 14 + (mine * (mine - 1) // 2).sum())))
    except Exception as e:          # the parent must not wait for its timeout
        q.put((rank, repr(e), 0, 0))
    finally:
        dist.destroy_process_group()


def test_eight_rank_process_group_on_one_gpu_equals_single_process_sample():
    """BASELINE configs[3]'s process layout as far as one GPU allows (VERDICT r3 #1b): EIGHT ranks (one process each, gloo process group,
    all on this box's one MI355X) run FlowMol.sample_distributed on a 512-molecule job with sizes drawn from the shipped GEOM-drugs
    histogram: LPT parts of unequal length, packed payloads of odd sizes, one all-gather.  noise='replicated' must reproduce the
    single-process sample() of the same seed BIT FOR BIT (tokens and coordinates: canonical arithmetic); noise='philox' -- what a
    throughput run uses -- must reproduce the single-process Philox sample bit for bit too (per-molecule streams keyed by the original
    molecule index).  What stays untested after this is only the RCCL/xGMI transport between eight devices."""
    import socket
    import torch.multiprocessing as mp
    import flowmol_amd as flowmol
    from flowmol_amd.model import load_n_atoms_hist
    from flowmol_amd import shard
    world, T, seed = 8, 8, 41
    vals, counts = load_n_atoms_hist('geom_full_kekulized')
    n_atoms = vals[torch.multinomial(counts.double(), 64 * world, replacement=True, generator=torch.Generator().manual_seed(4))]
    parts = shard.partition_lpt(n_atoms, world)
    assert len({len(p_) for p_ in parts}) > 1                                  # unequal shard lengths
    model = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
    single = {}
    torch.manual_seed(seed)
    single['replicated'], _ = model.sample(n_atoms, n_timesteps=T, return_tensors=True)
    torch.manual_seed(seed)
    single['philox'], _ = model.sample(n_atoms, n_timesteps=T, return_tensors=True, rng='philox')
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank_on_shared_gpu, args=(r, world, port, n_atoms.tolist(), T, seed, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    try:
        got = [q.get(timeout=900) for _ in procs]
    finally:
        for p_ in procs:
            p_.join(timeout=120)
            if p_.is_alive():
                p_.kill()
    errs = [g_ for g_ in got if isinstance(g_[1], str)]
    assert not errs, errs
    res = {r: d for r, d, _, _ in got}
    payloads = sorted(pb for _, _, _, pb in got)
    rep = {'ranks': world, 'molecules': int(n_atoms.numel()), 'molecules_per_rank': sorted(m for _, _, m, _ in got), 'payload_bytes_min_max': [payloads[0], payloads[-1]]}
    for mode in ('replicated', 'philox'):
        for r in range(1, world):
            for k in 'xace':
                assert np.array_equal(res[0][mode][k], res[r][mode][k]), (mode, r, k)          # every rank holds the same gathered batch
        full = {k: torch.from_numpy(v) for k, v in res[0][mode].items()}
        for k in 'ace':
            assert torch.equal(full[k], single[mode][k]), (mode, k, int((full[k] != single[mode][k]).sum()))
        rep[f'{mode}_x_max_abs_diff'] = float((full['x'] - single[mode]['x']).abs().max())
        assert torch.equal(full['x'], single[mode]['x']), (mode, rep[f'{mode}_x_max_abs_diff'])      # canonical arithmetic: bit for bit, whatever the sharding
    _report('eight_ranks_one_gpu', rep)


def _run_bench_ranks(world, backend, extra=(), full=True):
    """`python bench.py --gpus <world> ...` as a multi-GPU bench is started, with --full unless full=False (bench.py launches its ranks itself when no
    launcher environment is set); returns the parsed JSON line."""
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
    if backend == 'gloo':
        env['FM_BENCH_BACKEND'] = 'gloo'
    else:
        env.pop('FM_BENCH_BACKEND', None)
    cmd = [sys.executable, str(root / 'bench.py'), '--gpus', str(world), '--steps', '4', '--warmup', '2', '--mols-per-gpu', '32', *(['--full'] if full else []),
           '--no-cpu-baseline', '--no-api-e2e', *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500, cwd='/tmp')
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]             # rank 0 prints ONE line
    return json.loads(lines[0])


def _check_multi_gpu_line(d, world, backend):
    p = d['multi_gpu_parity']
    for k in ('token_diffs', 'x_rel', 'philox_token_diffs', 'world_size', 'distinct_pci_devices', 'rccl_version', 'all_gather_bytes', 'ranks_hold_the_same_batch', 'ok'):
        assert k in p, k
    assert p['ok'] and p['token_diffs'] == 0 and p['philox_token_diffs'] == 0 and p['x_rel'] < 1e-4 and p['philox_x_rel'] < 1e-4, p
    assert p['canonical'] and p['x_bit_identical'] and p['philox_x_bit_identical'] and p['x_rel'] == 0.0, p      # canonical arithmetic: sharding changes no bit
    assert p['world_size'] == world and p['molecules'] == 8 * world and p['n_timesteps'] == 12 and p['ranks_hold_the_same_batch']
    assert p['all_gather_bytes'] == world * p['all_gather_slot_bytes'] and p['backend'] == backend
    assert d['n_gpus'] == world and d['config']['global_molecules'] == 32 * world and d['config']['finite']
    assert d['config']['process_group']['size'] == world and d['config']['process_group']['backend'] == backend
    assert len(d['per_rank_ms_per_step']) == world and d['final_gather_ms'] is not None
    w = d['ms_per_step_windows']
    assert w['windows'] == 4 and w['min'] <= w['median'] <= w['max']
    return p


def test_bench_multi_gpu_line_carries_parity_block():
    """`bench.py --gpus N --full` proves itself before it times anything.  Here the whole
    command -- self-launch of 8 ranks, process group, the parity block BEFORE the timed region (sample_distributed in the replicated and the
    Philox noise mode on the ranks vs the single-process sample of the same seed on rank 0: 0 differing tokens, coordinates within 1e-4), the
    timed steps with their four sub-windows, the one all-gather -- runs with 8 ranks sharing this box's one MI355X (FM_BENCH_BACKEND=gloo: RCCL
    refuses two ranks on one device), and the line carries the block."""
    p = _check_multi_gpu_line(_run_bench_ranks(8, 'gloo'), 8, 'gloo')
    assert p['distinct_pci_devices'] == 1                      # eight ranks, one device: what this box has
    _report('bench_multi_gpu_parity[8 gloo ranks on one GPU]', p)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs at least two GPUs (RCCL between distinct devices)')
@pytest.mark.parametrize('which', ['two', 'all'])
def test_bench_multi_gpu_line_over_rccl_between_devices(which):
    """Switches itself on where the box has more than one GPU (the builder's boxes have one): the same command over real RCCL with 2 ranks and
    with one rank per visible device -- BASELINE configs[3]'s transport (xGMI) -- distinct PCI devices recorded in the block."""
    world = 2 if which == 'two' else torch.cuda.device_count()
    if which == 'all' and world == 2:
        pytest.skip('two devices: covered by the two-rank case')
    p = _check_multi_gpu_line(_run_bench_ranks(world, 'nccl'), world, 'nccl')
    assert p['distinct_pci_devices'] == world and p['rccl_version']
    _report(f'bench_multi_gpu_parity[{world} nccl ranks]', p)


def _replay_bench_leg(mols, n_steps, rank=0, n_atoms=47, T=250, device='cuda:0', lib=None):
    """bench.py's leg rebuilt from its seeds with the engine alone (not through bench.py): flowmol3, synthetic weights (seed 0), `mols` molecules of
    `n_atoms` atoms, prior positions from a generator seeded 1 + rank, torch noise from one seeded 2 + rank, `n_steps` integration steps from the
    prior.  Returns the state and the endpoint prediction after the last step as float32 arrays, named as --dump-outputs names them."""
    from flowmol_amd.engine import Engine, IntegrationRun, StepNoise, make_step_plan
    cfg = presets.flowmol3()
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device=device, lib=lib)
    eng.bind(torch.full((mols,), n_atoms, dtype=torch.int64))
    plan = make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cfg.cat_temperature)
    gen, g0 = torch.Generator(device=device), torch.Generator(device=device)
    gen.manual_seed(2 + rank)
    g0.manual_seed(1 + rank)
    x0 = torch.randn(eng.N, 3, device=device, generator=g0)
    eng.remove_com(x0)
    state = eng.prior_state(x0)
    run = IntegrationRun(eng, state, plan, lambda i, last: StepNoise.draw(eng.N, eng.U, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types, last, device,
                                                                          generator=gen))
    run.run(0, n_steps)
    eng.synchronize()
    out = {k: state[f'{k}_t'] for k in 'xace'} | {f'pred_{k}': v for k, v in run.last_dst().items()}
    out = {k: v.to('cpu', torch.float32).numpy() for k, v in out.items()}
    eng.close()
    return out


def test_bench_plain_line_and_dumped_outputs_repeat(tmp_path):
    """A plain `bench.py --gpus 1` run (no --full) prints one compact line with the headline fields, times exactly --steps steps and carries
    none of the --full figures; --dump-outputs writes the last timed step's state and endpoint prediction -- equal to the same trajectory
    rebuilt from the seeds and advanced warm-up + timed steps -- and a second run of the same arguments writes the same arrays bit for bit."""
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f'run{i}'
        cmd = [sys.executable, str(root / 'bench.py'), '--gpus', '1', '--steps', '5', '--warmup', '2', '--mols-per-gpu', '16', '--dump-outputs', str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        out = [l for l in r.stdout.splitlines() if l.startswith('{')]
        assert len(out) == 1, r.stdout[-2000:]
        assert len(out[0]) < 4096, len(out[0])
        lines.append(json.loads(out[0]))
        dumps.append({p.stem: np.load(p) for p in sorted(d.glob('*.npy'))})
    line = lines[0]
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, k
    assert line['steps'] == 5 and line['warmup'] == 2 and sum(line['ms_per_step_windows']['steps_per_window']) == 5
    assert line['ms_per_step'] > 0 and line['value'] > 0 and line['unit'] == 'molecules/s' and line['higher_is_better'] and line['config']['finite']
    for k in ('kernels', 'roofline', 'secondary', 'api_end_to_end', 'cpu_baseline'):
        assert k not in line, k
    N, U = 16 * 47, 16 * 47 * 46 // 2
    assert set(dumps[0]) == {'x', 'a', 'c', 'e', 'pred_x', 'pred_a', 'pred_c', 'pred_e'} and line['outputs']['row_sample'] is None
    assert dumps[0]['x'].shape == (N, 3) and dumps[0]['a'].shape == (N,) and dumps[0]['e'].shape == (U,) and dumps[0]['pred_e'].shape[0] == U
    for k, v in dumps[0].items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        assert np.array_equal(v, dumps[1][k]), k
    want = _replay_bench_leg(16, 2 + 5)
    for k, v in want.items():
        assert np.array_equal(dumps[0][k], v), k


def test_bench_plain_multi_rank_line_and_dumped_batch(tmp_path):
    """A plain `bench.py --gpus 2` (two gloo ranks sharing the one GPU, no --full): no parity block, both ranks timed, and --dump-outputs
    (written by rank 0) holds the gathered batch -- rank 0's molecules, then rank 1's, each equal to its rank's trajectory rebuilt from the seeds."""
    out = tmp_path / 'out'
    d = _run_bench_ranks(2, 'gloo', extra=('--dump-outputs', str(out)), full=False)
    assert d['n_gpus'] == 2 and d['multi_gpu_parity'] is None and not d['config']['full'] and 'value_geom_size_dist' not in d
    assert len(d['per_rank_ms_per_step']) == 2 and d['final_gather_ms'] is not None and d['config']['process_group']['backend'] == 'gloo'
    got = {p_.stem: np.load(p_) for p_ in sorted(out.glob('*.npy'))}
    assert set(got) == set('xace') and d['outputs']['row_sample'] is None
    ranks = [_replay_bench_leg(32, 2 + 4, rank=r) for r in range(2)]
    for k in 'xace':
        assert got[k].dtype == np.float32 and np.array_equal(got[k], np.concatenate([r_[k] for r_ in ranks])), k


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs at least two GPUs (RCCL between distinct devices)')
def test_sample_distributed_over_rccl_between_devices():
    """FlowMol.sample_distributed over real RCCL, one process per device: a 16-molecule-per-rank GEOM-distributed job in the replicated noise
    mode equals the single-process sample (tokens identical) on every rank."""
    import socket
    import torch.multiprocessing as mp
    import flowmol_amd as flowmol
    from flowmol_amd.model import load_n_atoms_hist
    world, T, seed = torch.cuda.device_count(), 8, 43
    vals, counts = load_n_atoms_hist('geom_full_kekulized')
    n_atoms = vals[torch.multinomial(counts.double(), 16 * world, replacement=True, generator=torch.Generator().manual_seed(5))]
    model = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
    torch.manual_seed(seed)
    single, _ = model.sample(n_atoms, n_timesteps=T, return_tensors=True)
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_nccl_rank_on_own_gpu, args=(r, world, port, n_atoms.tolist(), T, seed, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    try:
        got = [q.get(timeout=900) for _ in procs]
    finally:
        for p_ in procs:
            p_.join(timeout=120)
            if p_.is_alive():
                p_.kill()
    assert not [g_ for g_ in got if isinstance(g_[1], str)], got
    for _, full in got:
        for k in 'ace':
            assert np.array_equal(full[k], single[k].numpy()), k
        np.testing.assert_allclose(full['x'], single['x'].numpy(), rtol=1e-5, atol=1e-5)


def _nccl_rank_on_own_gpu(rank, world, port, sizes, T, seed, q):
    import os as _os
    _os.environ.update({'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'HSA_ENABLE_IPC_MODE_LEGACY': '0'})
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', rank))
    try:
        import flowmol_amd as flowmol
        model = flowmol.FlowMol.from_preset('flowmol3').to(f'cuda:{rank}').eval()
        torch.manual_seed(seed)
        full, _ = model.sample_distributed(torch.tensor(sizes), n_timesteps=T, return_tensors=True, noise='replicated')
        q.put((rank, {k: v.numpy().copy() for k, v in full.items()}))
    except Exception as e:
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


# ----------------------------------------------------------------------------------------------------------------------
# round 2: edge cases by construction, bench-size parity, packaging / CLI content, RCCL
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [0, 1, 2, 3, 4])
def test_ctmc_step_reference_edge_cases_bit_exact(golden_dir, case):
    """fm_ctmc_step on the fixture generated by the reference's OWN CTMCVectorField.step (fixed endpoint prediction;
    ctmc_vector_field.py:287-461, ctmc_utils.py:4-34): molecules with h = 0, m = h and m = 0, a one-pair molecule, an exact-zero
    probability, the hc = 0 branch and the last step -- by construction, not by chance.  Tokens, sampled endpoints and the
    Euler update bit-exact."""
    from parity_util import ctmc_step_golden
    cfg, sd, eng, orc = engine_for('flowmol3')
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / 'ctmc_step.npz').items()}
    res = ctmc_step_golden(eng, cfg, g, case, device='cuda:0')
    _report(f'ctmc_step_golden[{case}]', res)
    assert all(v == 0 for v in res.values()), res


def test_misc_campbell_fixture_through_the_kernel(golden_dir):
    """tests/golden/misc.npz ctmc.{0..3} (the reference's campbell_step on ALREADY tempered probabilities) through the HIP
    kernel: the kernel always tempers (softmax(log p / T), as step() does), so the fixture's p is fed with T = 1, which is the
    identity up to one rounding of log/exp -- decisions must still all agree (rows are the atoms of 2..9-atom molecules)."""
    from flowmol_amd.engine import StepNoise, make_step_plan
    cfg, sd, eng, orc = engine_for('flowmol3')
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / 'misc.npz').items()}
    sizes = g['ctmc.sizes']                                   # rows per molecule: 4, 7, 1, 9, 5 (a 1-atom molecule has no pair)
    eng.bind(sizes)
    N, U = eng.N, eng.U
    gen = torch.Generator().manual_seed(0)
    for case in range(4):
        hc, last, eta, alpha, dt = [float(v) for v in g[f'ctmc.{case}.params']]
        last = bool(last)
        sc = make_step_plan(250, eta, hc, 1.0).scalars[0]
        one, a_i, dt_t = torch.ones(()), torch.tensor(alpha), torch.tensor(dt)
        un = float(torch.clamp(dt_t * (one + eta * a_i) / (1 - a_i), min=0, max=1))
        mk = float(torch.clamp(dt_t * eta, min=0, max=1))
        for k in range(3):
            sc.unmask_prob[k] = un
            sc.mask_prob[k] = mk
        sc.last_step = int(last)
        sc.cat_temperature = 1.0
        nz = StepNoise(q_a=g[f'ctmc.{case}.noise0'].cuda(), u1_a=g[f'ctmc.{case}.noise1'].cuda(),
                       u2_a=None if last else g[f'ctmc.{case}.noise2'].cuda(),
                       q_c=torch.rand(N, cfg.n_charges, generator=gen).cuda() + 0.1, u1_c=torch.rand(N, generator=gen).cuda(), u2_c=torch.rand(N, generator=gen).cuda(),
                       q_e=torch.rand(U, cfg.n_bond_types, generator=gen).cuda() + 0.1, u1_e=torch.rand(U, generator=gen).cuda(), u2_e=torch.rand(U, generator=gen).cuda())
        state = eng.make_state(torch.zeros(N, 3), g['ctmc.xt'], torch.zeros(N, dtype=torch.long), torch.zeros(U, dtype=torch.long))
        dst = {'x': torch.zeros(N, 3).cuda(), 'a': g['ctmc.p'].cuda().contiguous(), 'c': torch.full((N, cfg.n_charges), 1.0 / cfg.n_charges).cuda(),
               'e': torch.full((U, cfg.n_bond_types), 1.0 / cfg.n_bond_types).cuda()}
        smp = {'a1': torch.zeros(N, dtype=torch.int32, device='cuda:0'), 'c1': torch.zeros(N, dtype=torch.int32, device='cuda:0'),
               'e1': torch.zeros(U, dtype=torch.int32, device='cuda:0')}
        eng.ctmc_step(state, dst, nz, sc, smp)
        eng.synchronize()
        assert torch.equal(state['a_t'].cpu().long(), g[f'ctmc.{case}.xt_new']), case
        assert torch.equal(smp['a1'].cpu().long(), g[f'ctmc.{case}.x1']), case


@pytest.mark.parametrize('B,mols', [
    (1024, (0, 127, 128, 600, 1023)),
    # BASELINE configs[3]'s WHOLE job bound on one GPU (VERDICT r3 #1a): 8192 molecules = 385,024 nodes, 17.7 M directed edges, ef = 9.07 GB
    # (31.5 GB workspace: 13.3 GB + the two pair-slab tables this batch size switches on) -- the first oracle comparison past 4 GiB of edge state: the far end of the batch (molecule 8191's ef rows start
    # 9.06 GB into the buffer), both sides of the middle (4095 | 4096), an XCD tile-chunk boundary (553,472 tiles / 8 = 1024 molecules) and
    # the first molecule whose ef rows lie beyond 2^32 bytes (3880).
    (8192, (0, 1023, 1024, 3879, 3880, 4095, 4096, 8191)),
])
def test_full_size_forward_matches_oracle_on_selected_molecules(B, mols):
    """BASELINE configs[2] at FULL batch size (1024 molecules x 47 atoms: 48,128 nodes, 2.2 M directed edges) and configs[3]'s 8192-molecule
    job on ONE GPU: one network evaluation at t = 0.5 with a previous endpoint; the listed molecules (1024: 0, 127 | 128 = either side of the
    first XCD tile-chunk boundary, 69,184 tiles / 8 XCDs = 8,648 tiles = 128 molecules, 600 and 1023) are compared with the oracle run on each
    molecule ALONE, per stage (node state after every conv, positions after every update, the last edge features) and on the outputs --
    norm-wise like the small-batch tests and element-wise (atol + rtol) on the outputs.  Then the same under parity_util.visible_weights() with the
    displacement stages, each molecule's against the gate measured on that molecule (worst error / gate over the molecules must stay below 1); the
    8192-molecule job too: a second engine's 31.5 GB workspace next to the cached one's fits the device several times over."""
    for visible in (False, True):
        _full_size_forward(B, mols, visible)


def _full_size_forward(B, mols, visible):
    cfg, sd, eng, orc = engine_for('flowmol3', visible=visible)
    n = 47
    u = n * (n - 1) // 2
    n_atoms = torch.full((B,), n)
    eng.bind(n_atoms)
    N, U, E = eng.N, eng.U, eng.E
    gen = torch.Generator().manual_seed(77)
    from parity_util import rand_tokens, onehots
    a, c, eu = rand_tokens(N, cfg.n_atom_types, 0.4, gen), rand_tokens(N, cfg.n_charges, 0.4, gen), rand_tokens(U, cfg.n_bond_types, 0.4, gen)
    x = torch.randn(N, 3, generator=gen) * 1.5
    prev = {'x': x + 0.3 * torch.randn(N, 3, generator=gen), 'a': torch.softmax(torch.randn(N, cfg.n_atom_types, generator=gen), -1),
            'c': torch.softmax(torch.randn(N, cfg.n_charges, generator=gen), -1), 'e': torch.softmax(torch.randn(U, cfg.n_bond_types, generator=gen), -1)}
    state = eng.make_state(x, a, c, eu)
    V = cfg.n_vec_channels
    sched = cfg.update_schedule()
    last_upd = max(i for i in range(cfg.n_convs) if sched[i] >= 0)
    bufs = {}
    for i in range(cfg.n_convs):
        bufs[f'conv{i}.s'] = torch.zeros(N, 256, device='cuda:0')
        bufs[f'conv{i}.v'] = torch.zeros(N, 3, V, device='cuda:0')
        if sched[i] >= 0:
            bufs[f'upd{i}.x'] = torch.zeros(N, 3, device='cuda:0')
    bufs[f'upd{last_upd}.ef'] = torch.zeros(E, 128, device='cuda:0')
    out = eng.forward(state, 0.5, prev={k: v.cuda().contiguous() for k, v in prev.items()}, remove_com=True, taps=bufs)
    eng.synchronize()
    worst, yard = {}, {}
    one = torch.tensor([n])
    batch1 = cpu_ref.build_batch(one)
    # internal (destination-major) index of the reference's edge (src, dst) inside one molecule
    src, dst = batch1.src, batch1.dst
    internal = dst * (n - 1) + (src - (src > dst).long())
    if B == 8192:
        assert E * 512 > 2 ** 33 and eng.workspace_bytes > 12 << 30
    for m in mols:
        ns_, ps_ = slice(m * n, (m + 1) * n), slice(m * u, (m + 1) * u)
        a1h, c1h, e1h = onehots(cfg, batch1, a[ns_], c[ns_], eu[ps_])
        orc.taps = {}
        with torch.no_grad():
            ref = orc.forward(batch1, x[ns_], a1h, c1h, e1h, torch.full((1,), 0.5), prev={'x': prev['x'][ns_], 'a': prev['a'][ns_], 'c': prev['c'][ns_], 'e': prev['e'][ps_]},
                              apply_softmax=True, remove_com=True)
        taps_o, orc.taps = orc.taps, None
        if visible:       # displacement stages of this molecule (parity_util.add_dx_stages on both sides), each scored in units of its own gate
            inp = {'batch': batch1, 'x': x[ns_], 'a': a[ns_], 'c': c[ns_], 'eu': eu[ps_], 'prev': {'x': prev['x'][ns_], 'a': prev['a'][ns_], 'c': prev['c'][ns_], 'e': prev['e'][ps_]}}
            upd = [k for k in bufs if k.endswith('.x')]
            got_m = add_dx_stages({**{k: bufs[k][ns_].cpu() for k in upd}, 'out.x': out['x'][ns_].cpu()}, cfg, inp)
            want_m = add_dx_stages({**{k: taps_o[k] for k in upd}, 'out.x': ref['x']}, cfg, inp)
            gates, detail = dx_gates(cfg, sd, one, 0.5, True, inp=inp)
            for k, e in stage_errors({k: v for k, v in got_m.items() if k.endswith('.dx')}, want_m).items():
                worst[k + ' / gate'] = max(worst.get(k + ' / gate', 0.0), e / gates[k] if e == e else float('inf'))
                yard[k] = {'gate': max(yard.get(k, {}).get('gate', 0.0), gates[k]), 'oracle_f32_vs_f64': max(yard.get(k, {}).get('oracle_f32_vs_f64', 0.0), detail[k]['f32_vs_f64'])}
        for k, buf in bufs.items():
            if k.endswith('.ef'):
                got = buf[m * n * (n - 1):(m + 1) * n * (n - 1)].cpu()[internal]
                want = taps_o[k]
            elif k.endswith('.v'):
                got, want = buf[ns_].cpu(), taps_o[k].transpose(1, 2)
            else:
                got, want = buf[ns_].cpu(), taps_o[k]
            worst[k] = max(worst.get(k, 0.0), float((got - want).abs().max() / want.abs().max()))
        for k in 'xac':
            got = out[k][ns_].cpu()
            worst['out.' + k] = max(worst.get('out.' + k, 0.0), float((got - ref[k]).abs().max() / ref[k].abs().max()))
            torch.testing.assert_close(got, ref[k], rtol=2e-4, atol=2e-6)        # element-wise: small-magnitude channels too
        got = out['e'][ps_].cpu()
        worst['out.e'] = max(worst.get('out.e', 0.0), float((got - ref['e']).abs().max() / ref['e'].abs().max()))
        torch.testing.assert_close(got, ref['e'], rtol=2e-4, atol=2e-6)
    _report(('c3_size_forward' if B == 1024 else f'c4_whole_job_forward[{B}x{n}]') + ('_visible' if visible else ''),
            {**worst, 'ef_bytes': E * 512, 'workspace_bytes': eng.workspace_bytes, **({'dx_yardsticks_worst_molecule': yard} if visible else {})})
    bad = {k: v for k, v in worst.items() if not (v < (1.0 if k.endswith('.dx / gate') else OUT_TOL if k.startswith('out.') else STAGE_TOL))}
    assert not bad, worst
    assert not visible or ('out.dx / gate' in worst and any(k.startswith('upd') for k in yard))
    if B == 8192:       # release the 13 GB of taps (the cached engine keeps its 31.5 GB workspace for the next 8192-molecule test)
        del bufs, out, state
        torch.cuda.empty_cache()


@pytest.mark.parametrize('name,sizes,t,prev', [('flowmol3', [5, 9, 12, 3, 2], 0.5, True), ('flowmol3', [70, 2, 47, 130], 0.3, True),
                                               ('geom_ctmc', [5, 17, 8, 30, 2], 0.5, False)])
def test_forward_outputs_elementwise(name, sizes, t, prev):
    """Element-wise (atol + rtol) agreement of the final outputs with the oracle: the norm-wise stage tolerance does not
    constrain small-magnitude entries individually (probabilities near 0, coordinates near the origin)."""
    cfg, sd, eng, orc = engine_for(name)
    errs, out, ref = forward_compare(eng, orc, cfg, torch.tensor(sizes), t, prev, taps=False)
    for k in 'xace':
        torch.testing.assert_close(out[k].cpu(), ref[k], rtol=2e-4, atol=2e-6)


def _oracle_run_with_tape(cfg, sd, n_atoms, T, seed):
    """Oracle trajectory + its recorded RNG tape + prior, for driving the PUBLIC API with identical draws."""
    orc = cpu_ref.OracleVF(cfg, sd)
    batch = cpu_ref.build_batch(n_atoms)
    torch.manual_seed(seed)
    prior = orc.sample_prior(batch)
    rec = cpu_ref.RecordingNoise()
    with torch.no_grad():
        ref = orc.integrate(batch, prior, T, noise=rec)
    return batch, prior, rec.tape, ref


def _tape_noise_fn(tape, device='cuda:0'):
    from flowmol_amd.engine import StepNoise
    pos = [0]

    def noise_for_step(i, last):
        nz, pos[0] = StepNoise.from_tape(tape, pos[0], last, device)
        return nz
    return noise_for_step


def test_sampled_molecule_fields_of_a_device_run_match_oracle():
    """SURVEY §8 a13 on the GPU: model.sample() (HIP integration + packaging) driven with the oracle's prior and RNG tape ->
    every SampledMolecule field equals the oracle's extract_moldata (pinned to the reference's extract_moldata_from_graph by
    tests/golden/moldata.npz) of the oracle's own final state: symbols, charges, bonds after fake-atom removal; positions 1e-4."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
    cfg = model.cfg
    sd = weights.synth_state_dict(cfg, 0)
    n_atoms = torch.tensor([9, 14, 5, 21, 12, 7])
    T = 12
    batch, prior, tape, ref = _oracle_run_with_tape(cfg, sd, n_atoms, T, seed=31)
    mols = model.sample(n_atoms, n_timesteps=T, prior={'x_0': prior['x_0'], 'a_0': prior['a_0'], 'c_0': prior['c_0'], 'e_0': prior['e_0'],
                                                       'fake_atoms': cfg.fake_atoms}, _noise_for_step=_tape_noise_fn(tape))
    assert len(mols) == len(n_atoms)
    no = eo = 0
    n_fake = 0
    for m, n in zip(mols, n_atoms.tolist()):
        e_n = n * (n - 1)
        pos, sym, chg, bt, bs, bd = cpu_ref.extract_moldata(ref['x_1'][no:no + n], ref['a_1'][no:no + n], ref['c_1'][no:no + n], ref['e_1'][eo:eo + e_n], n,
                                                            cfg.atom_type_map, cfg.fake_atoms, cfg.n_bond_types)
        no += n; eo += e_n
        assert m.atom_types == sym and torch.equal(m.atom_charges, chg)
        assert torch.equal(m.bond_types, bt) and torch.equal(m.bond_src_idxs, bs) and torch.equal(m.bond_dst_idxs, bd)
        assert m.num_atoms == len(sym)
        torch.testing.assert_close(m.positions, pos, rtol=1e-4, atol=1e-4)
        assert torch.equal(m.valencies, cpu_ref.compute_valencies(len(sym), bt, bs, bd))
        n_fake += n - len(sym)
    _report('sampled_molecule_fields', {'molecules': len(mols), 'fake_atoms_removed': n_fake})


def test_traj_frames_reference_format_matches_the_reference(golden_dir):
    """VERDICT r4 missing #2 on the GPU: a device run's SampledMolecule.traj_frames_reference() equals the reference's own traj_frames dicts
    (float one-hots incl. the mask column, all directed edges: bit for bit; coordinates 1e-4) -- frames written by the fused CTMC kernel."""
    import flowmol_amd as flowmol
    from parity_util import traj_frames_reference_compare
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(golden_dir / 'traj_frames.npz').items()}
    res = traj_frames_reference_compare(flowmol.FlowMol.from_preset('qm9').cuda().eval(), g, 'cuda:0')
    _report('traj_frames_reference', res)
    assert res['x_rel'] < 1e-4 and res['molecules'] == 3, res


def test_cli_sdf_content_matches_oracle_tokens(tmp_path, monkeypatch):
    """the CLI on the GPU (seeded, sizes drawn like test.py does), driven with the oracle's RNG tape, writes an SDF whose
    every line equals the blocks derived from the ORACLE's final tokens (atoms, charge column, bond lines, M  CHG); coordinates
    agree to the 4 printed decimals +- 1e-4.  The writer itself is pinned by tests/golden/cli_expected_blocks.sdf."""
    import flowmol_amd as flowmol
    from flowmol_amd import cli
    from flowmol_amd.molecule import mol_block
    seed, n_mols, T = 4, 5, 10
    args = cli.parse_args(['--preset', 'qm9', '--n_mols', str(n_mols), '--n_timesteps', str(T), '--max_batch_size', '8', '--seed', str(seed),
                           '--output_file', str(tmp_path / 'out.sdf'), '--baseline_comparison'])
    probe = flowmol.FlowMol.from_preset('qm9')
    torch.manual_seed(seed)
    n_atoms = probe.sample_n_atoms(n_mols)                       # what the CLI will draw first from the same seed
    cfg = probe.cfg
    sd = weights.synth_state_dict(cfg, 0)
    batch, prior, tape, ref = _oracle_run_with_tape(cfg, sd, n_atoms, T, seed=99)
    orig = flowmol.FlowMol.sample

    def driven(self, n_at, **kw):
        assert torch.equal(torch.as_tensor(n_at), n_atoms)
        return orig(self, n_at, prior={**{k: prior[k] for k in ('x_0', 'a_0', 'c_0', 'e_0')}, 'fake_atoms': cfg.fake_atoms},
                    _noise_for_step=_tape_noise_fn(tape), **kw)
    monkeypatch.setattr(flowmol.FlowMol, 'sample', driven)
    mols, t_s = cli.run(args)
    import pickle
    items, sampling_time = pickle.load(open(tmp_path / 'out.sdf', 'rb'))      # --baseline_comparison: (molecules, sampling_time) pickle
    assert len(items) == n_mols and sampling_time > 0 and items[0]['atom_types'] == mols[0].atom_types
    args2 = cli.parse_args(['--preset', 'qm9', '--n_mols', str(n_mols), '--n_timesteps', str(T), '--max_batch_size', '8', '--seed', str(seed),
                            '--output_file', str(tmp_path / 'out2.sdf')])
    cli.run(args2)
    got = (tmp_path / 'out2.sdf').read_text().split('$$$$\n')
    assert len(got) == n_mols + 1 and got[-1] == ''
    no = eo = 0
    for blk, n in zip(got, n_atoms.tolist()):
        e_n = n * (n - 1)
        pos, sym, chg, bt, bs, bd = cpu_ref.extract_moldata(ref['x_1'][no:no + n], ref['a_1'][no:no + n], ref['c_1'][no:no + n], ref['e_1'][eo:eo + e_n], n,
                                                            cfg.atom_type_map, cfg.fake_atoms, cfg.n_bond_types)
        no += n; eo += e_n
        want = mol_block(pos, sym, chg, bs, bd, bt).splitlines()
        have = blk.splitlines()
        assert len(have) == len(want)
        for lw, lh in zip(want, have):
            if lw == lh:
                continue
            # an atom line whose coordinates differ in the last printed digit: everything after the coordinates must be identical
            assert lw[30:] == lh[30:] and len(lw) == len(lh), (lw, lh)
            for k in range(3):
                assert abs(float(lw[10 * k:10 * k + 10]) - float(lh[10 * k:10 * k + 10])) <= 1.0001e-4, (lw, lh)


def test_rccl_one_rank_group_gather_and_cli(tmp_path, monkeypatch):
    """First execution of the RCCL code path (backend 'nccl' on one MI355X, world size 1): the single all_gather_into_tensor of
    shard.gather_results on DEVICE tensors holding a real packed result, FlowMol.sample_distributed against sample() with the
    same seed, and the CLI launched torchrun-style as one rank."""
    import socket
    import torch.distributed as dist
    import flowmol_amd as flowmol
    from flowmol_amd import cli, shard
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    for k, v in {'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'RANK': '0', 'LOCAL_RANK': '0', 'WORLD_SIZE': '1'}.items():
        monkeypatch.setenv(k, v)
    try:
        args = cli.parse_args(['--preset', 'qm9', '--n_mols', '7', '--n_timesteps', '6', '--max_batch_size', '4', '--seed', '2',
                               '--output_file', str(tmp_path / 'd.sdf')])
        mols, _ = cli.run(args)                                   # initialises the one-rank nccl group, shards, gathers, writes
        assert dist.is_initialized() and dist.get_backend() == 'nccl' and dist.get_world_size() == 1
        assert len(mols) == 7 and (tmp_path / 'd.sdf').read_text().count('$$$$') == 7
        model = flowmol.FlowMol.from_preset('qm9').cuda().eval()
        n_atoms = torch.tensor([9, 4, 17, 6, 12])
        torch.manual_seed(8)
        full, _ = model.sample_distributed(n_atoms, n_timesteps=5, return_tensors='device')
        assert all(v.is_cuda for v in full.values())              # results stay in HBM until packaging
        torch.manual_seed(8)
        single, _ = model.sample(n_atoms, n_timesteps=5, return_tensors=True)
        for k in 'xace':
            assert torch.equal(full[k].cpu(), single[k])          # one rank owns everything: identical draws, identical result
        # the collective itself on a packed device result with odd payload size
        local = {k: v.clone() for k, v in full.items()}
        out = shard.gather_results(local, n_atoms, [torch.arange(5)])
        for k in 'xace':
            assert out[k].is_cuda and torch.equal(out[k], full[k])
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize('name', ['flowmol3', 'geom_ctmc', 'qm9', 'dev', 'arch_variants', 'geom_arom', 'flowmol3_arom'])
def test_forward_matches_reference_fixture_directly(golden_dir, name):
    """The HIP forward against the REFERENCE's own outputs (tests/golden/forward_<name>.npz: EndpointVectorField.forward of the
    reference's modules, incl. configs/dev.yml with use_dst_feats) -- no oracle in between: bootstrap pass at t = 0 and a
    self-conditioned pass at t = 0.5, element-wise."""
    cfg, sd, eng, orc = engine_for(name)
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / f'forward_{name}.npz').items()}
    eng.bind(g['n_atoms'])
    worst = {}
    for tag, tval in (('t0', 0.0), ('th', 0.5)):
        state = eng.make_state(g[f'{tag}.x_t'], g[f'{tag}.a'], g[f'{tag}.c'], g[f'{tag}.e_upper'])
        prev = None
        if tag == 'th' and cfg.self_conditioning:
            prev = {k: g[f'th.prev.{k}'].cuda().contiguous() for k in 'xace'}
        out = eng.forward(state, tval, prev=prev, bootstrap=(tag == 't0'), remove_com=True)
        eng.synchronize()
        for k in 'xace':
            want = g[f'{tag}.out.{k}']
            torch.testing.assert_close(out[k].cpu(), want, rtol=2e-4, atol=2e-6)
            worst[f'{tag}.{k}'] = float((out[k].cpu() - want).abs().max() / want.abs().max())
    _report(f'forward_vs_reference_fixture[{name}]', worst)
    assert max(worst.values()) < OUT_TOL, worst


def test_philox_mode_on_gpu_is_batch_composition_independent():
    """rng='philox' on the GPU at BASELINE-like sizes: 48 GEOM-sized molecules sampled together vs. two of them sampled alone
    (as another shard would) with their global ids -- identical tokens AND bit-identical coordinates (canonical arithmetic); no mask tokens left."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
    torch.manual_seed(3)
    sizes = model.sample_n_atoms(48)
    full, _ = model.sample(sizes, n_timesteps=25, return_tensors=True, rng='philox', _philox=2024)
    assert torch.isfinite(full['x']).all() and (full['a'] != model.cfg.n_atom_types).all() and (full['e'] != model.cfg.n_bond_types).all()
    ids = torch.tensor([31, 7])
    part, _ = model.sample(sizes[ids], n_timesteps=25, return_tensors=True, rng='philox', _philox=2024, _mol_ids=ids)
    pairs = sizes * (sizes - 1) // 2
    noff, poff = torch.cumsum(sizes, 0) - sizes, torch.cumsum(pairs, 0) - pairs
    o_n = o_p = 0
    flips = 0
    for i in ids.tolist():
        n, u = int(sizes[i]), int(pairs[i])
        flips += int((part['a'][o_n:o_n + n] != full['a'][noff[i]:noff[i] + n]).sum() + (part['e'][o_p:o_p + u] != full['e'][poff[i]:poff[i] + u]).sum())
        assert torch.equal(part['x'][o_n:o_n + n], full['x'][noff[i]:noff[i] + n])
        assert torch.equal(part['c'][o_n:o_n + n], full['c'][noff[i]:noff[i] + n])
        o_n += n; o_p += u
    _report('philox_composition', {'flips': flips})
    assert flips == 0


def test_a_molecule_alone_equals_the_same_molecule_in_a_1024_batch_bit_for_bit():
    """Canonical arithmetic at the headline size: molecules 0, 517 and 1023 of BASELINE configs[2]'s 1024 x 47-atom batch -- which runs
    32-row edge and node tiles, 64-row MLP tiles and the pair slab -- sampled ALONE (16-row edge tiles, 4-node tiles of the node kernel and 4-row node MLPs on
    v_mfma_f32_4x4x1, 1024-thread CTMC workgroups) with their Philox ids give the same coordinates and tokens bit for bit over 12 steps; so does a ragged
    GEOM-sized batch against its members alone.  With canonical=False the pair slab follows the batch size (another summation order of the first scalar
    GEMM of two convolutions) and the same comparison agrees to f32 summation order only."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
    T = 12
    for sizes, ids in ((torch.full((1024,), 47), [0, 517, 1023]), (None, [3, 40, 95])):
        if sizes is None:
            torch.manual_seed(11)
            sizes = model.sample_n_atoms(96)
        full, _ = model.sample(sizes, n_timesteps=T, return_tensors=True, rng='philox', _philox=77)
        pairs = sizes * (sizes - 1) // 2
        noff, poff = torch.cumsum(sizes, 0) - sizes, torch.cumsum(pairs, 0) - pairs
        for i in ids:
            one, _ = model.sample(sizes[i:i + 1], n_timesteps=T, return_tensors=True, rng='philox', _philox=77, _mol_ids=torch.tensor([i]))
            n, u = int(sizes[i]), int(pairs[i])
            for k in 'xac':
                assert torch.equal(one[k], full[k][noff[i]:noff[i] + n]), (k, i)
            assert torch.equal(one['e'], full['e'][poff[i]:poff[i] + u]), i
    # the opt-in split precision runs the same aggregation / LayerNorm / gate orders: canonical too (another arithmetic, the same guarantee)
    half = flowmol.FlowMol.from_preset('flowmol3', precision='f16x3').cuda().eval()
    sizes = torch.full((256,), 47)
    full, _ = half.sample(sizes, n_timesteps=T, return_tensors=True, rng='philox', _philox=77)
    one, _ = half.sample(sizes[200:201], n_timesteps=T, return_tensors=True, rng='philox', _philox=77, _mol_ids=torch.tensor([200]))
    assert torch.equal(one['x'], full['x'][200 * 47:201 * 47]) and torch.equal(one['a'], full['a'][200 * 47:201 * 47])
    del half
    lat = flowmol.FlowMol.from_preset('flowmol3', canonical=False).cuda().eval()
    sizes = torch.full((256,), 47)
    full, _ = lat.sample(sizes, n_timesteps=T, return_tensors=True, rng='philox', _philox=77)
    one, _ = lat.sample(sizes[:1], n_timesteps=T, return_tensors=True, rng='philox', _philox=77, _mol_ids=torch.tensor([0]))
    rel = float((one['x'] - full['x'][:47]).abs().max() / full['x'][:47].abs().max())
    _report('latency_mode_composition', {'x_rel': rel, 'bitwise': bool(torch.equal(one['x'], full['x'][:47]))})
    assert rel < 1e-4


def test_cosine_schedule_trajectory_matches_reference_golden(golden_dir):
    """Cosine interpolant schedule (interpolant_scheduler.py:131-146) on the GPU against the reference's own free-running integrate()."""
    from flowmol_amd.engine import Engine
    from parity_util import cosine_cfg
    cfg = cosine_cfg(presets.qm9())
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / 'integrate_qm9_cosine.npz').items()}
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device='cuda:0')
    res, state = integrate_golden(eng, cfg, g, device='cuda:0')
    _report('integrate[cosine]', res)
    assert res['a_flips'] == 0 and res['c_flips'] == 0 and res['e_flips'] == 0 and res['traj0_a_flips'] == 0, res
    assert res['x_rel'] < 1e-4 and res['traj0_x_rel'] < 1e-4, res


def test_endpoint_parameterization_matches_reference_golden(golden_dir):
    """EndpointVectorField on the GPU (fm_forward_dense + fm_endpoint_step) against the reference's own module: network evaluation on
    continuous categorical features and the free-running Euler integration of x, a, c, e (vector_field.py:212-293, 388-569)."""
    from flowmol_amd.engine import Engine
    from parity_util import endpoint_cfg, endpoint_golden
    cfg = endpoint_cfg()
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / 'integrate_endpoint.npz').items()}
    eng = Engine(cfg, weights.synth_state_dict(cfg, 0), device='cuda:0')
    res = endpoint_golden(eng, g, device='cuda:0')
    _report('endpoint_golden', res)
    assert all(v < 1e-5 for v in res.values()), res


@pytest.mark.parametrize('name', ['flowmol3', 'dev'])
def test_engine_with_one_tensor_off_by_one_percent_fails_the_scoring(name):
    """End to end through the HIP kernels: an engine built with ONE tensor x1.01 against the oracle with the true weights must be reported out of
    tolerance by the scoring of the forward tests (visible weights, displacement stages), for each of parity_util.mutation_targets() -- the three GVPs
    of the last position updater, an EdgeUpdate matrix, the last convolution's last cross-product matrix: the engine reads the tensor and the test sees
    it.  One Engine per tensor (<= 16), each closed."""
    from flowmol_amd.engine import Engine
    cfg = presets.PRESETS[name]()
    sd = visible_weights(name, weights.synth_state_dict(cfg, 0))
    orc = cpu_ref.OracleVF(cfg, sd)
    sizes, t, prev = [5, 9, 12, 3, 2], 0.5, True
    gates, _ = dx_gates_for(name, sd, sizes, t, prev)
    targets = mutation_targets(cfg)
    assert len(targets) <= 16
    seen = {}
    for key in targets:
        eng = Engine(cfg, {**sd, key: sd[key] * 1.01}, device='cuda:0', precision='f32')
        errs, out, ref = forward_compare(eng, orc, cfg, torch.tensor(sizes), t, prev, dx=True)
        eng.close()
        bad = out_of_tolerance(errs, gates, STAGE_TOL, OUT_TOL)
        seen[key] = max(v / (gates[k] if k.endswith('.dx') else OUT_TOL if k.startswith('out.') else STAGE_TOL) for k, v in errs.items()) if bad else 0.0
    _report(f'engine_mutation[{name}] worst error / tolerance per tensor x1.01', seen)
    assert all(v > 0 for v in seen.values()), {k: v for k, v in seen.items() if not v > 0}


# ----------------------------------------------------------------------------------------------------------------------
# opt-in split precision (bf16x3 edge-message GEMMs): NOT the reference's f32 arithmetic -- errors are reported, gates are the
# same as the f32 path's where they hold, and nothing here feeds a parity claim of the default path
# ----------------------------------------------------------------------------------------------------------------------
_sp_engines = {}


def sp_engine_for(name):
    from flowmol_amd.engine import Engine
    if name not in _sp_engines:
        cfg = presets.PRESETS[name]()
        sd = weights.synth_state_dict(cfg, 0)
        _sp_engines[name] = (cfg, sd, Engine(cfg, sd, device='cuda:0', precision='bf16x3'), cpu_ref.OracleVF(cfg, sd))
    return _sp_engines[name]


@pytest.mark.parametrize('name,sizes,t,prev', [('flowmol3', [5, 9, 12, 3, 2], 0.5, True), ('flowmol3', [70, 2, 47, 130], 0.3, True),
                                               ('geom_ctmc', [5, 17, 8, 30, 2], 0.5, False)])
def test_split_precision_forward_errors(name, sizes, t, prev):
    """bf16x3 edge messages vs the f32 oracle, every stage: the per-edge scalar messages carry ~6e-6 relative error (f32 path: 1e-6),
    everything downstream of the first LayerNorm ~1e-6; gate: 5e-5 per stage, 2e-5 on the outputs (2.5x / 2x the f32 path's gates)."""
    cfg, sd, eng, orc = sp_engine_for(name)
    errs, out, ref = forward_compare(eng, orc, cfg, torch.tensor(sizes), t, prev)
    _report(f'split_precision_forward[{name},{sizes}]', errs)
    bad = {k: v for k, v in errs.items() if not (v < (2e-5 if k.startswith('out.') else 5e-5))}
    assert not bad, f'stages out of tolerance: {bad}'


@pytest.mark.parametrize('fname,name', [('integrate_flowmol3_F7.npz', 'flowmol3'), ('integrate_qm9_C1.npz', 'qm9'),
                                        ('integrate_geom_ctmc_C5s.npz', 'geom_ctmc')])
def test_split_precision_trajectories_flip_counts(golden_dir, fname, name):
    """Free-running golden trajectories in split precision: categorical flips against the reference are COUNTED and reported (a handful
    of near-tie decisions may differ -- it is not f32 arithmetic); coordinates must stay within the 1e-4 target wherever no flip occurred."""
    cfg, sd, eng, orc = sp_engine_for(name)
    g = {k: torch.from_numpy(v) for k, v in np.load(golden_dir / fname).items()}
    res, state = integrate_golden(eng, cfg, g, device='cuda:0')
    _report(f'split_precision_integrate[{fname}]', res)
    flips = res['a_flips'] + res['c_flips'] + res['e_flips']
    n_tokens = int(g['a_1'].numel() + g['c_1'].numel() + g['e_1_upper'].numel())
    assert flips <= max(2, n_tokens // 100), res
    if flips == 0:
        assert res['x_rel'] < 1e-4, res
    assert (state['a_t'] != cfg.n_atom_types).all() and (state['e_t'] != cfg.n_bond_types).all()


def test_split_precision_c3_full_size_properties():
    """BASELINE configs[2] at full size in the opt-in split precision (1024 x 47 atoms, 250 steps): finite, no mask tokens left,
    zero per-molecule centre of mass of the final coordinates -- the size-independent properties of the f32 path's C3 test."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('flowmol3', precision='bf16x3').cuda().eval()
    torch.manual_seed(21)
    out, n_atoms = model.sample(torch.full((1024,), 47), n_timesteps=250, return_tensors=True)
    assert torch.isfinite(out['x']).all()
    assert (out['a'] != model.cfg.n_atom_types).all() and (out['e'] != model.cfg.n_bond_types).all()
    assert out['x'].reshape(1024, 47, 3).mean(1).abs().max() < 1e-3


_pq_engines = {}


@pytest.mark.parametrize('seed', list(range(24)))
def test_forward_matches_oracle_on_random_batches(seed):
    """Seeded random batches (ragged sizes 1..90 with a degenerate / tile-edge size in every batch, random time, with / without a
    previous endpoint, every preset, both tile sizes): every stage and output of a network evaluation against the oracle.  Seeds 16..23:
    the self-conditioned presets with the pair-slab hoist forced on (it switches on by itself only for large batches) and a previous endpoint,
    so its tile-relative pair addressing meets ragged molecule boundaries, 1- and 2-atom molecules and both tile sizes."""
    from flowmol_amd.engine import Engine
    rng = np.random.default_rng(1234 + seed)
    pq = seed >= 16
    name = (['flowmol3', 'qm9', 'flowmol3_arom', 'arch_variants'][seed % 4] if pq else
            ['flowmol3', 'geom_ctmc', 'dev', 'dev_narrow', 'arch_variants', 'qm9', 'geom_arom', 'flowmol3_arom'][seed % 8])
    tile = [16, 32][int(rng.integers(0, 2))]
    nmol = int(rng.integers(2, 9))
    sizes = [int(v) for v in rng.integers(1, 91 if name in ('flowmol3', 'geom_ctmc', 'geom_arom', 'flowmol3_arom') else 40, size=nmol)]
    sizes[int(rng.integers(0, nmol))] = [1, 2, 17, 33][int(rng.integers(0, 4))]
    t = float(np.float32(rng.uniform(0.05, 0.95)))
    if pq:
        if (name, tile) not in _pq_engines:
            cfg = presets.PRESETS[name]()
            sd = weights.synth_state_dict(cfg, 0)
            _pq_engines[(name, tile)] = (cfg, sd, Engine(cfg, sd, device='cuda:0', precision='f32', tuning={'tile_edge': tile, 'tile_node': tile, 'pair_slab': 1}), cpu_ref.OracleVF(cfg, sd))
        cfg, sd, eng, orc = _pq_engines[(name, tile)]
        prev = True
    else:
        cfg, sd, eng, orc = engine_for(name, tile)
        prev = bool(rng.integers(0, 2)) and cfg.self_conditioning
    errs, out, ref = forward_compare(eng, orc, cfg, torch.tensor(sizes), t, prev)
    _report(f'forward_random[{seed}: {name},{sizes},{t:.3f},prev={prev},tile{tile},pair_slab={"forced" if pq else "auto"}]', errs)
    bad = {k: v for k, v in errs.items() if not (v < (OUT_TOL if k.startswith('out.') else STAGE_TOL))}
    assert not bad, f'{name} {sizes} t={t} tile={tile}: {bad}'
    if pq:
        if (name, tile, 'visible') not in _pq_engines:
            sd = visible_weights(name, weights.synth_state_dict(cfg, 0))
            _pq_engines[(name, tile, 'visible')] = (cfg, sd, Engine(cfg, sd, device='cuda:0', precision='f32', tuning={'tile_edge': tile, 'tile_node': tile, 'pair_slab': 1}), cpu_ref.OracleVF(cfg, sd))
        cfg, sd, eng, orc = _pq_engines[(name, tile, 'visible')]
    else:
        cfg, sd, eng, orc = engine_for(name, tile, visible=True)
    bad = visible_regime_failures(f'forward_random_visible[{seed}: {name},{sizes},{t:.3f},prev={prev},tile{tile}]', name, eng, orc, cfg, sd, sizes, t, prev)
    assert not bad, f'visible weights, {name} {sizes} t={t} tile={tile}: {bad}'


@pytest.mark.parametrize('regime,scale', [('unit weights', 1.0), ('all weights x3', 3.0)])
def test_three_term_split_is_f32_class_against_float64(regime, scale):
    """per-stage error of the f32 kernels, the two-term split (bf16x3) and the three-term split (bf16x6, edge-message GEMMs only) against
    the oracle evaluated in FLOAT64 -- the exact result, not the f32 reference arithmetic -- in the benign regime and with all weights x3 (rounding
    differences grow ~10x per convolution).  Acceptance for calling bf16x6 f32-equivalent: at EVERY stage its error is at most 1.5x the f32
    kernels' (plus 2e-7 of slack for stages where both sit at the noise floor of the comparison); bf16x3 is reported beside it (~10x)."""
    from flowmol_amd.engine import Engine
    from parity_util import oracle_f64, scaled_weights
    cfg = presets.flowmol3()
    sd = scaled_weights(weights.synth_state_dict(cfg, 0), scale)
    sizes = torch.tensor([5, 12, 47, 2, 33])
    o64 = oracle_f64(cfg, sd)
    errs = {}
    for prec in ('f32', 'bf16x3', 'bf16x6', 'f16x3'):
        eng = Engine(cfg, sd, device='cuda:0', precision=prec)
        errs[prec], out, _ = forward_compare(eng, o64, cfg, sizes, 0.5, True, dtype=torch.float64)
        assert all(torch.isfinite(v).all() for v in out.values())
        eng.close()
    common = [k for k in errs['f32'] if all(k in errs[p_] for p_ in ('bf16x3', 'bf16x6', 'f16x3'))]
    worst = {p_: max(errs[p_][k] / errs['f32'][k] for k in common if errs['f32'][k] > 0) for p_ in ('bf16x3', 'bf16x6', 'f16x3')}
    _report(f'three_term_split_vs_float64[{regime}]', {'stage_errors_vs_float64 [f32, bf16x3, bf16x6, f16x3]': {k: [errs[p_][k] for p_ in ('f32', 'bf16x3', 'bf16x6', 'f16x3')] for k in common},
                                                       'worst_ratio_bf16x6_over_f32': worst['bf16x6'], 'worst_ratio_bf16x3_over_f32': worst['bf16x3'], 'worst_ratio_f16x3_over_f32': worst['f16x3']})
    # Unit weights: the per-stage errors are stable properties of the arithmetic -- bf16x6 is held to 1.5x, the half split (22 of 24 mantissa bits) to 2x.
    # All weights x3: rounding differences are amplified ~10x per convolution until the output errors reach 0.1-0.3, so a stage's error is ONE DRAW of a wide
    # distribution that moves with every change of summation order (round 6's canonical order moved the f32 kernels' conv3.agg.v from 1.8e-4 to 5.8e-5 while
    # bf16x6 stayed at 1.7e-4: profiles/r05g_* vs r06e_*); there the modes are held to the same ORDER of error (4x), which still separates them from bf16x3 (25-70x).
    for p_, factor in (('bf16x6', 1.5 if scale == 1 else 4.0), ('f16x3', 2.0 if scale == 1 else 4.0)):
        bad = {k: (errs[p_][k], errs['f32'][k]) for k in common if not errs[p_][k] <= factor * errs['f32'][k] + 2e-7 * (scale ** 2)}
        assert not bad, (p_, bad)


@pytest.mark.parametrize('precision', ['bf16x6', 'f16x3'])
def test_three_term_split_decisions_on_the_20m_fixture(golden_dir, precision):
    """... and the f32-class modes' categorical decisions on the 64-molecule reference trajectory, audited like the f32 kernels' (teacher-forced, every
    differing decision must be a near-tie): the count is reported next to f32's one event."""
    from flowmol_amd.engine import Engine
    from parity_util import audit_long_decisions, integrate_long_teacher_forced
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(golden_dir / 'long_flowmol3_geom64_T250.npz').items()}
    cfg = presets.flowmol3()
    eng = Engine(cfg, weights.long_fixture_weights(cfg, g), device='cuda:0', precision=precision)
    traj, probs = integrate_long_teacher_forced(eng, cfg, g)
    res = audit_long_decisions(cfg, g, traj, probs)
    _report(f'teacher_forced_audit[flowmol3_geom64_T250, {precision}]', res)
    assert not res['unexplained'], res['unexplained'][:5]
    assert len(res['events']) <= 4, res['events']
    x = traj['x'][-1].cpu()
    assert float((x - g['x_1']).abs().max() / g['x_1'].abs().max()) < 1e-4
    eng.close()
    del traj, probs
    torch.cuda.empty_cache()


@pytest.mark.parametrize('precision', ['f32', 'bf16x3', 'bf16x6', 'f16x3'])
def test_error_tracks_the_reference_rounding_sensitivity(precision):
    """Ill-conditioned regime (all weight matrices x3: rounding differences grow ~10x per convolution, the f32 reference itself drifts
    percent-level from its own float64 evaluation by the last conv): every stage's error against the f32 oracle stays within a small
    multiple of the oracle's own f32-vs-f64 discrepancy at that stage -- the kernels are as accurate as the reference's arithmetic, not
    merely inside a tolerance tuned for benign weights.  The opt-in split-precision mode is held to its own (documented, ~10x) factor."""
    from flowmol_amd.engine import Engine
    from parity_util import oracle_rounding_sensitivity, scaled_weights
    cfg = presets.flowmol3()
    sd = scaled_weights(weights.synth_state_dict(cfg, 0), 3.0)
    sizes = torch.tensor([5, 12, 47, 2])
    sens = oracle_rounding_sensitivity(cfg, sd, sizes, 0.5, True)
    assert sens['conv5.s'] > 1e-3
    eng = Engine(cfg, sd, device='cuda:0', precision=precision)
    errs, out, ref = forward_compare(eng, cpu_ref.OracleVF(cfg, sd), cfg, sizes, 0.5, True)
    factor, floor = (80, 5e-4) if precision == 'bf16x3' else (8, 5e-5)          # the three-term split is held to the f32 kernels' own factor
    _report(f'rounding_sensitivity[{precision}]', {k: (errs[k], sens[k]) for k in errs if k in sens})
    bad = {k: (v, sens[k]) for k, v in errs.items() if k in sens and not v <= max(floor, factor * sens[k])}
    assert not bad, bad
    assert all(torch.isfinite(v).all() for v in out.values())


def test_load_pretrained_lightning_shaped_checkpoint_on_gpu(tmp_path, monkeypatch):
    """The documented usage (reference readme.md:44-49, flowmol/__init__.py:30-56) on the GPU from a Lightning-shaped checkpoint under
    $FLOWMOL_MODELS_DIR (hyper_parameters an AttributeDict of a package this image lacks, pathlib.PosixPath data files, `vector_field.*`
    keys): load_pretrained('flowmol3').cuda().eval().sample_random_sizes(...) equals the from_preset model with the same seed."""
    import flowmol_amd as flowmol
    from parity_util import write_lightning_shaped_checkpoint
    cfg = presets.flowmol3()
    write_lightning_shaped_checkpoint(tmp_path, 'flowmol3', weights.synth_state_dict(cfg, 0), 'flowmol3.yml')
    monkeypatch.setenv('FLOWMOL_MODELS_DIR', str(tmp_path))
    model = flowmol.load_pretrained('flowmol3').cuda().eval()
    torch.manual_seed(7)
    mols = model.sample_random_sizes(4, n_timesteps=6)
    ref = flowmol.FlowMol.from_preset('flowmol3').cuda().eval()
    torch.manual_seed(7)
    mols_ref = ref.sample_random_sizes(4, n_timesteps=6)
    assert len(mols) == 4
    for a, b in zip(mols, mols_ref):
        assert torch.equal(a.positions, b.positions) and a.atom_types == b.atom_types and torch.equal(a.atom_charges, b.atom_charges)
        assert torch.equal(a.bond_types, b.bond_types) and torch.equal(a.bond_src_idxs, b.bond_src_idxs)
    assert model.last_timing['precision'] == 'f32'


def test_remove_com_prior_entry_point_matches_oracle_prior():
    """fm_remove_com as the centring step of the position prior (priors.py:27-35 centered_normal_prior_batched_graph) against the oracle's
    sample_prior from the SAME randn draw, on a ragged batch incl. 1-atom and 181-atom molecules: within 1 ulp of the coordinate scale
    (the per-molecule mean is a different summation order), and exactly zero-mean to rounding."""
    cfg, sd, eng, orc = engine_for('flowmol3')
    n_atoms = torch.tensor([47, 1, 5, 181, 2, 33, 90, 3])
    batch = cpu_ref.build_batch(n_atoms)
    torch.manual_seed(123)
    prior = orc.sample_prior(batch)                     # randn(N,3) on the CPU generator, minus the per-molecule mean
    torch.manual_seed(123)
    raw = torch.randn(batch.N, 3)
    eng.bind(n_atoms)
    x = raw.cuda().contiguous()
    eng.remove_com(x)
    eng.synchronize()
    got = x.cpu()
    err = float((got - prior['x_0']).abs().max())
    _report('remove_com_prior', {'max_abs': err})
    assert err <= 2.4e-7 * float(raw.abs().max()), err                      # <= 2 ulp at the largest coordinate
    off = 0
    for n in n_atoms.tolist():
        assert float(got[off:off + n].mean(0).abs().max()) < 2e-6
        off += n
    assert torch.equal(got[47:48], torch.zeros(1, 3))                       # a 1-atom molecule is its own centre


def test_philox_streams_statistics_on_gpu():
    """rng='philox' is the mode an 8-GPU run uses: the in-kernel draws on the real device.  Position prior
    (fm_prior_philox): per-molecule mean 0, unit variance, Gaussian quantiles (KS), streams of different molecule ids and seeds
    uncorrelated, a molecule's draw independent of its position in the batch.  CTMC noise (fm_ctmc_step, FM_NOISE_PHILOX): the Exp(1) race
    reproduces the categorical probabilities and the U(0,1) thresholds reproduce the unmasking probability, per modality."""
    import ctypes as C
    import math
    from flowmol_amd.engine import make_step_plan
    cfg, sd, eng, orc = engine_for('flowmol3')
    B, n = 4096, 64                       # 786,432 draws: the standard error of the variance estimate is 1.6e-3
    eng.bind(torch.full((B,), n))
    eng.set_molecule_ids(None)
    x0 = eng.prior_philox(7).cpu().reshape(B, n, 3)
    assert float(x0.mean(1).abs().max()) < 2e-6
    raw_var = float(x0.var(dim=1, unbiased=True).mean())                  # centring removes 1/n of the variance; the unbiased estimate restores it
    assert abs(raw_var - 1.0) < 4 * math.sqrt(2 / (n - 1) / (3 * B)), raw_var
    z = (x0 * math.sqrt(n / (n - 1))).flatten().double().sort().values      # ~N(0,1) marginals
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    m = z.numel()
    ks = float(torch.max((torch.arange(1, m + 1) / m - cdf).abs().max(), (cdf - torch.arange(0, m) / m).abs().max()))
    assert ks < 1.63 / math.sqrt(m), ks                                    # 1 % critical value of the Kolmogorov-Smirnov statistic
    x0b = eng.prior_philox(8).cpu().reshape(B, n, 3)
    corr_seed = float((x0 * x0b).mean() / (x0.std() * x0b.std()))
    corr_mol = float((x0[:-1] * x0[1:]).mean() / x0.var())
    assert abs(corr_seed) < 4 / math.sqrt(m) and abs(corr_mol) < 4 / math.sqrt(m), (corr_seed, corr_mol)
    ids = torch.tensor([300, 17, 4095])
    eng.bind(torch.full((3,), n))
    eng.set_molecule_ids(ids)
    sub = eng.prior_philox(7).cpu().reshape(3, n, 3)
    torch.testing.assert_close(sub, x0[ids], rtol=0, atol=1e-6)              # same stream wherever the molecule sits (mean in another order)
    # CTMC draws: everything masked, fixed probabilities, hc = 0 (uniform unmasking branch), mid-trajectory step
    eng.bind(torch.tensor([64] * 16))
    eng.set_molecule_ids(None)
    N, U = eng.N, eng.U
    T = cfg.cat_temperature
    p_e = torch.tensor([0.1, 0.2, 0.3, 0.4])
    p_a = torch.softmax(torch.linspace(-1, 1, cfg.n_atom_types), 0)
    temper = lambda p: (p ** T / (p ** T).sum())                            # the kernel applies softmax(log(.)/T): feed p^T so that it samples from p
    plan = make_step_plan(250, cfg.stochasticity, 0.0, T, philox_seed=4242)
    for s_idx, last in ((len(plan.scalars) - 1, True), (100, False)):
        sc = plan.scalars[s_idx]
        state = eng.prior_state(torch.zeros(N, 3))
        dst = {'x': torch.zeros(N, 3, device='cuda:0'), 'a': temper(p_a).repeat(N, 1).contiguous().cuda(),
               'c': torch.full((N, cfg.n_charges), 1.0 / cfg.n_charges, device='cuda:0'), 'e': temper(p_e).repeat(U, 1).contiguous().cuda()}
        st_, d_ = eng._state_struct(state), eng._dst_struct(dst)
        smp = {'a1': torch.zeros(N, dtype=torch.int32, device='cuda:0'), 'c1': torch.zeros(N, dtype=torch.int32, device='cuda:0'),
               'e1': torch.zeros(U, dtype=torch.int32, device='cuda:0')}
        from flowmol_amd._lib import fm_sampled
        sm = fm_sampled(); sm.a1, sm.c1, sm.e1 = (C.c_void_p(smp[k].data_ptr()) for k in ('a1', 'c1', 'e1'))
        with eng._dev():
            eng._check(eng.lib.fm_ctmc_step(eng._ctx, eng._stream(), C.byref(st_), C.byref(d_), None, C.byref(sc), C.byref(sm)), 'fm_ctmc_step')
        eng.synchronize()
        fe = torch.bincount(smp['e1'].cpu().long(), minlength=4).float() / U         # the Exp(1) race = a categorical sample of p
        fa = torch.bincount(smp['a1'].cpu().long(), minlength=cfg.n_atom_types).float() / N
        assert torch.allclose(fe, p_e, atol=4 * math.sqrt(0.25 / U) + 1e-3), fe
        assert torch.allclose(fa, p_a, atol=4 * math.sqrt(0.25 / N) + 1e-3), fa
        e_t = state['e_t'].cpu().long()
        if last:
            assert (e_t != cfg.n_bond_types).all()
        else:                                                                          # U(0,1) thresholds: unmasked share = p_unmask (then re-masking with p_mask)
            pu, pm = sc.unmask_prob[2], sc.mask_prob[2]
            share = float((e_t != cfg.n_bond_types).float().mean())
            assert abs(share - pu) < 4 * math.sqrt(pu * (1 - pu) / U) + 2e-3, (share, pu, pm)


def test_c5_full_size_trajectory_properties():
    """BASELINE configs[4] at FULL size: geom_full_kekulized model, 128 molecules with sizes randint(5, 61, seed 0), n_timesteps = 500, with the
    trajectory sink on (--xt_traj / --ep_traj).  Size-independent properties: finite, no mask tokens in the result, frame 0 = the prior
    (masked tokens, the centred draw), last frame = the result, every endpoint frame COM-free, the frames' footprint within the compact-format
    budget (indices + fp32 coordinates instead of float one-hots over directed edges)."""
    import flowmol_amd as flowmol
    model = flowmol.FlowMol.from_preset('geom_ctmc').cuda().eval()
    n_atoms = torch.randint(5, 61, (128,), generator=torch.Generator().manual_seed(0))
    torch.manual_seed(31)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()          # other tests' cached engines (workspaces of up to 2 GB each) stay allocated: budget the increase
    mols = model.sample(n_atoms, n_timesteps=500, xt_traj=True, ep_traj=True)
    peak = torch.cuda.max_memory_allocated() - base
    cfg = model.cfg
    assert len(mols) == 128
    frame_bytes = 0
    for m, n in zip(mols, n_atoms.tolist()):
        tf = m.traj_frames
        u = n * (n - 1) // 2
        assert tf['x'].shape == (500, n, 3) and tf['x_1_pred'].shape == (499, n, 3) and tf['e'].shape == (500, u) and tf['e_1_pred'].shape == (499, u)
        assert torch.isfinite(tf['x']).all() and torch.isfinite(tf['x_1_pred']).all()
        assert (tf['a'][0] == cfg.n_atom_types).all() and (tf['c'][0] == cfg.n_charges).all() and (tf['e'][0] == cfg.n_bond_types).all()
        assert float(tf['x'][0].mean(0).abs().max()) < 2e-6                                  # the centred prior
        assert torch.equal(tf['x'][-1], m.x_1) and torch.equal(tf['a'][-1].long(), m.a_1) and torch.equal(tf['e'][-1].long(), m.e_1)
        assert (m.a_1 != cfg.n_atom_types).all() and (m.c_1 != cfg.n_charges).all() and (m.e_1 != cfg.n_bond_types).all()
        assert float(tf['x_1_pred'].mean(1).abs().max()) < 1e-4
        frame_bytes += sum(v.numel() * v.element_size() for v in tf.values())
    N, U = int(n_atoms.sum()), int((n_atoms * (n_atoms - 1) // 2).sum())
    compact = 2 * 500 * (N * (12 + 8) + U * 4)                     # x fp32 + a, c, e int32, state + endpoint frames
    reference_format = 2 * 500 * 4 * (N * (3 + cfg.n_atom_types + 1 + cfg.n_charges + 1) + 2 * U * (cfg.n_bond_types + 1))
    _report('c5_full_size', {'frame_bytes': frame_bytes, 'reference_format_bytes': reference_format, 'peak_device_bytes': int(peak),
                             'integrate_s': model.last_timing['integrate'], 'package_s': model.last_timing.get('package')})
    assert frame_bytes <= compact and frame_bytes < reference_format / 2
    assert peak < 4 << 30                         # workspace + 0.37 GB of frames on the device + per-chunk noise
    blocks = mols[3].traj_mol_blocks()
    assert len(blocks) == 500 and blocks[0].count('Se') == int(n_atoms[3])                    # frame 0: every atom still masked


@pytest.mark.parametrize('B,slots,n_steps', [
    (1024, (0, 127, 128, 511, 600, 895, 896, 1023), None),
    # BASELINE configs[3]'s whole 8192-molecule job bound on ONE GPU (VERDICT r3 #1a): the reference's eight molecules sit at both ends, either
    # side of the middle, either side of XCD tile-chunk boundaries (1024 molecules per chunk) and beyond 2^32 bytes of edge state; the first
    # 26 integration steps (bootstrap + 25 self-conditioned evaluations, 0.55 s each) against the reference's trajectory, every token of every step
    (8192, (0, 1023, 1024, 3880, 4095, 4096, 7168, 8191), 26),
])
def test_full_batch_reproduces_reference_long_trajectory(golden_dir, B, slots, n_steps):
    """BASELINE configs[2] at FULL size AND full horizon against the reference: a 1024 x 47-atom batch integrated for 250 steps in which
    eight molecules -- placed at both ends of the batch, either side of XCD tile-chunk boundaries (127|128, 895|896) and mid-chunk -- carry the
    prior and the per-step noise of tests/golden/long_flowmol3_47x8_T250.npz (the reference's own 8-molecule run), while the other 1016
    molecules draw their own.  Molecules never interact, so those eight must reproduce the reference's trajectory: every state token of every
    step, final coordinates within 1e-4 -- parity at the size and horizon the metric is quoted on, not only on an 8-molecule batch.
    The 8192-molecule case is configs[3]'s job on one GPU, over the first ``n_steps`` steps of the same trajectory."""
    from flowmol_amd.engine import IntegrationRun, StepNoise, make_step_plan
    cfg, sd, eng, orc = engine_for('flowmol3')
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(golden_dir / 'long_flowmol3_47x8_T250.npz').items()}
    T, n = int(g['T']), 47
    K = T - 1 if n_steps is None else n_steps            # integration steps run here
    u = n * (n - 1) // 2
    slots = torch.tensor(slots)
    node_rows = (slots[:, None] * n + torch.arange(n)[None]).flatten().cuda()
    pair_rows = (slots[:, None] * u + torch.arange(u)[None]).flatten().cuda()
    eng.bind(torch.full((B,), n))
    N, U = eng.N, eng.U
    gen = torch.Generator(device='cuda:0').manual_seed(99)
    x0 = torch.randn(N, 3, device='cuda:0', generator=gen)
    eng.remove_com(x0)
    x0[node_rows] = g['x_0'].cuda()
    state = eng.prior_state(x0)
    plan = make_step_plan(T, cfg.stochasticity, cfg.high_confidence_threshold, cfg.cat_temperature)
    torch.manual_seed(int(g['seed_noise']))

    def noise_for_step(i, last):
        small = StepNoise.draw(8 * n, 8 * u, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types, last, 'cpu')          # the reference's draws, from its seed
        big = StepNoise.draw(N, U, cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types, last, 'cuda:0', generator=gen)
        for k in big.__slots__:
            t = getattr(big, k)
            if t is not None:
                t[pair_rows if k.endswith('_e') else node_rows] = getattr(small, k).cuda()
        return big
    i32 = dict(dtype=torch.int32, device='cuda:0')
    traj = {'x': torch.zeros(K, N, 3, device='cuda:0'), 'a': torch.zeros(K, N, **i32), 'c': torch.zeros(K, N, **i32), 'e': torch.zeros(K, U, **i32)}
    run = IntegrationRun(eng, state, plan, noise_for_step, traj=traj)
    run.run(0, K, chunk=16)
    eng.synchronize()
    nr, pr = node_rows.cpu(), pair_rows.cpu()
    res = {'steps': K,
           'a_state_diffs_all_steps': int((traj['a'][:, node_rows].cpu().long() != g['traj.a'][1:K + 1].long()).sum()),
           'c_state_diffs_all_steps': int((traj['c'][:, node_rows].cpu().long() != g['traj.c'][1:K + 1].long()).sum()),
           'e_state_diffs_all_steps': int((traj['e'][:, pair_rows].cpu().long() != g['traj.e'][1:K + 1].long()).sum())}
    st = int(g['traj.x_stride'])
    got = traj['x'][st - 1::st][:, node_rows].cpu()
    ref = g['traj.x'][1:1 + got.shape[0]]
    res['x_frames_rel'] = float((got[:ref.shape[0]] - ref).abs().max() / ref.abs().max())
    norms = traj['x'][:, node_rows].reshape(K, 8, n * 3).norm(dim=2).cpu()              # (K, 8): per-molecule coordinate norm after every step
    res['x_norm_rel'] = float(((norms - g['traj.x_norm'][1:K + 1]).abs() / g['traj.x_norm'][1:K + 1]).max())
    if K == T - 1:
        res.update({'a_flips': int((state['a_t'].cpu()[nr].long() != g['a_1'].long()).sum()), 'c_flips': int((state['c_t'].cpu()[nr].long() != g['c_1'].long()).sum()),
                    'e_flips': int((state['e_t'].cpu()[pr].long() != g['e_1_upper'].long()).sum()),
                    'x_rel': float((state['x_t'].cpu()[nr] - g['x_1']).abs().max() / g['x_1'].abs().max())})
    _report('c3_full_batch_long' if B == 1024 else f'c4_whole_job_long[{B}x{n},{K} steps]', res)
    assert res['a_state_diffs_all_steps'] == 0 and res['c_state_diffs_all_steps'] == 0 and res['e_state_diffs_all_steps'] == 0, res
    assert res['x_frames_rel'] < 1e-4 and res['x_norm_rel'] < 1e-4, res
    assert torch.isfinite(state['x_t']).all()
    if K == T - 1:
        assert res['a_flips'] == res['c_flips'] == res['e_flips'] == 0 and res['x_rel'] < 1e-4, res
        assert (state['a_t'] != cfg.n_atom_types).all() and (state['e_t'] != cfg.n_bond_types).all()
    del traj
    torch.cuda.empty_cache()


@pytest.mark.parametrize('tag,name', [('flowmol3_47x8_T250', 'flowmol3'), ('flowmol3_mixed_T250_w2', 'flowmol3'), ('geom_ctmc_mixed_T500', 'geom_ctmc'),
                                      ('flowmol3_geom64_T250', 'flowmol3'), ('flowmol3_geom16_T250_pos128', 'flowmol3')])
def test_split_precision_long_horizon_flip_counts(golden_dir, tag, name):
    """The OPT-IN split precision on the reference's default-protocol trajectories: it is not f32 arithmetic, so token differences against the
    reference are COUNTED and reported (first divergent step, differing state tokens), not required to be zero; the run must stay finite, resolve
    every mask token, and -- where nothing flipped -- keep the coordinates within the 1e-4 target."""
    from flowmol_amd.engine import Engine
    from parity_util import integrate_long_golden
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(golden_dir / f'long_{tag}.npz').items()}
    cfg = presets.PRESETS[name]()
    scale = float(g['weight_scale']) * (float(g['pos_head_scale']) if 'pos_head_scale' in g else 1.0)
    eng = sp_engine_for(name)[2] if scale == 1 else Engine(cfg, weights.long_fixture_weights(cfg, g), device='cuda:0', precision='bf16x3')
    res = integrate_long_golden(eng, cfg, g)
    res['categorical_decisions'] = (int(g['T']) - 1) * int(2 * g['a_1'].numel() + g['e_1_upper'].numel())
    _report(f'split_precision_long[{tag}]', res)
    n_tokens = int(g['a_1'].numel() + g['c_1'].numel() + g['e_1_upper'].numel())
    flips = res['a_flips'] + res['c_flips'] + res['e_flips']
    assert flips <= max(4, n_tokens // 50), res
    if res['state_token_diffs_all_steps'] == 0:
        assert res['x_rel'] < 1e-4, res
