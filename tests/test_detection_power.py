"""Detection power of the parity scoring itself, on the CPU oracle alone (no GPU, no emulation): would the stage / output / displacement
errors that tests/test_emu_parity.py and tests/test_gpu_parity.py gate on notice a 1 % error, or two exchanged rows, in ANY ONE weight tensor?
The scoring is parity_util.stage_errors() in both places, so what is proven here about the oracle-vs-oracle score holds for the
engine-vs-oracle score."""
import pytest
import torch

from flowmol_amd import presets, weights
from oracle import cpu_ref
from parity_util import POS_HEAD_SCALE, oracle_mutation_audit, oracle_run, seeded_inputs, visible_weights

PRESETS = ['flowmol3', 'geom_ctmc', 'qm9', 'dev', 'dev_narrow', 'arch_variants', 'geom_arom', 'flowmol3_arom']      # every preset of the parity tests
SIZES, T, PREV = [5, 9, 12, 3, 2], 0.5, True          # the first case of test_forward_matches_oracle

MARGIN = 3        # a 1 % error in one tensor must stand this far above the gate: a condition, not a measurement -- it is the room that keeps the gates from being loosened

# Read tensors that no metric can see, per preset (capped at 2 % of the preset's read tensors below).
# conv_layers.0.edge_message.{0,1,2}.Wcp: the node vectors entering the first convolution are zero (vector_field.py:241), so every vector of an edge of
# conv 0 -- through all three message GVPs -- is a multiple of that edge's x_diff and the cross products these matrices feed are 0 in exact arithmetic
# (what is left is the rounding of a1*b2 - a2*b1).  A recycled stack (arch_variants) meets conv 0 again with non-zero vectors: nothing is listed there.
ALLOW = {name: ([f'conv_layers.0.edge_message.{g}.Wcp' for g in range(3)] if name != 'arch_variants' else []) for name in PRESETS}


def expected_unread(cfg, sd, with_prev, t):
    """The tensors one network evaluation never reads, or reads only as a factor of exact zeros -- derived from the config."""
    sched = cfg.update_schedule()
    used = {u for u in sched if u >= 0}
    out = set()
    for k, v in sd.items():
        if v.numel() == 0:                                                     # dropout.vector_dropout.dummy_param
            out.add(k)
        for u in range(cfg.n_updaters):                                        # separate updaters with one conv per update: updater 0 follows no conv
            if u not in used and (k.startswith(f'node_position_updaters.{u}.') or k.startswith(f'edge_updaters.{u}.')):
                out.add(k)
        # node vectors are zero entering conv 0 of the first pass: its destination-feature projection has no vector output to weigh or gate
        if cfg.use_dst_feats and getattr(cfg, 'n_recycles', 1) <= 1 and k.startswith('conv_layers.0.dst_feat_msg_projection.') \
                and k.endswith(('.Wh', '.Wu', 'scalar_to_vector_gates.weight', 'scalar_to_vector_gates.bias')):
            out.add(k)
        if k.startswith('self_conditioning_residual_layer.') and not (with_prev or t == 0):
            out.add(k)
    return out


@pytest.mark.parametrize('name', PRESETS)
def test_pos_head_scale_is_the_smallest_power_of_two_with_visible_displacements(name):
    """POS_HEAD_SCALE[name] is the smallest power of two for which every NodePositionUpdate call of the oracle under visible_weights() displaces the
    atoms by at least 1e-3 of max|x| (so the f32 subtraction floor of a `dx` stage, 4 ulp(max|x|) / max|dx| ~ 4 * 6e-8 / 1e-3, stays ~100x below a 1 %
    error).  Measured with MATRIX_GAIN = 2 and factor 1, smallest .. largest call: flowmol3 3.0e-2 .. 9.1e-2 (weights as drawn: 1.0e-5 .. 5.5e-5; as drawn
    with the heads x128: 1.3e-3 .. 7.0e-3), so the factor is 1 for every preset today; a preset whose displacements shrink makes this test name the factor."""
    cfg = presets.PRESETS[name]()
    sd0 = weights.synth_state_dict(cfg, 0)
    inp = seeded_inputs(cfg, torch.tensor(SIZES), PREV)

    def smallest(factor):
        orc = cpu_ref.OracleVF(cfg, visible_weights(name, sd0, pos_head_scale=factor))
        ratios, plain = [], orc.position_update

        def recording(u, s, x, v):
            x2 = plain(u, s, x, v)
            ratios.append(float((x2 - x).abs().max() / x.abs().max()))
            return x2
        orc.position_update = recording
        oracle_run(orc, cfg, inp, T)
        assert len(ratios) == sum(u >= 0 for u in cfg.update_schedule()) * getattr(cfg, 'n_recycles', 1)
        print(f'{name}: pos_head_scale {factor}: max|dx| / max|x| per update', ['%.2e' % r for r in ratios])
        return min(ratios)
    f = POS_HEAD_SCALE[name]
    assert f >= 1 and f & (f - 1) == 0
    assert smallest(f) >= 1e-3
    if f > 1:
        assert smallest(f // 2) < 1e-3


@pytest.mark.parametrize('name', PRESETS)
def test_parity_scoring_sees_one_percent_in_every_read_tensor(name, record_property):
    """parity_util.oracle_mutation_audit under the displacement metric and visible_weights(): every tensor the evaluation reads is flagged with
    error / tolerance >= MARGIN by its x1.01 or its row-swap perturbation, except the commented ALLOW list (<= 2 % of the read tensors); the
    unread tensors are exactly the ones the config implies.  Recorded, not asserted: the same count for the stages-and-outputs metric at the
    weights as drawn -- flowmol3: 199 of its 469 non-empty tensors pass a x1.01 error unseen there (172 read ones + the 27 of the unused updater 0)."""
    cfg = presets.PRESETS[name]()
    sd0 = weights.synth_state_dict(cfg, 0)
    sizes = torch.tensor(SIZES)
    want_unread = expected_unread(cfg, sd0, PREV, T)

    old = oracle_mutation_audit(cfg, sd0, sizes, T, PREV, 'x', kinds=('scale',))
    non_empty = [k for k in sd0 if sd0[k].numel()]
    old_unseen = [k for k in non_empty if not old[k]['scale'] >= 1]
    record_property('unseen_by_stage_metric_at_unit_weights', f'{len(old_unseen)} of {len(non_empty)}')
    print(f'{name}: x1.01 in one tensor unseen by the stage / output metric at the weights as drawn: {len(old_unseen)} of {len(non_empty)}')

    new = oracle_mutation_audit(cfg, visible_weights(name, sd0), sizes, T, PREV, 'dx')
    unread = {k for k, r in new.items() if r['unread']}
    assert unread == want_unread, (sorted(unread - want_unread), sorted(want_unread - unread))
    read = [k for k in new if k not in unread]
    power = {k: max(new[k]['scale'], new[k]['swap'] or 0.0) for k in read}
    weak = {k: v for k, v in power.items() if not v >= MARGIN}
    record_property('below_margin_under_displacement_metric', f'{len(weak)} of {len(read)}')
    print(f'{name}: below {MARGIN} x tolerance under the displacement metric / visible weights: {len(weak)} of {len(read)} read tensors: {weak}; '
          f'smallest flagged: {min(v for k, v in power.items() if k not in weak):.1f}')
    assert len(ALLOW[name]) <= 0.02 * len(read)
    assert set(weak) <= set(ALLOW[name]), {k: v for k, v in weak.items() if k not in ALLOW[name]}
