"""State hygiene: a result is a function of the call's arguments alone -- not of what the caller's arena held before the bind, not of earlier calls on
the context, not of how a trajectory is cut into fm_integrate calls -- and no kernel writes within 4 KiB outside a buffer it was given or into one of its
inputs.  Every comparison is bit for bit (the library is deterministic run to run and, for one plan, independent of the batch).  Every check runs on the host
emulation of the kernel sources (``emu_lib``) and, marked gpu, on the device; helpers, the ordering rule and what a guard band can see: hygiene_util.py.

Sections: A dirty arena under forward (every tap), B the other entry points and context history, C guard bands (every run of A, B and D is guarded: there
is no unguarded variant to compare with), D call patterns of fm_integrate."""
import pytest
import torch

import hygiene_util as hu
from parity_util import OUT_TOL, STAGE_TOL

PRED = [list(s) for s in hu.HISTORY_PREDECESSORS]
EMU_GATE = (2e-5, 2e-5)            # the oracle gate of tests/test_emu_parity.py
GPU_GATE = (STAGE_TOL, OUT_TOL)    # ... and of tests/test_gpu_parity.py

# preset, sizes, t, previous endpoint ('-' in the issue's table: t = 0.5 with a previous endpoint where the model is self-conditioned)
FORWARD_CASES = [('flowmol3', [5, 9, 12, 3, 2], 0.5, True),        # default case
                 ('flowmol3', [5, 9, 1, 3], 0.0, False),           # bootstrap: reads boot.*
                 ('qm9', [1], 0.5, True), ('qm9', [2], 0.5, True), ('qm9', [1, 1, 1], 0.5, True),        # E = 0 or 2
                 ('dev', [5, 1, 18, 2], 0.5, True),                # use_dst_feats: Psd / PVd
                 ('arch_variants', [5, 9, 1, 3, 2], 0.5, True),    # two recycles, 'mean' norm
                 ('geom_arom', [5, 17, 8, 2], 0.5, True)]          # 5 bond types
GPU_FORWARD_CASES = FORWARD_CASES + [('flowmol3', [70, 2, 47, 130], 0.5, True), ('flowmol3', [181, 2], 0.5, True)]     # up to 12 pieces per destination, destinations spanning tiles
TUNING_SIZES = [5, 18, 1, 3]
TUNINGS = [{'pair_slab': 1}, {'pair_slab': 1, 'pair_mlps': 1, 'mlp_small_tiles': -1}, {'tile_node': 4}, {'tile_node': 20}, {'tile_edge': 32},
           {'tile_edge': 64, 'tile_node': 64, 'tile_edge_update': 64}, {'mlp_small_tiles': 2}, {'xcd_swizzle': -1, 'fuse_node': -1}, {'ctmc_threads': 1024}]
PRECISIONS = ['bf16x3', 'bf16x6', 'f16x3']
EMU_SIZES = [4, 6, 3, 5]
GPU_SIZES = [3, 5, 24, 47, 70]          # the shapes tests/test_philox_modes.py argues for


def _ids(cases):
    return ['-'.join([c[0], 'x'.join(map(str, c[1]))] + [str(v) for v in c[2:]]) for c in cases]


def three_fills(eng, sizes, history, run):
    """``run(ws)`` -> (results, GuardSet or None) on a 'zero', a 'history' and then a 'ones' arena: arena bands, guard bands and inputs intact, every output
    written, and the results identical.  'ones' starts only after 'zero' and 'history' have passed.  -> the 'zero' results."""
    results = {}
    for fill in ('zero', 'history', 'ones'):
        ws, intact = hu.arena(eng, [sizes] + PRED, fill, history)
        res, gs = run(ws)
        assert intact(eng.workspace_bytes), f'{fill}: a write outside the arena handed to fm_batch_bind'
        if gs is not None:
            assert gs.check() == [], (fill, gs.check())
            assert gs.unwritten() == [], (fill, gs.unwritten())
        assert hu.non_finite(res) == [], (fill, hu.non_finite(res))
        results[fill] = res
        if fill != 'zero':
            assert hu.first_difference(results['zero'], res) is None, (fill, hu.first_difference(results['zero'], res))
    return results['zero']


# ================================================================================================================ A. dirty workspace, forward
def check_forward(lib, device, preset, sizes, t, prev, gate, tuning=None, precision=None):
    eng, cfg, sd = hu.engine(preset, lib, device, tuning, precision)
    inp = hu.forward_inputs(cfg, sizes, prev)
    seen = {}

    def run(ws):
        res, gs, stages = hu.forward_run(eng, inp, t, ws, sizes)
        if not seen and gate is not None:          # the 'zero' run: the three-way equality must not be of three wrong results
            seen['bad'] = hu.oracle_failures(eng, sd, inp, t, res, stages, *gate)
            assert not seen['bad'], seen['bad']
        seen.setdefault('stages', stages)
        return res, gs
    res = three_fills(eng, sizes, hu.forward_history, run)
    assert set(seen['stages']) <= set(res) and len(seen['stages']) >= 6


@pytest.mark.parametrize('preset,sizes,t,prev', FORWARD_CASES, ids=_ids(FORWARD_CASES))
def test_forward_does_not_depend_on_the_arena_on_emulation(emu_lib, preset, sizes, t, prev):
    check_forward(emu_lib, 'cpu', preset, sizes, t, prev, EMU_GATE)


@pytest.mark.gpu
@pytest.mark.parametrize('preset,sizes,t,prev', GPU_FORWARD_CASES, ids=_ids(GPU_FORWARD_CASES))
def test_forward_does_not_depend_on_the_arena_on_gpu(preset, sizes, t, prev):
    check_forward(None, 'cuda:0', preset, sizes, t, prev, GPU_GATE)


@pytest.mark.parametrize('tuning', TUNINGS, ids=[str(i) for i in range(len(TUNINGS))])
def test_forward_under_every_tuning_does_not_depend_on_the_arena_on_emulation(emu_lib, tuning):
    check_forward(emu_lib, 'cpu', 'flowmol3', TUNING_SIZES, 0.5, True, EMU_GATE, tuning=tuning)


@pytest.mark.gpu
@pytest.mark.parametrize('tuning', TUNINGS, ids=[str(i) for i in range(len(TUNINGS))])
def test_forward_under_every_tuning_does_not_depend_on_the_arena_on_gpu(tuning):
    check_forward(None, 'cuda:0', 'flowmol3', TUNING_SIZES, 0.5, True, GPU_GATE, tuning=tuning)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_forward_in_split_precision_does_not_depend_on_the_arena_on_emulation(emu_lib, precision):
    """(the split precisions have oracle gates of their own in the parity tests; here only the equality and the guards)"""
    check_forward(emu_lib, 'cpu', 'flowmol3', TUNING_SIZES, 0.5, True, None, precision=precision)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_forward_in_split_precision_does_not_depend_on_the_arena_on_gpu(precision):
    check_forward(None, 'cuda:0', 'flowmol3', TUNING_SIZES, 0.5, True, None, precision=precision)


# ================================================================================================================ B. the other entry points
def check_sample(lib, device, preset, sizes, dfm_type, nt=0):
    mdl = hu.model(preset, lib, device, nt)
    eng = mdl.engine

    def run(ws):
        eng.bind(torch.tensor(sizes), workspace=ws)          # model.sample binds the same sizes again and stays in this arena
        res = hu.sample_run(mdl, sizes, dfm_type)
        assert eng._ws is ws
        return res, None
    res = three_fills(eng, sizes, hu.sample_history, run)
    masks = {'a': mdl.cfg.n_atom_types, 'c': mdl.cfg.n_charges, 'e': mdl.cfg.n_bond_types}
    assert any(bool((res[f'final.{k}'] != m).any()) for k, m in masks.items())          # something was unmasked: not three untouched priors
    eng.close()


@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
@pytest.mark.parametrize('preset', ['qm9', 'flowmol3'])
def test_philox_sample_does_not_depend_on_the_arena_on_emulation(emu_lib, preset, dfm_type):
    check_sample(emu_lib, 'cpu', preset, EMU_SIZES, dfm_type)


@pytest.mark.gpu
@pytest.mark.parametrize('nt', [256, 1024])
@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
@pytest.mark.parametrize('preset', ['qm9', 'flowmol3'])
def test_philox_sample_does_not_depend_on_the_arena_on_gpu(preset, dfm_type, nt):
    check_sample(None, 'cuda:0', preset, GPU_SIZES, dfm_type, nt)


def _tuning(nt):
    return {'ctmc_threads': nt} if nt else None


def check_integrate(lib, device, preset, sizes, dfm_type, nt=0):
    eng, cfg, _ = hu.engine(preset, lib, device, _tuning(nt))
    res = three_fills(eng, sizes, hu.sample_history, lambda ws: hu.integrate_run(eng, sizes, dfm_type, ws))
    assert res['sink.x'].shape[0] == 5 and not torch.equal(res['sink.x'][0], res['sink.x'][4])


@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
@pytest.mark.parametrize('preset', ['qm9', 'flowmol3'])
def test_tensor_noise_integrate_with_every_sink_does_not_depend_on_the_arena_on_emulation(emu_lib, preset, dfm_type):
    check_integrate(emu_lib, 'cpu', preset, EMU_SIZES, dfm_type)


@pytest.mark.gpu
@pytest.mark.parametrize('nt', [256, 1024])
@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
@pytest.mark.parametrize('preset', ['qm9', 'flowmol3'])
def test_tensor_noise_integrate_with_every_sink_does_not_depend_on_the_arena_on_gpu(preset, dfm_type, nt):
    check_integrate(None, 'cuda:0', preset, GPU_SIZES, dfm_type, nt)


def check_small_calls(lib, device, preset, sizes, nt=0):
    eng, cfg, _ = hu.engine(preset, lib, device, _tuning(nt))
    for dfm_type in ('campbell', 'gat'):
        three_fills(eng, sizes, hu.sample_history, lambda ws: hu.ctmc_step_run(eng, sizes, dfm_type, ws))
    three_fills(eng, sizes, hu.sample_history, lambda ws: hu.small_calls_run(eng, sizes, ws))


@pytest.mark.parametrize('preset', ['qm9', 'flowmol3'])
def test_ctmc_step_priors_tape_stability_and_queries_do_not_depend_on_the_arena_on_emulation(emu_lib, preset):
    check_small_calls(emu_lib, 'cpu', preset, EMU_SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize('nt', [256, 1024])
@pytest.mark.parametrize('preset', ['qm9', 'flowmol3'])
def test_ctmc_step_priors_tape_stability_and_queries_do_not_depend_on_the_arena_on_gpu(preset, nt):
    check_small_calls(None, 'cuda:0', preset, GPU_SIZES, nt)


def check_endpoint(lib, device, sizes):
    eng, cfg, _ = hu.engine('endpoint_small', lib, device)

    def run(ws):
        res, gs, bad = hu.endpoint_run(eng, sizes, ws)
        assert bad == [], bad
        return res, gs
    three_fills(eng, sizes, hu.forward_history, run)


def test_endpoint_calls_do_not_depend_on_the_arena_on_emulation(emu_lib):
    check_endpoint(emu_lib, 'cpu', EMU_SIZES)


@pytest.mark.gpu
def test_endpoint_calls_do_not_depend_on_the_arena_on_gpu():
    check_endpoint(None, 'cuda:0', GPU_SIZES)


# ---------------------------------------------------------------------------------------------------------------- context history
def _philox_traj(eng, sizes, dfm_type, T, seed, ws, tspan=None, rebind=True):
    """Philox prior + integrate with the state frames on the engine as it is -> results."""
    if rebind:
        eng.bind(torch.tensor(sizes), workspace=ws)
    plan = hu.philox_plan(eng.cfg, T, seed, dfm_type, tspan=tspan)
    state = eng.prior_state(eng.prior_philox(seed))
    n = len(plan.scalars)
    traj = {'x': torch.zeros(n, eng.N, 3, device=eng.device), 'e': torch.zeros(n, eng.U, dtype=torch.int32, device=eng.device)}
    last = eng.integrate(state, plan, None, traj=traj)
    return hu.cpu({**state, **{f'sink.{k}': v for k, v in traj.items()}, **{f'last.{k}': v for k, v in last.items()}})


def _fresh(preset, lib, device, sizes, fill='zero'):
    eng, cfg, sd = hu.engine(preset, lib, device, fresh=True)
    ws, intact = hu.arena(eng, [sizes] + PRED, fill)
    return eng, ws, intact


def check_molecule_ids_do_not_survive_a_bind(lib, device, sizes):
    """set_molecule_ids([7, 8, 9]), then a re-bind: the new batch's streams are those of ids 0..B-1 (set explicitly on the fresh engine)."""
    ref_eng, ws, _ = _fresh('qm9', lib, device, sizes)
    ref_eng.bind(torch.tensor(sizes), workspace=ws)
    ref_eng.set_molecule_ids(torch.arange(len(sizes)))
    want = _philox_traj(ref_eng, sizes, 'campbell', 4, 31, ws, rebind=False)
    ref_eng.set_molecule_ids(torch.arange(len(sizes)) + 7)
    other = _philox_traj(ref_eng, sizes, 'campbell', 4, 31, ws, rebind=False)
    assert hu.first_difference(want, other) is not None          # the ids do move the streams
    ref_eng.close()
    for fill in ('zero', 'ones'):
        eng, ws, intact = _fresh('qm9', lib, device, sizes, fill)
        eng.bind(torch.tensor(sizes[:3]), workspace=ws)
        eng.set_molecule_ids(torch.tensor([7, 8, 9]))
        got = _philox_traj(eng, sizes, 'campbell', 4, 31, ws)
        assert intact() and hu.first_difference(want, got) is None, (fill, hu.first_difference(want, got))
        eng.close()


def test_molecule_ids_do_not_survive_a_bind_on_emulation(emu_lib):
    check_molecule_ids_do_not_survive_a_bind(emu_lib, 'cpu', EMU_SIZES)


@pytest.mark.gpu
def test_molecule_ids_do_not_survive_a_bind_on_gpu():
    check_molecule_ids_do_not_survive_a_bind(None, 'cuda:0', GPU_SIZES)


def check_forward_history(lib, device, sizes):
    """Taps registered by one forward are gone in the next; bootstrap and self-conditioned evaluations do not see each other; the profiler changes nothing.
    Each second half is compared with a fresh engine doing only that."""
    preset = 'flowmol3'
    ref, cfg, sd = hu.engine(preset, lib, device, fresh=True)
    eng, _, _ = hu.engine(preset, lib, device, fresh=True)
    n = torch.tensor(sizes)
    inp_p, inp_b = hu.forward_inputs(cfg, sizes, True), hu.forward_inputs(cfg, sizes, False)

    def fwd(e, inp, t, taps=None):
        st = e.make_state(inp['x'], inp['a'], inp['c'], inp['eu'])
        prev = None if inp['prev'] is None else {k: v.to(e.device).contiguous() for k, v in inp['prev'].items()}
        out = e.forward(st, t, prev=prev, bootstrap=(t == 0 and prev is None), taps=taps)
        e.synchronize()
        return hu.cpu(out)
    ws_r, _ = hu.arena(ref, [sizes], 'zero')
    ref.bind(n, workspace=ws_r)
    want_prev = fwd(ref, inp_p, 0.5)
    ref.close()
    ref, _, _ = hu.engine(preset, lib, device, fresh=True)
    ref.bind(n, workspace=ws_r)
    want_boot = fwd(ref, inp_b, 0.0)
    ref.close()
    assert hu.first_difference(want_prev, want_boot) is not None
    ws, intact = hu.arena(eng, [sizes], 'zero')
    eng.bind(n, workspace=ws)
    # a forward with taps, then one without: same result as the fresh engine, and the old tap buffers (refilled with a sentinel) stay untouched
    stages = hu.parity_stages(cfg, 0.5, True)
    taps = {k: torch.zeros(*s, device=eng.device) for k, s in hu.tap_shapes(eng, stages).items()}
    fwd(eng, inp_p, 0.5, taps)
    assert all(bool((v != 0).any()) for v in taps.values())
    for v in taps.values():
        v.fill_(-7.0)
    assert hu.first_difference(want_prev, fwd(eng, inp_p, 0.5)) is None
    assert all(bool((v == -7.0).all()) for v in taps.values())
    # bootstrap after prev, prev after bootstrap
    assert hu.first_difference(want_boot, fwd(eng, inp_b, 0.0)) is None
    assert hu.first_difference(want_prev, fwd(eng, inp_p, 0.5)) is None
    # the profiler in between
    eng.profile(True)
    assert hu.first_difference(want_boot, fwd(eng, inp_b, 0.0)) is None
    assert eng.profile_get('edge_message')[1] + eng.profile_get('node')[1] >= 0
    eng.profile(False)
    assert hu.first_difference(want_prev, fwd(eng, inp_p, 0.5)) is None
    assert intact(eng.workspace_bytes)
    eng.close()


def test_taps_bootstrap_and_profiler_leave_nothing_behind_on_emulation(emu_lib):
    check_forward_history(emu_lib, 'cpu', [5, 9, 1, 3])


@pytest.mark.gpu
def test_taps_bootstrap_and_profiler_leave_nothing_behind_on_gpu():
    check_forward_history(None, 'cuda:0', [5, 9, 1, 3, 47])


def check_integrate_after_another_plan(lib, device, sizes):
    """integrate under one plan (T = 6, campbell), then under another (T = 4, gat, another tspan) on the same bind = a fresh engine doing only the second:
    the table slots, boot.* and the CTMC scratch of the first trajectory are not seen."""
    tspan = torch.tensor([0.0, 0.2, 0.55, 1.0])
    ref, ws_r, _ = _fresh('flowmol3', lib, device, sizes)
    want = _philox_traj(ref, sizes, 'gat', 4, 9, ws_r, tspan=tspan)
    ref.close()
    eng, ws, intact = _fresh('flowmol3', lib, device, sizes)
    _philox_traj(eng, sizes, 'campbell', 6, 5, ws)
    got = _philox_traj(eng, sizes, 'gat', 4, 9, ws, tspan=tspan, rebind=False)
    assert intact(eng.workspace_bytes) and hu.first_difference(want, got) is None, hu.first_difference(want, got)
    eng.close()


def test_integrate_after_another_plan_on_emulation(emu_lib):
    check_integrate_after_another_plan(emu_lib, 'cpu', EMU_SIZES)


@pytest.mark.gpu
def test_integrate_after_another_plan_on_gpu():
    check_integrate_after_another_plan(None, 'cuda:0', GPU_SIZES)


# ================================================================================================================ D. call patterns of fm_integrate
def check_chunkings(lib, device, preset, sizes, dfm_type, T, chunks):
    """One Philox plan run as ONE fm_integrate call (FM_TAB_SLOTS = 32: the embedding tables are rebuilt inside the call, which the profiler confirms), and cut
    at and off the table boundary: identical final state, last endpoint prediction and frames at every step; all buffers guarded."""
    eng, cfg, _ = hu.engine(preset, lib, device)
    K = T - 1
    assert chunks[0] == K
    base = None
    for chunk in chunks:
        ws, intact = hu.arena(eng, [sizes], 'zero')
        res, gs, launches = hu.chunked_run(eng, sizes, dfm_type, T, chunk, ws, profile=True)
        assert intact(eng.workspace_bytes) and gs.check() == [] and gs.unwritten() == [], (chunk, gs.check(), gs.unwritten())
        calls = -(-K // chunk)
        want = sum(-(-min(chunk, K - c * chunk) // 32) for c in range(calls))
        assert launches == want, (chunk, launches, want)
        if base is None:
            assert launches == -(-K // 32) and launches >= 2          # the in-call rebuild did run
            base = res
        else:
            assert hu.first_difference(base, res) is None, (chunk, hu.first_difference(base, res))
    assert not torch.equal(base['sink.x'][0], base['sink.x'][K - 1])


@pytest.mark.parametrize('preset,sizes,dfm_type,T', [('dev', [3, 2, 4], 'campbell', 71), ('qm9', [3, 2, 4], 'gat', 36)])
def test_result_does_not_depend_on_how_the_trajectory_is_cut_on_emulation(emu_lib, preset, sizes, dfm_type, T):
    check_chunkings(emu_lib, 'cpu', preset, sizes, dfm_type, T, [T - 1, 32, 7])


@pytest.mark.gpu
@pytest.mark.parametrize('preset,sizes,dfm_type,T,chunks', [('dev', [3, 2, 4], 'campbell', 71, [70, 32, 7]), ('qm9', [3, 2, 4], 'gat', 36, [35, 32, 7]),
                                                           ('flowmol3', [47, 5], 'campbell', 71, [70, 33, 1])])
def test_result_does_not_depend_on_how_the_trajectory_is_cut_on_gpu(preset, sizes, dfm_type, T, chunks):
    check_chunkings(None, 'cuda:0', preset, sizes, dfm_type, T, chunks)


# ================================================================================================================ the product change
def test_bind_takes_a_caller_owned_workspace_and_refuses_unfit_ones(emu_lib):
    eng, cfg, _ = hu.engine('qm9', emu_lib, 'cpu', fresh=True)
    n = torch.tensor([3, 4])
    need = eng.workspace_need(n)
    raw = torch.zeros(need + 512, dtype=torch.uint8)
    off = (-raw.data_ptr()) % 256
    ws = raw[off:off + need]
    eng.bind(n, workspace=ws)
    assert eng._ws is ws and eng.workspace_bytes == need
    eng.bind(torch.tensor([2, 2]))                       # fits: stays in the caller's arena
    assert eng._ws is ws
    with pytest.raises(ValueError, match='256-byte aligned'):
        eng.bind(n, workspace=raw[off + 1:off + 1 + need])
    with pytest.raises(ValueError, match='bytes, the batch needs'):
        eng.bind(n, workspace=ws[:need - 256])
    with pytest.raises(ValueError, match='uint8'):
        eng.bind(n, workspace=torch.zeros(need, dtype=torch.float32))
    with pytest.raises(ValueError, match='must be on'):
        eng.bind(n, workspace=torch.zeros(need + 256, dtype=torch.uint8, device='meta'))
    eng.bind(torch.tensor([30, 30]))                     # does not fit: the engine allocates its own and leaves the caller's alone
    assert eng._ws is not ws and bool((raw[off + need:] == 0).all())
    eng.close()
