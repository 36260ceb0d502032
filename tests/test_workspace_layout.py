"""The workspace of a bound batch: fm_workspace_bytes against the formula of INTEGRATION.md ("Workspace size"), against recorded totals, and fm_batch_bind
into an arena of exactly that size; fm_integrate with a trajectory sink against the same steps made one by one with fm_forward + fm_ctmc_step.  The dirty-arena
and guard-band suites of test_state_hygiene.py prove that the regions do not overlap.  fm_integrate_mixed has no step-by-step counterpart here (fm_ctmc_step takes
one set of scalars for the batch): test_mixed_time.py holds it to every molecule run alone (through fm_integrate, so through the same step loop) and to the
oracle's replay (independent: tokens exact, positions to 1e-5).  That is a substitute for, not the same assertion as, a comparison against single steps."""
import ctypes as C

import pytest
import torch

import hygiene_util as hu
from flowmol_amd.engine import StepNoise

PRESETS = ['dev', 'flowmol3', 'geom_ctmc', 'arch_variants']          # dev (not arch_variants) is the preset with destination features, HX = 4: its Psd / PVd regions
                                                                     # have bytes and pair_slab does not change its totals, as RECORDED shows
SIZES = [[1], [2], [5, 1, 4], [2, 47, 9], [18, 17, 33]]              # the largest molecule crosses the 16-row chunk boundary: P = 1, 2, 2, 4, 3
TUNINGS = [{}, {'pair_slab': -1}, {'tile_edge': 16}, {'tile_edge': 32}]

# fm_workspace_bytes of the library BEFORE the workspace became one region list (commit 719f082), read from its host emulation: RECORDED[preset][tuning][sizes]
RECORDED = {
    'dev': [[4206080, 4219648, 4307968, 6080256, 5789440], [4206080, 4219648, 4307968, 6080256, 5789440], [4206080, 4219648, 4307968, 6081280, 5790208], [4206080, 4219648, 4307968, 6080256, 5789440]],
    'flowmol3': [[4205056, 4219648, 4332032, 8343552, 7419136], [4205056, 4217600, 4299264, 6053888, 5745920], [4205056, 4219648, 4332032, 8344576, 7419904], [4205056, 4219648, 4332032, 8343552, 7419136]],
    'geom_ctmc': [[4204032, 4215808, 4289792, 5976064, 5667328], [4204032, 4215808, 4289792, 5976064, 5667328], [4204032, 4215808, 4289792, 5977088, 5668096], [4204032, 4215808, 4289792, 5976064, 5667328]],
    'arch_variants': [[4204032, 4217856, 4322560, 8265728, 7340800], [4204032, 4215808, 4289792, 5976064, 5667584], [4204032, 4217856, 4322560, 8266752, 7341568], [4204032, 4217856, 4322560, 8265728, 7340800]],
}


def fixed(tuning):
    """The automatic edge-tile height depends on the CU count (the emulation reports 8, an MI355X 256): every case names its height.  So {} is the case
    {'tile_edge': 32} here (rows 0 and 3 of RECORDED are equal: 60 distinct totals)."""
    return {'tile_edge': 32, **tuning}


def documented_bytes(cfg, n_atoms, tuning):
    """INTEGRATION.md, "Workspace size", term by term."""
    r = lambda b: (b + 255) // 256 * 256                             # every region starts on a 256-byte boundary
    B, N, nmax = len(n_atoms), sum(n_atoms), max(n_atoms)
    E = sum(n * (n - 1) for n in n_atoms)
    U = E // 2
    V, HX = cfg.n_vec_channels, cfg.v_dst_feats
    na, nc, ne = cfg.n_atom_types, cfg.n_charges, cfg.n_bond_types
    PVW = ((V + 1 + HX + 4 + 7) // 8 * 8 + 8 + 15) // 16 * 16
    P = (nmax - 2) // 16 + 2 if nmax > 1 else 1
    tiles = sum(-(-n * (n - 1) // tuning['tile_edge']) for n in n_atoms)
    sched = cfg.update_schedule()
    slab = 0
    if tuning.get('pair_slab', 0) >= 0 and HX == 0 and cfg.self_conditioning and U > 0:
        slab = 2 if cfg.n_convs > 1 and sched[0] < 0 else 1
    tab_rows = -(-(na + 1) * (nc + 1) // 64) * 64
    total = 4 * r((B + 1) * 4) + r(tiles * 16)                       # molecule offsets (node, edge, pair, tile), tile descriptors
    total += 2 * r(N * 4) + 3 * r(E * 4) + 3 * r(U * 4)              # node, edge and pair index arrays
    total += 4 * r(N * 1024) + 2 * r(N * 12 * V) + 2 * r(N * 12)     # s, Ps, Asd, tap_s | v, tap_v | xw, boot.x
    total += r(E * 512) + r(N * 12 * PVW)                            # ef | PV
    total += (r(N * 1024) + r(N * 12 * PVW)) if HX else 0            # Psd | PVd
    total += r(N * P * 1024) + r(N * P * 12 * V)                     # part_s | part_v: P chunks per destination
    total += r(tab_rows * 1024 * 32)                                 # 32 embedding tables
    total += r(N * na * 4) + r(N * nc * 4) + r(U * ne * 4)           # boot.a, boot.c, boot.e
    total += r(B * 4) + 2 * r(N * 4) + r(U * 4)                      # molecule ids | endpoint tokens a, c | e
    total += slab * r(U * 1024)                                      # Q tables
    return total


def check_bytes(lib, device):
    for preset in PRESETS:
        for ti, tuning in enumerate(TUNINGS):
            eng, cfg, _ = hu.engine(preset, lib, device, tuning=fixed(tuning))
            for si, sizes in enumerate(SIZES):
                got = eng.workspace_need(torch.tensor(sizes))
                assert got == documented_bytes(cfg, sizes, fixed(tuning)), (preset, tuning, sizes, got, documented_bytes(cfg, sizes, fixed(tuning)))
                assert got == RECORDED[preset][ti][si], (preset, tuning, sizes, got, RECORDED[preset][ti][si])


def test_workspace_bytes_equal_the_documented_formula_on_emulation(emu_lib):
    check_bytes(emu_lib, 'cpu')


@pytest.mark.gpu
def test_workspace_bytes_equal_the_documented_formula_on_gpu():
    check_bytes(None, 'cuda:0')


def check_exact_arena(lib, device):
    """fm_batch_bind itself (Engine.bind checks the size before the library sees it)."""
    for preset, sizes in [('dev', [5, 1, 4]), ('flowmol3', [18, 17, 33])]:
        eng, cfg, _ = hu.engine(preset, lib, device, fresh=True)
        n = torch.tensor(sizes, dtype=torch.int32)
        need = eng.workspace_need(n)
        raw = torch.zeros(need + 256, dtype=torch.uint8, device=eng.device)
        base = (raw.data_ptr() + 255) // 256 * 256
        bind = lambda nbytes: eng.lib.fm_batch_bind(eng._ctx, eng._stream(), C.c_void_p(n.data_ptr()), n.numel(), C.c_void_p(base), C.c_size_t(nbytes))
        with eng._dev():
            assert bind(need - 1) != 0
            assert eng.lib.fm_last_error(eng._ctx).decode() == f'fm_batch_bind: workspace of {need - 1} bytes < required {need}'
            assert bind(need) == 0, eng.lib.fm_last_error(eng._ctx).decode()
        eng.synchronize()
        eng.close()


def test_bind_into_an_arena_of_exactly_the_reported_size_on_emulation(emu_lib):
    check_exact_arena(emu_lib, 'cpu')


@pytest.mark.gpu
def test_bind_into_an_arena_of_exactly_the_reported_size_on_gpu():
    check_exact_arena(None, 'cuda:0')


def check_integrate_equals_single_steps(lib, device, dfm_type):
    """T = 3 on [5, 1, 4]: one fm_integrate call with every frame of the trajectory sink, against fm_forward + fm_ctmc_step per step with the same scalars
    (campbell: Philox noise, gat: tensor noise, whose frames fm_integrate writes by copy).  States, frames and endpoint predictions bit for bit."""
    eng, cfg, _ = hu.engine('flowmol3', lib, device)
    sizes, T = [5, 1, 4], 3
    eng.bind(torch.tensor(sizes))
    plan = hu.philox_plan(cfg, T, 23, dfm_type) if dfm_type == 'campbell' else hu.tensor_plan(cfg, T, dfm_type)
    tape = None if dfm_type == 'campbell' else [StepNoise(**{k: None if getattr(nz, k) is None else getattr(nz, k).to(eng.device) for k in nz.__slots__})
                                                for nz in hu.noise_tape(cfg, eng.N, eng.U, plan, dfm_type)]
    K = len(plan.scalars)
    x0 = hu.prior_x0(eng.N).to(eng.device)
    f32, i32 = hu.sink_shapes(eng, K)
    traj = {**{k: torch.zeros(s_, device=eng.device) for k, s_ in f32.items()}, **{k: torch.zeros(s_, dtype=torch.int32, device=eng.device) for k, s_ in i32.items()}}
    state = eng.prior_state(x0.clone())
    eng.integrate(state, plan, None if tape is None else (lambda i, last: tape[i]), traj=traj)
    ref = eng.prior_state(x0.clone())
    prev = None
    for i, sc in enumerate(plan.scalars):
        dst = eng.forward(ref, float(plan.t[i]), prev=prev, bootstrap=prev is None and float(plan.t[i]) == 0.0)
        smp = {k: torch.zeros_like(traj[k][i]) for k in ('a1', 'c1', 'e1')}
        eng.ctmc_step(ref, dst, StepNoise() if tape is None else tape[i], sc, sampled=smp)
        eng.synchronize()
        for k, v in (('x', ref['x_t']), ('a', ref['a_t']), ('c', ref['c_t']), ('e', ref['e_t']), ('x1', dst['x']), ('a1', smp['a1']), ('c1', smp['c1']), ('e1', smp['e1'])):
            assert torch.equal(traj[k][i].cpu(), v.cpu().reshape(traj[k][i].shape)), (dfm_type, i, k)
        prev = dst
    for k in ('x_t', 'a_t', 'c_t', 'e_t'):
        assert torch.equal(state[k].cpu(), ref[k].cpu()), (dfm_type, k)


@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
def test_integrate_with_a_sink_equals_single_steps_on_emulation(emu_lib, dfm_type):
    check_integrate_equals_single_steps(emu_lib, 'cpu', dfm_type)


@pytest.mark.gpu
@pytest.mark.parametrize('dfm_type', ['campbell', 'gat'])
def test_integrate_with_a_sink_equals_single_steps_on_gpu(dfm_type):
    check_integrate_equals_single_steps(None, 'cuda:0', dfm_type)
