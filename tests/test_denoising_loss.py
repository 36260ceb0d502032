"""The denoising loss of given molecules: the reference's FlowMol.forward (flowmol/models/flowmol.py:297-415) on the HIP path -- the loss epilogue of the
output heads (logits stay on chip), the per-molecule reduction fm_k_denoise_reduce, the geometry distortion fm_k_distort_philox, the C entry points
fm_denoising_loss / fm_distort_philox, Engine.denoising_loss / distort and FlowMol.denoising_loss.

What is checked.  (1) the reduction alone on row terms written by the test, torch.equal a numpy restatement of the documented order; (2) the row terms
against the oracle's logits with torch's cross_entropy and the reference's ignore rule, within 4x the oracle's own float32-vs-float64 noise on the same
inputs; (3) the regime that needs logits: target probabilities that are exactly 0, finite nll; (4) exp(-nll) against the probabilities of the existing heads;
(5) a batch of mixed t bit-identical to every molecule alone, 33 distinct t in two binds included; (6) the distortion against an independent numpy Philox,
its formula, its switch and its moments; (7) the batch values against a torch restatement of flowmol.py:388-413, outer-product broadcast included;
(8) a guarded call and every refusal.  Every check runs on the CPU emulation of the kernel sources and, marked gpu, on the device.

Shapes.  Reduction and distortion (no network evaluation): the qm9 preset bound to 1, 2, 5, 24, 47 atoms -- 0 pairs, 1 pair, pair rows below (276 = 18
chunks) and above (1081 = 68 chunks) one 64-chunk pass of the wave, a molecule boundary behind each -- in three time groups.  Row terms: the narrow
self-conditioned `dev` model with 5, 3, 2, 1 atoms in three time groups; on the GPU also flowmol3 with 5 and 9 atoms."""
import ctypes as C

import numpy as np
import pytest
import torch

from flowmol_amd import _lib
from flowmol_amd.engine import fm_state
import loss_util as lu
import mixed_util as mu
import resample_util as ru

SEED = lu.SEED
MARGIN = 4.0          # over the measured float32-vs-float64 noise of the oracle: the margin STAGE_TOL has over measured stage noise in parity_util


# ---------------------------------------------------------------------------------------------------------------- 1. the reduction alone
def _check_reduction(lib, device):
    eng, cfg, _ = mu.engine('qm9', lib, device)
    sizes = lu.REDUCE_SIZES
    eng.bind(torch.tensor(sizes))
    gen = torch.Generator().manual_seed(5)
    x1 = ru.as_state(eng, ru.given(cfg, sizes))
    xt = {'x_t': x1['x_t']}
    for k in 'ace':          # about half of the rows masked, the 2-atom molecule's single pair among them
        tok = x1[f'{k}_t'].cpu().clone()
        tok[torch.rand(tok.shape, generator=gen) < 0.5] = lu.MASKS(cfg)[k]
        xt[f'{k}_t'] = tok.to(device)
    xt['e_t'][0] = cfg.n_bond_types
    rows = {'x': torch.rand(eng.N, generator=gen) * 3, 'a': torch.randn(eng.N, generator=gen).abs() * 2, 'c': torch.rand(eng.N, generator=gen) * 40,
            'e': torch.randn(eng.U, generator=gen).abs() * 5}
    res = eng.denoising_loss(xt, x1, lu.REDUCE_T, rows=rows)
    eng.synchronize()
    got = res['mol'].cpu()
    want = lu.mol_table(rows, {k: xt[f'{k}_t'].cpu() for k in 'ace'}, cfg, sizes)
    assert torch.equal(got, want), (got, want)
    assert got[0, 6] == 0 and got[0, 7] == 0          # the 1-atom molecule: no pairs
    assert got[1, 7] == 1 and got[1, 6] == rows['e'][0]
    assert torch.equal(got[:, 1], 3.0 * torch.tensor(sizes, dtype=torch.float32))
    for k in 'xace':
        assert torch.equal(res['rows'][k].cpu(), rows[k])          # the caller's terms are only read
    # the documented order is not the plain running sum: the restatement would not pass with another order
    assert float(want[4, 6]) != float(np.cumsum(rows['e'][-1081:].numpy(), dtype=np.float32)[-1])


def test_reduction_is_the_documented_order_on_emulation(emu_lib):
    _check_reduction(emu_lib, 'cpu')


@pytest.mark.gpu
def test_reduction_is_the_documented_order_on_gpu():
    _check_reduction(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 2. row terms against the reference
def _check_rows(lib, device, preset, sizes, times, head_scale=1.0):
    """The tolerance is the reference's own rounding noise on exactly these inputs -- the oracle in float32 against the oracle with its state dict cast to
    float64, per term as max |difference| / max |float64 value| -- times MARGIN = 4, measured in the run (it depends on the CPU's BLAS order).  Measured,
    oracle noise -> library error: dev 5/3/2/1 atoms on the emulation x 3.6e-8 -> 0, a 8.7e-8 -> 8.8e-8, c 9.8e-8 -> 1.1e-7, e 1.5e-7 -> 1.8e-7; on the
    MI355X a 5.2e-8 -> 8.8e-8, c 5.1e-8 -> 1.1e-7, e 2.1e-7 -> 3.6e-7; flowmol3 5/9 atoms on the MI355X x 7.6e-8 -> 0, a 8.3e-8 -> 1.7e-7, c 8.0e-8 -> 1.8e-7,
    e 1.8e-7 -> 1.7e-7.  (x: with weights-by-name the position update is below 0.1 % of the coordinates, its rounding differences vanish in the squared
    error.)"""
    case = lu.loss_case(preset, lib, device, sizes, times, head_scale)
    noise, want = lu.rounding_noise(case)
    tg = lu.targets(case)
    for k in 'xace':
        got = case['rows'][k]
        if k != 'x':
            ignored = tg[k] < 0
            assert torch.equal(got[ignored], torch.zeros(int(ignored.sum()))) and not bool(torch.signbit(got[ignored]).any()), k      # exactly +0.0
            assert bool((got[~ignored] > 0).all()), k                      # and nothing else is: the ignored rows are exactly the unmasked rows
            assert 0 < int(ignored.sum()) < got.numel(), k
        if want[k].numel():
            err = float((got.double() - want[k].double()).abs().max() / want[k].abs().max())
            print(f'{preset} x{head_scale} {device} {k}: error {err:.3e}, oracle noise {noise[k]:.3e}')
            assert err <= MARGIN * noise[k], (k, err, noise[k])
    assert torch.equal(case['mol'], lu.mol_table(case['rows'], {k: case['xt'][f'{k}_t'] for k in 'ace'}, case['cfg'], case['sizes']))
    return case, noise, want


def test_row_terms_match_the_reference_on_emulation(emu_lib):
    _check_rows(emu_lib, 'cpu', 'dev', lu.ROW_SIZES, lu.ROW_T)


@pytest.mark.gpu
@pytest.mark.parametrize('preset,sizes,times', [('dev', lu.ROW_SIZES, lu.ROW_T), ('flowmol3', lu.GPU_SIZES, lu.GPU_T)])
def test_row_terms_match_the_reference_on_gpu(preset, sizes, times):
    _check_rows(None, 'cuda:0', preset, sizes, times)


# ---------------------------------------------------------------------------------------------------------------- 3. the regime that motivates logits
def _check_zero_probabilities(lib, device):
    case = lu.loss_case('dev', lib, device, head_scale=256.0)
    noise, want = lu.rounding_noise(case)
    tg, seen = lu.targets(case), 0
    for k in 'ace':
        keep = tg[k] >= 0
        p = case['probs'][k][keep].gather(1, tg[k][keep].unsqueeze(1)).squeeze(1)
        zero = p == 0.0          # -log p = inf from the probabilities fm_forward returns
        seen += int(zero.sum())
        got, ref = case['rows'][k][keep][zero].double(), want[k][keep][zero].double()
        assert bool(torch.isfinite(got).all()) and bool((got > 80).all()), k          # p < 2^-149 means nll > 103; float32 exp underflows to 0 from 87.3 with s >= 1
        assert bool(((got - ref).abs() <= MARGIN * noise[k] * ref.abs()).all()), (k, got, ref, noise[k])
    assert seen >= 1


def test_zero_probability_targets_have_finite_nll_on_emulation(emu_lib):
    _check_zero_probabilities(emu_lib, 'cpu')


@pytest.mark.gpu
def test_zero_probability_targets_have_finite_nll_on_gpu():
    _check_zero_probabilities(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 4. consistency with the existing heads
def _check_heads_agree(lib, device):
    """With u = 2^-24 (half an ulp, relative) and expf / logf within 1 ulp = 2u:  p = expf(l_t - m) / s carries u |l_t - m| from the subtraction (the
    argument of an exponential: an absolute error there is a relative one here), 2u from expf and u from the division, and |l_t - m| <= |nll| + log K with
    log K <= log 16 < 3;  nll = (logf(s) + m) - l_t carries 2u |log s| <= 6u from logf, u |logf(s) + m| <= u (3 + L) from the addition (L = the largest
    |logit| of the head, taken from the oracle) and u |nll| from the subtraction, an absolute error of nll being a relative one of exp(-nll).  Sum:
    u (15 + L + 2 |nll|) <= u (15 + L) (1 + |nll|), the bound used, on the relative difference of exp(-nll) and p."""
    case = lu.loss_case('dev', lib, device)
    cfg, xt = case['cfg'], case['xt']
    batch = lu.cpu_ref.build_batch(torch.tensor(case['sizes']))
    a1h, c1h, e1h = lu.onehots(cfg, batch, xt['a_t'].long(), xt['c_t'].long(), xt['e_t'].long())
    with torch.no_grad():
        logits = lu.cpu_ref.OracleVF(cfg, case['sd']).forward(batch, xt['x_t'], a1h, c1h, e1h, case['t'], prev=None, apply_softmax=False, remove_com=False)
    tg, n = lu.targets(case), 0
    for k in 'ace':
        keep = tg[k] >= 0
        p = case['probs'][k][keep].gather(1, tg[k][keep].unsqueeze(1)).squeeze(1).double()
        nll = case['rows'][k][keep].double()
        normal = p >= 2.0 ** -126
        L = float(logits[k].abs().max())
        bound = 2.0 ** -24 * (15 + L) * (1 + nll.abs())
        rel = ((torch.exp(-nll) - p).abs() / p)[normal]
        assert bool((rel <= bound[normal]).all()), (k, rel, bound[normal])
        n += int(normal.sum())
    assert n >= 10


def test_nll_agrees_with_the_probability_heads_on_emulation(emu_lib):
    _check_heads_agree(emu_lib, 'cpu')


@pytest.mark.gpu
def test_nll_agrees_with_the_probability_heads_on_gpu():
    _check_heads_agree(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 5. batch independence
def _alone(mdl, mols, i, t, mol_id, **kw):
    return mdl.denoising_loss(ru.take(mols, [i]), float(t), seed=SEED, mol_ids=[mol_id], **kw)


def _same_molecule(batch, sizes, i, alone):
    n = [int(v) for v in sizes]
    p = [k * (k - 1) // 2 for k in n]
    if not torch.equal(batch['per_molecule'][i:i + 1], alone['per_molecule']):
        return False
    return all(torch.equal(batch['rows'][k][sum((p if k == 'e' else n)[:i]):sum((p if k == 'e' else n)[:i + 1])], alone['rows'][k]) for k in 'xace')


def _check_batch_independence(lib, device):
    mdl = mu.model('dev', lib, device)
    sizes, t, ids = [5, 3, 2, 1, 4], torch.tensor([0.3, 0.7, 0.3, 0.55, 0.0]), [40, 2, 1000003, 9, 5]
    mols = ru.given(mdl.cfg, sizes)
    kw = dict(distort=(0.6, 0.5))
    order = [3, 0, 4, 2, 1]          # shuffled
    batch = mdl.denoising_loss(ru.take(mols, order), t[order], seed=SEED, mol_ids=[ids[i] for i in order], **kw)
    assert bool(torch.isfinite(batch['per_molecule']).all()) and float(batch['per_molecule'][:, 3].sum()) > 0
    for pos, i in enumerate(order):
        assert _same_molecule(batch, [sizes[j] for j in order], pos, _alone(mdl, mols, i, t[i], ids[i], **kw)), i
    # 33 distinct t: two binds (32 + 1); the molecules either side of the cut and the two ends alone
    sizes = [1 + i % 3 for i in range(33)]
    t = torch.tensor([(7 * i % 33 + 1) / 40 for i in range(33)])
    mols = ru.given(mdl.cfg, sizes, seed=4)
    batch = mdl.denoising_loss(mols, t, seed=SEED)
    by_t = sorted(range(33), key=lambda i: float(t[i]))
    for i in (by_t[0], by_t[31], by_t[32], 0):
        assert _same_molecule(batch, sizes, i, _alone(mdl, mols, i, t[i], i)), i


def test_batch_of_mixed_t_equals_molecules_alone_on_emulation(emu_lib):
    _check_batch_independence(emu_lib, 'cpu')


@pytest.mark.gpu
def test_batch_of_mixed_t_equals_molecules_alone_on_gpu():
    _check_batch_independence(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 6. distortion
def _check_distortion(lib, device):
    eng, cfg, _ = mu.engine('qm9', lib, device)
    sizes, ids, p = lu.REDUCE_SIZES, [11, 3, 40, 7, 1000003], 0.35
    on = torch.tensor([True, False, True, True, False])          # the caller's t > distort_t
    eng.bind(torch.tensor(sizes))
    eng.set_molecule_ids(torch.tensor(ids))
    x_in = ru.given(cfg, sizes)[0]['x']
    x, tape = eng.distort(x_in.to(device).contiguous().clone(), p, on, seed=SEED, tape=True)
    eng.synchronize()
    x, z, u = x.cpu(), tape['z'].cpu(), tape['u'].cpu()
    assert torch.equal(u, ru.row_uniforms(sizes, ids, 0, SEED, 0xFFFFFFFF, 2))          # the new stream entry: block 2 word 0 of the atom
    node_on = on.repeat_interleave(torch.tensor(sizes))
    mask = ((u < p) & node_on).float().unsqueeze(-1)
    assert torch.equal(x, x_in + (z * mask) * 0.5)          # flowmol.py:337, three separately rounded operations
    assert torch.equal(x[~node_on], x_in[~node_on]) and 0 < int(mask.sum()) < int(node_on.sum())
    # block 1 is not the position prior's block 0
    x0 = eng.prior_philox(SEED).cpu()
    assert float((z[-47:] - x0[-47:]).abs().max()) > 0.5
    # alone = in batch
    for i in (1, 3):
        eng.bind(torch.tensor([sizes[i]]))
        eng.set_molecule_ids(torch.tensor([ids[i]]))
        _, alone = eng.distort(torch.zeros(sizes[i], 3, device=device), p, True, seed=SEED, tape=True)
        lo = sum(sizes[:i])
        assert torch.equal(alone['z'].cpu(), z[lo:lo + sizes[i]]) and torch.equal(alone['u'].cpu(), u[lo:lo + sizes[i]])
    # moments over 40 x 50 atoms: n = 6000 normals, 2000 uniforms; 5 standard errors each
    eng.bind(torch.tensor([50] * 40))
    eng.set_molecule_ids(None)
    _, tape = eng.distort(torch.zeros(2000, 3, device=device), p, True, seed=SEED, tape=True)
    z, u = tape['z'].cpu().double().reshape(-1), tape['u'].cpu().double()
    n = z.numel()
    assert n == 6000 and abs(float(z.mean())) < 5 / n ** 0.5
    assert abs(float(z.var(unbiased=False)) - 1) < 5 * (2 / n) ** 0.5
    assert abs(float((u < p).double().mean()) - p) < 5 * (p * (1 - p) / u.numel()) ** 0.5


def test_distortion_draws_and_formula_on_emulation(emu_lib):
    _check_distortion(emu_lib, 'cpu')


@pytest.mark.gpu
def test_distortion_draws_and_formula_on_gpu():
    _check_distortion(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 7. batch values
def _check_batch_values(lib, device):
    """Agreement to float32 reduction order: a value is a sum (or a product of two sums) of n non-negative terms, each summation order off by at most
    n 2^-24 sum |terms| = n 2^-24 |value|; the bound is (2 n + 8) 2^-24 |value| with n the number of rows, the 8 for the few operations after the sums."""
    mdl = mu.model('dev', lib, device)
    sizes, t = [5, 3, 2, 1], torch.tensor([0.3, 0.7, 0.02, 0.55])          # 0.02: alpha / (1 - alpha) below the clamp at 0.05
    mols = ru.given(mdl.cfg, sizes)
    for time_scaled in (False, True):
        res = mdl.denoising_loss(mols, t, seed=SEED, time_scaled=time_scaled, total_loss_weights={'x': 3.0, 'e': 0.5})
        rows, tab = res['rows'], res['per_molecule']
        n = torch.tensor(sizes)
        keep = {k: (tab[:, 3 + 2 * f]).sum() for f, k in enumerate('ace')}
        terms = {'x': (rows['x'] / 3).unsqueeze(-1).expand(-1, 3), 'a': rows['a'], 'c': rows['c'], 'e': rows['e'],
                 'keep_a': keep['a'], 'keep_c': keep['c'], 'keep_e': keep['e']}
        want = lu.reference_losses(terms, t, sizes, mdl.cfg, time_scaled)
        for k in 'xace':
            nrows = int((n * (n - 1) // 2).sum()) if k == 'e' else int(n.sum())
            bound = (2 * nrows + 8) * 2.0 ** -24 * abs(float(want[k]))
            assert abs(float(res['losses'][k]) - float(want[k])) <= bound, (time_scaled, k, res['losses'][k], want[k])
            assert float(want[k]) > 0
        total = 3.0 * want['x'] + want['a'] + want['c'] + 0.5 * want['e']
        assert abs(float(res['total']) - float(total)) <= 64 * 2.0 ** -24 * float(total)
    assert 'total' not in mdl.denoising_loss(mols, t, seed=SEED)
    # nothing masked: 0 / 0, NaN as in torch
    late = mdl.denoising_loss(ru.take(mols, [3]), 0.9999999, seed=SEED)
    if float(late['per_molecule'][0, 3]) == 0:
        assert bool(torch.isnan(late['losses']['a']))
    assert bool(torch.isnan(late['losses']['e']))          # a single atom has no pair rows


def test_batch_values_restate_the_reference_on_emulation(emu_lib):
    _check_batch_values(emu_lib, 'cpu')


@pytest.mark.gpu
def test_batch_values_restate_the_reference_on_gpu():
    _check_batch_values(None, 'cuda:0')


# ---------------------------------------------------------------------------------------------------------------- 8. hygiene and refusals
def _check_guarded_call(lib, device):
    case = lu.loss_case('dev', lib, device)
    want = {**case['rows'], 'mol': case['mol']}
    zero, bad, intact, unwritten = lu.guarded_denoising_loss(case, 'zero')
    assert bad == [] and intact and unwritten == []
    ones, bad, intact, unwritten = lu.guarded_denoising_loss(case, 'ones')          # every f32 of the arena a NaN
    assert bad == [] and intact and unwritten == []
    assert mu.first_difference(zero, ones) is None and mu.first_difference(zero, want) is None


def _check_c_refusals(lib, device):
    eng, cfg, _ = mu.engine('qm9', lib, device)
    eng.bind(torch.tensor([3, 2]))
    x1 = ru.as_state(eng, ru.given(cfg, [3, 2]))
    xt = {k: v.clone() for k, v in x1.items()}
    f32 = lambda n: torch.zeros(n, device=device)
    rows = {'x': f32(5), 'a': f32(5), 'c': f32(5), 'e': f32(4)}
    mol, temb, group = f32(16), f32(33 * cfg.time_embedding_dim), torch.zeros(2, dtype=torch.int32, device=device)
    err = lambda e=eng: e.lib.fm_last_error(e._ctx)

    def call(rw=rows, G=1, grp=None, out=mol, s_t=None, e=eng):
        rs = _lib.fm_loss_rows()
        rs.x, rs.a, rs.c, rs.e = (mu._ptr(rw[k]) for k in 'xace')
        s_t = s_t if s_t is not None else e._state_struct(xt)
        return e.lib.fm_denoising_loss(e._ctx, e._stream(), C.byref(s_t), C.byref(e._state_struct(x1)), mu._ptr(temb), G, mu._ptr(grp), C.byref(rs), mu._ptr(out))
    for G in (0, 33):
        assert call(G=G, grp=group) == -1 and b'n_groups' in err()
    assert call(G=2) == -1 and b'mol_group' in err()
    for k in 'xace':
        assert call(rw={**rows, k: None}) == -1 and f'rows->{k} is NULL'.encode() in err(), k
    assert call(rw={**rows, 'x': xt['x_t']}) == -1 and b'rows->x aliases an input' in err()
    assert call(rw={**rows, 'e': temb}) == -1 and b'rows->e aliases an input' in err()
    assert call(out=x1['x_t']) == -1 and b'mol_out aliases an input' in err()
    assert call(rw={**rows, 'c': rows['a']}) == -1 and b'aliases' in err()
    assert call() == 0          # the context stays usable
    eng.synchronize()
    on = torch.ones(1, dtype=torch.int32, device=device)
    dis = lambda p, G, grp, tape=None: eng.lib.fm_distort_philox(eng._ctx, eng._stream(), C.c_uint64(1), C.c_float(p), G, mu._ptr(grp), mu._ptr(on), mu._ptr(xt['x_t']), tape)
    assert dis(0.2, 0, None) == -1 and b'n_groups' in err()
    assert dis(0.2, 2, None) == -1 and b'mol_group' in err()
    assert dis(1.5, 1, None) == -1 and b'probability' in err()
    tp = _lib.fm_distort_tape()
    tp.z = mu._ptr(xt['x_t'])
    assert dis(0.2, 1, None, C.byref(tp)) == -1 and b'aliases x' in err()
    end = mu.model('endpoint_small', lib, device).engine
    end.bind(torch.tensor([3, 2]))
    assert call(s_t=fm_state(), e=end) == -1 and b'endpoint' in err(end)


def _check_python_refusals(lib, device):
    mdl = mu.model('dev', lib, device)
    cfg = mdl.cfg
    mols = ru.given(cfg, [3, 2])
    rng_state = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match='endpoint'):
        mu.model('endpoint_small', lib, device).denoising_loss(mols, 0.5, seed=SEED)
    for hp, what in (({'weight_ae': True}, 'weight_ae'), ({'target_blur': 0.1}, 'target_blur')):
        mdl.loss_hparams = hp
        try:
            with pytest.raises(NotImplementedError, match=what):
                mdl.denoising_loss(mols, 0.5, seed=SEED)
        finally:
            mdl.loss_hparams = {}
    with pytest.raises(ValueError, match='seed'):
        mdl.denoising_loss(mols, 0.5)
    for bad_t in (1.0, -0.1, [0.5, 1.5], float('nan')):
        with pytest.raises(ValueError, match=r'\[0, 1\)'):
            mdl.denoising_loss(mols, bad_t, seed=SEED)
    with pytest.raises(ValueError, match='one value per molecule'):
        mdl.denoising_loss(mols, [0.5, 0.5, 0.5], seed=SEED)
    for f, K in (('a', cfg.n_atom_types), ('c', cfg.n_charges), ('e', cfg.n_bond_types)):
        t = {k: v.clone() for k, v in mols[0].items()}
        t[f][0] = K          # the mask token
        with pytest.raises(ValueError, match='real categories'):
            mdl.denoising_loss((t, mols[1]), 0.5, seed=SEED)
    with pytest.raises(ValueError, match='seed'):
        mdl.engine.distort(torch.zeros(1, 3), 0.2, True)
    assert torch.equal(torch.get_rng_state(), rng_state)
    # the checkpoint's hparams are the defaults
    mdl.loss_hparams = {'distort_p': 0.9, 'distort_t': 0.1, 'time_scaled_loss': True}
    try:
        a, b = mdl.denoising_loss(mols, 0.5, seed=SEED), mdl.denoising_loss(mols, 0.5, seed=SEED, distort=(0.9, 0.1), time_scaled=True)
        off = mdl.denoising_loss(mols, 0.5, seed=SEED, distort=False, time_scaled=False)
    finally:
        mdl.loss_hparams = {}
    assert torch.equal(a['per_molecule'], b['per_molecule']) and float(a['losses']['x']) == float(b['losses']['x'])
    assert not torch.equal(a['per_molecule'], off['per_molecule'])
    assert torch.equal(off['per_molecule'], mdl.denoising_loss(mols, 0.5, seed=SEED)['per_molecule'])          # presets: off


def test_denoising_loss_call_between_guard_bands_on_emulation(emu_lib):
    _check_guarded_call(emu_lib, 'cpu')


@pytest.mark.gpu
def test_denoising_loss_call_between_guard_bands_on_gpu():
    _check_guarded_call(None, 'cuda:0')


def test_denoising_loss_refusals_on_emulation(emu_lib):
    _check_c_refusals(emu_lib, 'cpu')
    _check_python_refusals(emu_lib, 'cpu')


@pytest.mark.gpu
def test_denoising_loss_refusals_on_gpu():
    _check_c_refusals(None, 'cuda:0')
    _check_python_refusals(None, 'cuda:0')
