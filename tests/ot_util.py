"""Helpers of tests/test_ot_align.py: the inputs, the restated cost matrix, the host references of the assignment and of the rigid fit."""
from __future__ import annotations

import math

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

NAMES = ('one', 'two', 'three', 'five', 'cloud47', 'n65', 'n130', 'mirror', 'ties', 'far')
UNIQUE = tuple(n for n in NAMES if n not in ('ties', 'three', 'two'))          # perm must equal scipy's: the optimum of the float32 matrix is unique
COORDS = ('five', 'cloud47', 'n65', 'n130', 'mirror', 'far')                   # the optimal transform is unique: coordinates are compared too
BATCH5 = ('cloud47', 'one', 'five', 'n65', 'mirror')

_CACHE = {}


def inputs():
    """{name: (x0, x1c)} in float32 from one fixed generator.  x1c is centred in float32 and so is x0 (the prior is COM-free by construction), except in
    'far', where both are shifted by 500, and in 'one'."""
    if 'inputs' in _CACHE:
        return _CACHE['inputs']
    gen = torch.Generator().manual_seed(1609)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    centre = lambda x: (x.float() - x.float().mean(0, keepdim=True))
    out = {'one': (rnd(1, 3).float(), (rnd(1, 3) * 1.5).float())}          # not centred: a centred single atom is the origin, which would show nothing
    for name, n in (('two', 2), ('three', 3), ('five', 5), ('cloud47', 47), ('n65', 65), ('n130', 130)):
        out[name] = (centre(rnd(n, 3)), centre(rnd(n, 3) * 1.5))
    # a chiral 12-ring: radii and heights differ atom by atom; the mirror image through its mean plane, rows shuffled.  Neighbours are 1.2 apart, an atom
    # and its own image at most 0.7: the assignment is the shuffle
    ang = torch.arange(12, dtype=torch.float64) * (math.pi / 6)
    rad = 2.3 + 0.3 * torch.rand(12, generator=gen, dtype=torch.float64)
    z = torch.tensor([0.3, -0.2, 0.25, 0.1, -0.35, 0.15, -0.1, 0.3, -0.25, 0.2, -0.15, 0.35], dtype=torch.float64)
    ring = centre(torch.stack([rad * ang.cos(), rad * ang.sin(), z], dim=1))
    shuffle = torch.randperm(12, generator=gen)
    out['mirror'] = ((ring * torch.tensor([1.0, 1.0, -1.0]))[shuffle].contiguous(), ring)
    lattice = torch.tensor([[i, j, k] for i in (0.0, 1.5) for j in (0.0, 1.5) for k in (0.0, 1.5)], dtype=torch.float64)
    x0 = rnd(8, 3)
    x0[5] = x0[2]
    out['ties'] = (x0.float(), centre(lattice))
    out['far'] = (centre(rnd(47, 3)) + 500.0, centre(rnd(47, 3) * 1.5) + 500.0)
    _CACHE['inputs'] = out
    return out


def cost_f32(x0, x1c):
    """The kernel's cost matrix restated in torch float32, operation by operation: c(i, j) = sqrt(((dx dx) + (dy dy)) + (dz dz)), d = x1c[i] - x0[j].
    The square root is taken in float64 and rounded to float32, which IS the correctly rounded float32 root (53 >= 2 * 24 + 2 bits: the second rounding
    cannot move it) on every host; torch.sqrt on a float32 tensor is an ulp off on some vectorised CPU builds (0.7 % of these entries where this was written)."""
    d = x1c.float()[:, None, :] - x0.float()[None, :, :]
    sq = d * d
    return torch.sqrt(((sq[..., 0] + sq[..., 1]) + sq[..., 2]).double()).float()


def assignment_of(cost):
    """scipy's optimum of a cost matrix (rows = atoms) in float64 -> (column indices, optimal cost)."""
    c = cost.double().numpy()
    rows, cols = linear_sum_assignment(c)
    return torch.from_numpy(cols.astype(np.int64)), float(c[rows, cols].sum())


def assignment(x0, x1c):
    """scipy's optimum of the restated float32 matrix: the reference of the kernel's assignment."""
    return assignment_of(cost_f32(x0, x1c))


def is_unique(x0, x1c):
    """Is the optimum of the restated matrix unique?  Forbidding any one of its pairs must cost strictly more."""
    c = cost_f32(x0, x1c).double().numpy()
    rows, cols = linear_sum_assignment(c)
    best = c[rows, cols].sum()
    for i, j in zip(rows, cols):
        if c.shape[0] == 1:
            break
        c2 = c.copy()
        c2[i, j] = 1e9
        r2, k2 = linear_sum_assignment(c2)
        if not c2[r2, k2].sum() > best:
            return False
    return True


def rigid_reference(x0p, x1c, dtype, reflect):
    """Kabsch of x0p onto x1c in ``dtype`` as the reference writes it (priors.py:128-169: R = V U^T, no determinant correction) -- reflect=False: R = V diag(1, 1,
    det) U^T -- with the translation of the kernel's statement, R (x0p - mean0) + mean1 -> (rmsd of x0p - x1c, rmsd after the fit, the moved rows).  The
    reference's own translation adds mean0 - R mean0, which vanishes for a COM-free prior (test_reference_translation_on_centred_priors)."""
    a0, b0 = x0p.to(dtype), x1c.to(dtype)
    m0, m1 = a0.mean(0, keepdim=True), b0.mean(0, keepdim=True)
    a, b = a0 - m0, b0 - m1
    U, _, Vh = torch.linalg.svd(a.T @ b)
    D = torch.eye(3, dtype=dtype)
    if not reflect:
        D[2, 2] = torch.sign(torch.linalg.det(Vh.T @ U.T))
    R = Vh.T @ D @ U.T
    moved = a @ R.T + m1
    rms = lambda d: (d ** 2).sum(1).mean().sqrt()
    return float(rms(a0 - b0)), float(rms(moved - b0)), moved


def f32_errors():
    """The measurement behind test_ot_align.F32_ERR: |float32 restatement - float64| of (rmsd after the permutation, rmsd after the fit, coordinates), the
    larger of the two reflection settings."""
    out = {}
    for name, (x0, x1c) in inputs().items():
        cols, _ = assignment(x0, x1c)
        e = [0.0, 0.0, 0.0]
        for reflect in (True, False):
            p64, r64, x64 = rigid_reference(x0[cols], x1c, torch.float64, reflect)
            p32, r32, x32 = rigid_reference(x0[cols], x1c, torch.float32, reflect)
            e = [max(e[0], abs(p32 - p64)), max(e[1], abs(r32 - r64)), max(e[2], float((x32.double() - x64).abs().max()))]
        out[name] = tuple(e)
    return out


def cdist_eps():
    """max |torch.cdist float32 - float64 distance| / c_max over the inputs: the relative error of the reference's own cost recipe."""
    worst = 0.0
    for name, (x0, x1c) in inputs().items():
        c32 = torch.cdist(x1c, x0, p=2).double()
        c64 = torch.cdist(x1c.double(), x0.double(), p=2, compute_mode='donot_use_mm_for_euclid_dist')
        worst = max(worst, float((c32 - c64).abs().max() / c64.max()))
    return worst
