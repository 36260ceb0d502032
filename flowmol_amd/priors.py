"""Host side of the priors: the reference's categorical prior functions on torch's CPU generator (reference flowmol/models/priors.py:8-107 as
``FlowMol.sample_prior`` calls them, flowmol.py:417-448), the shipped marginal distributions they default to, and the adaptation of a caller's
reference-format prior dict to the bound batch (flowmol.py:534-545).  The in-kernel Philox priors are ``Engine.prior_philox`` / ``prior_philox_dense``."""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Optional

import torch

from .config import VFConfig
from .shard import upper_half_rows

PKG = Path(__file__).resolve().parent


def load_marginal_dists(name: str):
    """(p_a, p_c, p_e, p_c_given_a) of a dataset: the reference's data/<set>/train_data_marginal_dists.pt as shipped JSON."""
    data = json.loads((PKG / 'data' / 'marginal_dists.json').read_text())
    if name not in data:
        raise KeyError(f'no marginal distributions named {name!r}; have {sorted(data)}')
    d = data[name]
    return tuple(torch.tensor(d[k], dtype=torch.float32) for k in ('p_a', 'p_c', 'p_e', 'p_c_given_a'))


def simplex_projection(x: torch.Tensor) -> torch.Tensor:
    """Euclidean projection of every row onto the probability simplex (Wang & Carreira-Perpinan, arXiv:1309.1541), the operation the
    reference's blurred barycenter prior applies (priors.py:36-44 -> flowmol/utils/dirflow.py:35-49): with the row sorted descending,
    u, and c_j = (sum_{i<=j} u_i - 1) / j, the threshold is c_rho for rho = #{j : u_j > c_j}; the result is max(x - c_rho, 0)."""
    y = x.reshape(-1, x.shape[-1])
    u, _ = torch.sort(y, dim=-1, descending=True)
    c = (torch.cumsum(u, dim=-1) - 1) / torch.arange(1, y.shape[1] + 1, dtype=y.dtype, device=y.device).unsqueeze(0)
    rho = (u > c).sum(dim=1, keepdim=True)
    tau = torch.gather(c, 1, rho - 1)
    return torch.max(y - tau, torch.zeros_like(y)).view(x.shape)


def categorical_prior(kind: str, n: int, d: int, kw: dict, a_0: Optional[torch.Tensor] = None, default_p=None) -> torch.Tensor:
    """The reference's categorical prior functions on the CPU generator, as FlowMol.sample_prior calls them (priors.py:8-107;
    flowmol.py:426-441) -- same draws in the same order.  'marginal' / 'c-given-a' take their distribution from the prior kwargs
    (`p` / `p_c_given_a`, as the reference would) or, when absent, from the shipped marginals of the model's dataset (`default_p`)."""
    F = torch.nn.functional
    if kind == 'gaussian':
        p = torch.randn(n, d) * kw.get('std', 1.0)
        return p + 1 / d if kw.get('simplex_center', False) else p
    if kind == 'uniform-simplex':
        sample = torch.distributions.Exponential(torch.tensor(1.0)).sample((n, d))
        return sample / sample.sum(dim=1, keepdim=True)
    if kind == 'barycenter':
        p = torch.ones(n, d) / d
        blur = kw.get('blur', 0.0)
        if blur != 0.0:
            p = simplex_projection(p + torch.randn_like(p) * blur)
        return p
    if kind == 'biased-simplex':          # priors.py:47-56
        vp, std, vi = kw.get('vertex_prob', 0.75), kw.get('std', 0.2), kw.get('vertex_idx', 0)
        mu = torch.ones(d) * ((1 - vp) / (d - 1))
        mu[vi] = vp
        return F.softmax((mu.unsqueeze(0) + torch.randn(n, d) * std) / (1 / d), dim=1)
    if kind in ('marginal', 'c-given-a'):
        key = 'p' if kind == 'marginal' else 'p_c_given_a'
        p = kw.get(key, default_p)
        if p is None:
            raise ValueError(f"prior {kind!r} needs kwargs[{key!r}] (or a dataset whose shipped marginals have {d} categories)")
        p = torch.as_tensor(p, dtype=torch.float32)
        if p.shape[-1] != d:
            raise ValueError(f"prior {kind!r}: distribution has {p.shape[-1]} categories, the model {d}")
        if kind == 'marginal':            # priors.py:67-79
            idx = torch.multinomial(p, n, replacement=True)
        else:                             # priors.py:81-98: charges conditioned on the sampled atom-type prior
            if a_0 is None:
                raise ValueError("the 'c-given-a' prior needs the atom-type prior")
            idx = torch.multinomial(p[a_0.argmax(dim=1)], 1, replacement=True).squeeze(-1)
        one = F.one_hot(idx, num_classes=d).float()
        blur = kw.get('blur')
        if blur is not None:
            one = F.softmax((one + torch.randn_like(one) * blur) / (1 / d), dim=1)
        return one
    raise NotImplementedError(f'prior type {kind!r}')


def default_marginals(cfg: VFConfig, prior_types: Optional[Dict[str, str]] = None) -> Dict[str, Optional[torch.Tensor]]:
    """Per modality 'a', 'c', 'e': the shipped marginal of the model's dataset the 'marginal' / 'c-given-a' priors fall back to (for 'c' the
    conditional table when its prior is 'c-given-a'), or None where the dataset ships none or its category count does not fit the model."""
    try:
        p_a, p_c, p_e, p_ca = load_marginal_dists(cfg.n_atoms_hist)
    except KeyError:
        return {'a': None, 'c': None, 'e': None}
    types = prior_types if prior_types is not None else cfg.prior_types
    cand = {'a': (p_a, cfg.n_atom_types), 'c': (p_ca if types.get('c') == 'c-given-a' else p_c, cfg.n_charges), 'e': (p_e, cfg.n_bond_types)}
    return {k: (p if p.shape[-1] == d else None) for k, (p, d) in cand.items()}


def draw_categorical_priors(cfg: VFConfig, N: int, U: int, prior_types: Optional[Dict[str, str]] = None, prior_kwargs: Optional[Dict[str, dict]] = None,
                            default_p: Optional[Dict[str, torch.Tensor]] = None):
    """(a_0 (N,na), c_0 (N,nc), e_0 (U,ne)) of an endpoint-parameterised model on the CPU generator in the reference's order a, c, e, with `c` seeing
    a_0 (flowmol.py:426-441).  ``prior_types`` / ``prior_kwargs`` default to the model's config, ``default_p`` to no fall-back distribution."""
    types = prior_types if prior_types is not None else cfg.prior_types
    kws = prior_kwargs if prior_kwargs is not None else cfg.prior_kwargs
    dp = default_p or {}
    a0 = categorical_prior(types['a'], N, cfg.n_atom_types, kws.get('a', {}), default_p=dp.get('a'))
    c0 = categorical_prior(types['c'], N, cfg.n_charges, kws.get('c', {}), a_0=a0, default_p=dp.get('c'))
    e0 = categorical_prior(types['e'], U, cfg.n_bond_types, kws.get('e', {}), default_p=dp.get('e'))
    return a0, c0, e0


def adapt_prior(prior: dict, n_atoms: torch.Tensor, cfg: VFConfig, E: int, only_missing_column: bool):
    """A caller's reference-format prior dict -- x_0 (N,3), a_0 / c_0 (N,*), e_0 per directed edge (E,*) with every molecule's upper block first, or per
    unordered pair (U,*) -- as (x_0, a_0, c_0, e_0 per unordered pair) for the bound batch of sizes ``n_atoms``.  The fake-atom column is adapted to
    the model as the reference does (flowmol.py:540-545): dropped when the prior has it and the model does not; prepended as zeros when the model
    has it and the prior does not flag it -- always (the CTMC path), or with ``only_missing_column`` only when a_0 is exactly one column short (the
    endpoint path, whose shape check follows)."""
    a0 = prior['a_0']
    flagged = prior.get('fake_atoms', False)
    if flagged and not cfg.fake_atoms:
        a0 = a0[:, 1:]
    elif not flagged and cfg.fake_atoms and (not only_missing_column or a0.shape[-1] == cfg.n_atom_types - 1):
        a0 = torch.cat([torch.zeros(a0.shape[0], 1, device=a0.device, dtype=a0.dtype), a0], dim=-1)
    e0 = prior['e_0']
    if e0.shape[0] == E:
        e0 = e0[upper_half_rows(n_atoms)]
    return prior['x_0'], a0, prior['c_0'], e0
