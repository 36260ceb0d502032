"""Host logic of the pair-slab choice (fm_engine.cpp, plan of a batch): the pair-slab instance of the edge-message kernel addresses a tile's Q rows with
31-bit byte offsets inside one molecule's pairs, which holds up to 2048 atoms.  A batch with a larger molecule must run the full instance on every
convolution -- forced, canonical or automatic alike.  The plan is read through fm_workspace_bytes: the Q tables (pairs x 1 KB per slab convolution)
are part of the workspace exactly when the batch uses them.  No kernel runs here."""
import pytest
import torch

import hygiene_util as hu


def _q_bytes(lib, sizes, tuning):
    """Bytes the pair-slab tables take in the workspace of `sizes` under `tuning`: the total minus the total with the slab switched off."""
    with_, _, _ = hu.engine('flowmol3', lib, 'cpu', tuning={'tile_edge': 32, **tuning})
    without, _, _ = hu.engine('flowmol3', lib, 'cpu', tuning={'tile_edge': 32, 'pair_slab': -1})
    n = torch.tensor(sizes)
    return with_.workspace_need(n) - without.workspace_need(n)


@pytest.mark.parametrize('tuning', [{}, {'pair_slab': 1}], ids=['canonical', 'forced'])
def test_pair_slab_is_refused_to_batches_with_a_molecule_beyond_2048_atoms(emu_lib, tuning):
    r = lambda b: (b + 255) // 256 * 256
    pairs = lambda sizes: sum(n * (n - 1) // 2 for n in sizes)
    for sizes in ([47, 9], [2048], [5, 2048]):          # 2048 atoms: the largest offset is (2048 * 2047 / 2 - 1) * 1024 < 2^31
        assert (2048 * 2047 // 2 - 1) * 1024 < 2 ** 31
        assert _q_bytes(emu_lib, sizes, tuning) == 2 * r(pairs(sizes) * 1024), sizes          # flowmol3: two convolutions in front of the first update
    for sizes in ([2049], [47, 2049, 9]):               # 2049 atoms: (2049 * 2048 / 2 - 1) * 1024 >= 2^31
        assert (2049 * 2048 // 2 - 1) * 1024 >= 2 ** 31
        assert _q_bytes(emu_lib, sizes, tuning) == 0, sizes
