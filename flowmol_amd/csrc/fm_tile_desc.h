// Edge-message tile descriptor and the closed-form row -> endpoints map of the internal edge order.  Plain C++ with no HIP builtin in it: the kernels
// include it through fm_kernels.h, and a host compiler builds it as it is (tests/test_tile_rows.py checks it against fm_k_batch_setup's own formulas).
//
// A molecule of n atoms with first node `node_off` and first directed-edge row `moff` holds edge (dst = i, src = j), j != i, at row
// moff + i (n - 1) + (j - (j > i)) (fm_kernels.h "Internal edge order"), and its unordered pairs start at pair moff / 2 (every molecule has twice as many
// directed edges as pairs).  A tile is `left` consecutive rows from row e0 of ONE molecule, so its 16-byte descriptor names the molecule and the
// destination i0 of its first row, and a row's endpoints follow from the row number with one small quotient: no index array is read.
//
// Field widths follow from the limits of a bound batch (fm_engine.cpp plan_batch: fewer than 2^29 directed edges, at most 2,097,151 nodes; n (n - 1) < 2^29
// gives n <= 23,170):   x = e0 (29 bits)   y = moff (29)   z = node_off (21) | left << 21 (7: 1 .. 64)   w = n (15) | i0 << 15 (15)
#pragma once

#if defined(__HIPCC__)
#define FM_HD __host__ __device__ __forceinline__
#else
#define FM_HD inline
#endif

#ifndef FM_CHUNK_E
#define FM_CHUNK_E 16      // rows per aggregation chunk, counted from the molecule's first row (fm_kernels.h "CANONICAL AGGREGATION ORDER")
#endif

struct FmTile {
    int e0;         // first edge row of the tile
    int left;       // rows that exist (1 .. tile height)
    int moff;       // the molecule's first edge row (e0 - moff is a multiple of the tile height)
    int n;          // the molecule's atoms (>= 2: a molecule without edges owns no tile)
    int node_off;   // the molecule's first node
    int i0;         // destination (molecule-local) of row e0: (e0 - moff) / (n - 1)
};

struct FmTileRow {
    int src, dst;   // global node ids
    int piece;      // chunk of the row minus the first chunk of its destination, both counted from the molecule's first row
    int pair;       // global id (reference order) of the unordered pair {src, dst}
};

FM_HD void fm_tile_encode(const FmTile& t, int& x, int& y, int& z, int& w) {
    x = t.e0; y = t.moff; z = t.node_off | (t.left << 21); w = t.n | (t.i0 << 15);
}

FM_HD FmTile fm_tile_decode(int x, int y, int z, int w) {
    FmTile t;
    t.e0 = x; t.moff = y; t.node_off = z & 0x1fffff; t.left = (int)((unsigned)z >> 21); t.n = w & 0x7fff; t.i0 = (int)((unsigned)w >> 15);
    return t;
}

// Row `row` (0 .. 63) of the tile.  `inv` is 1 / (n - 1) as a float, correct to a few ulp (the kernels pass v_rcp_f32's): the only quotient is
// q / (n - 1) with q < n - 1 + 64 < 2^15, exact in a float, so the truncated product misses the quotient by at most one and the two compare steps settle it.
// Rows at or past `left` give endpoints outside the molecule; callers mask them.
FM_HD FmTileRow fm_tile_row(const FmTile& t, float inv, int row) {
    const int m = t.n - 1;
    const int local = t.e0 - t.moff + row;      // row counted from the molecule's first
    const int q = local - t.i0 * m;             // ... from the first row of destination i0
    int di = (int)((float)q * inv);
    int k = q - di * m;
    if (k < 0) { --di; k += m; }
    if (k >= m) { ++di; k -= m; }
    const int i = t.i0 + di, j = k + (k >= i ? 1 : 0);
    const int a = i < j ? i : j, c = i < j ? j : i;
    FmTileRow r;
    r.dst = t.node_off + i;
    r.src = t.node_off + j;
    static_assert(FM_CHUNK_E == 16, "chunk quotients are shifts");
    r.piece = (local >> 4) - ((local - k) >> 4);                         // every operand is >= 0: the shifts are the setup kernel's divisions
    r.pair = (t.moff >> 1) + ((a * (2 * t.n - a - 1)) >> 1) + (c - a - 1);
    return r;
}
