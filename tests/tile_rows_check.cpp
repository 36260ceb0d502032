// TEST TOOLING: host check of flowmol_amd/csrc/fm_tile_desc.h (built and run by tests/test_tile_rows.py).
// Every tile descriptor a batch-setup kernel would write for a molecule is encoded, decoded and asked for the endpoints of each of its rows; the answers
// are compared with the definition of the internal edge order, written with / and % exactly as fm_k_batch_setup writes e_src, e_dst, e_pair and
// node_first_edge (64-bit here, so that the definition itself cannot wrap).
//   tile_rows_check          all molecules, the reciprocal exact and 2 ulp to either side (the kernels pass the hardware's approximate reciprocal)
//   tile_rows_check quick    exact reciprocal only (the run under the sanitizers)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../flowmol_amd/csrc/fm_tile_desc.h"

static long long g_rows = 0, g_bad = 0;

static void fail(const char* what, int n, int tm, long long tile, int row, long long got, long long want) {
    if (g_bad++ < 20) std::fprintf(stderr, "MISMATCH %s: n=%d tile_rows=%d tile=%lld row=%d got=%lld want=%lld\n", what, n, tm, tile, row, got, want);
}

// one tile of the molecule (n atoms, first node node_off, first edge row moff) under tile height tm
static void check_tile(int n, int tm, int node_off, int moff, long long tile, int n_inv) {
    const long long m = n - 1, rows = (long long)n * m;
    const long long e0 = moff + tile * tm;
    const long long left = rows - tile * tm < tm ? rows - tile * tm : tm;
    FmTile t{(int)e0, (int)left, moff, n, node_off, (int)((e0 - moff) / m)};      // what fm_k_batch_setup encodes
    int x, y, z, w;
    fm_tile_encode(t, x, y, z, w);
    const FmTile d = fm_tile_decode(x, y, z, w);
    if (d.e0 != t.e0) fail("e0", n, tm, tile, -1, d.e0, t.e0);
    if (d.left != t.left) fail("left", n, tm, tile, -1, d.left, t.left);
    if (d.moff != t.moff) fail("moff", n, tm, tile, -1, d.moff, t.moff);
    if (d.n != t.n) fail("n", n, tm, tile, -1, d.n, t.n);
    if (d.node_off != t.node_off) fail("node_off", n, tm, tile, -1, d.node_off, t.node_off);
    if (d.i0 != t.i0) fail("i0", n, tm, tile, -1, d.i0, t.i0);
    float inv[3];
    inv[0] = 1.0f / (float)(n - 1);
    inv[1] = std::nextafterf(std::nextafterf(inv[0], 0.f), 0.f);
    inv[2] = std::nextafterf(std::nextafterf(inv[0], 2.f), 2.f);
    for (int v = 0; v < n_inv; ++v)
        for (int row = 0; row < (int)left; ++row) {
            const FmTileRow r = fm_tile_row(d, inv[v], row);
            const long long e = e0 + row, local = e - moff;
            const long long i = local / m, k = local % m, j = k + (k >= i ? 1 : 0);
            const long long a = i < j ? i : j, c = i < j ? j : i;
            const long long pair = moff / 2 + a * (2 * n - a - 1) / 2 + (c - a - 1);
            const long long first = moff + i * m;                                      // node_first_edge[dst]
            const long long piece = (e - moff) / FM_CHUNK_E - (first - moff) / FM_CHUNK_E;
            if (r.dst != node_off + i) fail("dst", n, tm, tile, row, r.dst, node_off + i);
            if (r.src != node_off + j) fail("src", n, tm, tile, row, r.src, node_off + j);
            if (r.piece != piece) fail("piece", n, tm, tile, row, r.piece, piece);
            if (r.pair != pair) fail("pair", n, tm, tile, row, r.pair, pair);
            ++g_rows;
        }
}

int main(int argc, char** argv) {
    const int n_inv = (argc > 1 && !std::strcmp(argv[1], "quick")) ? 1 : 3;
    const int heights[3] = {16, 32, 64};
    const int node_limit = 2097151, edge_limit = 0x7fffffff / 4;      // fm_engine.cpp plan_batch: nodes and directed edges of a bound batch
    for (int n = 2; n <= 300; ++n)
        for (int tm : heights) {
            const long long rows = (long long)n * (n - 1), tiles = (rows + tm - 1) / tm;
            // offsets: small and odd-sized in front, or the molecule at the very end of the largest batch (moff stays even: pairs start at moff / 2)
            const bool far = n % 2 == 0;
            const int node_off = far ? node_limit - 1 - n : 3 * n + 1;
            const int moff = far ? (int)((edge_limit - 1 - rows) & ~1LL) : 2 * (7 * n + 5);
            for (long long tile = 0; tile < tiles; ++tile) check_tile(n, tm, node_off, moff, tile, n_inv);
        }
    const int big[3] = {4097, 23169, 23170};
    for (int n : big)
        for (int tm : heights) {
            const long long rows = (long long)n * (n - 1), tiles = (rows + tm - 1) / tm;
            const int node_off = node_limit - 1 - n;
            const int moff = (int)((edge_limit - 1 - rows) & ~1LL);
            const long long pick[9] = {0, 1, 2, tiles / 2 - 1, tiles / 2, tiles / 2 + 1, tiles - 3, tiles - 2, tiles - 1};
            for (long long tile : pick) check_tile(n, tm, node_off, moff, tile, n_inv);
            check_tile(n, tm, 0, 0, tiles - 1, n_inv);
        }
    std::printf("rows checked: %lld, mismatches: %lld\n", g_rows, g_bad);
    return g_bad ? 1 : 0;
}
