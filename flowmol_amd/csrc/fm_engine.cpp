// Host side of libflowmol_hip.so: the C ABI of include/flowmol_hip.h.
//  - fm_create    : validates the config, decides the model's ModelPlan, looks the reference's state-dict tensors up by name, repacks them
//                   module by module into MFMA B-fragment order (fm_device.h) with the algebraic hoists of SURVEY.md §7, uploads once
//  - fm_batch_bind: carves the caller's workspace, builds the destination-sorted edge layout on device
//  - fm_forward / fm_ctmc_step / fm_integrate: enqueue the kernel sequence on the caller's stream
// Compiled as HIP for gfx950 (flowmol_amd/build.py).  No host synchronisation on the hot path.
#include "fm_host.h"

namespace fmh { thread_local std::string g_create_error; }

namespace {

// ---------------------------------------------------------------------------------------- weight blob access
struct Blob {
    const float* base; const fm_tensor_desc* t; int n;
    std::string err;
    const float* get(const std::string& name, int64_t d0, int64_t d1 = -1) {
        for (int i = 0; i < n; ++i)
            if (name == t[i].name) {
                const bool ok = (d1 < 0) ? (t[i].ndim == 1 && t[i].shape[0] == d0)
                                         : (t[i].ndim == 2 && t[i].shape[0] == d0 && t[i].shape[1] == d1);
                if (!ok) {
                    char b[256];
                    snprintf(b, sizeof b, "tensor %s: shape (%lld,%lld) != expected (%lld,%lld)", name.c_str(),
                             (long long)t[i].shape[0], (long long)(t[i].ndim > 1 ? t[i].shape[1] : -1), (long long)d0, (long long)d1);
                    if (err.empty()) err = b;
                    return nullptr;
                }
                return base + t[i].offset;
            }
        if (err.empty()) err = "missing tensor " + name;
        return nullptr;
    }
    bool ok() const { return err.empty(); }      // every get() so far found its tensor
};

// host-side staging arena; device pointers are offsets into the final device arena
struct Arena {
    std::vector<float> h;
    size_t add(const std::vector<float>& v) {
        size_t off = align_up(h.size(), 64);
        h.resize(off, 0.f);
        h.insert(h.end(), v.begin(), v.end());
        return off;
    }
};

// A logical weight matrix W[k][n] as the kernels' GEMMs see it.  Each is written once (linear() or a lambda) and packed into whichever layouts the
// ModelPlan asks for: fragment order (pack), quad-row (pack4), split planes (pack_sp).
using WFn = std::function<float(int, int)>;
using KMap = std::function<int(int)>;

// a row-major (out, in) Linear weight read through a k-map: W[k][n] = weight[n][kmap(k)], 0 for n >= out or an unmapped k
WFn linear(const float* W, int out, int in, KMap kmap = [](int k) { return k; }) {
    return [=](int k, int n) -> float {
        if (n >= out) return 0.f;
        const int kk = kmap(k);
        return (kk >= 0 && kk < in) ? W[(size_t)n * in + kk] : 0.f;
    };
}
KMap below(int n) { return [n](int k) { return k < n ? k : -1; }; }      // the first n input columns of a zero-padded tile

// pack W_logical[k][n] (K x N, K%8==0, N%16==0) into fragment order
std::vector<float> pack(int K, int N, const WFn& w) {
    const int K8 = K / 8, NT = N / 16;
    std::vector<float> out((size_t)K8 * NT * 64 * 2);
    for (int ks = 0; ks < K8; ++ks)
        for (int nt = 0; nt < NT; ++nt)
            for (int lane = 0; lane < 64; ++lane) {
                const int j = lane & 15, h = lane >> 4;
                const size_t o = (((size_t)ks * NT + nt) * 64 + lane) * 2;
                out[o] = w(8 * ks + 2 * h, 16 * nt + j);
                out[o + 1] = w(8 * ks + 2 * h + 1, 16 * nt + j);
            }
    return out;
}

// quad-row packing for fm_wave_gemm4 (4-row tiles on v_mfma_f32_4x4x1_16B_f32): W_logical[k][n] (K x 256, K%4==0); entry (kq, g, lane) = the four
// weights W[4kq .. 4kq+3][64g + lane] -- one 1-KB buffer_load_dwordx4 per quad step and wave
std::vector<float> pack4(int K, const WFn& w, int G = 4) {      // G column groups of 64: N = 64 G
    const int KQ = K / 4;
    std::vector<float> out((size_t)KQ * G * 64 * 4);
    for (int kq = 0; kq < KQ; ++kq)
        for (int g = 0; g < G; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 4; ++i) out[(((size_t)kq * G + g) * 64 + lane) * 4 + i] = w(4 * kq + i, 64 * g + lane);
    return out;
}

// split-precision packing (fm_device.h "bf16x3"): W_logical[k][n] (K x N, K padded with zeros to a multiple of 32, N%16==0) as hi/lo bf16 planes in
// v_mfma_f32_16x16x32_bf16 B-fragment order: entry (kb, nt, plane, lane) = 8 bf16 = W[32kb + 8(lane>>4) + q][16nt + (lane&15)], q = 0..7
inline uint16_t bf16_rne(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);       // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_f32(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }
// 16-bit plane formats of the split modes (fm_device.h): 0 = bf16, 1 = IEEE half (round to nearest even, subnormals kept, clamped to +-65504)
inline uint16_t f16_rne(float f) { f = std::fmin(std::fmax(f, -65504.f), 65504.f); const _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }
inline float f16_f32(uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (float)h; }
std::vector<float> pack_sp(int K, int N, const WFn& w, int npl, int fmt) {      // npl planes: hi, lo (| hi, mid, lo of the three-term mode)
    const int KB = (K + 31) / 32, NT = N / 16;
    std::vector<uint16_t> out((size_t)KB * NT * npl * 64 * 8);
    for (int kb = 0; kb < KB; ++kb)
        for (int nt = 0; nt < NT; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int q = 0; q < 8; ++q) {
                    const int k = 32 * kb + 8 * (lane >> 4) + q;
                    float r = k < K ? w(k, 16 * nt + (lane & 15)) * (fmt == 1 ? FM_F16_WSCALE : 1.0f) : 0.f;      // half planes: weights times 2^6 (fm_device.h)
                    const size_t e = (((size_t)kb * NT + nt) * npl) * 64 * 8;
                    for (int p_ = 0; p_ < npl; ++p_) {
                        const uint16_t h = fmt == 1 ? f16_rne(r) : bf16_rne(r);
                        out[e + (size_t)p_ * 64 * 8 + (size_t)lane * 8 + q] = h;
                        r -= fmt == 1 ? f16_f32(h) : bf16_f32(h);          // exact in f32
                    }
                }
    std::vector<float> f(out.size() / 2);
    memcpy(f.data(), out.data(), out.size() * 2);
    return f;
}

struct Fix { const void** slot; size_t off; };

// One fm_create's packing: the weight blob, the host arena and the slots its entries are bound to after the upload, and the model's ModelPlan
struct Builder {
    Blob bl; const ModelPlan& m;
    Arena A; std::vector<Fix> fix;
    template <class T> void put(const T*& slot, const std::vector<float>& v) { fix.push_back({(const void**)&slot, A.add(v)}); }
    std::vector<float> sp(int K, int N, const WFn& w, int npl) { return pack_sp(K, N, w, npl, m.half_planes ? 1 : 0); }
    void pad_vec(const float*& slot, const float* v, int n, int np) {
        std::vector<float> t(np, 0.f);
        for (int i = 0; i < n; ++i) t[i] = v[i];
        put(slot, t);
    }
    // a two-layer MLP on K1p -> H -> O tiles: biases of n1 / n2 real columns
    void mlp(MlpW& w, int K1p, int H, int O, const WFn& w1, const float* b1, int n1, const WFn& w2, const float* b2, int n2) {
        w.K1p = K1p; w.H = H; w.O = O;
        put(w.W1, pack(K1p, H, w1)); pad_vec(w.b1, b1, n1, H);
        put(w.W2, pack(H, O, w2)); pad_vec(w.b2, b2, n2, O);
    }
};

// one non-first GVP (vin = V, hidden = V, S real scalar channels in a 256-wide tile): reference gvp.py:30-88 parameter shapes.  npl: 16-bit planes of
// the split copies of Ws / Wg (0: none); quad: the quad-row copy of Ws (RG node instances)
bool pack_gvp(Builder& B, const std::string& key, int V, int S, int vout, FmGvpW& g, int npl, bool quad) {
    const int vop = vout < 16 ? 16 : vout;
    const float* Wh = B.bl.get(key + ".Wh", V, V);
    const float* Wcp = B.bl.get(key + ".Wcp", V, 8);
    const float* Wu = B.bl.get(key + ".Wu", V + 4, vout);
    const float* Ws = B.bl.get(key + ".to_feats_out.0.weight", S, V + 4 + S);
    const float* bs = B.bl.get(key + ".to_feats_out.0.bias", S);
    const float* Wg = B.bl.get(key + ".scalar_to_vector_gates.weight", vout, S);
    const float* bg = B.bl.get(key + ".scalar_to_vector_gates.bias", vout);
    if (!B.bl.ok()) return false;
    B.put(g.Wv1, pack(V, V + 16, [&](int k, int n) -> float {
        if (n < V) return Wh[k * V + n];
        if (n < V + 8) return Wcp[k * 8 + (n - V)];
        return 0.f; }));
    B.put(g.Wu, pack(V + 8, vop, [&](int k, int n) -> float { return (k < V + 4 && n < vout) ? Wu[k * vout + n] : 0.f; }));
    // tile K order [s (256 columns, S real) | norms of the V hidden channels | cp norm 0, 0, cp norm 1, 0, cp norm 2, 0, cp norm 3, 0]: the four
    // cross-product norms sit on the even k-slots of the last k-superstep (fm_gvp_core: its all-zero second MFMA pass is skipped);
    // reference order [s (S) | sh (V+4)]
    const int KS = 256 + V + 8;
    const WFn ws = linear(Ws, S, V + 4 + S, [=](int k) { if (k < 256) return k < S ? k : -1;
                                                          const int o = k - 256; if (o < V) return S + o;
                                                          return ((o - V) & 1) ? -1 : S + V + (o - V) / 2; });
    const WFn wg = linear(Wg, vout, S, below(S));
    B.put(g.Ws, pack(KS, 256, ws));
    if (quad) B.put(g.Ws4, pack4(KS, ws));
    B.pad_vec(g.bs, bs, S, 256);
    B.put(g.Wg, pack(256, vop, wg));
    B.pad_vec(g.bg, bg, vout, vop);
    if (npl) { B.put(g.Ws_sp, B.sp(KS, 256, ws, npl)); B.put(g.Wg_sp, B.sp(256, vop, wg, npl)); }
    return true;
}

void fill_mlp(FmMlpArgs& a, const MlpW& w, int rows) {
    a.rows = rows; a.K1p = w.K1p; a.H = w.H; a.O = w.O;
    a.W1 = w.W1; a.b1 = w.b1; a.W2 = w.W2; a.b2 = w.b2;
    a.ldx = ld_for(w.K1p > w.O ? w.K1p : w.O); a.ldh = ld_for(w.H);
    if (a.slabQ0 && a.ldh < 164) a.ldh = 164;      // SC_EDGE with the fused pair slab: the hidden tile later holds the K = 160 rows [rbf | ef]
}
// ---------------------------------------------------------------------------------------- instance lists of this unit's families (fm_host.h)
using MlpFn = decltype(&fm_k_mlp2<FM_MLP_TABLE>);
using MlpPairFn = decltype(&fm_k_mlp2_pair<FM_MLP_SC_NODE, FM_MLP_SC_EDGE>);
using Mlp4Fn = decltype(&fm_k_mlp4<FM_MLP4_SC_NODE>);
using Mlp4PairFn = decltype(&fm_k_mlp4_pair<FM_MLP4_SC_NODE, FM_MLP_SC_EDGE>);
using ProjFn = decltype(&fm_k_node_proj<32>);
using EdgeUpdFn = decltype(&fm_k_edge_update<32, false>);
using EdgeUpdSpFn = decltype(&fm_k_edge_update_sp<32>);
// MLP tiles are opted into the widest input row any model has (K1 = 256 + 16 + 16 + 32); 32-row tiles into the 64-row size
inline size_t lds_mlp_max(int tm) { return lds_mlp(ld_for(pad8(256 + 16 + 16 + 32)), 260, tm == 16 ? 16 : FM_TM); }
template <int MODE, int TM = FM_TM> Inst<MlpFn> mlp_inst() { return {{MODE, TM}, fm_k_mlp2<MODE, TM>, lds_mlp_max(TM)}; }
template <int A, int B, int TM = FM_TM> Inst<MlpPairFn> mlp_pair_inst() { return {{A, B, TM}, fm_k_mlp2_pair<A, B, TM>, lds_mlp_max(TM)}; }
template <int MODE> Inst<Mlp4Fn> mlp4_inst() { return {{MODE}, fm_k_mlp4<MODE>, (size_t)FM_MLP4_LDS_BYTES}; }
template <int MODE4, int B> Inst<Mlp4PairFn> mlp4_pair_inst() { return {{MODE4, B}, fm_k_mlp4_pair<MODE4, B>, lds_mlp_max(16)}; }
template <int V, int TM = FM_TM> Inst<ProjFn> proj_inst() { return {{V, TM}, fm_k_node_proj<V, TM>, lds_proj(V, TM)}; }
template <int TM, bool NARROW, bool HEAD = false, bool LOSS = false> Inst<EdgeUpdFn> eupd_inst() { return {{TM, NARROW, HEAD, LOSS}, fm_k_edge_update<TM, NARROW, HEAD, LOSS>, lds_edge_upd(TM)}; }
template <int TM, int FMT> Inst<EdgeUpdSpFn> eupd_sp_inst() { return {{TM, FMT}, fm_k_edge_update_sp<TM, FMT>, lds_edge_upd_sp(TM)}; }

const InstList<MlpFn> mlp_instances{"mode, tile_rows", {
    mlp_inst<FM_MLP_TABLE>(), mlp_inst<FM_MLP_SC_NODE>(), mlp_inst<FM_MLP_NODE_HEAD>(), mlp_inst<FM_MLP_EDGE_HEAD>(), mlp_inst<FM_MLP_SC_EDGE>(),
    mlp_inst<FM_MLP_SC_EDGE, 32>(), mlp_inst<FM_MLP_EDGE_HEAD, 32>(),
    mlp_inst<FM_MLP_SC_NODE, 16>(), mlp_inst<FM_MLP_NODE_HEAD, 16>(), mlp_inst<FM_MLP_EDGE_HEAD, 16>(), mlp_inst<FM_MLP_SC_EDGE, 16>(),
    mlp_inst<FM_MLP_TABLE, 16>(),         // compiled and opted in, never selected: the token / dense embeddings run 64-row tiles
    // the heads with the loss epilogue (fm_denoising_loss): one instance per head instance above
    mlp_inst<FM_MLP_NODE_LOSS>(), mlp_inst<FM_MLP_EDGE_LOSS>(), mlp_inst<FM_MLP_EDGE_LOSS, 32>(), mlp_inst<FM_MLP_NODE_LOSS, 16>(), mlp_inst<FM_MLP_EDGE_LOSS, 16>()}};
const InstList<MlpPairFn> mlp_pair_instances{"mode_a, mode_b, tile_rows", {
    mlp_pair_inst<FM_MLP_SC_NODE, FM_MLP_SC_EDGE>(), mlp_pair_inst<FM_MLP_NODE_HEAD, FM_MLP_EDGE_HEAD>(),
    mlp_pair_inst<FM_MLP_SC_NODE, FM_MLP_SC_EDGE, 16>(), mlp_pair_inst<FM_MLP_NODE_HEAD, FM_MLP_EDGE_HEAD, 16>(),
    mlp_pair_inst<FM_MLP_NODE_LOSS, FM_MLP_EDGE_LOSS>(), mlp_pair_inst<FM_MLP_NODE_LOSS, FM_MLP_EDGE_LOSS, 16>()}};
const InstList<Mlp4Fn> mlp4_instances{"mode", {mlp4_inst<FM_MLP4_SC_NODE>(), mlp4_inst<FM_MLP4_NODE_HEAD>(), mlp4_inst<FM_MLP4_PROJ0>(), mlp4_inst<FM_MLP4_NODE_LOSS>()}};
const InstList<Mlp4PairFn> mlp4_pair_instances{"mode_a, mode_b", {mlp4_pair_inst<FM_MLP4_SC_NODE, FM_MLP_SC_EDGE>(), mlp4_pair_inst<FM_MLP4_NODE_HEAD, FM_MLP_EDGE_HEAD>(),
                                                                          mlp4_pair_inst<FM_MLP4_NODE_LOSS, FM_MLP_EDGE_LOSS>()}};
const InstList<ProjFn> node_proj_instances{"V, tile_rows", {proj_inst<32>(), proj_inst<16>(), proj_inst<32, 16>(), proj_inst<16, 16>()}};
const InstList<EdgeUpdFn> edge_update_instances{"tile_rows, narrow, head, loss", {eupd_inst<32, false>(), eupd_inst<64, false>(), eupd_inst<32, true>(), eupd_inst<32, false, true>(),
                                                                                eupd_inst<32, false, true, true>()}};
const InstList<EdgeUpdSpFn> edge_update_sp_instances{"tile_rows, half_planes", {eupd_sp_inst<32, 0>(), eupd_sp_inst<32, 1>()}};
// fused campbell step, keyed like its gat sibling (ctmc_gat_instances, fm_host.h); per-molecule time (`mixed`) is a kernel with an argument struct of its own,
// hence a list of its own.  No dynamic LDS; the workgroup size is BatchPlan::ctmc_threads
const InstList<decltype(&fm_k_ctmc_fused_mixed<256>)> ctmc_mixed_instances{"ctmc_threads", {{{1024}, fm_k_ctmc_fused_mixed<1024>, 0}, {{256}, fm_k_ctmc_fused_mixed<256>, 0}}};
const InstList<decltype(&fm_k_ctmc_fused<256>)> ctmc_instances{"ctmc_threads", {{{1024}, fm_k_ctmc_fused<1024>, 0}, {{256}, fm_k_ctmc_fused<256>, 0}}};
// the same three kernels with frozen rows (fm_ctmc_step_inpaint / fm_integrate_inpaint): lists of their own, so the lists above launch what they always did
const InstList<decltype(&fm_k_ctmc_fused_keep<256>)> ctmc_keep_instances{"ctmc_threads", {{{1024}, fm_k_ctmc_fused_keep<1024>, 0}, {{256}, fm_k_ctmc_fused_keep<256>, 0}}};
const InstList<decltype(&fm_k_ctmc_fused_mixed_keep<256>)> ctmc_mixed_keep_instances{"ctmc_threads", {{{1024}, fm_k_ctmc_fused_mixed_keep<1024>, 0}, {{256}, fm_k_ctmc_fused_mixed_keep<256>, 0}}};
const InstList<decltype(&fm_k_ctmc_gat_fused_keep<256>)> ctmc_gat_keep_instances{"ctmc_threads", {{{1024}, fm_k_ctmc_gat_fused_keep<1024>, 0}, {{256}, fm_k_ctmc_gat_fused_keep<256>, 0}}};

// fm_k_mlp2<mode, tm> over `rows` rows
void launch_mlp(Launch& L, int mode, const char* name, FmMlpArgs a, const MlpW& w, int rows, int tm = FM_TM) {
    fill_mlp(a, w, rows);
    launch_inst(L, mlp_instances, {mode, tm}, name, dim3((rows + tm - 1) / tm), dim3(FM_THREADS), lds_mlp(a.ldx, a.ldh, tm), a);
}

// The node-side MLP (N rows) and the pair-side MLP (U rows) of one stage -- the self-conditioning layer or the output heads -- with the same inputs.
// While the batch is small they share one launch (two launches less per step where launches are what a step costs).  The shared launch allocates the
// LARGER tile's LDS (node tiles: 147 KB -> one workgroup per CU) for every workgroup, so once the pair tiles alone fill the chip they run as a launch of
// their own at two workgroups per CU (profiles/r02n: 1.16 -> 0.94 ms and 0.83 -> 0.68 ms per step at 1024 molecules).  BatchPlan::pair_mlps decides;
// the node side runs 4-row tiles when mlp4 holds (BatchPlan::mlp4, never for dense inputs), the pair side 32-row tiles when pair32 holds and its
// tiles are not small.  pair = nullptr: the node side only.
void launch_mlp_stage(Launch& L, const BatchPlan& p, bool mlp4, int mode4, int mode_n, int mode_p, const char* both, const char* node, const char* pair,
                      const FmMlp4Args& a4, FmMlpArgs a, const MlpW& wn, FmMlpArgs e, const MlpW& wp, bool pair32) {
    const int N = p.N, U = p.U;
    const bool small = p.small_node && p.small_pair;
    const dim3 blk(FM_THREADS);
    if (pair && p.pair_mlps && mlp4 && small) {
        fill_mlp(e, wp, U);
        const int ta = (N + 3) / 4, tb = (U + 15) / 16;
        launch_inst(L, mlp4_pair_instances, {mode4, mode_p}, both, dim3(ta + tb), blk, std::max((size_t)FM_MLP4_LDS_BYTES, lds_mlp(e.ldx, e.ldh, 16)), a4, e, ta);
    } else if (pair && p.pair_mlps) {
        fill_mlp(a, wn, N); fill_mlp(e, wp, U);
        const int tm = small ? 16 : FM_TM, ta = (N + tm - 1) / tm, tb = (U + tm - 1) / tm;
        launch_inst(L, mlp_pair_instances, {mode_n, mode_p, tm}, both, dim3(ta + tb), blk, std::max(lds_mlp(a.ldx, a.ldh, tm), lds_mlp(e.ldx, e.ldh, tm)), a, e, ta);
    } else {
        if (mlp4) launch_inst(L, mlp4_instances, {mode4}, node, dim3((N + 3) / 4), blk, (size_t)FM_MLP4_LDS_BYTES, a4);
        else launch_mlp(L, mode_n, node, a, wn, N, p.small_node ? 16 : FM_TM);
        if (pair) launch_mlp(L, mode_p, pair, e, wp, U, p.small_pair ? 16 : pair32 ? 32 : FM_TM);
    }
}

// ---------------------------------------------------------------------------------------- one network evaluation
// node_proj instances (small kernels of this unit): V = 16 | 32 vector channels, 64- or 16-row tiles
void launch_node_proj(Launch& L, const char* name, int V, bool small, int N, const FmProjArgs& pa) {
    const int tm = small ? 16 : FM_TM;
    launch_inst(L, node_proj_instances, {V, tm}, name, dim3((N + tm - 1) / tm), dim3(FM_THREADS), lds_proj(V, tm), pa);
}

// One network evaluation of the bound batch is a short sequence of stages (evaluate, below); every stage takes the Launch, the context and what varies.  The
// kernel instances are selected from the model (vector channels V, destination-feature vectors HX), the batch plan (tile heights, fusions, MLP tiles:
// plan_batch) and the call (prev given, dense inputs, taps); the heavy families live in translation units of their own (fm_host.h).
// the 4-row-tile arguments (fm_k_mlp4) of a stage's node side from its regular ones: same sources and destinations, the quad-row weight copies (the heads'
// copy so also carries the rbf constants, which the parent left 0 there and NODE_HEAD never reads)
FmMlp4Args mlp4_args(const FmMlpArgs& a, int N, const MlpW& w, const void* W1q, const void* W2q) {
    FmMlp4Args q{};
    q.N = N; q.W1q = W1q; q.b1 = w.b1; q.W2q = W2q; q.b2 = w.b2;
    q.s_tab = a.s_tab; q.tok_a = a.tok_a; q.tok_c = a.tok_c; q.n_c1 = a.n_c1; q.tab_slot = a.tab_slot; q.node_mol = a.node_mol; q.slot_rows = a.slot_rows;
    q.prev_a = a.prev_a; q.prev_c = a.prev_c; q.prev_x = a.prev_x; q.x_t = a.x_t;
    q.na = a.na; q.nc = a.nc; q.rbf_mu_step = a.rbf_mu_step; q.rbf_inv_sigma = a.rbf_inv_sigma;
    q.in = a.in; q.out = a.out; q.out2 = a.out2; q.tgt_a = a.tgt_a; q.tgt_c = a.tgt_c;
    return q;
}

// Input stage: s and ef from dense inputs (endpoint-parameterised models), from the tokens and a previous endpoint prediction (the self-conditioning
// layer; n_pq > 0: and the first convolutions' pair slab), or from the tokens alone (rows of the embedding tables)
void input_stage(Launch& L, fm_ctx* c, const FmMlpArgs& base, const fm_state* state, const fm_dst* prev, const fm_dense_state* dense, const float* temb,
                 bool mlp4, int n_pq) {
    const Workspace& w = c->ws;
    const FmBatch& b = w.b;
    if (dense) {
        // the categorical inputs are continuous vectors, so the embeddings are real MLPs over the N node rows [a_t | c_t | temb] and the U pair rows e_t
        // (vector_field.py:226-261) -- the same two-layer kernel the token tables use, fed with dense rows; pair rows are written to both directed
        // edges.  Ps is free scratch until the first node_proj.
        const int kp = c->node_embed.K1p;
        L("dense_in", fm_k_dense_node_in, dim3(std::min(2048, (int)(((size_t)b.N * kp + 255) / 256))), dim3(256), 0, w.Ps, kp, b.N,
          (const float*)dense->a_t, c->na, (const float*)dense->c_t, c->nc, temb, c->cfg.time_embedding_dim);
        FmMlpArgs a{};
        a.in = w.Ps; a.in_ld = kp; a.out = w.s; a.out_ld = 256; a.ln_g = c->node_ln_g; a.ln_b = c->node_ln_b; a.ln_n = c->S;
        launch_mlp(L, FM_MLP_TABLE, "embed_nodes", a, c->node_embed, b.N);
        FmMlpArgs e{};
        e.in = dense->e_t; e.in_ld = c->ne; e.in_w = c->ne; e.out = w.ef; e.out_ld = 128; e.ln_g = c->edge_ln_g; e.ln_b = c->edge_ln_b; e.ln_n = c->F;
        e.p_e0 = b.p_e0; e.p_e1 = b.p_e1;
        launch_mlp(L, FM_MLP_TABLE, "embed_pairs", e, c->edge_embed, b.U);
    } else if (prev) {
        FmMlpArgs a = base, e = base;
        a.s_tab = c->s_tab; a.tok_a = state->a_t; a.tok_c = state->c_t; a.n_c1 = c->nc + 1;
        a.tab_slot = c->tab_slot; a.node_mol = b.node_mol; a.slot_rows = (int)(c->tab_slot_floats / 256);
        a.prev_a = prev->a; a.prev_c = prev->c; a.prev_x = prev->x; a.x_t = state->x_t;
        a.out = w.s;
        e.e_src = b.e_src; e.e_dst = b.e_dst; e.e_pair = b.e_pair; e.tok_e = state->e_t;
        e.prev_e = prev->e; e.prev_x = prev->x; e.x_t = state->x_t; e.T1 = c->T1; e.ef_tab = c->ef_tab;
        e.out = w.ef; e.p_e0 = b.p_e0; e.p_e1 = b.p_e1;
        if (n_pq > 0) {      // the self-conditioning layer produces the edge features the first convolutions see: their pair slab in the same kernel
            e.slabW0 = c->conv[0].Ws_slab; e.slabQ0 = w.Q[0];
            if (n_pq > 1) { e.slabW1 = c->conv[1].Ws_slab; e.slabQ1 = w.Q[1]; }
        }
        // one row per unordered pair, written to both directed edges; with the pair slab the edge kernel is matrix-pipe work followed by 3 KB of row
        // stores per pair: 32-row tiles (38 KB of LDS) put four independent workgroups on a CU instead of two, so that one's stores overlap the others' GEMMs
        launch_mlp_stage(L, c->plan, mlp4, FM_MLP4_SC_NODE, FM_MLP_SC_NODE, FM_MLP_SC_EDGE, "sc", "sc_node", "sc_edge",
                         mlp4_args(a, b.N, c->sc_node, c->sc_node_W1q, c->sc_node_W2q), a, c->sc_node, e, c->sc_edge, n_pq > 0);
    } else {
        L("gather_s", fm_k_gather_rows, dim3(std::min(2048, (b.N * 64 + 255) / 256)), dim3(256), 0, w.s, (const float*)c->s_tab, 256, b.N,
          (const int*)state->a_t, (const int*)state->c_t, c->nc + 1, (const int*)nullptr, c->tab_slot, (const int*)b.node_mol, (int)(c->tab_slot_floats / 256));
        L("gather_ef", fm_k_gather_rows, dim3(std::min(4096, (int)(((size_t)b.E * 32 + 255) / 256))), dim3(256), 0, w.ef, c->ef_tab, 128, b.E,
          (const int*)state->e_t, (const int*)nullptr, 0, (const int*)b.e_pair, (const int*)nullptr, (const int*)nullptr, 0);
    }
}

// Pass `it` of n_pass: node projections (pass 0, or every pass of the unfused sequence), edge messages, node update.  x_t: copied into the working
// positions by pass 0; pq: a pair-slab convolution of this evaluation (FmMlpArgs::slabQ0)
void conv_pass(Launch& L, fm_ctx* c, const Taps& tap, int it, int n_pass, const float* x_t, bool mlp4, bool pq) {
    const BatchPlan& p = c->plan;
    const Workspace& w = c->ws;
    const fm_config& cf = c->cfg;
    const int V = c->V, TN = p.tm_node, HX = c->HX, N = w.b.N;
    const int i = it % cf.n_convs, u = cf.update_after[i];
    const ConvW& cw = c->conv[i];
    const ConvW* nx = it + 1 < n_pass ? &c->conv[(i + 1) % cf.n_convs] : nullptr;      // the next pass's convolution
    const dim3 blk(FM_THREADS), gnt((N + TN - 1) / TN);
    if (it == 0 || !p.fuse_node) {      // later convs: projected in the previous conv's node_update
        if (it == 0 && mlp4) {
            FmMlp4Args p4{};
            p4.N = N; p4.in = w.s; p4.Wps4 = cw.Wps4; p4.Ps = w.Ps; p4.PV = w.PV; p4.pv_w = c->PVW; p4.v_init = w.v; p4.V = V; p4.x_src = x_t; p4.x_dst = w.xw;
            launch_inst(L, mlp4_instances, {FM_MLP4_PROJ0}, "node_proj", dim3((N + 3) / 4), blk, (size_t)FM_MLP4_LDS_BYTES, p4);
        } else {
            FmProjArgs pa{};
            pa.N = N; pa.s = w.s; pa.v = w.v; pa.Wps = cw.Wps; pa.Ps = w.Ps; pa.Wpv = cw.Wpv; pa.PV = w.PV; pa.pv_w = c->PVW;
            if (it == 0) { pa.v_init = w.v; pa.x_src = x_t; pa.x_dst = w.xw; }     // v = 0, working copy of x (no memset / memcpy nodes)
            launch_node_proj(L, "node_proj", V, p.small_node, N, pa);
        }
    }
    FmMsgArgs m{};
    m.b = w.b; m.x = w.xw; m.ef = w.ef; m.Ps = w.Ps; m.PV = w.PV; m.w0 = cw.w0;
    if (HX > 0) {       // use_dst_feats: projection GVP of the conv's input features + its per-node hoists
        FmDstProjArgs dp{};
        dp.N = N; dp.s = w.s; dp.v = w.v; dp.g = cw.dproj; dp.Wsd = cw.Wsd; dp.Psd = w.Psd; dp.Wpvd = cw.Wpvd; dp.PVd = w.PVd; dp.pv_w = c->PVW;
        fm_launch_dst_proj(L, V, TN, HX, gnt, dp);
        m.Psd = w.Psd; m.PVd = w.PVd;
    }
    m.g0 = cw.msg[0]; m.g1 = cw.msg[1]; m.g2 = cw.msg[2]; m.part_s = w.part_s; m.part_v = w.part_v;
    m.rbf_mu_step = c->rbf_mu_step; m.rbf_inv_sigma = c->rbf_inv_sigma;
    // per-edge message taps are written straight into the caller's buffers (both must be registered)
    m.dbg_s = it == 0 && tap.find("conv0.msg.v") ? (float*)tap.find("conv0.msg.s") : nullptr;
    m.dbg_v = m.dbg_s ? (float*)tap.find("conv0.msg.v") : nullptr;
    dim3 gmsg(p.n_tiles_msg);      // edge tiles: molecule-aligned, FmBatch::tile_desc
    if (p.xcd_swizzle) { m.xcd_chunk = (p.n_tiles_msg + 7) / 8; gmsg = dim3(8 * m.xcd_chunk); }
    if (pq) { m.Q = w.Q[it]; m.g0.Ws = cw.Ws_sh; }          // GVP0's scalar GEMM: K = KU0 (hidden-vector norms); the rest arrives through Q
    fm_launch_edge_message(L, V, p.tm_edge, HX, cf.precision, pq, gmsg, m);
    FmNodeUpdArgs nu{};
    nu.b = w.b; nu.s = w.s; nu.v = w.v; nu.part_s = w.part_s; nu.part_v = w.part_v; nu.inv_z = cf.msg_z < 0.f ? -1.0f : 1.0f / cf.msg_z;
    nu.g0 = cw.upd[0]; nu.g1 = cw.upd[1]; nu.g2 = cw.upd[2];
    nu.ln1_g = cw.ln1_g; nu.ln1_b = cw.ln1_b; nu.ln2_g = cw.ln2_g; nu.ln2_b = cw.ln2_b;
    // aggregated-message taps go through scratch of their own (Ps / PV, which served in round 1, are outputs of the fused kernel)
    const bool tagg = tap.find("conv", i, ".agg.s") || tap.find("conv", i, ".agg.v");
    nu.agg_s = tagg ? w.tap_s : nullptr; nu.agg_v = tagg ? w.tap_v : nullptr;
    if (p.fuse_node) {
        if (nx) { nu.Wps = nx->Wps; nu.Wps4 = nx->Wps4; nu.Ps = w.Ps; nu.Wpv = nx->Wpv; nu.PV = w.PV; }
        if (u >= 0) {
            const UpdW& uw = c->upd[u];
            nu.Wasd = uw.Wasd; nu.Wasd4 = uw.Wasd4; nu.Asd = w.Asd; nu.p0 = uw.pos[0]; nu.p1 = uw.pos[1]; nu.p2 = uw.pos[2]; nu.x = w.xw;
        }
    }
    nu.s_real = c->S;
    // instance of the node kernel: split precision, 4 rg nodes per workgroup (one tile per CU), narrow, or the regular one
    if (p.node_sp) {
        if (nx) nu.Wps_sp = nx->Wps_sp;
        if (u >= 0) nu.Wasd_sp = c->upd[u].Wasd_sp;
    }
    const int rg = p.node_rg;
    const size_t lds = p.node_sp ? lds_gvp_sp(V, TN) - (size_t)TN * 9 * 4 : lds_gvp(V, TN, false);
    fm_launch_node_update(L, V, TN, p.node_sp || c->mp.narrow_s, p.node_sp, rg, rg ? dim3((N + 4 * rg - 1) / (4 * rg)) : gnt, lds, nu);
    if (tagg) { tap(w.tap_s, (size_t)N * 256 * 4, "conv", i, ".agg.s"); tap(w.tap_v, (size_t)N * 3 * V * 4, "conv", i, ".agg.v"); }
    tap(w.s, (size_t)N * 256 * 4, "conv", i, ".s"); tap(w.v, (size_t)N * 3 * V * 4, "conv", i, ".v");
}

// The molecule update after convolution i: positions and EdgeUpdate's node terms (kernels of their own in the unfused sequence, else done by node_update),
// then EdgeUpdate.  last: the evaluation's last pass, whose EdgeUpdate may run the edge head as its epilogue -- returns whether it did
bool mol_update(Launch& L, fm_ctx* c, const Taps& tap, int i, bool last, const fm_dst* out, const fm_state* xt, const fm_state* loss_x1) {
    const BatchPlan& p = c->plan;
    const Workspace& w = c->ws;
    const int V = c->V, TN = p.tm_node, N = w.b.N, E = w.b.E;
    const UpdW& uw = c->upd[c->cfg.update_after[i]];
    const dim3 blk(FM_THREADS);
    const bool head_done = !c->mp.node_sp && last && p.fuse_head && !tap.find("upd", i, ".ef");      // a registered upd<i>.ef tap keeps the head unfused
    if (!p.fuse_node) {
        FmPosArgs pp{};
        pp.N = N; pp.s = w.s; pp.v = w.v; pp.x = w.xw; pp.g0 = uw.pos[0]; pp.g1 = uw.pos[1]; pp.g2 = uw.pos[2];
        fm_launch_pos_update(L, V, TN, dim3((N + TN - 1) / TN), pp);
        FmProjArgs pa2{};
        pa2.N = N; pa2.s = w.s; pa2.v = w.v; pa2.Wasd = uw.Wasd; pa2.Asd = w.Asd;
        launch_node_proj(L, "node_proj_asd", V, p.small_node, N, pa2);
    }
    FmEdgeUpdArgs eu{};
    eu.b = w.b; eu.x = w.xw; eu.Asd = w.Asd; eu.ef = w.ef; eu.W1 = uw.W1; eu.b1 = uw.b1; eu.W2 = uw.W2; eu.b2 = uw.b2;
    eu.ln_g = uw.ln_g; eu.ln_b = uw.ln_b; eu.rbf_mu_step = c->rbf_mu_step; eu.rbf_inv_sigma = c->rbf_inv_sigma; eu.f_real = c->F;
    if (c->mp.node_sp) {
        const FmEdgeUpdSpW sw{uw.W1_sp, uw.W2_sp};
        launch_inst(L, edge_update_sp_instances, {32, c->mp.half_planes}, "edge_update", dim3((E + 31) / 32), blk, lds_edge_upd_sp(32), eu, sw);
    } else if (head_done) {
        // the evaluation's last EdgeUpdate: its rows feed the edge head and nothing else -- tiles of 16 pairs, the head as the epilogue, no ef store
        eu.hW1 = c->edge_head.W1; eu.hb1 = c->edge_head.b1; eu.hW2 = c->edge_head.W2; eu.hb2 = c->edge_head.b2; eu.out_e = out->e; eu.ne = c->ne;
        if (loss_x1) { eu.tok_e = xt->e_t; eu.tgt_e = loss_x1->e_t; }
        launch_inst(L, edge_update_instances, {32, false, true, loss_x1 ? 1 : 0}, "edge_update_head", dim3((w.b.U + 15) / 16), blk, lds_edge_upd(32), eu);
    } else {
        const int tm = p.tm_eupd;
        launch_inst(L, edge_update_instances, {tm, c->mp.narrow_f, false}, "edge_update", dim3((E + tm - 1) / tm), blk, lds_edge_upd(tm), eu);
    }
    tap(w.xw, (size_t)N * 3 * 4, "upd", i, ".x");
    if (!head_done) tap(w.ef, (size_t)E * 128 * 4, "upd", i, ".ef");
    return head_done;
}

// The output heads.  head_done: the edge head ran as the epilogue of the last EdgeUpdate, only the node head is left.  loss_x1 (fm_denoising_loss): the same
// launches with the heads' loss instances -- out->a / c / e receive one nll per row, from the tokens of xt and the target tokens of loss_x1
void heads(Launch& L, fm_ctx* c, const FmMlpArgs& base, bool mlp4, bool head_done, const fm_dst* out, const fm_state* xt, const fm_state* loss_x1) {
    FmMlpArgs a = base, e = base;
    a.in = c->ws.s; a.out = out->a; a.out2 = out->c;
    e.ef = c->ws.ef; e.p_e0 = c->ws.b.p_e0; e.p_e1 = c->ws.b.p_e1; e.out = out->e;
    if (loss_x1) {
        a.tok_a = xt->a_t; a.tok_c = xt->c_t; a.tgt_a = loss_x1->a_t; a.tgt_c = loss_x1->c_t;
        e.tok_e = xt->e_t; e.tgt_e = loss_x1->e_t;
    }
    launch_mlp_stage(L, c->plan, mlp4, loss_x1 ? FM_MLP4_NODE_LOSS : FM_MLP4_NODE_HEAD, loss_x1 ? FM_MLP_NODE_LOSS : FM_MLP_NODE_HEAD,
                     loss_x1 ? FM_MLP_EDGE_LOSS : FM_MLP_EDGE_HEAD, "heads", "node_head", head_done ? nullptr : "edge_head",
                     mlp4_args(a, c->ws.b.N, c->node_head, c->node_head_W1q, c->node_head_W2q), a, c->node_head, e, c->edge_head, c->plan.edge_head32);
}

int evaluate(fm_ctx* c, hipStream_t st, const fm_state* state, const fm_dst* prev, int remove_com, const fm_dst* out,
             bool taps_on, const fm_dense_state* dense = nullptr, const float* temb = nullptr, const fm_state* loss_x1 = nullptr) {
    Launch L{c, st};
    const Taps tap{L, taps_on && !c->taps.empty()};
    const fm_config& cf = c->cfg;
    const bool mlp4 = c->plan.mlp4 && !dense, sc = prev && !dense;
    const int n_pq = sc ? c->plan.n_pq : 0;      // pair-slab convolutions of this evaluation (first passes only)
    FmMlpArgs base{};      // the fields every MLP stage shares
    base.na = c->na; base.nc = c->nc; base.ne = c->ne; base.rbf_mu_step = c->rbf_mu_step; base.rbf_inv_sigma = c->rbf_inv_sigma;
    input_stage(L, c, base, state, prev, dense, temb, mlp4, n_pq);
    tap(c->ws.s, (size_t)c->ws.b.N * 256 * 4, sc ? "sc.s" : "embed.s");
    tap(c->ws.ef, (size_t)c->ws.b.E * 128 * 4, sc ? "sc.ef" : "embed.ef");
    const int n_pass = cf.n_convs * (cf.n_recycles > 1 ? cf.n_recycles : 1);       // vector_field.py:307: the whole stack again, same weights
    bool head_done = false;
    for (int it = 0; it < n_pass; ++it) {
        conv_pass(L, c, tap, it, n_pass, dense ? dense->x_t : state->x_t, mlp4, it < n_pq);
        if (cf.update_after[it % cf.n_convs] >= 0) head_done = mol_update(L, c, tap, it % cf.n_convs, it == n_pass - 1, out, state, loss_x1);
    }
    heads(L, c, base, mlp4, head_done, out, state, loss_x1);
    if (remove_com != 2) {       // 2: the caller's fused CTMC kernel centres the raw positions (ws.xw) and writes out->x itself
        L.copy(out->x, c->ws.xw, (size_t)c->ws.b.N * 3 * 4);
        if (remove_com) L("remove_com", fm_k_remove_com, dim3(c->ws.b.B), dim3(64), 0, out->x, (const int*)c->ws.b.mol_node_off);
    }
    return L.rc;
}

// The (atom type, charge) embedding table(s) of `n_tables` consecutive time points (temb: n_tables x time_embedding_dim) into the
// workspace's table slots 0..n_tables-1, ONE launch: the table depends on the time only, so fm_integrate builds the tables of a
// whole chunk of steps up front (a launch that fills the chip) instead of one 2-tile launch on every step's critical path.
int embed_table(fm_ctx* c, hipStream_t st, const float* temb, int n_tables = 1) {
    Launch L{c, st};
    const fm_config& cf = c->cfg;
    FmMlpArgs a{};
    a.in = nullptr; a.n_c1 = c->nc + 1;          // rows = (a,c) token pairs; the input row is built in the kernel's prologue
    a.emb_a = c->emb_a; a.emb_c = c->emb_c; a.temb = temb;
    a.ta = cf.a_token_dim ? cf.a_token_dim : c->na + 1; a.tc = cf.c_token_dim ? cf.c_token_dim : c->nc + 1; a.tt = cf.time_embedding_dim;
    a.out = c->ws.s_tab_base; a.out_ld = 256; a.ln_g = c->node_ln_g; a.ln_b = c->node_ln_b; a.ln_n = c->S;
    fill_mlp(a, c->node_embed, c->tab_rows);
    a.tab_tiles = (c->tab_rows + FM_TM - 1) / FM_TM; a.tab_stride = a.tab_tiles * FM_TM * 256;
    launch_inst(L, mlp_instances, {FM_MLP_TABLE, FM_TM}, "embed_table", dim3(a.tab_tiles * n_tables), dim3(FM_THREADS), lds_mlp(a.ldx, a.ldh), a);
    return L.rc;
}

// table_slot >= 0: the caller (step_driver) has already built this step's table into that slot, and temb is not read (it may be null); else the n_tables
// tables are built here from temb's rows.  tab_slot (per-molecule time): device (n_mols) slot of every molecule's table, counted from `table_slot`
int forward_impl(fm_ctx* c, hipStream_t st, const fm_state* state, const float* temb, const fm_dst* prev, int bootstrap,
                 int remove_com, const fm_dst* out, int table_slot = -1, const int* tab_slot = nullptr, int n_tables = 1, const fm_state* loss_x1 = nullptr) {
    int rc = 0;
    if (table_slot < 0) { table_slot = 0; rc = embed_table(c, st, temb, n_tables); }
    if (rc) return rc;
    c->s_tab = c->ws.s_tab_base + (size_t)table_slot * c->tab_slot_floats;
    c->tab_slot = tab_slot;
    const bool sc = c->cfg.self_conditioning != 0;
    if (sc && !prev && bootstrap) {
        const fm_dst& boot = c->ws.boot;
        rc = evaluate(c, st, state, nullptr, 0, &boot, false);
        if (rc) return rc;
        if (!c->taps.empty() && c->taps.count("boot.x")) {      // the bootstrap prediction's taps: asked for by registering boot.x
            Launch L{c, st};
            const Taps tap{L, true};
            const size_t N = c->ws.b.N, U = c->ws.b.U;
            tap(boot.x, N * 12, "boot.x"); tap(boot.a, N * c->na * 4, "boot.a"); tap(boot.c, N * c->nc * 4, "boot.c"); tap(boot.e, U * c->ne * 4, "boot.e");
            if (L.rc) return L.rc;
        }
        prev = &boot;
    }
    if (!sc) prev = nullptr;
    return evaluate(c, st, state, prev, remove_com, out, true, nullptr, nullptr, loss_x1);
}

__global__ void fm_k_noop() {}

// device arrays of one call-step of fm_integrate_mixed (FmCtmcMixedArgs)
struct MixedStep { const fm_step_scalars* steps; const int* active; const int* mol_group; };
// frozen rows of one step (fm_ctmc_step_inpaint / fm_integrate_inpaint): the kernels' FmKeepArgs -- alpha filled for a batch at one time -- and, with per-molecule
// time, this call-step's (n_groups, 4) row of the caller's device alpha_next array
struct KeepStep { FmKeepArgs k; const float* alpha_dev; };

// frame: this step's slice of the trajectory sink (x, a, c, e, x1 used; a1 / c1 / e1 travel in `smp`); campbell steps write it inside the fused kernel
int ctmc_impl(fm_ctx* c, hipStream_t st, const Modality (&md)[3], const fm_state* state, const fm_dst* dst, const fm_step_noise* nz,
              const fm_step_scalars* sc, const fm_sampled* smp, const float* x_raw = nullptr, const fm_traj_sink* frame = nullptr,
              const MixedStep* mixed = nullptr, const KeepStep* keep = nullptr) {
    Launch L{c, st};
    // profiling only: an event pair around an empty kernel, once per step.  Its elapsed time is what a pair adds to every profiled launch
    // (event signalling + the dispatch that cannot overlap the previous kernel's tail); fm_profile_get("event_overhead") lets the caller
    // subtract it, which matters for the sub-millisecond kernels of small batches (HIP events vs rocprofv3: +12 % on a 350 us kernel).
    if (c->prof) L("event_overhead", fm_k_noop, dim3(1), dim3(64), 0);
    const FmBatch& b = c->ws.b;
    static const fm_step_noise no_noise{};
    const char* const missing = "fm_ctmc_step: noise tensors missing (noise_mode FM_NOISE_TENSORS)";
    const bool philox = sc->noise_mode == FM_NOISE_PHILOX;
    if (!nz && !philox) return fail(c, FM_ERR_INVALID, "%s", missing);
    if (!nz) nz = &no_noise;      // Philox steps draw inside the kernel
    // what the per-modality structs of the three kernels share: K, p, xt, x1 (the caller's buffer or the workspace's), and for the fused ones off, sink_t
    auto fill_mod = [&](auto& d, int m) {
        int32_t* const x1 = smp ? pick3(m, smp->a1, smp->c1, smp->e1) : nullptr;
        d.K = md[m].K; d.p = pick3(m, dst->a, dst->c, dst->e); d.xt = md[m].tok; d.x1 = x1 ? x1 : md[m].x1;
    };
    auto fill_fused = [&](auto& f) {      // + the position job and the Philox stream of a fused kernel (fm_ctmc_x_job)
        for (int m = 0; m < 3; ++m) {
            fill_mod(f.mod[m], m);
            f.mod[m].off = md[m].off; f.mod[m].sink_t = frame ? pick3(m, frame->a, frame->c, frame->e) : nullptr;
        }
        f.x_t = state->x_t; f.x1 = dst->x; f.node_off = b.mol_node_off; f.coef = sc->x_coef; f.dt = sc->dt; f.scale = sc->x_scale;
        f.x_raw = x_raw; f.x1_out = dst->x;
        if (frame) { f.sink_x = frame->x; f.sink_x1 = frame->x1; }
        if (philox) { f.seed_lo = sc->philox_seed_lo; f.seed_hi = sc->philox_seed_hi; f.step = sc->step_index; f.mol_gid = c->ws.mol_gid; }
    };
    const int nt = c->plan.ctmc_threads;
    const dim3 grid(b.B, 4), blk(nt);
    if (sc->dfm_type == FM_DFM_GAT && philox) {      // in-kernel noise: the whole step in one launch (fm_k_ctmc_gat_fused)
        FmGatFusedArgs f{};
        fill_fused(f);
        for (int m = 0; m < 3; ++m) { f.mod[m].cf = sc->gat_cf[m]; f.mod[m].cb = sc->gat_cb[m]; }
        f.temp = sc->cat_temperature; f.fw = sc->gat_fw; f.bw = sc->gat_bw; f.dt_cat = sc->dt;
        if (keep) launch_inst(L, ctmc_gat_keep_instances, {nt}, "ctmc_keep", grid, blk, 0, f, keep->k);
        else launch_inst(L, ctmc_gat_instances(), {nt}, "ctmc", grid, blk, 0, f);
        return L.rc;
    }
    if (sc->dfm_type == FM_DFM_GAT) {      // tensor noise: the Euler step and one flat kernel per modality
        if (!nz->q_a) return fail(c, FM_ERR_INVALID, "%s", missing);
        if (keep) L("x_step_keep", fm_k_x_step_keep, dim3((b.N * 3 + 255) / 256), dim3(256), 0, state->x_t, (const float*)dst->x, sc->x_coef, sc->dt, sc->x_scale, b.N * 3,
                    FmKeepX{keep->k.keep_x, keep->k.x0, keep->k.x1c, keep->k.alpha[0]});
        else L("x_step", fm_k_x_step, dim3((b.N * 3 + 255) / 256), dim3(256), 0, state->x_t, (const float*)dst->x, sc->x_coef, sc->dt, sc->x_scale, b.N * 3);
        for (int m = 0; m < 3; ++m) {
            if (md[m].rows == 0) continue;
            FmGatArgs a{};
            fill_mod(a, m);
            a.rows = md[m].rows; a.q = pick3(m, nz->q_a, nz->q_c, nz->q_e);
            a.temp = sc->cat_temperature; a.cf = sc->gat_cf[m]; a.cb = sc->gat_cb[m]; a.fw = sc->gat_fw; a.bw = sc->gat_bw; a.dt = sc->dt;
            if (keep) L("ctmc_gat_keep", fm_k_ctmc_gat_keep, dim3((a.rows + 255) / 256), dim3(256), 0, a,
                        FmKeepMod{keep->k.keep[m], keep->k.tok1[m], keep->k.u[m], 1.0f - keep->k.alpha[1 + m]});
            else L("ctmc_gat", fm_k_ctmc_gat, dim3((a.rows + 255) / 256), dim3(256), 0, a);
        }
        return L.rc;
    }
    if (sc->dfm_type != FM_DFM_CAMPBELL) return fail(c, FM_ERR_INVALID, "fm_ctmc_step: unknown dfm_type %d", sc->dfm_type);
    FmCtmcFusedArgs f{};
    fill_fused(f);
    for (int m = 0; m < 3; ++m) {
        FmCtmcMod& d = f.mod[m];
        d.q = pick3(m, nz->q_a, nz->q_c, nz->q_e); d.u1 = pick3(m, nz->u1_a, nz->u1_c, nz->u1_e); d.u2 = pick3(m, nz->u2_a, nz->u2_c, nz->u2_e);
        d.unmask_prob = sc->unmask_prob[m]; d.mask_prob = sc->mask_prob[m];
    }
    f.temp = sc->cat_temperature; f.hc_thresh = sc->hc_thresh; f.last_step = sc->last_step; f.philox = philox;
    if (!philox && (!nz->q_a || !nz->u1_a || !nz->q_e)) return fail(c, FM_ERR_INVALID, "%s", missing);
    // per-molecule time: the scalars of `f` are unused, every molecule reads its group's from the caller's device arrays
    if (mixed && keep) launch_inst(L, ctmc_mixed_keep_instances, {nt}, "ctmc_mixed_keep", grid, blk, 0, FmCtmcMixedArgs{f, mixed->steps, mixed->active, mixed->mol_group}, keep->k, keep->alpha_dev);
    else if (keep) launch_inst(L, ctmc_keep_instances, {nt}, "ctmc_keep", grid, blk, 0, f, keep->k);
    else if (mixed) launch_inst(L, ctmc_mixed_instances, {nt}, "ctmc_mixed", grid, blk, 0, FmCtmcMixedArgs{f, mixed->steps, mixed->active, mixed->mol_group});
    else launch_inst(L, ctmc_instances, {nt}, "ctmc", grid, blk, 0, f);
    return L.rc;
}

// The step loop of fm_integrate and fm_integrate_mixed: the endpoint predictions ping-pong between dst_a and dst_b from prev0 on, the embedding tables of a
// chunk of steps are built in one launch (`tabs` tables per step, temb: n_steps x tabs rows; tab_slot: forward_impl), every step is one evaluation and one CTMC
// step with its frame of the sink.  keep_of(i): step i's frozen rows (fm_integrate_inpaint), absent for every other caller.  step(i, prev, sc, nz, mixed) sets what differs per step (mixed.mol_group stays null for a batch at one time) and returns
// the bootstrap flag (no previous prediction and t = 0, vector_field.py:269-272); the entry points check their arguments first: a refused call enqueues nothing.
template <class StepFn>
int step_driver(fm_ctx* c, hipStream_t st, const fm_state* state, int n_steps, int tabs, const int* tab_slot, const float* temb, const fm_dst* prev0,
                const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst, StepFn step,
                const std::function<const KeepStep*(int)>& keep_of = nullptr) {
    const int tt = c->cfg.time_embedding_dim, spc = FM_TAB_SLOTS / tabs;      // steps per table launch: every table of a chunk owns a slot
    const Modality md[3] = {modality(c, 0, state), modality(c, 1, state), modality(c, 2, state)};
    const fm_dst* prev = prev0;
    int cur = (prev0 && prev0->x == dst_a->x) ? 1 : 0;
    for (int i = 0; i < n_steps; ++i) {
        const fm_dst* out = cur == 0 ? dst_a : dst_b;
        const fm_step_scalars* sc = nullptr;
        const fm_step_noise* nz = nullptr;
        MixedStep mixed{};
        const int boot = step(i, prev, sc, nz, mixed);
        // campbell steps: the COM removal of the endpoint positions runs inside the fused CTMC kernel (one launch and one copy less)
        // (so do gat steps with in-kernel noise: fm_k_ctmc_gat_fused shares the campbell kernel's position job)
        const bool defer_com = sc->dfm_type == FM_DFM_CAMPBELL || (sc->dfm_type == FM_DFM_GAT && sc->noise_mode == FM_NOISE_PHILOX);
        if (i % spc == 0) {
            const int rc0 = embed_table(c, st, temb + (size_t)i * tabs * tt, std::min(n_steps - i, spc) * tabs);
            if (rc0) return rc0;
        }
        int rc = forward_impl(c, st, state, nullptr, prev, boot, defer_com ? 2 : 1, out, (i % spc) * tabs, tab_slot);
        if (rc) return rc;
        fm_sampled smp{};
        fm_traj_sink frame{};      // step i's frames: the fused CTMC kernel writes them next to the state (no copy nodes per step)
        if (sink) {
            auto tok = [&](int32_t* p, int m) { return p ? p + (size_t)i * md[m].rows : nullptr; };
            auto pos = [&](float* p) { return p ? p + (size_t)i * md[0].rows * 3 : nullptr; };
            smp = {tok(sink->a1, 0), tok(sink->c1, 1), tok(sink->e1, 2)};
            frame.x = pos(sink->x); frame.a = tok(sink->a, 0); frame.c = tok(sink->c, 1); frame.e = tok(sink->e, 2); frame.x1 = pos(sink->x1);
        }
        const bool in_kernel = sink && defer_com;      // the fused kernels write the frames too
        rc = ctmc_impl(c, st, md, state, out, nz, sc, &smp, defer_com ? c->ws.xw : nullptr, in_kernel ? &frame : nullptr, mixed.mol_group ? &mixed : nullptr,
                       keep_of ? keep_of(i) : nullptr);
        if (rc) return rc;
        if (sink && !in_kernel) {      // tensor-noise 'gat' steps (three small kernels): frames by copy
            Launch L{c, st};
            L.copy(frame.x, state->x_t, frame.x ? (size_t)md[0].rows * 12 : 0);
            for (int m = 0; m < 3; ++m) { int32_t* f = pick3(m, frame.a, frame.c, frame.e); L.copy(f, md[m].tok, f ? (size_t)md[m].rows * 4 : 0); }
            L.copy(frame.x1, out->x, frame.x1 ? (size_t)md[0].rows * 12 : 0);
            if (L.rc) return L.rc;
        }
        prev = out;
        cur ^= 1;
    }
    if (final_dst) *final_dst = cur ^ 1;
    return FM_OK;
}

// ---------------------------------------------------------------------------------------- fm_create: validate, plan, pack by module, upload
int validate(const fm_config& cf) {
    if (cf.abi_version != FM_ABI_VERSION) return fail(nullptr, FM_ERR_INVALID, "fm_create: ABI version %d != %d", cf.abi_version, FM_ABI_VERSION);
    // The kernels' tiles are 256 scalar / 128 edge-feature columns wide.  Narrower models (configs/dev.yml: 64 / 64) run on the
    // same tiles: weights, biases and LayerNorm affine parameters are zero-padded when they are repacked, so the extra columns
    // stay exactly 0 through every Linear / SiLU / residual, and LayerNorm takes its statistics over the REAL width only.
    auto pow2 = [](int v) { return v >= 8 && (v & (v - 1)) == 0; };      // LayerNorm mean = sum * (1/n): exact division only for a power-of-two width
    if (!pow2(cf.n_hidden_scalars) || cf.n_hidden_scalars > 256 || !pow2(cf.n_hidden_edge_feats) || cf.n_hidden_edge_feats > 128 || cf.rbf_dim != 32)
        return fail(nullptr, FM_ERR_INVALID, "fm_create: need power-of-two widths 8 <= n_hidden_scalars <= 256, 8 <= n_hidden_edge_feats <= 128, and rbf_dim == 32");
    if (cf.n_vec_channels != 16 && cf.n_vec_channels != 32) return fail(nullptr, FM_ERR_INVALID, "fm_create: n_vec_channels must be 16 or 32");
    if (cf.n_convs < 1 || cf.n_convs > FM_MAX_CONVS) return fail(nullptr, FM_ERR_INVALID, "fm_create: bad n_convs");
    if (cf.n_recycles < 0 || cf.n_recycles > 64) return fail(nullptr, FM_ERR_INVALID, "fm_create: n_recycles must be 0..64");
    if (cf.msg_z == 0.f) return fail(nullptr, FM_ERR_INVALID, "fm_create: msg_z must be > 0 (divisor) or < 0 (mean over the in-edges)");
    if (cf.n_atom_types + 1 > 16 || cf.n_charges + 1 > 16 || cf.n_bond_types + 1 > 16 || cf.n_atom_types + cf.n_charges > 32)
        return fail(nullptr, FM_ERR_INVALID, "fm_create: categorical widths exceed kernel limits");
    const bool tok = cf.a_token_dim > 0;
    if (!cf.has_mask && (tok || cf.self_conditioning)) return fail(nullptr, FM_ERR_INVALID, "fm_create: endpoint-parameterised models (has_mask = 0) take raw categorical vectors (token dims 0) and no self-conditioning");
    if ((cf.c_token_dim > 0) != tok || (cf.e_token_dim > 0) != tok) return fail(nullptr, FM_ERR_INVALID, "fm_create: token dims must be all zero or all non-zero");
    const int HX = cf.v_dst_feats, SD = cf.s_dst_feats;
    if ((HX > 0) != (SD > 0) || HX < 0 || HX > 8 || SD > 256 || (HX > 0 && HX != cf.n_vec_channels / 4))
        return fail(nullptr, FM_ERR_INVALID, "fm_create: destination-feature widths must be both 0 or v = n_vec_channels/4 (<= 8), s <= 256");
    if (cf.precision != FM_PREC_F32 && cf.precision != FM_PREC_BF16X3 && cf.precision != FM_PREC_BF16X6 && cf.precision != FM_PREC_F16X3) return fail(nullptr, FM_ERR_INVALID, "fm_create: unknown precision %d", cf.precision);
    if (cf.precision != FM_PREC_F32 && HX > 0) return fail(nullptr, FM_ERR_INVALID, "fm_create: split precision is built for models without destination features");
    // launch-tuning overrides (fm_config, ABI 5; 0 = automatic everywhere): read per batch by plan_batch
    auto tile_ok = [](int t) { return t == 0 || t == 16 || t == 32 || t == 64; };
    auto rg_tile = [](int t) { return t == 4 || t == 8 || t == 12 || t == 20; };
    if (!tile_ok(cf.tile_edge) || !(tile_ok(cf.tile_node) || rg_tile(cf.tile_node)))
        return fail(nullptr, FM_ERR_INVALID, "fm_create: fm_config.tile_edge must be 0 (automatic), 16, 32 or 64; tile_node additionally 4, 8, 12 or 20");
    if (cf.ctmc_threads != 0 && cf.ctmc_threads != 256 && cf.ctmc_threads != 1024) return fail(nullptr, FM_ERR_INVALID, "fm_create: fm_config.ctmc_threads must be 0 (automatic), 256 or 1024");
    return FM_OK;
}

ModelPlan model_plan(const fm_config& cf) {
    ModelPlan m;
    const bool f32 = cf.precision == FM_PREC_F32, two_plane = prec_two_plane(cf.precision), dst = cf.v_dst_feats > 0;
    m.narrow_s = cf.n_hidden_scalars != 256;
    m.narrow_f = cf.n_hidden_edge_feats != 128;
    m.quad_mlp = !m.narrow_s && !dst && !two_plane;
    m.quad_node = m.quad_mlp && f32 && cf.fuse_node >= 0;      // the fused node sequence (BatchPlan::fuse_node) of full-width f32 models
    m.msg_planes = two_plane ? 2 : cf.precision == FM_PREC_BF16X6 ? 3 : 0;
    m.node_sp = two_plane ? (cf.precision == FM_PREC_F16X3 ? 3 : 1) : 0;
    m.half_planes = cf.precision == FM_PREC_F16X3;
    // the pair slab: self-conditioned f32 models without destination features; the slab GEMM reads [rbf | ef] rows at the pitch 164 of a 128-wide hidden tile
    if (cf.pair_slab >= 0 && !dst && f32 && cf.self_conditioning && ld_for(128) <= 164)
        m.slab_convs = cf.n_convs > 1 && cf.update_after[0] < 0 ? 2 : 1;      // the first two convolutions, unless a molecule update runs after the first
    return m;
}

// token tables, the scalar embedding, and the edge embedding: its table of the ne+1 distinct inputs (ef_tab), and for endpoint models the dense MLP
bool pack_embeddings(fm_ctx* c, Builder& B, std::vector<float>& ef_tab) {
    const fm_config& cf = c->cfg;
    const int S = c->S, F = c->F, na = c->na, nc = c->nc, ne = c->ne;
    const bool tok = cf.a_token_dim > 0;
    const int mk = cf.has_mask ? 1 : 0;       // CTMC models: one mask category per categorical input
    const int ta = tok ? cf.a_token_dim : na + mk, tc = tok ? cf.c_token_dim : nc + mk, te = tok ? cf.e_token_dim : ne + mk;
    const float* emb_e = nullptr;
    if (tok) {
        const float* ea = B.bl.get("token_embeddings.a.weight", na + 1, ta);
        const float* ec = B.bl.get("token_embeddings.c.weight", nc + 1, tc);
        emb_e = B.bl.get("token_embeddings.e.weight", ne + 1, te);
        if (!B.bl.ok()) return false;
        B.put(c->emb_a, std::vector<float>(ea, ea + (na + 1) * ta));
        B.put(c->emb_c, std::vector<float>(ec, ec + (nc + 1) * tc));
    }
    const int kin = ta + tc + cf.time_embedding_dim;
    const float* W1 = B.bl.get("scalar_embedding.0.weight", S, kin); const float* b1 = B.bl.get("scalar_embedding.0.bias", S);
    const float* W2 = B.bl.get("scalar_embedding.2.weight", S, S); const float* b2 = B.bl.get("scalar_embedding.2.bias", S);
    const float* g = B.bl.get("scalar_embedding.4.weight", S); const float* be = B.bl.get("scalar_embedding.4.bias", S);
    if (!B.bl.ok()) return false;
    B.mlp(c->node_embed, pad8(kin), 256, 256, linear(W1, S, kin), b1, S, linear(W2, S, S), b2, S);
    B.pad_vec(c->node_ln_g, g, S, 256); B.pad_vec(c->node_ln_b, be, S, 256);
    c->tab_rows = (na + 1) * (nc + 1);
    const float* eW1 = B.bl.get("edge_embedding.0.weight", F, te); const float* eb1 = B.bl.get("edge_embedding.0.bias", F);
    const float* eW2 = B.bl.get("edge_embedding.2.weight", F, F); const float* eb2 = B.bl.get("edge_embedding.2.bias", F);
    const float* eg = B.bl.get("edge_embedding.4.weight", F); const float* ebe = B.bl.get("edge_embedding.4.bias", F);
    if (!B.bl.ok()) return false;
    // edge-embedding table (ne+1 rows): the edge embedding has only ne+1 distinct inputs;
    // evaluated once here on the host in f32 (same op order as a row of the device MLP is not required: 1e-7 class)
    ef_tab.assign((size_t)(ne + 1) * 128, 0.f);
    for (int t = 0; t <= ne; ++t) {
        std::vector<float> in(te, 0.f), h1(F), h2(F);
        if (tok) for (int k = 0; k < te; ++k) in[k] = emb_e[t * te + k]; else if (t < te) in[t] = 1.f;
        for (int n = 0; n < F; ++n) { float acc = eb1[n]; for (int k = 0; k < te; ++k) acc = fmaf(eW1[n * te + k], in[k], acc); h1[n] = acc / (1.0f + expf(-acc)); }
        for (int n = 0; n < F; ++n) { float acc = eb2[n]; for (int k = 0; k < F; ++k) acc = fmaf(eW2[n * F + k], h1[k], acc); h2[n] = acc / (1.0f + expf(-acc)); }
        double mean = 0; for (float x : h2) mean += x; mean /= F;
        double var = 0; for (float x : h2) var += (x - mean) * (x - mean); var /= F;
        const float rstd = (float)(1.0 / std::sqrt(var + 1e-5));
        for (int n = 0; n < F; ++n) ef_tab[(size_t)t * 128 + n] = (h2[n] - (float)mean) * rstd * eg[n] + ebe[n];      // columns F..127 stay 0
    }
    B.put(c->ef_tab, ef_tab);
    if (!mk) {      // dense edge embedding of endpoint models: the same MLP as a device kernel over the pair rows
        B.mlp(c->edge_embed, pad8(te), 128, 128, linear(eW1, F, te), eb1, F, linear(eW2, F, F), eb2, F);
        B.pad_vec(c->edge_ln_g, eg, F, 128); B.pad_vec(c->edge_ln_b, ebe, F, 128);
    }
    return true;
}

// the self-conditioning layer's node and edge MLPs, and T1: its edge MLP's first layer applied to the edge-embedding table
bool pack_self_conditioning(fm_ctx* c, Builder& B, const std::vector<float>& ef_tab) {
    if (!c->cfg.self_conditioning) return true;
    const int S = c->S, F = c->F, na = c->na, nc = c->nc, ne = c->ne;
    const std::string p = "self_conditioning_residual_layer.";
    const int kin = S + na + nc + 32, kinp = 256 + na + nc + 32;       // reference / tile input widths: [s | p_a | p_c | rbf]
    const float* W1 = B.bl.get(p + "node_residual_mlp.0.weight", S, kin); const float* b1 = B.bl.get(p + "node_residual_mlp.0.bias", S);
    const float* W2 = B.bl.get(p + "node_residual_mlp.2.weight", S, S); const float* b2 = B.bl.get(p + "node_residual_mlp.2.bias", S);
    const int kie = F + ne + 32;
    const float* E1 = B.bl.get(p + "edge_residual_mlp.0.weight", F, kie); const float* eb1 = B.bl.get(p + "edge_residual_mlp.0.bias", F);
    const float* E2 = B.bl.get(p + "edge_residual_mlp.2.weight", F, F); const float* eb2 = B.bl.get(p + "edge_residual_mlp.2.bias", F);
    if (!B.bl.ok()) return false;
    const WFn w1 = linear(W1, S, kin, [=](int k) { return k < 256 ? (k < S ? k : -1) : S + (k - 256); }), w2 = linear(W2, S, S);
    B.mlp(c->sc_node, pad8(kinp), 256, 256, w1, b1, S, w2, b2, S);
    if (c->mp.quad_mlp) { B.put(c->sc_node_W1q, pack4(320, w1)); B.put(c->sc_node_W2q, pack4(256, w2)); }      // 4-row node tiles (fm_k_mlp4): K padded to 320
    B.mlp(c->sc_edge, pad8(ne + 32), 128, 128, linear(E1, F, kie, [=](int k) { return k < ne + 32 ? F + k : -1; }), eb1, F, linear(E2, F, F), eb2, F);
    std::vector<float> T1((size_t)(ne + 1) * 128, 0.f);
    for (int t = 0; t <= ne; ++t)
        for (int n = 0; n < F; ++n) {
            float acc = eb1[n];
            for (int k = 0; k < F; ++k) acc = fmaf(E1[(size_t)n * kie + k], ef_tab[(size_t)t * 128 + k], acc);
            T1[(size_t)t * 128 + n] = acc;
        }
    B.put(c->T1, T1);
    return true;
}

bool pack_convolution(fm_ctx* c, Builder& B, int i) {
    const ModelPlan& m = c->mp;
    const int V = c->V, S = c->S, F = c->F, HX = c->HX, SD = c->SD, PVW = c->PVW;
    const int H0 = V + 1 + HX, KU0 = pad8(H0 + 4);
    ConvW& cw = c->conv[i];
    const std::string p = "conv_layers." + std::to_string(i) + ".", k0 = p + "edge_message.0";
    const int kin0 = S + 32 + F + SD + H0 + 4;
    const float* Wh = B.bl.get(k0 + ".Wh", H0, H0);        // input vectors [x_diff | v_src (V) | v_dst_msg (HX)], hidden = max(in, out) = H0
    const float* Wcp = B.bl.get(k0 + ".Wcp", H0, 8);
    const float* Wu = B.bl.get(k0 + ".Wu", H0 + 4, V);
    const float* Ws = B.bl.get(k0 + ".to_feats_out.0.weight", S, kin0);
    const float* bs = B.bl.get(k0 + ".to_feats_out.0.bias", S);
    const float* Wg = B.bl.get(k0 + ".scalar_to_vector_gates.weight", V, S);
    const float* bg = B.bl.get(k0 + ".scalar_to_vector_gates.bias", V);
    if (!B.bl.ok()) return false;
    // hoisted per-node parts (input vector 0 is the displacement; 1.. are v_src); the quad-row projection: conv 0's in fm_k_mlp4, every conv's in the RG
    // node instances (the previous node_update projects the next conv)
    const WFn ps = linear(Ws, S, kin0, below(S));
    B.put(cw.Wps, pack(256, 256, ps));
    if (m.quad_node || (i == 0 && m.quad_mlp)) B.put(cw.Wps4, pack4(256, ps));
    if (m.node_sp) B.put(cw.Wps_sp, B.sp(256, 256, ps, 2));
    // hidden-vector row layout (FmGvpTile): [hidden (H0) | cp (4, filled by the kernel) | 0 .. KU0) | Vcp sources (8) | 0 .. PVW)
    auto hrow = [&](int vin_row, int n) -> float {
        if (n < H0) return Wh[(size_t)vin_row * H0 + n];
        if (n >= KU0 && n < KU0 + 8) return Wcp[(size_t)vin_row * 8 + (n - KU0)];
        return 0.f; };
    B.put(cw.Wpv, pack(V, PVW, [&](int k, int n) -> float { return hrow(1 + k, n); }));
    std::vector<float> w0(PVW);
    for (int n = 0; n < PVW; ++n) w0[n] = hrow(0, n);
    B.put(cw.w0, w0);
    FmGvpW& g0 = cw.msg[0];
    g0.Wv1 = nullptr;
    B.put(g0.Wu, pack(KU0, V, [&](int k, int n) -> float { return k < H0 + 4 ? Wu[k * V + n] : 0.f; }));
    // K order of the first scalar linear: [rbf(32) | ef(128 columns, F real) | sh(V+5) | 0]; reference column order
    // [s_src(S) | rbf(32) | ef(F) | sh(V+5)] (gvp.py:532-539,118)
    const WFn g0s = linear(Ws, S, kin0, [=](int k) {
        if (k < 32) return S + k;
        if (k < 160) return k - 32 < F ? S + 32 + (k - 32) : -1;
        return k < 160 + H0 + 4 ? S + 32 + F + SD + (k - 160) : -1; });
    const WFn g0g = linear(Wg, V, S, below(S));
    B.put(g0.Ws, pack(160 + KU0, 256, g0s));
    if (i < m.slab_convs) {      // pair-slab convolutions: the [rbf | ef] rows (K = 160) and the hidden-vector norm rows (K = KU0) apart
        B.put(cw.Ws_slab, pack(160, 256, g0s));
        B.put(cw.Ws_sh, pack(KU0, 256, [&](int k, int n) { return g0s(160 + k, n); }));
    }
    B.pad_vec(g0.bs, bs, S, 256);
    B.put(g0.Wg, pack(256, V, g0g));
    B.pad_vec(g0.bg, bg, V, V);
    if (m.msg_planes) { B.put(g0.Ws_sp, B.sp(160 + KU0, 256, g0s, m.msg_planes)); B.put(g0.Wg_sp, B.sp(256, V, g0g, m.msg_planes)); }
    if (HX > 0) {
        // destination-node terms of the first edge GVP, hoisted per node: vectors through [Wh | Wcp] rows V+1.., scalars through Ws columns S+32+F..
        B.put(cw.Wpvd, pack(8, PVW, [&](int k, int n) -> float { return k < HX ? hrow(V + 1 + k, n) : 0.f; }));
        B.put(cw.Wsd, pack(256, 256, linear(Ws, S, kin0, [=](int k) { return k < SD ? S + 32 + F + k : -1; })));
        // the projection GVP itself (gvp.py:304-311): V -> HX vectors, S -> SD scalars, hidden V, no cross-product features
        const std::string kp = p + "dst_feat_msg_projection";
        const float* pWh = B.bl.get(kp + ".Wh", V, V); const float* pWu = B.bl.get(kp + ".Wu", V, HX);
        const float* pWs = B.bl.get(kp + ".to_feats_out.0.weight", SD, V + S); const float* pbs = B.bl.get(kp + ".to_feats_out.0.bias", SD);
        const float* pWg = B.bl.get(kp + ".scalar_to_vector_gates.weight", HX, SD); const float* pbg = B.bl.get(kp + ".scalar_to_vector_gates.bias", HX);
        if (!B.bl.ok()) return false;
        FmGvpW& dp = cw.dproj;
        B.put(dp.Wv1, pack(V, V + 16, [&](int k, int n) -> float { return n < V ? pWh[k * V + n] : 0.f; }));         // Wcp = 0
        B.put(dp.Wu, pack(V + 8, 16, [&](int k, int n) -> float { return (k < V && n < HX) ? pWu[k * HX + n] : 0.f; }));
        B.put(dp.Ws, pack(256 + V + 8, 256, linear(pWs, SD, V + S, [=](int k) { return k < 256 ? (k < S ? k : -1) : (k < 256 + V ? S + (k - 256) : -1); })));
        B.pad_vec(dp.bs, pbs, SD, 256);
        B.put(dp.Wg, pack(256, 16, linear(pWg, HX, SD, below(SD))));
        B.pad_vec(dp.bg, pbg, HX, 16);
    }
    for (int g = 1; g < 3; ++g) if (!pack_gvp(B, p + "edge_message." + std::to_string(g), V, S, V, cw.msg[g], m.msg_planes, false)) return false;
    for (int g = 0; g < 3; ++g) if (!pack_gvp(B, p + "node_update." + std::to_string(g), V, S, V, cw.upd[g], m.node_sp ? 2 : 0, m.quad_node)) return false;
    const float* l1g = B.bl.get(p + "message_layer_norm.feat_norm.weight", S); const float* l1b = B.bl.get(p + "message_layer_norm.feat_norm.bias", S);
    const float* l2g = B.bl.get(p + "update_layer_norm.feat_norm.weight", S); const float* l2b = B.bl.get(p + "update_layer_norm.feat_norm.bias", S);
    if (!B.bl.ok()) return false;
    B.pad_vec(cw.ln1_g, l1g, S, 256); B.pad_vec(cw.ln1_b, l1b, S, 256);
    B.pad_vec(cw.ln2_g, l2g, S, 256); B.pad_vec(cw.ln2_b, l2b, S, 256);
    return true;
}

// one molecule updater: NodePositionUpdate's three GVPs and EdgeUpdate
bool pack_updater(fm_ctx* c, Builder& B, int u) {
    const ModelPlan& m = c->mp;
    const int V = c->V, S = c->S, F = c->F;
    UpdW& uw = c->upd[u];
    const std::string p = "node_position_updaters." + std::to_string(u) + ".gvps.";
    for (int g = 0; g < 3; ++g) if (!pack_gvp(B, p + std::to_string(g), V, S, g < 2 ? V : 1, uw.pos[g], m.node_sp ? 2 : 0, m.quad_node)) return false;
    const std::string q = "edge_updaters." + std::to_string(u) + ".";
    const bool with_d = !c->cfg.edge_update_no_distance;
    const int kin = 2 * S + F + (with_d ? 32 : 0);
    const float* W1 = B.bl.get(q + "edge_update_fn.0.weight", F, kin); const float* b1 = B.bl.get(q + "edge_update_fn.0.bias", F);
    const float* W2 = B.bl.get(q + "edge_update_fn.2.weight", F, F); const float* b2 = B.bl.get(q + "edge_update_fn.2.bias", F);
    const float* g = B.bl.get(q + "edge_norm.weight", F); const float* be = B.bl.get(q + "edge_norm.bias", F);
    if (!B.bl.ok()) return false;
    // input order [s_src(S) | s_dst(S) | ef(F) | d(32)] (vector_field.py:870-877); tile: Asd = [W1_src s | W1_dst s] (2 x 128 columns)
    const WFn asd = [=](int k, int n) -> float {
        const int o = n < 128 ? n : n - 128;
        if (k >= S || o >= F) return 0.f;
        return W1[(size_t)o * kin + (n < 128 ? 0 : S) + k]; };
    // without update_edge_w_distance the rbf(d) block of the tile meets zero weights
    const WFn w1 = linear(W1, F, kin, [=](int k) { return k < 128 ? (k < F ? 2 * S + k : -1) : (with_d ? 2 * S + F + (k - 128) : -1); });
    const WFn w2 = linear(W2, F, F);
    B.put(uw.Wasd, pack(256, 256, asd));
    if (m.quad_node) B.put(uw.Wasd4, pack4(256, asd));
    B.put(uw.W1, pack(160, 128, w1));
    B.pad_vec(uw.b1, b1, F, 128);
    B.put(uw.W2, pack(128, 128, w2));
    B.pad_vec(uw.b2, b2, F, 128);
    if (m.node_sp) { B.put(uw.Wasd_sp, B.sp(256, 256, asd, 2)); B.put(uw.W1_sp, B.sp(160, 128, w1, 2)); B.put(uw.W2_sp, B.sp(128, 128, w2, 2)); }
    B.pad_vec(uw.ln_g, g, F, 128); B.pad_vec(uw.ln_b, be, F, 128);
    return true;
}

bool pack_heads(fm_ctx* c, Builder& B) {
    const int S = c->S, F = c->F, na = c->na, nc = c->nc, ne = c->ne;
    const float* W1 = B.bl.get("node_output_head.0.weight", S, S); const float* b1 = B.bl.get("node_output_head.0.bias", S);
    const float* W2 = B.bl.get("node_output_head.2.weight", na + nc, S); const float* b2 = B.bl.get("node_output_head.2.bias", na + nc);
    const float* E1 = B.bl.get("to_edge_logits.0.weight", F, F); const float* eb1 = B.bl.get("to_edge_logits.0.bias", F);
    const float* E2 = B.bl.get("to_edge_logits.2.weight", ne, F); const float* eb2 = B.bl.get("to_edge_logits.2.bias", ne);
    if (!B.bl.ok()) return false;
    const WFn w1 = linear(W1, S, S), w2 = linear(W2, na + nc, S);
    B.mlp(c->node_head, 256, 256, pad16(na + nc), w1, b1, S, w2, b2, na + nc);
    if (c->mp.quad_mlp) {
        B.put(c->node_head_W1q, pack4(256, w1));
        B.put(c->node_head_W2q, pack4(256, w2, 1));      // N = 64 (na + nc <= 32 real columns): one column group, K over all eight waves
    }
    B.mlp(c->edge_head, 128, 128, 16, linear(E1, F, F), eb1, F, linear(E2, ne, F), eb2, ne);
    return true;
}

int upload(fm_ctx* c, const Builder& B) {
    c->arena_bytes = B.A.h.size() * sizeof(float);
    hipError_t e = hipMalloc((void**)&c->arena, c->arena_bytes);
    if (e != hipSuccess) { c->arena = nullptr; return fail(nullptr, FM_ERR_NOMEM, "fm_create: hipMalloc(%zu) failed: %s", c->arena_bytes, hipGetErrorString(e)); }
    e = hipMemcpy(c->arena, B.A.h.data(), c->arena_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(nullptr, FM_ERR_HIP, "fm_create: weight upload failed: %s", hipGetErrorString(e));
    for (const Fix& f : B.fix) *f.slot = c->arena + f.off * sizeof(float);
    return FM_OK;
}

}  // namespace

// ================================================================================================= C ABI
extern "C" {

const char* fm_last_error(const fm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
int fm_abi_version(void) { return FM_ABI_VERSION; }

int fm_create(const fm_config* cfg, const fm_tensor_desc* tensors, int n_tensors, const float* host_blob, fm_ctx** out) {
    if (!cfg || !tensors || !host_blob || !out) return fail(nullptr, FM_ERR_INVALID, "fm_create: null argument");
    int rc = validate(*cfg);
    if (rc) return rc;
    std::unique_ptr<fm_ctx, int (*)(fm_ctx*)> c(new fm_ctx(), fm_destroy);      // an error below releases the context as fm_destroy does
    c->cfg = *cfg;
    c->V = cfg->n_vec_channels; c->S = cfg->n_hidden_scalars; c->F = cfg->n_hidden_edge_feats;
    c->HX = cfg->v_dst_feats; c->SD = cfg->s_dst_feats; c->PVW = pvw_of(c->V, c->HX);
    c->na = cfg->n_atom_types; c->nc = cfg->n_charges; c->ne = cfg->n_bond_types;
    c->rbf_mu_step = cfg->rbf_dmax / (float)(cfg->rbf_dim - 1);
    c->rbf_inv_sigma = 1.0f / (cfg->rbf_dmax / (float)cfg->rbf_dim);
    c->mp = model_plan(*cfg);
    Builder B{{host_blob, tensors, n_tensors, {}}, c->mp};
    std::vector<float> ef_tab;
    bool ok = pack_embeddings(c.get(), B, ef_tab) && pack_self_conditioning(c.get(), B, ef_tab);
    c->conv.resize(cfg->n_convs);
    for (int i = 0; ok && i < cfg->n_convs; ++i) ok = pack_convolution(c.get(), B, i);
    c->upd.resize(cfg->n_updaters);
    for (int u = 0; ok && u < cfg->n_updaters; ++u)       // only the updaters the schedule uses (index 0 is dead when convs_per_update == 1)
        if (std::count(cfg->update_after, cfg->update_after + cfg->n_convs, u)) ok = pack_updater(c.get(), B, u);
    if (!ok || !pack_heads(c.get(), B)) return fail(nullptr, FM_ERR_WEIGHTS, "fm_create: %s", B.bl.err.c_str());
    if ((rc = upload(c.get(), B))) return rc;
    {
        int dev = 0; hipDeviceProp_t prop{};
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            c->n_cus = prop.multiProcessorCount;
    }
    // ---- dynamic LDS opt-in (up to 160 KiB per workgroup on gfx950): every instance list of the library
    fm_opt_in_msg_v32(); fm_opt_in_msg_v16(); fm_opt_in_node();      // the heavy families, in their own translation units
    opt_in(mlp_instances); opt_in(mlp_pair_instances); opt_in(mlp4_instances); opt_in(mlp4_pair_instances);
    opt_in(node_proj_instances); opt_in(edge_update_instances); opt_in(edge_update_sp_instances);
    *out = c.release();
    return FM_OK;
}

int fm_destroy(fm_ctx* c) {
    if (!c) return FM_OK;
    for (auto& pe : c->prof_events) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto& e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->arena) (void)hipFree(c->arena);
    if (c->stage_ev) { (void)hipEventSynchronize(c->stage_ev); (void)hipEventDestroy(c->stage_ev); }
    if (c->stage) (void)hipHostFree(c->stage);
    delete c;
    return FM_OK;
}

// ---------------------------------------------------------------------------------------- batch plan
// Every launch choice that depends on the batch, made here only, from the model's ModelPlan (which instances have their weights), its fm_config overrides
// (0 = automatic), the CU count and the molecule sizes: the workspace is laid out for the plan, fm_batch_bind keeps it in the context, evaluate / ctmc_impl read it.
static int plan_batch(fm_ctx* c, const int32_t* n_atoms, int B, BatchPlan& p) {
    if (B <= 0) return fail(c, FM_ERR_INVALID, "batch of %d molecules", B);
    long long N = 0, E = 0;
    int nmax = 0;
    for (int i = 0; i < B; ++i) {
        const int n = n_atoms[i];
        if (n < 1) return fail(c, FM_ERR_INVALID, "molecule %d has %d atoms", i, n);      // a 1-atom molecule has no edges: its node rows simply receive no messages
        N += n; E += (long long)n * (n - 1); nmax = n > nmax ? n : nmax;
    }
    if (E > 0x7fffffffLL / 4) return fail(c, FM_ERR_INVALID, "batch too large for int32 edge indexing (%lld edges)", E);
    // per-node tables (Ps, Asd: 1 KiB rows) are gathered through buffer descriptors with 31-bit byte offsets
    if (N > 0x7fffffffLL / 1024) return fail(c, FM_ERR_INVALID, "batch too large: %lld nodes (limit %lld per bind; split the batch)", N, 0x7fffffffLL / 1024);
    const fm_config& cf = c->cfg;
    const int n_cus = c->n_cus;
    const ModelPlan& m = c->mp;
    p = BatchPlan{};
    p.B = B; p.N = (int)N; p.E = (int)E; p.U = (int)(E / 2); p.nmax = nmax;
    const int U = p.U;
    p.P = nmax > 1 ? (nmax - 2) / FM_CHUNK_E + 2 : 1;      // chunks of FM_CHUNK_E rows a destination's n - 1 in-edges can touch
    // Edge-message tiles.  The kernel is bound by a CU's matrix pipe, so a launch takes (tiles per CU, rounded up) rounds of one tile time plus the
    // first tile's latency: measured on the MI355X (flowmol3 model, 1 .. 64 molecules x 47 atoms, profiles/r06t_*, r06u_*) 11 + 18 r16 us with 16-row tiles and
    // 13.5 + 31 r32 us with 32-row tiles, r = ceil(tiles / CUs) -- 32-row tiles do 16 rows in 15.5 instead of 18 us, 16-row tiles quantise in half the step.  The
    // cheaper of the two by that model (one molecule: 16 rows; 4, 5, 8, 9 molecules: 16; everything from 14 molecules on: 32).  Both give the same bits (canonical
    // arithmetic), so the choice is free to follow the batch size.  fm_config.tile_edge (16 | 32 | 64) forces a height.
    {
        long long t16 = 0, t32 = 0;
        for (int i = 0; i < B; ++i) { const long long e = (long long)n_atoms[i] * (n_atoms[i] - 1); t16 += (e + 15) / 16; t32 += (e + 31) / 32; }
        const long long r16 = (t16 + n_cus - 1) / n_cus, r32 = (t32 + n_cus - 1) / n_cus;
        p.tm_edge = cf.tile_edge ? cf.tile_edge : (36 * r16 + 22 < 62 * r32 + 27 ? 16 : 32);
    }
    if ((c->HX || !cf.has_mask) && (p.tm_edge > 32)) p.tm_edge = 32;
    long long nt = 0;
    for (int i = 0; i < B; ++i) nt += ((long long)n_atoms[i] * (n_atoms[i] - 1) + p.tm_edge - 1) / p.tm_edge;      // every molecule starts a tile
    p.n_tiles_msg = (int)nt;
    p.xcd_swizzle = cf.xcd_swizzle >= 0;      // fm_config.xcd_swizzle = -1 disables
    // fm_config.fuse_node = -1 keeps round 1's launch sequence: node_proj / pos_update / node_proj_asd as kernels of their own (0 / 1 = fused);
    // destination-feature models keep the unfused node sequence (their projection GVP reuses the tile)
    p.fuse_node = cf.fuse_node >= 0 && c->HX == 0;
    // node tiles: 32 rows once the chip is full, 16 while 32-row tiles would leave CUs idle -- and, for full-width f32 models on the fused node
    // sequence, tiles of 4 / 8 / 12 nodes in the 16-row frame or 20 nodes in the 32-row frame (RG instances of fm_k_node_update) whenever such
    // tiles fit ONE per CU: the node kernel is a serial chain per tile whose scalar GEMMs scale with the tile height, so the smallest tile that
    // still gives every tile a CU of its own is the fastest (beyond one tile per CU the small tiles lose: each streams the full weights).
    // fm_config.tile_node (16 | 32 | 64, or 4 / 8 / 12 / 20 nodes) forces a size.
    int tn = cf.tile_node;
    if (!tn) {
        tn = (N + 31) / 32 <= n_cus ? 16 : 32;
        if (m.quad_node) {      // the 4 RG-node instances keep the regular tiles' summation order (fm_wave_gemm4): the choice may follow the batch size in canonical mode
            static const int cand[] = {4, 8, 12, 16, 20};
            for (int r : cand) if ((N + r - 1) / r <= n_cus) { tn = r; break; }
        }
    }
    if (tn == 4 || tn == 8 || tn == 12 || tn == 20) {
        if (m.quad_node) p.node_rg = tn / 4;
        tn = tn == 20 ? 32 : 16;          // models the instances do not exist for take the frame's regular tile
    }
    p.tm_node = tn;
    if ((c->HX || !cf.has_mask) && (p.tm_node > 32)) p.tm_node = 32;
    // split-precision node kernel: the fused sequence of the two-plane modes, 16- / 32-row tiles
    p.node_sp = p.fuse_node && p.tm_node <= 32 ? m.node_sp : 0;
    // EdgeUpdate: fm_config.tile_edge_update = 64 selects 64-row tiles for full-width f32 models (the narrow and split-precision instances are 32 rows)
    p.tm_eupd = cf.tile_edge_update == 64 && !m.narrow_f && !m.node_sp ? 64 : 32;
    // the edge head as the epilogue of the last EdgeUpdate (fm_config.fuse_node = 2 | -1: separate): the tile's pair rows are gathered with 31-bit offsets
    // inside ONE molecule's edge rows (n < 2048 atoms); larger: separate head
    p.fuse_head = (cf.fuse_node == 0 || cf.fuse_node == 1) && !m.narrow_f && p.tm_eupd == 32 && !m.node_sp
                  && (long long)nmax * (nmax - 1) * 512 < 0x7ffffe00LL;
    // Pair-slab convolutions: the convolutions that run before any molecule update see pair-symmetric edge features and distances (self-conditioned f32
    // models; fm_config.pair_slab = -1: none).  The hoist is on for batches with at least four rounds of 32-row pair tiles (measured neutral below: the
    // table costs a kernel phase, the saving is matrix-pipe time small batches are not bound by), when fm_config.pair_slab = 1 forces it, or in canonical
    // mode.  fm_config.canonical >= 0 (default): the ONE launch choice that selects another f32 summation order -- the pair slab (slab + K = 40 chain
    // instead of one K = 200 chain) -- is FIXED: computed in every evaluation that can use it, so that a molecule's result does not depend on the size or
    // composition of its batch (see FM_CHUNK_E in fm_kernels.h for the aggregation order).  Tile heights -- incl. the 4 RG-node instances and the 4-row node
    // MLPs, whose GEMMs keep the regular tiles' order since round 6 (fm_wave_gemm4) -- follow the batch size in both modes.  -1: the pair slab follows the
    // batch size too (round 5's rule).  The Q tables (U KB each) exist in the workspace only when the batch uses them.
    // The pair-slab instance gathers a tile's Q rows with 31-bit byte offsets (pair - the tile's smallest pair) * 1024 inside ONE molecule's pairs: like the
    // fused edge head above that holds for n < 2049 atoms; a batch with a larger molecule runs the full instance on every convolution (forced or canonical alike).
    const bool pq_fits = (long long)nmax * (nmax - 1) * 512 < 0x7ffffe00LL;
    if (U > 0 && pq_fits && (cf.pair_slab > 0 || cf.canonical >= 0 || (U + 31) / 32 >= 16LL * n_cus)) p.n_pq = m.slab_convs;      // ModelPlan::slab_convs: which models
    // Node- and pair-side MLPs with the same inputs share one launch while the batch is small (launch_mlp_stage); fm_config.pair_mlps = 1 | -1 forces either
    const int mlp_tiles = (p.N + FM_TM - 1) / FM_TM + (U + FM_TM - 1) / FM_TM;
    p.pair_mlps = cf.fuse_node >= 0 && (cf.pair_mlps ? cf.pair_mlps > 0 : mlp_tiles <= n_cus);
    // 16-row MLP tiles while even those do not fill the chip (4 per CU fit in LDS): a tile's two dependent GEMMs are matrix-pipe time on one CU,
    // so a quarter of the rows is a quarter of the latency (fm_config.mlp_small_tiles = 1 | -1 forces either, 0 = this rule)
    p.small_node = cf.mlp_small_tiles ? cf.mlp_small_tiles > 0 : (p.N + 15) / 16 <= 4 * n_cus;      // decided per side: the node side
    p.small_pair = cf.mlp_small_tiles ? cf.mlp_small_tiles > 0 : (U + 15) / 16 <= 4 * n_cus;        // stays small ~25x longer than the pair side
    // node-side MLPs on 4-row tiles (fm_k_mlp4) while such tiles fit one per CU: a 16-row tile's two 256-wide layers are ~7 us of matrix time on one CU
    // whatever the batch, four rows on v_mfma_f32_4x4x1 are the layers' weight stream; fm_config.mlp_small_tiles = 2 forces it (1 / -1: never).  The regular
    // tiles' bits (fm_rows4_linear): the choice may follow the batch size in canonical mode
    p.mlp4 = m.quad_mlp && (cf.mlp_small_tiles ? cf.mlp_small_tiles == 2 : (p.N + 3) / 4 <= n_cus);
    // large batches: a separate edge head is a gather of two 512-byte rows per pair in front of 17 k MAC -- latency / HBM work; 32-row tiles (34 KB of LDS)
    // put four workgroups on a CU instead of two
    p.edge_head32 = (U + 31) / 32 >= 16 * n_cus;
    // CTMC: a few molecules: 1024-thread workgroups (one per molecule and modality is all the parallelism there is) -- and batches whose LARGEST molecule has
    // more than 4096 pairs (n >= 92): its pair rows are one workgroup's serial loop, 35 rounds of 256 threads at 134 atoms (GEOM size distribution: 135 us of a
    // 67.8-ms step against 39 us at 1024 x 47 atoms); else 256.  Same arithmetic either way (integer counts, per-row decisions).
    // The fused gat kernel (fm_k_ctmc_gat_fused) has the same shape -- one workgroup per (molecule, modality), a serial loop over its rows -- and takes the
    // same choice.  fm_config.ctmc_threads (256 | 1024) forces a size.
    p.ctmc_threads = cf.ctmc_threads ? cf.ctmc_threads : (B * 4 <= n_cus && nmax > 23) || nmax >= 92 ? 1024 : 256;
    return FM_OK;
}

// ---------------------------------------------------------------------------------------- workspace
// The ONE list of the workspace's regions, in layout order, every region on a 256-byte boundary: "this pointer gets so many bytes".  Sets the pointers of `w`
// from `base` (all null from a null base: fm_workspace_bytes) and returns the bytes the workspace needs; INTEGRATION.md ("Workspace size") states the sum.
static size_t ws_carve(const fm_ctx* c, const BatchPlan& p, char* base, Workspace& w) {
    const size_t B = p.B, N = p.N, E = p.E, U = p.U, V = c->V, PVW = c->PVW;
    size_t o = 0;
    auto take = [&](auto*& ptr, size_t bytes) {
        ptr = base ? reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + o) : nullptr;
        o = align_up(o + bytes, 256);
    };
    take(w.b.mol_tile_off, (B + 1) * 4); take(w.b.tile_desc, (size_t)p.n_tiles_msg * 16);
    take(w.b.mol_node_off, (B + 1) * 4); take(w.b.mol_edge_off, (B + 1) * 4); take(w.b.mol_pair_off, (B + 1) * 4);
    take(w.b.node_mol, N * 4); take(w.b.node_first_edge, N * 4);
    take(w.b.e_src, E * 4); take(w.b.e_dst, E * 4); take(w.b.e_pair, E * 4);
    take(w.b.p_e0, U * 4); take(w.b.p_e1, U * 4); take(w.b.pair_mol, U * 4);
    take(w.s, N * 256 * 4); take(w.v, N * 3 * V * 4); take(w.xw, N * 3 * 4);
    take(w.ef, E * 128 * 4);
    take(w.Ps, N * 256 * 4); take(w.Asd, N * 256 * 4); take(w.PV, N * 3 * PVW * 4);
    take(w.Psd, c->HX ? N * 256 * 4 : 0); take(w.PVd, c->HX ? N * 3 * PVW * 4 : 0);
    take(w.part_s, N * p.P * 256 * 4); take(w.part_v, N * p.P * 3 * V * 4);
    take(w.s_tab_base, align_up(c->tab_rows, FM_TM) * 256 * 4 * FM_TAB_SLOTS);
    take(w.boot.x, N * 3 * 4); take(w.boot.a, N * c->na * 4); take(w.boot.c, N * c->nc * 4); take(w.boot.e, U * c->ne * 4);
    take(w.tap_s, N * 256 * 4); take(w.tap_v, N * 3 * V * 4);
    take(w.mol_gid, B * 4);
    take(w.x1[0], N * 4); take(w.x1[1], N * 4); take(w.x1[2], U * 4);
    // the pair-slab tables are as large as `ef` each: only batches that use them pay for them (8192 x 47 atoms: 13.3 GB without, 31.5 GB with)
    take(w.Q[0], p.n_pq > 0 ? U * 256 * 4 : 0); take(w.Q[1], p.n_pq > 1 ? U * 256 * 4 : 0);
    return o;
}

int fm_workspace_bytes(fm_ctx* c, const int32_t* n_atoms, int B, size_t* bytes) {
    if (!c || !n_atoms || !bytes) return fail(c, FM_ERR_INVALID, "fm_workspace_bytes: null argument");
    BatchPlan p;
    const int rc = plan_batch(c, n_atoms, B, p);
    if (rc) return rc;
    Workspace scratch;
    *bytes = ws_carve(c, p, nullptr, scratch);
    return FM_OK;
}

// Pinned staging for `n_ints` int32 about to be copied to the device on a stream: waits (host-side) only for the copies of the PREVIOUS
// use of the staging buffer, never for the stream.
static int stage_acquire(fm_ctx* c, hipStream_t st, size_t n_ints) {
    {   // setup calls wait on an event and (re)allocate pinned memory: both are illegal while the stream is being captured
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(c, FM_ERR_STATE, "fm_batch_bind / fm_set_molecule_ids are setup calls and must stay outside a stream capture");
    }
    if (!c->stage_ev) FM_HIP(c, hipEventCreateWithFlags(&c->stage_ev, hipEventDisableTiming));
    if (c->stage_busy) { FM_HIP(c, hipEventSynchronize(c->stage_ev)); c->stage_busy = false; }
    if (c->stage_cap < n_ints) {
        if (c->stage) { FM_HIP(c, hipHostFree(c->stage)); c->stage = nullptr; c->stage_cap = 0; }
        const size_t cap = n_ints < 4096 ? 4096 : n_ints + n_ints / 2;
        FM_HIP(c, hipHostMalloc((void**)&c->stage, cap * sizeof(int32_t), hipHostMallocDefault));
        c->stage_cap = cap;
    }
    return FM_OK;
}

static int stage_release(fm_ctx* c, hipStream_t st) {
    FM_HIP(c, hipEventRecord(c->stage_ev, st));
    c->stage_busy = true;
    return FM_OK;
}

int fm_batch_bind(fm_ctx* c, void* stream, const int32_t* n_atoms, int B, void* workspace, size_t bytes) {
    if (!c || !n_atoms || !workspace) return fail(c, FM_ERR_INVALID, "fm_batch_bind: null argument");
    BatchPlan p;
    int rc = plan_batch(c, n_atoms, B, p);
    if (rc) return rc;
    Workspace w;
    const size_t need = ws_carve(c, p, (char*)workspace, w);
    if (bytes < need) return fail(c, FM_ERR_INVALID, "fm_batch_bind: workspace of %zu bytes < required %zu", bytes, need);
    if ((uintptr_t)workspace % 256) return fail(c, FM_ERR_INVALID, "fm_batch_bind: workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    FmBatch& b = w.b;
    b.B = B; b.N = p.N; b.E = p.E; b.U = p.U; b.P = p.P;
    b.n_tiles = p.n_tiles_msg; b.tile_rows = p.tm_edge;
    const size_t B1 = (size_t)B + 1;
    rc = stage_acquire(c, st, 4 * B1 + (size_t)B);
    if (rc) return rc;
    int32_t* no = c->stage; int32_t* eo = no + B1; int32_t* po = eo + B1; int32_t* to = po + B1; int32_t* ids = to + B1;
    no[0] = eo[0] = po[0] = to[0] = 0;
    for (int i = 0; i < B; ++i) {
        const int n = n_atoms[i];
        no[i + 1] = no[i] + n; eo[i + 1] = eo[i] + n * (n - 1); po[i + 1] = po[i] + n * (n - 1) / 2; ids[i] = i;
        to[i + 1] = to[i] + (n * (n - 1) + p.tm_edge - 1) / p.tm_edge;
    }
    {   // a copy that fails after earlier ones were enqueued must not leave the staging buffer unguarded: the event is recorded either way
        const struct { const int* dst; const int32_t* src; size_t n; } copies[] = {
            {b.mol_node_off, no, B1}, {b.mol_edge_off, eo, B1}, {b.mol_pair_off, po, B1}, {b.mol_tile_off, to, B1}, {w.mol_gid, ids, (size_t)B}};
        hipError_t e_ = hipSuccess;
        for (const auto& k : copies) if (e_ == hipSuccess) e_ = hipMemcpyAsync(const_cast<int*>(k.dst), k.src, k.n * 4, hipMemcpyHostToDevice, st);
        rc = stage_release(c, st);
        if (e_ != hipSuccess) return fail(c, FM_ERR_HIP, "fm_batch_bind: descriptor copy failed: %s", hipGetErrorString(e_));
        if (rc) return rc;
    }
    c->ws = w;
    c->node_off_h.assign(no, no + B1);
    c->s_tab = w.s_tab_base;
    c->tab_slot_floats = (size_t)align_up(c->tab_rows, FM_TM) * 256;
    Launch L{c, st};
    const int work = p.E > p.N ? p.E : p.N;
    L("batch_setup", fm_k_batch_setup, dim3((work + 255) / 256), dim3(256), 0, b);
    if (L.rc) return L.rc;
    c->bound = true; c->plan = p;
    return FM_OK;
}

int fm_remove_com(fm_ctx* c, void* stream, float* x) {
    if (const int rc = bound_check(c, "fm_remove_com", x)) return rc;
    Launch L{c, (hipStream_t)stream};
    L("remove_com", fm_k_remove_com, dim3(c->ws.b.B), dim3(64), 0, x, (const int*)c->ws.b.mol_node_off);
    return L.rc;
}

int fm_set_molecule_ids(fm_ctx* c, void* stream, const int32_t* ids_host) {
    if (!c) return fail(c, FM_ERR_INVALID, "fm_set_molecule_ids: null context");
    if (!c->bound) return fail(c, FM_ERR_STATE, "fm_set_molecule_ids: no batch bound");
    int rc = stage_acquire(c, (hipStream_t)stream, (size_t)c->ws.b.B);
    if (rc) return rc;
    for (int i = 0; i < c->ws.b.B; ++i) c->stage[i] = ids_host ? ids_host[i] : i;
    const hipError_t e_ = hipMemcpyAsync(c->ws.mol_gid, c->stage, (size_t)c->ws.b.B * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
    rc = stage_release(c, (hipStream_t)stream);
    if (e_ != hipSuccess) return fail(c, FM_ERR_HIP, "fm_set_molecule_ids: copy failed: %s", hipGetErrorString(e_));
    return rc;
}

int fm_prior_philox(fm_ctx* c, void* stream, uint64_t seed, float* x0) {
    if (const int rc = bound_check(c, "fm_prior_philox", x0)) return rc;
    Launch L{c, (hipStream_t)stream};
    L("prior_philox", fm_k_prior_philox, dim3(c->ws.b.B), dim3(64), 0, x0, (const int*)c->ws.b.mol_node_off, (const int*)c->ws.mol_gid,
      (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32));
    return L.rc;
}

int fm_prior_philox_dense(fm_ctx* c, void* stream, uint64_t seed, const fm_prior_spec* spec, const fm_dense_state* out) {
    if (const int rc = bound_check(c, "fm_prior_philox_dense", spec && out && out->x_t && out->a_t && out->c_t && out->e_t)) return rc;
    if (c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "fm_prior_philox_dense: this is a CTMC model (masked prior): use fm_prior_philox");
    const FmBatch& b = c->ws.b;
    FmPriorDenseArgs a{};
    static const char* const tag[3] = {"a", "c", "e"};
    for (int m = 0; m < 3; ++m) {
        const fm_prior_mod& s = spec->mod[m];
        const int d = modality(c, m).K;
        if (s.kind < FM_PRIOR_GAUSSIAN || s.kind > FM_PRIOR_C_GIVEN_A) return fail(c, FM_ERR_INVALID, "fm_prior_philox_dense: unknown prior kind %d for modality %s", s.kind, tag[m]);
        if (s.kind == FM_PRIOR_C_GIVEN_A && m != 1) return fail(c, FM_ERR_INVALID, "fm_prior_philox_dense: the c-given-a prior is for modality c, not %s", tag[m]);
        if ((s.kind == FM_PRIOR_MARGINAL || s.kind == FM_PRIOR_C_GIVEN_A) && !s.p) return fail(c, FM_ERR_INVALID, "fm_prior_philox_dense: modality %s needs its distribution p", tag[m]);
        if (s.kind == FM_PRIOR_BIASED_SIMPLEX && (d < 2 || s.vertex_idx < 0 || s.vertex_idx >= d)) return fail(c, FM_ERR_INVALID, "fm_prior_philox_dense: biased-simplex vertex_idx %d outside the %d categories of %s", s.vertex_idx, d, tag[m]);
        FmPriorMod& k = a.mod[m];
        k.kind = s.kind; k.d = d; k.std = s.std; k.simplex_center = s.simplex_center; k.blur = s.blur; k.has_blur = s.has_blur;
        k.vertex_prob = s.vertex_prob; k.vertex_idx = s.vertex_idx; k.p = s.p; k.out = pick3(m, out->a_t, out->c_t, out->e_t); k.off = modality(c, m).off;
    }
    a.x = out->x_t; a.node_off = b.mol_node_off; a.mol_gid = c->ws.mol_gid;
    a.seed_lo = (unsigned)(seed & 0xffffffffu); a.seed_hi = (unsigned)(seed >> 32);
    Launch L{c, (hipStream_t)stream};
    L("prior_philox_dense", fm_k_prior_philox_dense, dim3(b.B, 4), dim3(256), 0, a);
    return L.rc;
}

int fm_philox_tape(fm_ctx* c, void* stream, const fm_step_scalars* sc, const fm_step_noise* out) {
    if (const int rc = bound_check(c, "fm_philox_tape", sc && out && out->q_a && out->q_c && out->q_e)) return rc;
    if (sc->noise_mode != FM_NOISE_PHILOX) return fail(c, FM_ERR_INVALID, "fm_philox_tape: the step's noise_mode is not FM_NOISE_PHILOX");
    if (sc->dfm_type != FM_DFM_CAMPBELL && sc->dfm_type != FM_DFM_GAT) return fail(c, FM_ERR_INVALID, "fm_philox_tape: unknown dfm_type %d", sc->dfm_type);
    FmTapeArgs a{};
    auto w = [](const float* p) { return const_cast<float*>(p); };      // caller-owned output tensors travelling in the (read-only) noise struct
    for (int m = 0; m < 3; ++m)
        a.mod[m] = {modality(c, m).K, modality(c, m).off, w(pick3(m, out->q_a, out->q_c, out->q_e)), w(pick3(m, out->u1_a, out->u1_c, out->u1_e)), w(pick3(m, out->u2_a, out->u2_c, out->u2_e))};
    a.gat = sc->dfm_type == FM_DFM_GAT; a.seed_lo = sc->philox_seed_lo; a.seed_hi = sc->philox_seed_hi; a.step = sc->step_index; a.mol_gid = c->ws.mol_gid;
    Launch L{c, (hipStream_t)stream};
    L("philox_tape", fm_k_philox_tape, dim3(c->ws.b.B, 3), dim3(256), 0, a);
    return L.rc;
}

// fm_conditional_path (x0_in = nullptr: the prior is drawn) and fm_conditional_path_x0 (the caller's prior): one kernel, one set of refusals
static int conditional_path(fm_ctx* c, const char* fn, void* stream, uint64_t seed, const fm_state* x1, int n_groups, const int32_t* mol_group, const float* alpha,
                            const fm_state* out, const fm_cond_tape* tape, const float* x0_in) {
    if (const int rc = bound_check(c, fn, x1 && alpha && out)) return rc;
    if (!c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "%s: endpoint models (has_mask = 0) have no masked conditional path", fn);
    if (n_groups < 1) return fail(c, FM_ERR_INVALID, "%s: n_groups = %d, need at least 1", fn, n_groups);
    if (n_groups > 1 && !mol_group) return fail(c, FM_ERR_INVALID, "%s: mol_group is NULL with n_groups = %d", fn, n_groups);
    const FmBatch& b = c->ws.b;
    if (!x1->x_t || !out->x_t) return fail(c, FM_ERR_INVALID, "%s: null argument", fn);
    if (out->x_t == x1->x_t) return fail(c, FM_ERR_INVALID, "%s: out->x_t aliases x1->x_t (the call is not in-place)", fn);
    if (x0_in && (x0_in == out->x_t || (tape && x0_in == tape->x0))) return fail(c, FM_ERR_INVALID, "%s: x0_in aliases out->x_t or tape->x0", fn);
    FmCondArgs a{};
    static const char* const tag[3] = {"a_t", "c_t", "e_t"};
    for (int m = 0; m < 3; ++m) {
        const Modality md = modality(c, m);
        const int32_t* const t1 = pick3(m, x1->a_t, x1->c_t, x1->e_t);
        int32_t* const to = pick3(m, out->a_t, out->c_t, out->e_t);
        if (md.rows > 0 && (!t1 || !to)) return fail(c, FM_ERR_INVALID, "%s: null argument", fn);
        if (to && to == t1) return fail(c, FM_ERR_INVALID, "%s: out->%s aliases x1->%s (the call is not in-place)", fn, tag[m], tag[m]);
        a.mod[m] = {md.K, t1, to, tape ? pick3(m, tape->u_a, tape->u_c, tape->u_e) : nullptr, md.off};
    }
    a.x1 = x1->x_t; a.x_t = out->x_t; a.x0 = tape ? tape->x0 : nullptr; a.node_off = b.mol_node_off;
    a.mol_gid = c->ws.mol_gid; a.mol_group = n_groups > 1 ? mol_group : nullptr; a.alpha = alpha;
    a.seed_lo = (unsigned)(seed & 0xffffffffu); a.seed_hi = (unsigned)(seed >> 32);
    a.x0_in = x0_in;
    Launch L{c, (hipStream_t)stream};
    L("conditional_path", fm_k_conditional_path, dim3(b.B, 4), dim3(256), 0, a);
    return L.rc;
}

int fm_conditional_path(fm_ctx* c, void* stream, uint64_t seed, const fm_state* x1, int n_groups, const int32_t* mol_group, const float* alpha,
                        const fm_state* out, const fm_cond_tape* tape) {
    return conditional_path(c, "fm_conditional_path", stream, seed, x1, n_groups, mol_group, alpha, out, tape, nullptr);
}

int fm_conditional_path_x0(fm_ctx* c, void* stream, uint64_t seed, const fm_state* x1, int n_groups, const int32_t* mol_group, const float* alpha,
                           const fm_state* out, const fm_cond_tape* tape, const float* x0_in) {
    return conditional_path(c, "fm_conditional_path_x0", stream, seed, x1, n_groups, mol_group, alpha, out, tape, x0_in);
}

int fm_forward(fm_ctx* c, void* stream, const fm_state* state, const float* temb, const fm_dst* prev, int bootstrap, int remove_com,
               const fm_dst* out) {
    if (const int rc = bound_check(c, "fm_forward", state && temb && out)) return rc;
    if (!c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "fm_forward: endpoint-parameterised model (continuous inputs): use fm_forward_dense");
    return forward_impl(c, (hipStream_t)stream, state, temb, prev, bootstrap, remove_com ? 1 : 0, out);
}

int fm_forward_dense(fm_ctx* c, void* stream, const fm_dense_state* state, const float* temb, int remove_com, const fm_dst* out) {
    if (const int rc = bound_check(c, "fm_forward_dense", state && temb && out)) return rc;
    if (c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "fm_forward_dense: this is a CTMC model (token inputs): use fm_forward");
    return evaluate(c, (hipStream_t)stream, nullptr, nullptr, remove_com ? 1 : 0, out, true, state, temb);
}

int fm_endpoint_step(fm_ctx* c, void* stream, const fm_dense_state* state, const fm_dst* dst, const fm_endpoint_scalars* sc) {
    if (const int rc = bound_check(c, "fm_endpoint_step", state && dst && sc)) return rc;
    const FmBatch& b = c->ws.b;
    FmEndpointStepArgs a{};
    float* xt[4] = {state->x_t, state->a_t, state->c_t, state->e_t};
    const float* x1[4] = {dst->x, dst->a, dst->c, dst->e};
    const int n[4] = {b.N * 3, b.N * c->na, b.N * c->nc, b.U * c->ne};
    int nmax = 0;
    for (int f = 0; f < 4; ++f) { a.xt[f] = xt[f]; a.x1[f] = x1[f]; a.n[f] = n[f]; a.coef[f] = sc->coef[f]; nmax = std::max(nmax, n[f]); }
    a.scale = sc->scale; a.dt = sc->dt;
    Launch L{c, (hipStream_t)stream};
    L("endpoint_step", fm_k_endpoint_step, dim3(std::min(4096, (nmax + 255) / 256), 4), dim3(256), 0, a);
    return L.rc;
}

int fm_ctmc_step(fm_ctx* c, void* stream, const fm_state* state, const fm_dst* dst, const fm_step_noise* noise, const fm_step_scalars* sc,
                 const fm_sampled* sampled) {
    if (const int rc = bound_check(c, "fm_ctmc_step", state && dst && sc)) return rc;
    const Modality md[3] = {modality(c, 0, state), modality(c, 1, state), modality(c, 2, state)};
    return ctmc_impl(c, (hipStream_t)stream, md, state, dst, noise, sc, sampled);
}

int fm_integrate(fm_ctx* c, void* stream, const fm_state* state, int n_steps, const fm_step_scalars* steps, const float* temb,
                 const fm_step_noise* noise, const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink,
                 int* final_dst) {
    if (const int rc = bound_check(c, "fm_integrate", state && steps && temb && dst_a && dst_b)) return rc;
    return step_driver(c, (hipStream_t)stream, state, n_steps, 1, nullptr, temb, prev0, dst_a, dst_b, sink, final_dst,
                       [&](int i, const fm_dst* prev, const fm_step_scalars*& sc, const fm_step_noise*& nz, MixedStep&) {
        sc = &steps[i]; nz = noise ? &noise[i] : nullptr;
        return !prev && steps[i].t == 0.0f ? 1 : 0; });
}

// what both per-molecule-time entry points refuse: bound_check's, and the model families whose time does not enter through the embedding table alone
static int mixed_check(fm_ctx* c, const char* fn, bool args_ok, int n_groups) {
    if (const int rc = bound_check(c, fn, args_ok)) return rc;
    if (!c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "%s: endpoint models (has_mask = 0) are not supported with per-molecule time", fn);
    if (n_groups < 1 || n_groups > FM_TAB_SLOTS) return fail(c, FM_ERR_INVALID, "%s: n_groups = %d outside 1..%d (FM_TAB_SLOTS embedding tables per bound batch)", fn, n_groups, FM_TAB_SLOTS);
    return FM_OK;
}

int fm_forward_mixed(fm_ctx* c, void* stream, const fm_state* state, const float* temb, int n_groups, const int32_t* mol_group, const fm_dst* prev,
                     int bootstrap, int remove_com, const fm_dst* out) {
    if (const int rc = mixed_check(c, "fm_forward_mixed", state && temb && mol_group && out, n_groups)) return rc;
    return forward_impl(c, (hipStream_t)stream, state, temb, prev, bootstrap, remove_com ? 1 : 0, out, -1, mol_group, n_groups);
}

int fm_denoising_loss(fm_ctx* c, void* stream, const fm_state* xt, const fm_state* x1, const float* temb, int n_groups, const int32_t* mol_group,
                      const fm_loss_rows* rows, float* mol_out) {
    const char* const fn = "fm_denoising_loss";
    if (const int rc = bound_check(c, fn, xt && x1 && rows && mol_out)) return rc;
    if (!c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "%s: endpoint models (has_mask = 0) are not supported: the loss of the masked (CTMC) parameterisation only", fn);
    if (n_groups < 1 || n_groups > FM_TAB_SLOTS) return fail(c, FM_ERR_INVALID, "%s: n_groups = %d outside 1..%d (FM_TAB_SLOTS embedding tables per bound batch)", fn, n_groups, FM_TAB_SLOTS);
    if (n_groups > 1 && !mol_group) return fail(c, FM_ERR_INVALID, "%s: mol_group is NULL with n_groups = %d", fn, n_groups);
    if (!rows->x || !rows->a || !rows->c || !rows->e) return fail(c, FM_ERR_INVALID, "%s: rows->%s is NULL (all four row buffers are required)", fn,
                                                                  !rows->x ? "x" : !rows->a ? "a" : !rows->c ? "c" : "e");
    const FmBatch& b = c->ws.b;
    if (!xt->x_t || !xt->a_t || !xt->c_t || !x1->x_t || !x1->a_t || !x1->c_t || (b.U > 0 && (!xt->e_t || !x1->e_t))) return fail(c, FM_ERR_INVALID, "%s: null argument", fn);
    // cnt_e is a float: exact up to 2^24 rows per molecule
    if ((int64_t)c->plan.nmax * (c->plan.nmax - 1) / 2 > (1 << 24))
        return fail(c, FM_ERR_INVALID, "%s: a molecule of %d atoms has more than 2^24 pair rows: its row count is not exact in float32", fn, c->plan.nmax);
    const void* const in[] = {xt->x_t, xt->a_t, xt->c_t, xt->e_t, x1->x_t, x1->a_t, x1->c_t, x1->e_t, temb, mol_group};
    const void* const outp[] = {rows->x, rows->a, rows->c, rows->e, mol_out};
    static const char* const out_tag[] = {"rows->x", "rows->a", "rows->c", "rows->e", "mol_out"};
    for (int o = 0; o < 5; ++o) {
        for (const void* p : in) if (p && p == outp[o]) return fail(c, FM_ERR_INVALID, "%s: %s aliases an input", fn, out_tag[o]);
        for (int q = 0; q < o; ++q) if (outp[q] == outp[o]) return fail(c, FM_ERR_INVALID, "%s: %s aliases %s", fn, out_tag[o], out_tag[q]);
    }
    const hipStream_t st = (hipStream_t)stream;
    if (temb) {      // one evaluation, the heads in their loss variant: the raw positions stay in the workspace (remove_com = 2: no copy, no COM removal)
        const fm_dst out{nullptr, rows->a, rows->c, rows->e};
        if (const int rc = forward_impl(c, st, xt, temb, nullptr, 0, 2, &out, -1, n_groups > 1 ? mol_group : nullptr, n_groups, x1)) return rc;
    }
    FmLossReduceArgs a{};
    a.node_off = b.mol_node_off; a.pair_off = b.mol_pair_off;
    a.x_pred = temb ? c->ws.xw : nullptr; a.x_tgt = x1->x_t; a.rows_x = rows->x;
    for (int m = 0; m < 3; ++m) { a.rows[m] = pick3(m, rows->a, rows->c, rows->e); a.tok_t[m] = pick3(m, xt->a_t, xt->c_t, xt->e_t); a.mask[m] = modality(c, m).K; }
    a.out = mol_out;
    Launch L{c, st};
    L("denoise_reduce", fm_k_denoise_reduce, dim3(b.B), dim3(64), 0, a);
    return L.rc;
}

int fm_distort_philox(fm_ctx* c, void* stream, uint64_t seed, float p, int n_groups, const int32_t* mol_group, const int32_t* group_on, float* x,
                      const fm_distort_tape* tape) {
    const char* const fn = "fm_distort_philox";
    if (const int rc = bound_check(c, fn, group_on && x)) return rc;
    if (n_groups < 1) return fail(c, FM_ERR_INVALID, "%s: n_groups = %d, need at least 1", fn, n_groups);
    if (n_groups > 1 && !mol_group) return fail(c, FM_ERR_INVALID, "%s: mol_group is NULL with n_groups = %d", fn, n_groups);
    if (!(p >= 0.0f && p <= 1.0f)) return fail(c, FM_ERR_INVALID, "%s: p = %g is not a probability", fn, (double)p);
    if (tape && (tape->z == x || tape->u == x)) return fail(c, FM_ERR_INVALID, "%s: the tape aliases x", fn);
    FmDistortArgs a{};
    a.x = x; a.node_off = c->ws.b.mol_node_off; a.mol_gid = c->ws.mol_gid; a.mol_group = n_groups > 1 ? mol_group : nullptr; a.group_on = group_on;
    a.p = p; a.seed_lo = (unsigned)(seed & 0xffffffffu); a.seed_hi = (unsigned)(seed >> 32);
    if (tape) { a.z = tape->z; a.u = tape->u; }
    Launch L{c, (hipStream_t)stream};
    L("distort_philox", fm_k_distort_philox, dim3(c->ws.b.B), dim3(64), 0, a);
    return L.rc;
}

int fm_integrate_mixed(fm_ctx* c, void* stream, const fm_state* state, int n_steps, int n_groups, const fm_step_scalars* steps,
                       const fm_step_scalars* steps_dev, const int32_t* active, const int32_t* active_dev, const int32_t* mol_group, const float* temb,
                       const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst) {
    const bool args_ok = state && steps && steps_dev && active && active_dev && mol_group && temb && dst_a && dst_b;
    if (const int rc = mixed_check(c, "fm_integrate_mixed", args_ok, n_groups)) return rc;
    if (sink) return fail(c, FM_ERR_INVALID, "fm_integrate_mixed: a trajectory sink is not supported with per-molecule time");
    // the launch decisions are made from the host copy, before anything is enqueued
    for (int i = 0; i < n_steps * n_groups; ++i) {
        if (!active[i]) continue;
        if (steps[i].dfm_type != FM_DFM_CAMPBELL) return fail(c, FM_ERR_INVALID, "fm_integrate_mixed: dfm_type gat is not supported with per-molecule time (step %d, group %d)", i / n_groups, i % n_groups);
        if (steps[i].noise_mode != FM_NOISE_PHILOX) return fail(c, FM_ERR_INVALID, "fm_integrate_mixed: FM_NOISE_TENSORS is not supported with per-molecule time: the reference's draw order depends on last_step (step %d, group %d)", i / n_groups, i % n_groups);
    }
    int boot0 = 0;
    if (!prev0 && n_steps > 0) {      // prev is None and (t == 0).all(), vector_field.py:269-272, over the groups that take the step
        int at0 = 0, later = 0;
        for (int g = 0; g < n_groups; ++g) if (active[g]) (steps[g].t == 0.0f ? at0 : later) += 1;
        if (at0 && later) return fail(c, FM_ERR_INVALID, "fm_integrate_mixed: prev0 is NULL and only %d of %d active groups are at t = 0: start the groups at t = 0 in a call of their own", at0, at0 + later);
        boot0 = at0 ? 1 : 0;
    }
    static const fm_step_scalars philox_step = [] { fm_step_scalars s{}; s.dfm_type = FM_DFM_CAMPBELL; s.noise_mode = FM_NOISE_PHILOX; return s; }();
    return step_driver(c, (hipStream_t)stream, state, n_steps, n_groups, mol_group, temb, prev0, dst_a, dst_b, nullptr, final_dst,
                       [&](int i, const fm_dst*, const fm_step_scalars*& sc, const fm_step_noise*&, MixedStep& mixed) {
        sc = &philox_step; mixed = {steps_dev + (size_t)i * n_groups, active_dev + (size_t)i * n_groups, mol_group};
        return i == 0 ? boot0 : 0; });
}

// What the frozen-row entry points of ABI 12 refuse, before anything is enqueued, and the kernels' view of the caller's struct.  others: every pointer the call
// writes through or reads as the evolving state (state, endpoint buffers, sampled tokens, sink).
static int inpaint_check(fm_ctx* c, const char* fn, const fm_inpaint* inp, std::initializer_list<const void*> others, FmKeepArgs& k) {
    if (!c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "%s: endpoint models (has_mask = 0) have no masked conditional path to freeze rows on", fn);
    const bool pairs = c->ws.b.U > 0;
    const void* const mem[] = {inp->keep_atom, inp->keep_pair, inp->x0, inp->x1c, inp->a1, inp->c1, inp->e1, inp->u_a, inp->u_c, inp->u_e};
    static const char* const tag[] = {"keep_atom", "keep_pair", "x0", "x1c", "a1", "c1", "e1", "u_a", "u_c", "u_e"};
    static const bool pair_only[] = {false, true, false, false, false, false, true, false, false, true};
    for (int i = 0; i < 10; ++i) {
        if (!mem[i] && (pairs || !pair_only[i])) return fail(c, FM_ERR_INVALID, "%s: fm_inpaint.%s is NULL", fn, tag[i]);
        for (const void* o : others) if (mem[i] && o == mem[i]) return fail(c, FM_ERR_INVALID, "%s: fm_inpaint.%s aliases the state, an endpoint buffer or the sink", fn, tag[i]);
    }
    k = FmKeepArgs{};
    k.keep_x = k.keep[0] = k.keep[1] = inp->keep_atom; k.keep[2] = inp->keep_pair;
    k.tok1[0] = inp->a1; k.tok1[1] = inp->c1; k.tok1[2] = inp->e1;
    k.u[0] = inp->u_a; k.u[1] = inp->u_c; k.u[2] = inp->u_e;
    k.x0 = inp->x0; k.x1c = inp->x1c;
    return FM_OK;
}
// The same for ABI 13's fm_freeze: four independent keep arrays, all inputs.  A modality whose keep pointer is NULL is free, and its path inputs are not read (the kernels
// branch around its select); a modality whose keep pointer is given needs its path inputs -- the pair modality only in a batch that has pairs.
static int freeze_check(fm_ctx* c, const char* fn, const fm_freeze* fz, std::initializer_list<const void*> others, FmKeepArgs& k) {
    if (!c->cfg.has_mask) return fail(c, FM_ERR_INVALID, "%s: endpoint models (has_mask = 0) have no masked conditional path to freeze rows on", fn);
    const void* const mem[] = {fz->keep_x, fz->keep_a, fz->keep_c, fz->keep_e, fz->x0, fz->x1c, fz->a1, fz->c1, fz->e1, fz->u_a, fz->u_c, fz->u_e};
    static const char* const tag[] = {"keep_x", "keep_a", "keep_c", "keep_e", "x0", "x1c", "a1", "c1", "e1", "u_a", "u_c", "u_e"};
    static const int owner[] = {0, 1, 2, 3, 0, 0, 1, 2, 3, 1, 2, 3};      // the keep array (mem[0..3]) a member belongs to
    for (int i = 0; i < 12; ++i) {
        if (!mem[i] && mem[owner[i]] && (owner[i] != 3 || c->ws.b.U > 0))
            return fail(c, FM_ERR_INVALID, "%s: fm_freeze.%s is NULL while fm_freeze.%s is given", fn, tag[i], tag[owner[i]]);
        for (const void* o : others) if (mem[i] && o == mem[i]) return fail(c, FM_ERR_INVALID, "%s: fm_freeze.%s aliases the state, an endpoint buffer or the sink", fn, tag[i]);
    }
    k = FmKeepArgs{};
    k.keep_x = fz->keep_x; k.keep[0] = fz->keep_a; k.keep[1] = fz->keep_c; k.keep[2] = c->ws.b.U > 0 ? fz->keep_e : nullptr;
    k.tok1[0] = fz->a1; k.tok1[1] = fz->c1; k.tok1[2] = fz->e1;
    k.u[0] = fz->u_a; k.u[1] = fz->u_c; k.u[2] = fz->u_e;
    k.x0 = fz->x0; k.x1c = fz->x1c;
    return FM_OK;
}
// keep_pair of fm_inpaint from keep_atom: one launch per call, ahead of the steps
static int keep_pairs(fm_ctx* c, hipStream_t st, const fm_inpaint* inp) {
    const FmBatch& b = c->ws.b;
    Launch L{c, st};
    L("keep_pairs", fm_k_keep_pairs, dim3((b.U + 255) / 256), dim3(256), 0, (const unsigned char*)inp->keep_atom, (unsigned char*)inp->keep_pair,
      (const int*)b.p_e0, (const int*)b.e_src, (const int*)b.e_dst, b.U);
    return L.rc;
}

// One step with frozen rows, behind the entry point's argument checks: ks.k holds the four keep pointers and the path inputs.  inp: fm_ctmc_step_inpaint's struct, whose
// keep_pair is filled first; NULL for fm_ctmc_step_freeze, which brings its pair flags.
static int step_keep(fm_ctx* c, const char* fn, hipStream_t st, const fm_state* state, const fm_dst* dst, const fm_step_noise* noise, const fm_step_scalars* sc,
                     const fm_sampled* sampled, KeepStep& ks, const float* alpha_next, const fm_inpaint* inp) {
    if (sc->dfm_type != FM_DFM_CAMPBELL && sc->dfm_type != FM_DFM_GAT) return fail(c, FM_ERR_INVALID, "%s: unknown dfm_type %d", fn, sc->dfm_type);
    if (sc->noise_mode != FM_NOISE_PHILOX && !noise) return fail(c, FM_ERR_INVALID, "%s: noise tensors missing (noise_mode FM_NOISE_TENSORS)", fn);
    for (int k = 0; k < 4; ++k) ks.k.alpha[k] = alpha_next[k];
    if (inp) if (const int rc = keep_pairs(c, st, inp)) return rc;
    const Modality md[3] = {modality(c, 0, state), modality(c, 1, state), modality(c, 2, state)};
    return ctmc_impl(c, st, md, state, dst, noise, sc, sampled, nullptr, nullptr, nullptr, &ks);
}

int fm_ctmc_step_inpaint(fm_ctx* c, void* stream, const fm_state* state, const fm_dst* dst, const fm_step_noise* noise, const fm_step_scalars* sc,
                         const fm_sampled* sampled, const fm_inpaint* inp, const float* alpha_next) {
    const char* const fn = "fm_ctmc_step_inpaint";
    if (const int rc = bound_check(c, fn, state && dst && sc && inp && alpha_next)) return rc;
    KeepStep ks{};
    if (const int rc = inpaint_check(c, fn, inp, {state->x_t, state->a_t, state->c_t, state->e_t, dst->x, dst->a, dst->c, dst->e,
                                                  sampled ? sampled->a1 : nullptr, sampled ? sampled->c1 : nullptr, sampled ? sampled->e1 : nullptr}, ks.k)) return rc;
    return step_keep(c, fn, (hipStream_t)stream, state, dst, noise, sc, sampled, ks, alpha_next, inp);
}

int fm_ctmc_step_freeze(fm_ctx* c, void* stream, const fm_state* state, const fm_dst* dst, const fm_step_noise* noise, const fm_step_scalars* sc,
                        const fm_sampled* sampled, const fm_freeze* fz, const float* alpha_next) {
    const char* const fn = "fm_ctmc_step_freeze";
    if (const int rc = bound_check(c, fn, state && dst && sc && fz && alpha_next)) return rc;
    KeepStep ks{};
    if (const int rc = freeze_check(c, fn, fz, {state->x_t, state->a_t, state->c_t, state->e_t, dst->x, dst->a, dst->c, dst->e,
                                                sampled ? sampled->a1 : nullptr, sampled ? sampled->c1 : nullptr, sampled ? sampled->e1 : nullptr}, ks.k)) return rc;
    return step_keep(c, fn, (hipStream_t)stream, state, dst, noise, sc, sampled, ks, alpha_next, nullptr);
}

// fm_integrate_inpaint / fm_integrate_freeze behind their argument checks (k0: the keep pointers and path inputs; inp as in step_keep)
static int integrate_keep(fm_ctx* c, const char* fn, hipStream_t st, const fm_state* state, int n_steps, int n_groups, const fm_step_scalars* steps,
                          const fm_step_scalars* steps_dev, const int32_t* active, const int32_t* active_dev, const int32_t* mol_group, const float* temb,
                          const fm_step_noise* noise, const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst,
                          const FmKeepArgs& k0, const fm_inpaint* inp, const float* alpha_next, const float* alpha_next_dev) {
    const bool one = n_groups == 1;
    std::vector<KeepStep> ks((size_t)std::max(n_steps, 0));
    for (int i = 0; i < n_steps; ++i) {
        ks[i].k = k0;
        if (one) for (int q = 0; q < 4; ++q) ks[i].k.alpha[q] = alpha_next[(size_t)i * 4 + q];
        else ks[i].alpha_dev = alpha_next_dev + (size_t)i * n_groups * 4;
    }
    const auto keep_of = [&](int i) { return (const KeepStep*)&ks[i]; };
    if (one) {      // a batch at one time: fm_integrate's steps (campbell or gat, either noise mode, trajectory sink) through the single-schedule kernels
        for (int i = 0; i < n_steps; ++i) {
            if (steps[i].dfm_type != FM_DFM_CAMPBELL && steps[i].dfm_type != FM_DFM_GAT) return fail(c, FM_ERR_INVALID, "%s: unknown dfm_type %d (step %d)", fn, steps[i].dfm_type, i);
            if (steps[i].noise_mode != FM_NOISE_PHILOX && !noise) return fail(c, FM_ERR_INVALID, "%s: noise tensors missing (noise_mode FM_NOISE_TENSORS, step %d)", fn, i);
        }
        if (inp) if (const int rc = keep_pairs(c, st, inp)) return rc;
        return step_driver(c, st, state, n_steps, 1, nullptr, temb, prev0, dst_a, dst_b, sink, final_dst,
                           [&](int i, const fm_dst* prev, const fm_step_scalars*& sc, const fm_step_noise*& nz, MixedStep&) {
            sc = &steps[i]; nz = noise ? &noise[i] : nullptr;
            return !prev && steps[i].t == 0.0f ? 1 : 0; }, keep_of);
    }
    // per-molecule time: fm_integrate_mixed's refusals and launch decisions
    if (sink) return fail(c, FM_ERR_INVALID, "%s: a trajectory sink is not supported with per-molecule time", fn);
    for (int i = 0; i < n_steps * n_groups; ++i) {
        if (!active[i]) continue;
        if (steps[i].dfm_type != FM_DFM_CAMPBELL) return fail(c, FM_ERR_INVALID, "%s: dfm_type gat is not supported with per-molecule time (step %d, group %d)", fn, i / n_groups, i % n_groups);
        if (steps[i].noise_mode != FM_NOISE_PHILOX) return fail(c, FM_ERR_INVALID, "%s: FM_NOISE_TENSORS is not supported with per-molecule time (step %d, group %d)", fn, i / n_groups, i % n_groups);
    }
    int boot0 = 0;
    if (!prev0 && n_steps > 0) {
        int at0 = 0, later = 0;
        for (int g = 0; g < n_groups; ++g) if (active[g]) (steps[g].t == 0.0f ? at0 : later) += 1;
        if (at0 && later) return fail(c, FM_ERR_INVALID, "%s: prev0 is NULL and only %d of %d active groups are at t = 0: start the groups at t = 0 in a call of their own", fn, at0, at0 + later);
        boot0 = at0 ? 1 : 0;
    }
    if (inp) if (const int rc = keep_pairs(c, st, inp)) return rc;
    static const fm_step_scalars philox_step = [] { fm_step_scalars s{}; s.dfm_type = FM_DFM_CAMPBELL; s.noise_mode = FM_NOISE_PHILOX; return s; }();
    return step_driver(c, st, state, n_steps, n_groups, mol_group, temb, prev0, dst_a, dst_b, nullptr, final_dst,
                       [&](int i, const fm_dst*, const fm_step_scalars*& sc, const fm_step_noise*&, MixedStep& mixed) {
        sc = &philox_step; mixed = {steps_dev + (size_t)i * n_groups, active_dev + (size_t)i * n_groups, mol_group};
        return i == 0 ? boot0 : 0; }, keep_of);
}

// the argument checks fm_integrate_inpaint and fm_integrate_freeze share, up to their struct's own (check: inpaint_check / freeze_check on the pointers of the call)
static int integrate_keep_entry(fm_ctx* c, const char* fn, const fm_state* state, int n_groups, const fm_step_scalars* steps, const fm_step_scalars* steps_dev,
                                const int32_t* active, const int32_t* active_dev, const int32_t* mol_group, const float* temb, const fm_dst* dst_a, const fm_dst* dst_b,
                                const fm_traj_sink* sink, const void* spec, const float* alpha_next, const float* alpha_next_dev,
                                const std::function<int(std::initializer_list<const void*>)>& check) {
    const bool one = n_groups == 1;
    const bool args_ok = state && steps && temb && dst_a && dst_b && spec && alpha_next && (one || (steps_dev && active && active_dev && mol_group && alpha_next_dev));
    if (const int rc = bound_check(c, fn, args_ok)) return rc;
    if (n_groups < 1 || n_groups > FM_TAB_SLOTS) return fail(c, FM_ERR_INVALID, "%s: n_groups = %d outside 1..%d (FM_TAB_SLOTS embedding tables per bound batch)", fn, n_groups, FM_TAB_SLOTS);
    static const fm_traj_sink no_sink{};
    const fm_traj_sink& sk = sink ? *sink : no_sink;
    return check({state->x_t, state->a_t, state->c_t, state->e_t, dst_a->x, dst_a->a, dst_a->c, dst_a->e, dst_b->x, dst_b->a, dst_b->c, dst_b->e,
                  sk.x, sk.a, sk.c, sk.e, sk.x1, sk.a1, sk.c1, sk.e1});
}

int fm_integrate_inpaint(fm_ctx* c, void* stream, const fm_state* state, int n_steps, int n_groups, const fm_step_scalars* steps,
                         const fm_step_scalars* steps_dev, const int32_t* active, const int32_t* active_dev, const int32_t* mol_group, const float* temb,
                         const fm_step_noise* noise, const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst,
                         const fm_inpaint* inp, const float* alpha_next, const float* alpha_next_dev) {
    const char* const fn = "fm_integrate_inpaint";
    FmKeepArgs k0{};
    if (const int rc = integrate_keep_entry(c, fn, state, n_groups, steps, steps_dev, active, active_dev, mol_group, temb, dst_a, dst_b, sink, inp, alpha_next, alpha_next_dev,
                                            [&](std::initializer_list<const void*> others) { return inpaint_check(c, fn, inp, others, k0); })) return rc;
    return integrate_keep(c, fn, (hipStream_t)stream, state, n_steps, n_groups, steps, steps_dev, active, active_dev, mol_group, temb, noise, prev0, dst_a, dst_b, sink,
                          final_dst, k0, inp, alpha_next, alpha_next_dev);
}

int fm_integrate_freeze(fm_ctx* c, void* stream, const fm_state* state, int n_steps, int n_groups, const fm_step_scalars* steps,
                        const fm_step_scalars* steps_dev, const int32_t* active, const int32_t* active_dev, const int32_t* mol_group, const float* temb,
                        const fm_step_noise* noise, const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst,
                        const fm_freeze* fz, const float* alpha_next, const float* alpha_next_dev) {
    const char* const fn = "fm_integrate_freeze";
    FmKeepArgs k0{};
    if (const int rc = integrate_keep_entry(c, fn, state, n_groups, steps, steps_dev, active, active_dev, mol_group, temb, dst_a, dst_b, sink, fz, alpha_next, alpha_next_dev,
                                            [&](std::initializer_list<const void*> others) { return freeze_check(c, fn, fz, others, k0); })) return rc;
    return integrate_keep(c, fn, (hipStream_t)stream, state, n_steps, n_groups, steps, steps_dev, active, active_dev, mol_group, temb, noise, prev0, dst_a, dst_b, sink,
                          final_dst, k0, nullptr, alpha_next, alpha_next_dev);
}

// Aligned RMSD of two coordinate sets of the bound batch, molecule by molecule (fm_k_align_rmsd: one wave per molecule, everything on the device)
int fm_align_rmsd(fm_ctx* c, void* stream, const float* xa, const float* xb, const uint8_t* select, float* out, float* xa_aligned) {
    const char* const fn = "fm_align_rmsd";
    if (const int rc = bound_check(c, fn, xa && xb && out)) return rc;
    const void* const in[] = {xa, xb, select};
    for (const void* p : in) {
        if (p && p == (const void*)out) return fail(c, FM_ERR_INVALID, "%s: out aliases an input", fn);
        if (p && xa_aligned && p == (const void*)xa_aligned) return fail(c, FM_ERR_INVALID, "%s: xa_aligned aliases an input", fn);
    }
    if (xa_aligned && (const void*)xa_aligned == (const void*)out) return fail(c, FM_ERR_INVALID, "%s: xa_aligned aliases out", fn);
    Launch L{c, (hipStream_t)stream};
    L("align_rmsd", fm_k_align_rmsd, dim3(c->ws.b.B), dim3(64), 0, xa, xb, (const unsigned char*)select, (const int*)c->ws.b.mol_node_off, out, xa_aligned);
    return L.rc;
}

// Equivariant-OT coupling of a position prior to the given positions of the bound batch (fm_k_ot_align: one wave per molecule, assignment then rigid fit).  The
// size cap is checked on the bind's host copy of the offsets: nothing is enqueued for a batch with a molecule above it.
int fm_ot_align(fm_ctx* c, void* stream, const float* x0, const float* x1c, int allow_reflection, float* x0_aligned, int32_t* perm, float* out) {
    const char* const fn = "fm_ot_align";
    if (!c || !x0 || !x1c || !x0_aligned || !out) return fail(c, FM_ERR_INVALID, "%s: null argument", fn);
    if (!c->bound) return fail(c, FM_ERR_INVALID, "%s: no batch bound", fn);
    if (allow_reflection != 0 && allow_reflection != 1) return fail(c, FM_ERR_INVALID, "%s: allow_reflection = %d, need 0 or 1", fn, allow_reflection);
    const void* const in[] = {x0, x1c};
    const void* const outs[] = {x0_aligned, perm, out};
    for (int a = 0; a < 3; ++a) {
        if (!outs[a]) continue;
        for (const void* p : in)
            if (p == outs[a]) return fail(c, FM_ERR_INVALID, "%s: an output aliases an input", fn);
        for (int b = a + 1; b < 3; ++b)
            if (outs[b] == outs[a]) return fail(c, FM_ERR_INVALID, "%s: an output aliases another output", fn);
    }
    const std::vector<int32_t>& off = c->node_off_h;
    for (int m = 0; m < c->ws.b.B; ++m)
        if (off[m + 1] - off[m] > FM_OT_MAX_ATOMS)
            return fail(c, FM_ERR_INVALID, "%s: molecule %d has %d atoms, more than the %d the assignment kernel takes", fn, m, off[m + 1] - off[m], FM_OT_MAX_ATOMS);
    Launch L{c, (hipStream_t)stream};
    FmOtArgs g{};
    g.x0 = x0; g.x1c = x1c; g.node_off = c->ws.b.mol_node_off; g.x0_al = x0_aligned; g.perm = perm; g.out = out; g.allow_reflection = allow_reflection;
    L("ot_align", fm_k_ot_align, dim3(c->ws.b.B), dim3(64), 0, g);
    return L.rc;
}

// Stereo check of two coordinate sets of the bound batch, molecule by molecule (fm_k_stereo: one wave per molecule, lanes strided over its element rows)
int fm_stereo(fm_ctx* c, void* stream, const float* x, const float* x_ref, const int32_t* elem_set, const int32_t* set_off, const int32_t* elems, int n_sets,
              float flat_tol, int32_t* out, const int32_t* val_off, float* values, float* x_out) {
    const char* const fn = "fm_stereo";
    if (!c || !x || !x_ref || !out) return fail(c, FM_ERR_INVALID, "%s: null argument", fn);
    if (!c->bound) return fail(c, FM_ERR_INVALID, "%s: no batch bound", fn);
    const bool table = elem_set || set_off || elems;
    if (table && !(elem_set && set_off && elems && n_sets >= 1))
        return fail(c, FM_ERR_INVALID, "%s: elem_set, set_off and elems come together with n_sets >= 1, or all NULL with n_sets = 0 (no element)", fn);
    if (!table && n_sets != 0) return fail(c, FM_ERR_INVALID, "%s: n_sets = %d without an element table", fn, n_sets);
    if (!(flat_tol >= 0.f)) return fail(c, FM_ERR_INVALID, "%s: flat_tol = %g must be a number >= 0", fn, (double)flat_tol);
    if (values && !val_off) return fail(c, FM_ERR_INVALID, "%s: values without val_off", fn);
    const void* const in[] = {x, x_ref, elem_set, set_off, elems, val_off};
    const void* const outs[] = {out, values, x_out};
    for (int a = 0; a < 3; ++a) {
        if (!outs[a]) continue;
        for (const void* p : in)
            if (p && p == outs[a]) return fail(c, FM_ERR_INVALID, "%s: an output aliases an input", fn);
        for (int b = a + 1; b < 3; ++b)
            if (outs[b] == outs[a]) return fail(c, FM_ERR_INVALID, "%s: an output aliases another output", fn);
    }
    Launch L{c, (hipStream_t)stream};
    FmStereoArgs g{};
    g.x = x; g.x_ref = x_ref; g.node_off = c->ws.b.mol_node_off; g.elem_set = elem_set; g.set_off = set_off; g.elems = elems; g.n_sets = n_sets;
    g.flat_tol = flat_tol; g.out = out; g.val_off = values ? val_off : nullptr; g.vals = values; g.x_out = x_out;
    L("stereo", fm_k_stereo, dim3(c->ws.b.B), dim3(64), 0, g);
    return L.rc;
}

// Symmetry-aware aligned RMSD of pairs of molecules of the bound batch (fm_k_pair_rmsd: one wave per pair, one lane per permutation row).  pairs_host is read
// here, for the refusals; the kernel reads the device copy.
int fm_pair_rmsd(fm_ctx* c, void* stream, const float* x, int n_pairs, const int32_t* pairs_host, const int32_t* pairs, const uint8_t* select,
                 const int32_t* perm_set, const int32_t* set_off, const int32_t* perms, int n_sets, float* out, int32_t* best_perm) {
    const char* const fn = "fm_pair_rmsd";
    if (const int rc = bound_check(c, fn, x && out && (n_pairs <= 0 || (pairs_host && pairs)))) return rc;
    if (n_pairs < 0) return fail(c, FM_ERR_INVALID, "%s: n_pairs = %d", fn, n_pairs);
    const bool table = perm_set || set_off || perms;
    if (table && !(perm_set && set_off && perms && n_sets >= 1))
        return fail(c, FM_ERR_INVALID, "%s: perm_set, set_off and perms come together with n_sets >= 1, or all NULL with n_sets = 0 (the identity only)", fn);
    if (!table && n_sets != 0) return fail(c, FM_ERR_INVALID, "%s: n_sets = %d without a permutation table", fn, n_sets);
    const void* const in[] = {x, pairs, select, perm_set, set_off, perms};
    for (const void* p : in) {
        if (p && p == (const void*)out) return fail(c, FM_ERR_INVALID, "%s: out aliases an input", fn);
        if (p && best_perm && p == (const void*)best_perm) return fail(c, FM_ERR_INVALID, "%s: best_perm aliases an input", fn);
    }
    if (best_perm && (const void*)best_perm == (const void*)out) return fail(c, FM_ERR_INVALID, "%s: best_perm aliases out", fn);
    const int B = c->ws.b.B;
    const std::vector<int32_t>& off = c->node_off_h;
    for (int p = 0; p < n_pairs; ++p) {
        const int a = pairs_host[2 * p], b = pairs_host[2 * p + 1];
        if (a < 0 || a >= B || b < 0 || b >= B) return fail(c, FM_ERR_INVALID, "%s: pair %d = (%d, %d) names a molecule outside 0..%d", fn, p, a, b, B - 1);
        if (off[a + 1] - off[a] != off[b + 1] - off[b])
            return fail(c, FM_ERR_INVALID, "%s: pair %d = (%d, %d): molecules of unequal size, %d and %d atoms", fn, p, a, b, off[a + 1] - off[a], off[b + 1] - off[b]);
    }
    Launch L{c, (hipStream_t)stream};
    FmPairRmsdArgs g{};
    g.x = x; g.node_off = c->ws.b.mol_node_off; g.pairs = pairs; g.sel = select; g.perm_set = perm_set; g.set_off = set_off; g.perms = perms; g.n_sets = n_sets;
    g.out = out; g.best = best_perm;
    L("pair_rmsd", fm_k_pair_rmsd, dim3(n_pairs), dim3(64), 0, g);
    return L.rc;
}

// Greedy RMSD-threshold pruning of conformer groups (fm_k_prune_rmsd: one wave per group).  Needs no bound batch: every array is the caller's.
int fm_prune_rmsd(fm_ctx* c, void* stream, int n_groups, const int32_t* group_off, const float* d, const int32_t* tri_off, float threshold, uint8_t* keep,
                  int32_t* rep) {
    const char* const fn = "fm_prune_rmsd";
    if (!c || !group_off || !tri_off || !keep || !rep) return fail(c, FM_ERR_INVALID, "%s: null argument", fn);
    if (n_groups < 0) return fail(c, FM_ERR_INVALID, "%s: n_groups = %d", fn, n_groups);
    const void* const in[] = {group_off, d, tri_off};
    for (const void* p : in)
        if (p && (p == (const void*)keep || p == (const void*)rep)) return fail(c, FM_ERR_INVALID, "%s: keep or rep aliases an input", fn);
    if ((const void*)keep == (const void*)rep) return fail(c, FM_ERR_INVALID, "%s: keep aliases rep", fn);
    Launch L{c, (hipStream_t)stream};
    L("prune_rmsd", fm_k_prune_rmsd, dim3(n_groups), dim3(64), 0, group_off, d, tri_off, threshold, (unsigned char*)keep, rep);
    return L.rc;
}

int fm_set_tap(fm_ctx* c, const char* name, void* dst) {
    if (!c || !name) return fail(c, FM_ERR_INVALID, "fm_set_tap: null argument");
    if (dst) c->taps[name] = dst; else c->taps.erase(name);
    return FM_OK;
}
int fm_clear_taps(fm_ctx* c) { if (c) c->taps.clear(); return FM_OK; }

int fm_batch_query(fm_ctx* c, void* stream, const char* name, int32_t* dst) {
    if (const int rc = bound_check(c, "fm_batch_query", name && dst)) return rc;
    const FmBatch& b = c->ws.b;
    const struct { const char* name; const int* src; int cnt; } arrays[] = {{"e_src", b.e_src, b.E}, {"e_dst", b.e_dst, b.E}, {"e_pair", b.e_pair, b.E},
        {"p_e0", b.p_e0, b.U}, {"p_e1", b.p_e1, b.U}, {"node_mol", b.node_mol, b.N}, {"pair_mol", b.pair_mol, b.U}};
    for (const auto& a : arrays)
        if (!strcmp(name, a.name)) { FM_HIP(c, hipMemcpyAsync(dst, a.src, (size_t)a.cnt * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream)); return FM_OK; }
    return fail(c, FM_ERR_INVALID, "fm_batch_query: unknown array %s", name);
}

#ifdef FM_TRACE
int fm_trace_read(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(fm_trace), 16384 * 16 * 8); return 0; }
#endif
#ifdef FM_PHASE_TIMING
// dev-only (not part of the ABI header): read / reset the phase-cycle accumulators of a -DFM_PHASE_TIMING build
int fm_tlog_read(unsigned long long* out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(fm_tlog), 64 * 8);
    if (reset) { unsigned long long z[64] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(fm_tlog), z, 64 * 8); }
    return 0;
}
#endif

int fm_stability(fm_ctx* c, void* stream, const fm_state* state, const uint32_t* table, int n_types, int fake_atom_token,
                 int explicit_aromaticity, int32_t* out) {
    if (const int rc = bound_check(c, "fm_stability", state && table && out)) return rc;
    if (!state->a_t || !state->c_t || !state->e_t) return fail(c, FM_ERR_INVALID, "fm_stability: state tokens missing");
    Launch L{c, (hipStream_t)stream};
    FmStabArgs a{};
    a.b = c->ws.b; a.a = state->a_t; a.c = state->c_t; a.e = state->e_t; a.table = table; a.n_types = n_types; a.n_charges = c->nc;
    a.fake_tok = fake_atom_token; a.ne = c->ne; a.arom = explicit_aromaticity; a.out = out;
    L("stability", fm_k_stability, dim3(c->ws.b.B), dim3(64), (size_t)c->plan.nmax * 8, a);
    return L.rc;
}

int fm_profile_enable(fm_ctx* c, int on) {
    if (!c) return FM_ERR_INVALID;
    c->prof = on != 0;
    if (on) {
        for (auto& pe : c->prof_events) { c->ev_pool.push_back(pe.a); c->ev_pool.push_back(pe.b); }
        c->prof_events.clear(); c->prof_acc.clear();
    }
    return FM_OK;
}

int fm_profile_get(fm_ctx* c, const char* kernel, double* total_ms, int64_t* launches) {
    if (!c || !kernel || !total_ms || !launches) return fail(c, FM_ERR_INVALID, "fm_profile_get: null argument");
    for (auto& pe : c->prof_events) {       // fold finished events into the accumulators
        FM_HIP(c, hipEventSynchronize(pe.b));
        float ms = 0.f;
        FM_HIP(c, hipEventElapsedTime(&ms, pe.a, pe.b));
        auto& acc = c->prof_acc[c->prof_names[pe.kid]];
        acc.first += ms; acc.second += 1;
        c->ev_pool.push_back(pe.a); c->ev_pool.push_back(pe.b);
    }
    c->prof_events.clear();
    auto it = c->prof_acc.find(kernel);
    if (it == c->prof_acc.end()) { *total_ms = 0; *launches = 0; return FM_OK; }
    *total_ms = it->second.first; *launches = it->second.second;
    return FM_OK;
}

}  // extern "C"
