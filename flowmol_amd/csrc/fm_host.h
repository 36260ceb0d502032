// Host-side declarations shared by the translation units of libflowmol_hip.so, compiled in parallel (flowmol_amd/build.py) -- fm_engine.cpp: C ABI, weight
// packing, the batch plan, workspace, the launch sequence and the small kernels; fm_tu_msg32.cpp / fm_tu_msg16.cpp: the edge-message instances; fm_tu_node.cpp:
// the node-kernel instances.  The engine reaches the heavy kernels through the launcher functions declared at the end of this file (no unit instantiates
// another unit's kernels).  Which weight copies a model has is decided once, by fm_create (fm_engine.cpp), into the ModelPlan that the packing and plan_batch
// read; every launch choice that depends on the batch is made once, by plan_batch, into the BatchPlan that the workspace layout and the launches read; every
// kernel family names its instances once, in an instance list that its launcher and the LDS opt-in both read.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/flowmol_hip.h"
#include "fm_kernels.h"

namespace fmh {

constexpr int FM_TAB_SLOTS = 32;      // embedding tables kept per bound batch: fm_integrate builds those of up to 32 steps in one launch

extern thread_local std::string g_create_error;      // defined in fm_engine.cpp (fm_last_error(NULL))

struct ProfEvent { int kid; hipEvent_t a, b; };

struct MlpW { const float2* W1; const float* b1; const float2* W2; const float* b2; int K1p, H, O; };

struct ConvW {
    const float2* Wps; const float2* Wpv; const float* w0;
    const float2* Ws_slab = nullptr;   // pair-slab convolutions: [rbf | ef] rows of GVP0's scalar linear (K = 160), multiplied per pair in the SC_EDGE kernel
    const float2* Ws_sh = nullptr;     //                         and its remaining rows, the hidden-vector norms (K = KU0)
    const void* Wps_sp = nullptr;      // split precision
    const void* Wps4 = nullptr;        // quad-row packed (4-node tiles)
    FmGvpW dproj{}; const float2* Wsd = nullptr; const float2* Wpvd = nullptr;     // use_dst_feats: projection GVP + hoisted destination terms
    FmGvpW msg[3]; FmGvpW upd[3];
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
};
struct UpdW {
    FmGvpW pos[3];
    const float2* Wasd; const float2* W1; const float* b1; const float2* W2; const float* b2;
    const float *ln_g, *ln_b;
    const void *W1_sp = nullptr, *W2_sp = nullptr, *Wasd_sp = nullptr;      // split-precision builds
    const void* Wasd4 = nullptr;       // quad-row packed (4-node tiles)
};

// The weight layouts of one model (model_plan, fm_engine.cpp): a function of its fm_config only.  fm_create packs a copy exactly when this says so, and
// plan_batch selects an instance only when this says its copies exist.
struct ModelPlan {
    bool narrow_s = false;    // n_hidden_scalars < 256: LayerNorm statistics over the real width (narrow node instances)
    bool narrow_f = false;    // n_hidden_edge_feats < 128 (narrow EdgeUpdate instance)
    bool quad_mlp = false;    // quad-row copies of the 4-row node MLPs and conv 0's projection (fm_k_mlp4): sc_node_W1q / W2q, node_head_W1q / W2q, conv[0].Wps4
    bool quad_node = false;   // quad-row copies of the RG node instances: node-side FmGvpW::Ws4, every conv's Wps4, UpdW::Wasd4
    int msg_planes = 0;       // 16-bit planes of the edge-message split copies (FmGvpW::Ws_sp / Wg_sp of the message GVPs): 0 = none, 2, 3 (bf16x6)
    int node_sp = 0;          // two-plane split copies of the node and EdgeUpdate kernels (BatchPlan::node_sp): 0 = none, 1 = bf16 planes, 3 = half planes
    bool half_planes = false; // every split copy in IEEE-half planes (f16x3), else bf16
    int slab_convs = 0;       // convolutions that carry the pair-slab rows ConvW::Ws_slab / Ws_sh (0..2; BatchPlan::n_pq)
};

// The launch choices of one bound batch (plan_batch, fm_engine.cpp): made from the model, its fm_config overrides, the CU count and the molecule
// sizes.  What varies per call (prev given, dense inputs, taps, the last pass) is decided by the evaluation itself.
struct BatchPlan {
    int B = 0, N = 0, E = 0, U = 0, nmax = 0;      // molecules, atoms, directed edges, pairs; atoms of the largest molecule
    int P = 1;                // partial-sum chunks per destination node (FmBatch::P)
    int tm_edge = 32;         // edge-message tile rows (16 | 32 | 64)
    int n_tiles_msg = 0;      // molecule-aligned edge-message tiles (FmBatch::n_tiles)
    bool xcd_swizzle = true;  // edge-message tile -> workgroup mapping: contiguous tile range per XCD
    int tm_node = 32;         // node-kernel tile rows (16 | 32 | 64)
    int node_rg = 0;          // node kernel on tiles of 4 * node_rg nodes (RG instances; 1, 2, 3 in the 16-row frame, 5 in the 32-row frame), 0 = off
    int node_sp = 0;          // split-precision node kernel: 1 (bf16 planes) | 3 (half planes), 0 = f32
    bool fuse_node = true;    // node_update also runs the next conv's projections, EdgeUpdate's node terms and NodePositionUpdate
    int tm_eupd = 32;         // EdgeUpdate tile rows (32 | 64)
    bool fuse_head = true;    // the evaluation's last EdgeUpdate may run the edge output head on its pairs (fm_k_edge_update<32, false, true>)
    int n_pq = 0;             // pair-slab convolutions of a self-conditioned evaluation (0..2; the workspace holds their Q tables)
    bool pair_mlps = false;   // node- and pair-side MLPs of a stage share one launch
    bool small_node = false, small_pair = false;      // 16-row MLP / node_proj tiles on the node / pair side
    bool mlp4 = false;        // node-side MLPs on 4-row tiles (fm_k_mlp4)
    bool edge_head32 = false; // a separate edge head runs 32-row tiles
    int ctmc_threads = 256;   // workgroup size of fm_k_ctmc_fused and fm_k_ctmc_gat_fused (256 | 1024)
};

// The bound batch's pointers into the caller's workspace: ws_carve (fm_engine.cpp) names every region once, in layout order, with its size
struct Workspace {
    FmBatch b{};              // the destination-sorted edge layout (fm_k_batch_setup fills the arrays)
    float *s = nullptr, *v = nullptr, *xw = nullptr, *ef = nullptr, *Ps = nullptr, *Asd = nullptr, *PV = nullptr, *Psd = nullptr, *PVd = nullptr;
    float *part_s = nullptr, *part_v = nullptr, *s_tab_base = nullptr, *tap_s = nullptr, *tap_v = nullptr, *Q[2] = {nullptr, nullptr};
    fm_dst boot{};            // the bootstrap evaluation's endpoint prediction
    int* mol_gid = nullptr;   // [B] global molecule ids of the Philox noise streams
    int32_t* x1[3] = {nullptr, nullptr, nullptr};      // sampled endpoint tokens a, c, e of a step whose caller passes no fm_sampled
};

}  // namespace fmh
using namespace fmh;

struct fm_ctx {
    fm_config cfg{};
    std::string err;
    int V = 32, S = 256, F = 128, na = 0, nc = 0, ne = 0;
    int HX = 0, SD = 0, PVW = 48;     // use_dst_feats: destination vectors / scalars per message; width of the hoisted hidden-vector rows
    int n_cus = 256;          // compute units of the device (fm_create); read by plan_batch only
    ModelPlan mp{};           // the weight copies this model has (fm_create)
    const void *sc_node_W1q = nullptr, *sc_node_W2q = nullptr, *node_head_W1q = nullptr, *node_head_W2q = nullptr;      // quad-row packed copies for fm_k_mlp4
    float rbf_mu_step = 0.f, rbf_inv_sigma = 0.f;
    // ---- weights (one device arena)
    char* arena = nullptr; size_t arena_bytes = 0;
    const float *emb_a = nullptr, *emb_c = nullptr;
    MlpW node_embed{}, edge_embed{}, sc_node{}, sc_edge{}, node_head{}, edge_head{};
    const float *node_ln_g = nullptr, *node_ln_b = nullptr, *edge_ln_g = nullptr, *edge_ln_b = nullptr;
    const float *ef_tab = nullptr, *T1 = nullptr;          // (ne+1,128) each
    std::vector<ConvW> conv;
    std::vector<UpdW> upd;
    int tab_rows = 0;
    // ---- batch binding
    bool bound = false;
    BatchPlan plan{};         // the bound batch's launch choices (plan_batch)
    Workspace ws{};           // the bound batch's pointers into the caller's workspace (ws_carve)
    std::vector<int32_t> node_off_h;      // [B+1] host copy of ws.b.mol_node_off: what fm_pair_rmsd checks its molecule indices against
    float* s_tab = nullptr; size_t tab_slot_floats = 0;      // the current step's embedding table, one of the FM_TAB_SLOTS at ws.s_tab_base; floats per slot
    const int* tab_slot = nullptr;      // per-molecule time: the caller's device (n_mols) table slot of every molecule, counted from s_tab; null = one table (set with s_tab)
    // ---- pinned host staging of the per-molecule descriptor arrays (fm_batch_bind / fm_set_molecule_ids: 16 B per molecule).  The copies
    // read it asynchronously; `stage_ev` marks their completion, so the next writer waits for THAT event only (long complete by then) and
    // no entry point ever synchronises the stream.
    int32_t* stage = nullptr; size_t stage_cap = 0; hipEvent_t stage_ev = nullptr; bool stage_busy = false;
    // ---- taps / profiling
    std::map<std::string, void*> taps;
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;          // recycled timing events: creating a pair per launch made the host the bottleneck of a profiled step
    std::vector<ProfEvent> prof_events;
    std::vector<std::string> prof_names;
    std::map<std::string, std::pair<double, int64_t>> prof_acc;
};

namespace fmh {

inline int fail(fm_ctx* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define FM_HIP(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return fail((c), FM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

inline bool prec_two_plane(int p) { return p == FM_PREC_BF16X3 || p == FM_PREC_F16X3; }      // the modes whose node / EdgeUpdate kernels run split precision too
inline int pad8(int k) { return (k + 7) / 8 * 8; }
inline int pad16(int k) { return (k + 15) / 16 * 16; }
inline int ld_for(int k) { int ld = (k + 3) / 4 * 4; while (((ld / 4) & 1) == 0) ld += 4; return ld; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int pvw_of(int V, int HX) { return (pad8(V + 1 + HX + 4) + 8 + 15) / 16 * 16; }     // FmGvpTile::PVW
inline size_t lds_gvp_sp(int V, int TM, int npl = 2) {       // split-precision edge message: npl bf16 planes instead of the f32 scalar tile, gates inside Vh
    size_t fl = (size_t)TM * FM_LDP * npl / 2 + 3 * TM * (V + 4) + 3 * TM * (pvw_of(V, 0) + 4);
    return fl * 4 + (size_t)TM * 9 * 4;
}
inline size_t lds_gvp(int V, int TM, bool with_meta, int HX = 0) {
    size_t fl = (size_t)TM * FM_LDX + 3 * TM * (V + 4) + 3 * TM * (pvw_of(V, HX) + 4) + TM * FM_LDG;
    return fl * 4 + (with_meta ? (size_t)TM * 9 * 4 + 64 : 0);      // + one slot for the tile's smallest pair id (PQ instances)
}
inline size_t lds_mlp(int ldx, int ldh, int tm = FM_TM) { return ((size_t)tm * ldx + (size_t)tm * ldh) * 4 + 5 * (size_t)tm * 4; }
inline size_t lds_proj(int V, int tm = FM_TM) { return ((size_t)tm * 260 + 3 * (size_t)tm * (V + 4)) * 4; }
inline size_t lds_edge_upd(int TM) { return ((size_t)TM * 164 + TM * 132) * 4 + TM * 4 * 4 + 16; }
inline size_t lds_edge_upd_sp(int TM) { return (size_t)TM * 132 * 4 + (size_t)TM * 176 * 2 * 2 + TM * 3 * 4; }

inline int bound_check(fm_ctx* c, const char* fn, bool args_ok) {      // what every entry point on the bound batch refuses first; args_ok: no required pointer is null
    if (!c || !args_ok) return fail(c, FM_ERR_INVALID, "%s: null argument", fn);
    return c->bound ? FM_OK : fail(c, FM_ERR_STATE, "%s: no batch bound", fn);
}

// The categorical modalities of the bound batch, m = 0: atom types, 1: charges (both over the node rows), 2: bond orders (over the unordered pairs).  Every
// per-modality loop of the engine reads this table, and the kernels' own Fm*Mod structs are filled from it.
struct Modality {
    int rows, K;                    // rows of the batch, real categories (mask token = K)
    const int *off, *mol;           // [B+1] first row of every molecule, [rows] molecule of every row
    int32_t *tok, *x1;              // [rows] the state's tokens (null without a state), the workspace's endpoint-token buffer
};
inline Modality modality(const fm_ctx* c, int m, const fm_state* state = nullptr) {
    const FmBatch& b = c->ws.b;
    int32_t* const tok = !state ? nullptr : m == 0 ? state->a_t : m == 1 ? state->c_t : state->e_t;
    if (m == 2) return {b.U, c->ne, b.mol_pair_off, b.pair_mol, tok, c->ws.x1[2]};
    return {b.N, m == 0 ? c->na : c->nc, b.mol_node_off, b.node_mol, tok, c->ws.x1[m]};
}
template <class T> T pick3(int m, T a, T c, T e) { return m == 0 ? a : m == 1 ? c : e; }      // the a / c / e member of a struct that spells the modalities out

// ---------------------------------------------------------------------------------------- launch helper
inline int kid_of(fm_ctx* c, const char* name) {
    for (size_t i = 0; i < c->prof_names.size(); ++i) if (c->prof_names[i] == name) return (int)i;
    c->prof_names.push_back(name);
    return (int)c->prof_names.size() - 1;
}

struct Launch {
    fm_ctx* c; hipStream_t st; int rc = FM_OK;
    template <class K, class... Args>
    void operator()(const char* name, K kernel, dim3 grid, dim3 block, size_t shmem, Args... args) {
        if (rc != FM_OK || grid.x == 0) return;
        ProfEvent pe{};
        if (c->prof) {
            pe.kid = kid_of(c, name);
            auto take = [&](hipEvent_t& e) { if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); } else (void)hipEventCreate(&e); };
            take(pe.a); take(pe.b);
            (void)hipEventRecord(pe.a, st);
        }
        hipLaunchKernelGGL(kernel, grid, block, shmem, st, args...);
        hipError_t e = hipGetLastError();
        if (c->prof) { (void)hipEventRecord(pe.b, st); c->prof_events.push_back(pe); }
        if (e != hipSuccess) rc = fail(c, FM_ERR_HIP, "launch of %s failed: %s", name, hipGetErrorString(e));
    }
    void copy(void* dst, const void* src, size_t bytes) {
        if (rc != FM_OK || bytes == 0) return;
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) rc = fail(c, FM_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
    }
};

// The taps of one evaluation, resolved once: `on` is false when the evaluation takes none or none is registered (every production step), and then no name
// is built and no lookup made.  Indexed names are "<stem><i><suffix>" (conv0.s, upd1.ef).
struct Taps {
    Launch& L; bool on;
    void* find(const char* stem, int i = -1, const char* suffix = "") const {       // the registered destination of "<stem>" (i < 0) or "<stem><i><suffix>", or null
        if (!on) return nullptr;
        const auto it = L.c->taps.find(i < 0 ? std::string(stem) : stem + std::to_string(i) + suffix);
        return it == L.c->taps.end() ? nullptr : it->second;
    }
    void operator()(const void* src, size_t bytes, const char* stem, int i = -1, const char* suffix = "") const { if (void* d = find(stem, i, suffix)) L.copy(d, src, bytes); }
};

// ---------------------------------------------------------------------------------------- kernel instance lists
// A kernel family that needs more than the default dynamic LDS lists its compiled instances ONCE: {key the launcher selects it by, kernel, LDS bytes
// it is opted into}.  fm_create walks every list (opt_in); launchers launch only through a list (launch_inst), so an instance that is not listed cannot be
// launched, and a launch that asks for more LDS than its entry was opted into fails with FM_ERR_INVALID before it reaches HIP.
using InstKey = std::array<int, 5>;
template <class Fn> struct Inst { InstKey key; Fn fn; size_t lds; };
template <class Fn> struct InstList { const char* key_names; std::vector<Inst<Fn>> v; };      // key_names ("V, tile_node, ..."): for error messages

template <class Fn> void opt_in(const InstList<Fn>& list) {
    for (const Inst<Fn>& i : list.v) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(i.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)i.lds);
}

template <class Fn, class... Args>
void launch_inst(Launch& L, const InstList<Fn>& list, const InstKey& key, const char* name, dim3 grid, dim3 block, size_t lds, Args... args) {
    if (L.rc != FM_OK) return;
    for (const Inst<Fn>& i : list.v)
        if (i.key == key) {
            if (lds > i.lds) L.rc = fail(L.c, FM_ERR_INVALID, "launch of %s asks for %zu bytes of LDS, its instance is opted into %zu", name, lds, i.lds);
            else L(name, i.fn, grid, block, lds, args...);
            return;
        }
    char k[96]; int n = 0;
    for (int f = 0, nf = 1 + (int)std::count(list.key_names, list.key_names + strlen(list.key_names), ','); f < nf; ++f)
        n += snprintf(k + n, sizeof k - n, f ? ", %d" : "%d", key[f]);
    L.rc = fail(L.c, FM_ERR_INVALID, "no %s instance for (%s) = (%s)", name, list.key_names, k);
}

// fused gat step (fm_k_ctmc_gat_fused<NT>): no dynamic LDS; the workgroup size is BatchPlan::ctmc_threads
using GatFusedFn = decltype(&fm_k_ctmc_gat_fused<256>);
inline const InstList<GatFusedFn>& ctmc_gat_instances() {
    static const InstList<GatFusedFn> list{"ctmc_threads", {{{256}, fm_k_ctmc_gat_fused<256>, 0}, {{1024}, fm_k_ctmc_gat_fused<1024>, 0}}};
    return list;
}

// ---------------------------------------------------------------------------------------- launchers of the heavy kernel families (one translation unit each)
// Every launcher selects the instance from run-time parameters and reports an unsupported combination through L.rc; fm_opt_in_* walk the unit's instance
// lists (called once by fm_create).
void fm_launch_edge_message(Launch& L, int V, int TE, int HX, int precision, bool pq, dim3 grid, const FmMsgArgs& m);      // fm_tu_msg32.cpp / fm_tu_msg16.cpp
void fm_launch_edge_message_v32(Launch& L, int TE, int HX, int precision, bool pq, dim3 grid, const FmMsgArgs& m);
void fm_launch_edge_message_v16(Launch& L, int TE, int HX, int precision, bool pq, dim3 grid, const FmMsgArgs& m);
void fm_opt_in_msg_v32(); void fm_opt_in_msg_v16();
// node kernels (fm_tu_node.cpp): narrow = LayerNorm statistics over a real width < 256; sp = 0 | 1 (bf16x3) | 3 (f16x3); rg = 0 | 1 | 2 | 3 | 5 (4 rg nodes per tile)
void fm_launch_node_update(Launch& L, int V, int TN, bool narrow, int sp, int rg, dim3 grid, size_t lds, const FmNodeUpdArgs& nu);
void fm_launch_pos_update(Launch& L, int V, int TN, dim3 grid, const FmPosArgs& pp);
void fm_launch_dst_proj(Launch& L, int V, int TN, int HX, dim3 grid, const FmDstProjArgs& dp);
void fm_opt_in_node();

}  // namespace fmh
