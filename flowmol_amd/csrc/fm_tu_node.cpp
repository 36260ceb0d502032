// Translation unit of the node-kernel instances: fm_k_node_update<V, TN, NARROW, SP, RG> (V = 16 | 32; TN = 16 | 32 | 64 rows; NARROW: LayerNorm statistics over
// a real width < 256; SP = 1 | 3: the split-precision instances (16 / 32 rows); RG = 1 | 2 | 3 (16-row frame) | 5 (32-row frame): 4 RG nodes per workgroup),
// fm_k_pos_update<V, TN> (unfused sequence), fm_k_dst_proj<V, TN, V / 4> (use_dst_feats).  Compiled in parallel with the other units (fm_host.h).
#include "fm_host.h"

namespace fmh {

using NodeFn = decltype(&fm_k_node_update<32, 32, false, 0>);
template <int V, int TN, bool NARROW, int SP, int RG = 0> Inst<NodeFn> node_inst() {
    return {{V, TN, NARROW, SP, RG}, fm_k_node_update<V, TN, NARROW, SP, RG>, SP ? lds_gvp_sp(V, TN) : lds_gvp(V, TN, false)};
}
template <int... Vs> InstList<NodeFn> node_update_list() {
    return {"V, tile_node, narrow, split, nodes_per_tile / 4", {
        node_inst<Vs, 16, false, 0>()..., node_inst<Vs, 16, true, 0>()..., node_inst<Vs, 32, false, 0>()..., node_inst<Vs, 32, true, 0>()...,
        node_inst<Vs, 64, false, 0>()..., node_inst<Vs, 64, true, 0>()...,
        node_inst<Vs, 16, true, 1>()..., node_inst<Vs, 16, true, 3>()..., node_inst<Vs, 32, true, 1>()..., node_inst<Vs, 32, true, 3>()...,
        // 4 RG-node instances (fm_wave_gemm4: the regular tiles' summation order)
        node_inst<Vs, 16, false, 0, 1>()..., node_inst<Vs, 16, false, 0, 2>()..., node_inst<Vs, 16, false, 0, 3>()..., node_inst<Vs, 32, false, 0, 5>()...}};
}
const InstList<NodeFn>& node_update_instances() { static const auto list = node_update_list<32, 16>(); return list; }

using PosFn = decltype(&fm_k_pos_update<32, 32>);
template <int V, int TN> Inst<PosFn> pos_inst() { return {{V, TN}, fm_k_pos_update<V, TN>, lds_gvp(V, TN, false)}; }
template <int... Vs> InstList<PosFn> pos_update_list() { return {"V, tile_node", {pos_inst<Vs, 16>()..., pos_inst<Vs, 32>()..., pos_inst<Vs, 64>()...}}; }
const InstList<PosFn>& pos_update_instances() { static const auto list = pos_update_list<32, 16>(); return list; }

using DstProjFn = decltype(&fm_k_dst_proj<32, 32, 8>);
template <int V, int TN, int HX> Inst<DstProjFn> dst_proj_inst() { return {{V, TN, HX}, fm_k_dst_proj<V, TN, HX>, lds_gvp(V, TN, false)}; }
template <int... Vs> InstList<DstProjFn> dst_proj_list() { return {"V, tile_node, dst_vectors", {dst_proj_inst<Vs, 16, Vs / 4>()..., dst_proj_inst<Vs, 32, Vs / 4>()...}}; }
const InstList<DstProjFn>& dst_proj_instances() { static const auto list = dst_proj_list<32, 16>(); return list; }

void fm_launch_node_update(Launch& L, int V, int TN, bool narrow, int sp, int rg, dim3 grid, size_t lds, const FmNodeUpdArgs& nu) {
    launch_inst(L, node_update_instances(), {V, TN, narrow, sp, rg}, "node_update", grid, dim3(FM_THREADS), lds, nu);
}
void fm_launch_pos_update(Launch& L, int V, int TN, dim3 grid, const FmPosArgs& pp) {
    launch_inst(L, pos_update_instances(), {V, TN}, "pos_update", grid, dim3(FM_THREADS), lds_gvp(V, TN, false), pp);
}
void fm_launch_dst_proj(Launch& L, int V, int TN, int HX, dim3 grid, const FmDstProjArgs& dp) {
    launch_inst(L, dst_proj_instances(), {V, TN, HX}, "dst_proj", grid, dim3(FM_THREADS), lds_gvp(V, TN, false), dp);
}
void fm_opt_in_node() { opt_in(node_update_instances()); opt_in(pos_update_instances()); opt_in(dst_proj_instances()); }

}  // namespace fmh
