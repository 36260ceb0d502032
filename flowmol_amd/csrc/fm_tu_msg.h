// The edge-message instances of ONE vector width (FM_TU_V = 32 | 16): included by fm_tu_msg32.cpp / fm_tu_msg16.cpp, which are compiled in parallel with the
// other translation units of the library (fm_host.h).  fm_k_edge_message<V, TE, 512, HX, SP, PQ>: TE = 16 | 32 | 64 rows; SP = 0 f32, 1 bf16x3, 2 bf16x6
// (16 / 32 rows), 3 f16x3; PQ = 1 the pair-slab instance (f32); HX = V / 4 destination-feature vectors (f32, 16 / 32 rows).
#pragma once
#include "fm_host.h"

namespace fmh {

using MsgFn = decltype(&fm_k_edge_message<32, 32, 512, 0, 0>);
inline size_t lds_msg(int V, int TE, int HX, int SP) { return SP ? lds_gvp_sp(V, TE, SP == 2 ? 3 : 2) : lds_gvp(V, TE, true, HX); }
template <int V, int TE, int HX, int SP, int PQ = 0> Inst<MsgFn> msg_inst() { return {{TE, HX, SP, PQ}, fm_k_edge_message<V, TE, 512, HX, SP, PQ>, lds_msg(V, TE, HX, SP)}; }

template <int V>
const InstList<MsgFn>& msg_instances() {
    constexpr int HXV = V / 4;
    static const InstList<MsgFn> list{"tile_edge, dst_vectors, split, pair_slab", {
        msg_inst<V, 16, 0, 0>(), msg_inst<V, 16, 0, 0, 1>(), msg_inst<V, 16, 0, 1>(), msg_inst<V, 16, 0, 3>(), msg_inst<V, 16, 0, 2>(), msg_inst<V, 16, HXV, 0>(),
        msg_inst<V, 32, 0, 0>(), msg_inst<V, 32, 0, 0, 1>(), msg_inst<V, 32, 0, 1>(), msg_inst<V, 32, 0, 3>(), msg_inst<V, 32, 0, 2>(), msg_inst<V, 32, HXV, 0>(),
        msg_inst<V, 64, 0, 0>(), msg_inst<V, 64, 0, 0, 1>(), msg_inst<V, 64, 0, 1>(), msg_inst<V, 64, 0, 3>()}};
    return list;
}

template <int V>
void fm_launch_edge_message_v(Launch& L, int TE, int HX, int precision, bool pq, dim3 grid, const FmMsgArgs& m) {
    const int sp = precision == FM_PREC_BF16X3 ? 1 : precision == FM_PREC_BF16X6 ? 2 : precision == FM_PREC_F16X3 ? 3 : 0;
    if (sp == 2 && TE > 32 && L.rc == FM_OK) {
        L.rc = fail(L.c, FM_ERR_INVALID, "the three-term split precision runs 16- or 32-row edge tiles (three planes of a 64-row tile exceed the LDS)");
        return;
    }
    launch_inst(L, msg_instances<V>(), {TE, HX, sp, pq}, pq ? "edge_message_pq" : "edge_message", grid, dim3(512), lds_msg(V, TE, HX, sp), m);
}

}  // namespace fmh
