/* C ABI of libflowmol_hip.so -- the MI355X-native replacement for the FlowMol3 sampling hot path.
 *
 * The reference (Dunni3/FlowMol) is pure Python and has NO FFI; this header declares the boundary a
 * maintainer would bind with ctypes (INTEGRATION.md shows the stub).  Each entry point cites the
 * reference code it replaces (paths are into the reference tree):
 *
 *   fm_create           weights of flowmol/models/ctmc_vector_field.py:CTMCVectorField (state-dict keys
 *                       "vector_field.*"), repacked for MFMA
 *   fm_batch_bind       graph batching: flowmol/models/flowmol.py:509-529 (dgl.graph/dgl.batch),
 *                       flowmol/data_processing/utils.py:4-46 (edge list, upper-edge mask, batch idxs)
 *   fm_forward          EndpointVectorField.forward, flowmol/models/vector_field.py:212-369
 *                       (incl. GVPConv gvp.py:435-543, NodePositionUpdate/EdgeUpdate vector_field.py:813-880,
 *                       SelfConditioningResidualLayer self_conditioning.py:37-85)
 *   fm_ctmc_step        the part of CTMCVectorField.step after the network evaluation,
 *                       ctmc_vector_field.py:328-411 + campbell_step :414-461 + purity_sampling ctmc_utils.py:4-34
 *   fm_integrate        CTMCVectorField.integrate, ctmc_vector_field.py:145-285
 *   fm_forward_mixed    the same forward with the reference's per-graph time: t of shape (B,), vector_field.py:212-243 (t[node_batch_idx])
 *   fm_integrate_mixed  CTMCVectorField.integrate for a batch whose molecules follow different schedules (no reference counterpart: its integrate
 *                       takes one tspan; what a molecule computes is its own integrate call)
 *   fm_prior_philox_dense   the categorical priors of flowmol/data_processing/priors.py:8-107 as FlowMol.sample_prior draws them
 *                       (flowmol/models/flowmol.py:417-448), from per-molecule counter-based streams instead of the CPU generator
 *   fm_philox_tape      the draws of CTMCVectorField.step's torch.multinomial / torch.rand calls (ctmc_vector_field.py:349-357,
 *                       373-388, 414-510) as the in-kernel noise mode makes them, materialised in the reference's shapes
 *   fm_conditional_path CTMCVectorField.sample_conditional_path, ctmc_vector_field.py:97-143: g_t ~ p(g_t | g_0, g_1) for given molecules g_1 at a
 *                       per-graph time, with x_0 and the uniforms from the per-molecule counter-based streams instead of torch's generator
 *   fm_denoising_loss   the part of FlowMol.forward after sample_conditional_path, flowmol/models/flowmol.py:339-413: one evaluation on logits
 *                       (vector_field.py:217 apply_softmax=False, remove_com=False), CrossEntropyLoss / MSELoss row terms, per-molecule sums
 *   fm_distort_philox   the geometry distortion of FlowMol.forward, flowmol.py:333-337, from the per-molecule counter-based streams
 *   fm_ctmc_step_inpaint, fm_integrate_inpaint   fm_ctmc_step / fm_integrate / fm_integrate_mixed with frozen atoms (replacement conditioning; no reference entry
 *                       point): after every step the kept rows are put back onto sample_conditional_path (ctmc_vector_field.py:97-143) of the given molecule
 *   fm_ot_align         the coupling of the position prior to a data sample that every shipped training config switches on (prior_config.x.align: True):
 *                       flowmol/data_processing/priors.py:109-169 align_prior(permutation=True, rigid_body=True) -- scipy's linear_sum_assignment on
 *                       torch.cdist(x_1, x_0), then rigid_alignment, Kabsch without a determinant correction -- as coupled_node_prior :267-303 calls it
 *                       for every sample of the training and validation loaders
 *   fm_conditional_path_x0   fm_conditional_path on a caller-supplied position prior (the coupled one): flowmol.py:316-324 interpolates from the dataset's x_0
 *
 * Conventions
 *   - every function returns 0 on success or a negative fm_status; the message is available from
 *     fm_last_error(ctx) (ctx may be NULL for errors of fm_create).  Nothing throws across the ABI.
 *   - all tensor arguments are DEVICE pointers to caller-owned memory (torch tensors passed as
 *     data_ptr()); the library never frees caller memory.  After fm_create the library allocates
 *     no DEVICE memory: per-batch scratch lives in the caller-provided workspace of fm_batch_bind.
 *     (Host side: one pinned staging buffer of 16 bytes per molecule for the descriptor arrays of
 *     fm_batch_bind / fm_set_molecule_ids, grown on demand.)
 *   - kernels are enqueued on the hipStream_t passed in (as void*); no call synchronises the stream
 *     or the device.  fm_batch_bind / fm_set_molecule_ids copy their host arrays through the pinned
 *     staging buffer and wait (on an event) only for the copies of the PREVIOUS such call, which
 *     have completed long before in any realistic call sequence; they are setup calls and, because
 *     of that event wait, must stay outside a stream capture.
 *   - the library reads no environment variables; every switch is a field of fm_config.
 *   - a context is bound to the device current at fm_create and is not thread-safe.
 *   - categorical state is exchanged as int32 token indices (mask token = number of real categories);
 *     edge state is per UNORDERED pair in the reference's upper-triangle order
 *     (torch.triu_indices(n,n,1) row-major per molecule, molecules concatenated) -- both directed
 *     edges of a pair always carry the same token in the reference (ctmc_vector_field.py:397-409).
 *   - probabilities ("dst") are float32: x (N,3), a (N,n_atom_types), c (N,n_charges), e (U,n_bond_types).
 */
#ifndef FLOWMOL_HIP_H
#define FLOWMOL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_ABI_VERSION 16
#define FM_MAX_CONVS 16

typedef enum fm_status {
    FM_OK = 0,
    FM_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    FM_ERR_WEIGHTS = -2,      /* missing tensor or wrong shape */
    FM_ERR_HIP = -3,          /* a HIP runtime call or kernel launch failed */
    FM_ERR_STATE = -4,        /* call order (no batch bound, ...) */
    FM_ERR_NOMEM = -5
} fm_status;

typedef struct fm_ctx fm_ctx;

/* mirrors flowmol_amd.config.VFConfig (the reference's vector_field: YAML block) */
typedef struct fm_config {
    int32_t abi_version;          /* FM_ABI_VERSION */
    int32_t n_atom_types;         /* real atom categories incl. the fake-atom type, excl. mask */
    int32_t n_charges;
    int32_t n_bond_types;
    int32_t n_vec_channels;       /* 16 or 32 */
    int32_t n_hidden_scalars;     /* power of two, 8..256 (flowmol3: 256, configs/dev.yml: 64); narrower models run on zero-padded 256-column tiles */
    int32_t n_hidden_edge_feats;  /* power of two, 8..128 (flowmol3: 128, dev.yml: 64) */
    int32_t rbf_dim;              /* 32 */
    int32_t n_convs;
    int32_t n_updaters;
    int32_t update_after[FM_MAX_CONVS];   /* updater index run after conv i, or -1 (vector_field.py:320-326) */
    int32_t self_conditioning;
    int32_t time_embedding_dim;   /* 1 = raw t */
    int32_t a_token_dim, c_token_dim, e_token_dim;   /* 0 = one-hot input */
    float rbf_dmax;
    float msg_z;                  /* divisor of the aggregated messages (1 for message_norm 'sum'); < 0: message_norm 'mean' -- every node's
                                   * sum is divided by its in-degree n_i - 1 (DGL fn.mean, gvp.py:401-404; 0 for a 1-atom molecule) */
    /* --- ABI 3: use_dst_feats (flowmol/models/gvp.py:300-316,472-473,527-537): widths of the projected destination-node
     * features that join every message's inputs; 0 / 0 = off */
    int32_t s_dst_feats;          /* int(n_hidden_scalars / dst_feat_msg_reduction_factor) */
    int32_t v_dst_feats;          /* int(n_vec_channels / dst_feat_msg_reduction_factor), <= 8 */
    /* --- ABI 3: 1 = CTMC model (categorical inputs are tokens with a mask state, CTMCVectorField); 0 = endpoint-parameterised model
     * (EndpointVectorField, flowmol/models/vector_field.py:15-211: categorical inputs are continuous (rows, n) vectors, token dims 0) */
    int32_t has_mask;
    /* --- ABI 3: arithmetic of the edge-message GEMMs.  FM_PREC_F32 (default): exact f32 MFMAs, the reference's arithmetic.
     * FM_PREC_BF16X3: OPT-IN split precision -- the scalar and gate GEMMs of GVPConv.message run on the bf16 matrix cores with every
     * f32 operand carried as hi + lo bf16 and three products per term (~2^-17 relative per product instead of 2^-24).  Not f32
     * arithmetic: per-stage errors are ~10x larger; meant for throughput runs, never for parity claims.
     * FM_PREC_BF16X6 (round 5, OPT-IN, edge-message kernel only; node kernels and EdgeUpdate stay f32): three-term split -- hi + mid + lo bf16 = all 24
     * mantissa bits, six products per term, dropped products <= 3 * 2^-24 relative: f32-class accuracy on the bf16 matrix cores at the price of 6-byte
     * operands (weight stream, LDS).  Measured (profiles/r05c_*): every stage within 1.32x the f32 kernels' error against float64,
     * 71 molecules/s at C3 (f32: 63): three planes leave room for ONE workgroup per CU.  A separately reported mode like FM_PREC_BF16X3.
     * FM_PREC_F16X3 (round 5, OPT-IN): FM_PREC_BF16X3's kernels with IEEE-half planes -- hi + lo half = 22 of f32's 24 mantissa bits in the same 4 bytes per
     * element and the same three products (v_mfma_f32_16x16x32_f16).  RANGE is the price: |activations| beyond 65504 are clamped (a finite, wrong result). */
    int32_t precision;
    /* --- ABI 4: remaining architecture switches of EndpointVectorField.__init__ that no shipped YAML enables */
    int32_t n_recycles;           /* vector_field.py:307: the conv / update stack runs n_recycles times over the same weights (0 or 1 = once) */
    int32_t edge_update_no_distance;   /* 1 = update_edge_w_distance False: EdgeUpdate's first Linear has no rbf(d) columns (vector_field.py:851-853,876-877) */
    /* --- ABI 5: launch-tuning overrides -- 0 = automatic for every one of them (what the product always passes).  They exist for the
     * A/B measurements under profiles/ and for the parity tests that run every tile size; up to ABI 4 they were environment variables
     * read inside fm_create, which hid them from the interface.  The library reads NO environment variable. */
    int32_t tile_edge;            /* rows per workgroup tile of the edge kernels: 0 = per batch (the cheaper of 16 / 32 by a rounds-per-CU model: 16 for a few molecules, 32 for large batches; same bits) | 16 | 32 | 64 */
    int32_t tile_node;            /* same for the node kernels; additionally 4 | 8 | 12 (nodes per workgroup in the 16-row frame) | 20 (in the 32-row frame), scalar GEMMs
                                   * on v_mfma_f32_4x4x1: the automatic choice is the smallest of 4 / 8 / 12 / 16 / 20 whose tiles fit one per CU */
    int32_t tile_edge_update;     /* EdgeUpdate tile: 0 = 32 | 32 | 64 */
    int32_t xcd_swizzle;          /* edge-message tile -> workgroup map: 0 / 1 = one contiguous tile range per XCD | -1 = identity */
    int32_t fuse_node;            /* 0 / 1 = node_update also runs the next conv's projections + NodePositionUpdate, and the last EdgeUpdate the edge output head
                                     | 2 = the node fusion only (edge head as a kernel of its own) | -1 = separate launches */
    int32_t pair_mlps;            /* node-side and pair-side MLPs of a stage in ONE launch: 0 = while the pair tiles do not fill the chip | 1 always | -1 never */
    int32_t mlp_small_tiles;      /* 16-row tiles for the MLP kernels: 0 = while they do not fill the chip (and 4-row NODE tiles, fm_k_mlp4, while those fit one per CU)
                                     | 1 always 16 rows | -1 never | 2 = 16-row pair tiles + 4-row node tiles whatever the batch */
    /* --- ABI 6 */
    int32_t pair_slab;            /* [rbf | ef] slab of the first edge GVP once per unordered pair for the convolutions before the first molecule
                                   * update (pair-symmetric inputs; self-conditioned f32 models without destination features): 0 = in evaluations
                                   * whose pair tiles fill the chip (canonical mode: in every one) | 1 = in every self-conditioned evaluation | -1 = off */
    /* --- ABI 7: canonical arithmetic.  In the reference a molecule's result is a function of the molecule and its noise rows only -- every reduction is per
     * molecule (flowmol/models/gvp.py:491-492, flowmol/utils/ctmc_utils.py:11-20, flowmol/models/vector_field.py:347-350).  0 / 1 (default): the library gives the
     * same guarantee BIT FOR BIT: the f32 summation order of everything computed for a molecule depends on the molecule alone -- edge-message tiles start at the
     * molecule's first edge row and in-edges are summed in 16-row chunks counted from it, LayerNorm statistics and gate sums have one order for every tile
     * height, the 4-row instances of the node kernels (small batches) run the regular tiles' fma chains, and the one launch choice that selects another order
     * (pair slab on / off) is fixed instead of following the batch size.  A molecule alone, inside a 1024-batch, in any shard of it and on 1 or 8 GPUs gives
     * identical coordinates and tokens for identical noise.  Holds for every automatic tile height and across explicit tile_edge 16 | 32, tile_node 4 .. 32,
     * mlp_small_tiles; 64-row tiles, pair_slab -1 and fuse_node 2 | -1 (the edge head as a kernel of its own, also taken by batches with a molecule of >= 2048
     * atoms) are other (self-consistent) orders.
     * -1: the pair slab follows the batch size (round 5's rule); results then agree between differently composed batches to f32 summation order only.  (Up to
     * round 5 this was a "latency mode" with its own 4-row kernels; since the 4-row kernels are canonical it gains nothing measurable: one molecule 0.55 vs 0.56 ms.) */
    int32_t canonical;
    /* --- ABI 8: workgroup size of the fused CTMC kernels (campbell and gat): 0 = per batch (1024 for a few molecules or a very large one, else 256) | 256 | 1024.
     * Same bits either way (per-row decisions, integer counts); exists for the parity tests that run both instances on small batches. */
    int32_t ctmc_threads;
} fm_config;

enum fm_precision { FM_PREC_F32 = 0, FM_PREC_BF16X3 = 1, FM_PREC_BF16X6 = 2, FM_PREC_F16X3 = 3 };

/* one tensor of the reference state dict inside the host weight blob */
typedef struct fm_tensor_desc {
    const char* name;             /* reference state-dict key without the "vector_field." prefix */
    int64_t offset;               /* in floats from the start of the blob */
    int32_t ndim;
    int64_t shape[2];
} fm_tensor_desc;

typedef struct fm_dst {           /* endpoint prediction ("dst_dict" of the reference) */
    float* x;                     /* (N,3) */
    float* a;                     /* (N,n_atom_types) probabilities */
    float* c;                     /* (N,n_charges) */
    float* e;                     /* (U,n_bond_types) */
} fm_dst;

typedef struct fm_state {         /* g.ndata['x_t','a_t','c_t'], g.edata['e_t'] of the reference */
    float* x_t;                   /* (N,3) */
    int32_t* a_t;                 /* (N) */
    int32_t* c_t;                 /* (N) */
    int32_t* e_t;                 /* (U) */
} fm_state;

typedef struct fm_dense_state {   /* endpoint-parameterised models: g.ndata['x_t','a_t','c_t'], g.edata['e_t'][upper] as float features */
    float* x_t;                   /* (N,3) */
    float* a_t;                   /* (N,n_atom_types) */
    float* c_t;                   /* (N,n_charges) */
    float* e_t;                   /* (U,n_bond_types), per unordered pair */
} fm_dense_state;

typedef struct fm_endpoint_scalars {   /* EndpointVectorField.step, vector_field.py:501-564, host-computed in float32 */
    float dt;                     /* s_i - t_i */
    float coef[4];                /* x, a, c, e: alpha'/(1 - alpha) */
    float scale;                  /* inv_temp_func(t_i): 1, or continuous_inv_temp_max * (1 - t_i) */
} fm_endpoint_scalars;

typedef struct fm_step_noise {    /* draws of one CTMC step, in the reference's order and shapes */
    const float* q_a;  const float* u1_a;  const float* u2_a;    /* (N,na) Exp(1), (N) U, (N) U */
    const float* q_c;  const float* u1_c;  const float* u2_c;
    const float* q_e;  const float* u1_e;  const float* u2_e;    /* (U,ne), (U), (U) */
    /* dfm_type FM_DFM_GAT: one Categorical draw per modality over K+1 classes (mask included), so q_* are
     * (rows, K+1) and u1_*, u2_* are unused (may be NULL) */
} fm_step_noise;

enum fm_dfm_type { FM_DFM_CAMPBELL = 0, FM_DFM_GAT = 1 };   /* reference ctmc_vector_field.py:357 / :373 */

typedef struct fm_step_scalars {  /* host-computed with the reference's float32 arithmetic */
    float t;                      /* t_i */
    float dt;                     /* s_i - t_i */
    float x_coef;                 /* alpha'_x / (1 - alpha_x) */
    float unmask_prob[3];         /* a, c, e: clamp(dt*(alpha' + eta*alpha)/(1-alpha), 0, 1) */
    float mask_prob[3];           /* clamp(dt*eta, 0, 1) */
    float hc_thresh;              /* purity threshold; 0 = uniform unmasking branch */
    float cat_temperature;        /* cat_temp_func(t_i): 0.05 by default, or the 'decay' schedule */
    int32_t last_step;
    /* --- ABI 2 */
    float x_scale;                /* inv_temp_func(t_i) of the reference's step(): x_t += (dt*vf)*x_scale; 1 by default */
    int32_t dfm_type;             /* fm_dfm_type */
    float gat_cf[3];              /* a, c, e: alpha'/(1 - alpha)        (gat_step, ctmc_vector_field.py:481) */
    float gat_cb[3];              /* a, c, e: alpha'/(alpha + 1e-8)     (:488) */
    float gat_fw, gat_bw;         /* forward_weight_func(t_i) and forward_weight - 1 (:491-492) */
    /* --- ABI 3: noise source of this step (campbell; since ABI 8 also gat).  FM_NOISE_TENSORS: the caller's fm_step_noise (the reference's draws,
     * bit-exact parity mode).  FM_NOISE_PHILOX: drawn inside the kernel from Philox4x32-10 streams keyed by (philox_seed, global
     * molecule id, step_index, modality, row) -- no noise tensors, and a molecule's trajectory does not depend on how the
     * batch is sharded; fm_step_noise may then be NULL.  A gat step with FM_NOISE_PHILOX is ONE launch (Euler step, the three
     * modalities, trajectory frames) instead of four; its K+1 Exp(1) draws per row are draws 0..K of the row's stream (fm_philox_tape writes them out) */
    int32_t noise_mode;
    int32_t step_index;
    uint32_t philox_seed_lo, philox_seed_hi;
} fm_step_scalars;

enum fm_noise_mode { FM_NOISE_TENSORS = 0, FM_NOISE_PHILOX = 1 };

typedef struct fm_sampled {       /* sampled endpoint tokens of a step ("*_1_pred"), optional (may be NULL) */
    int32_t* a1; int32_t* c1; int32_t* e1;
} fm_sampled;

typedef struct fm_traj_sink {     /* optional per-step frames (xt_traj / ep_traj); any pointer may be NULL */
    float* x;  int32_t* a;  int32_t* c;  int32_t* e;             /* (n_steps, ...) state after each step */
    float* x1; int32_t* a1; int32_t* c1; int32_t* e1;            /* (n_steps, ...) endpoint predictions */
} fm_traj_sink;

/* --- ABI 8: categorical priors of the endpoint-parameterised models, one fm_prior_mod per modality (a, c, e).  Replaces the prior functions of
 * flowmol/data_processing/priors.py as flowmol/models/flowmol.py:417-448 (FlowMol.sample_prior) calls them; the fields are their keyword arguments. */
enum fm_prior_kind {
    FM_PRIOR_GAUSSIAN = 0,        /* priors.py:8-13   gaussian: randn * std (+ 1/d when simplex_center) */
    FM_PRIOR_UNIFORM_SIMPLEX = 1, /* priors.py:15-22  Exp(1) draws over their row sum */
    FM_PRIOR_BARYCENTER = 2,      /* priors.py:36-44  1/d; blur != 0: simplex projection (flowmol/utils/dirflow.py:35-49) of 1/d + randn * blur */
    FM_PRIOR_BIASED_SIMPLEX = 3,  /* priors.py:47-56  softmax((mu + randn * std) / (1/d)), mu = vertex_prob at vertex_idx, (1 - vertex_prob)/(d - 1) elsewhere */
    FM_PRIOR_MARGINAL = 4,        /* priors.py:67-79  one-hot of a draw from p; has_blur: softmax((one_hot + randn * blur) / (1/d)) */
    FM_PRIOR_C_GIVEN_A = 5        /* priors.py:81-98  the same with p = p_c_given_a[argmax of the node's atom-type prior]; modality c only */
};
typedef struct fm_prior_mod {
    int32_t kind;                 /* fm_prior_kind */
    float std;
    int32_t simplex_center;
    float blur;
    int32_t has_blur;             /* marginal / c-given-a: blur given (the reference tests `blur is not None`) */
    float vertex_prob;
    int32_t vertex_idx;
    const float* p;               /* DEVICE: marginal p (d) | c-given-a p_c_given_a (n_atom_types, d); else NULL */
} fm_prior_mod;
typedef struct fm_prior_spec { fm_prior_mod mod[3]; } fm_prior_spec;      /* a, c, e */

const char* fm_last_error(const fm_ctx* ctx);
int fm_abi_version(void);

int fm_create(const fm_config* cfg, const fm_tensor_desc* tensors, int n_tensors, const float* host_blob,
              fm_ctx** out);
int fm_destroy(fm_ctx* ctx);

/* bytes of caller-provided device workspace needed for a batch of molecules with the given sizes */
int fm_workspace_bytes(fm_ctx* ctx, const int32_t* n_atoms_host, int n_mols, size_t* bytes);
/* bind a batch: builds the internal destination-sorted edge layout inside `workspace` */
int fm_batch_bind(fm_ctx* ctx, void* stream, const int32_t* n_atoms_host, int n_mols, void* workspace, size_t bytes);

/* x -= per-molecule mean, in place, for the bound batch: the centring step of the position prior
 * (centered_normal_prior_batched_graph, flowmol/data_processing/priors.py:27-35) */
int fm_remove_com(fm_ctx* ctx, void* stream, float* x);

/* Philox mode: global ids of the bound batch's molecules (host array of n_mols; NULL = 0..n_mols-1, the default after
 * fm_batch_bind), and the position prior x0 ~ N(0, I) - per-molecule mean (priors.py:27-35) drawn from the same streams */
int fm_set_molecule_ids(fm_ctx* ctx, void* stream, const int32_t* ids_host);
int fm_prior_philox(fm_ctx* ctx, void* stream, uint64_t seed, float* x0);

/* Philox mode of the endpoint-parameterised models (has_mask == 0): the whole prior of the bound batch in one launch -- out->x_t = fm_prior_philox's
 * bits, out->a_t / c_t / e_t (e per unordered pair) = the categorical priors of `spec` (priors.py:8-107 through flowmol.py:417-448), every row from the
 * stream (global molecule id, row inside the molecule): normals and Exp(1) draws as laid out in csrc/fm_device.h (fm_philox4x32) and DESIGN.md section 6. */
int fm_prior_philox_dense(fm_ctx* ctx, void* stream, uint64_t seed, const fm_prior_spec* spec, const fm_dense_state* out);

/* one network evaluation.  temb: device (time_embedding_dim) floats (raw t when dim == 1).
 * prev: previous endpoint for self-conditioning or NULL.  bootstrap != 0 reproduces the reference's
 * first-step behaviour (vector_field.py:269-282): an extra evaluation with remove_com=False whose
 * result is used as `prev`.  out.a/c/e receive softmax probabilities, out.x is COM-free iff remove_com. */
int fm_forward(fm_ctx* ctx, void* stream, const fm_state* state, const float* temb, const fm_dst* prev,
               int bootstrap, int remove_com, const fm_dst* out);

/* Endpoint-parameterised models (has_mask == 0): one network evaluation on continuous categorical features (no self-conditioning),
 * and the Euler step of all four modalities  x_s = x_t + ((coef * (x_1 - x_t)) * scale) * dt  given the endpoint prediction `dst`
 * (EndpointVectorField.forward / .step, flowmol/models/vector_field.py:212-293, 501-564). */
int fm_forward_dense(fm_ctx* ctx, void* stream, const fm_dense_state* state, const float* temb, int remove_com, const fm_dst* out);
int fm_endpoint_step(fm_ctx* ctx, void* stream, const fm_dense_state* state, const fm_dst* dst, const fm_endpoint_scalars* sc);

/* Euler step for x and the CTMC update of a, c, e given the endpoint prediction `dst` */
int fm_ctmc_step(fm_ctx* ctx, void* stream, const fm_state* state, const fm_dst* dst,
                 const fm_step_noise* noise, const fm_step_scalars* sc, const fm_sampled* sampled);

/* Noise tape: the draws a FM_NOISE_PHILOX step with these scalars (philox seed, step_index, dfm_type) consumes for the bound batch, written to the
 * caller's tensors `out` in the reference's shapes and order (ctmc_vector_field.py:349-357 campbell: q (rows,K), u1, u2 (rows); :373-388 gat: q (rows,K+1);
 * u1 / u2 pointers may be NULL).  Same device functions and counters as the kernels: fm_ctmc_step with FM_NOISE_TENSORS and this tape gives the
 * FM_NOISE_PHILOX step's bits, and the reference's integrate fed with it replays the run. */
int fm_philox_tape(fm_ctx* ctx, void* stream, const fm_step_scalars* sc, const fm_step_noise* out);

/* n_steps Euler/CTMC steps: per step fm_forward (+bootstrap on step 0 for self-conditioned models when
 * steps[0].t == 0) then fm_ctmc_step.  temb: device (n_steps, time_embedding_dim); noise: host array of
 * n_steps fm_step_noise (device pointers); prev0: endpoint of the step before the first one (NULL at the
 * start of a trajectory; dst_a or dst_b when a trajectory is integrated in several calls);
 * dst_a/dst_b: two caller-provided endpoint buffers used alternately (the one holding the final
 * prediction is returned in *final_dst, 0 or 1). */
int fm_integrate(fm_ctx* ctx, void* stream, const fm_state* state, int n_steps, const fm_step_scalars* steps,
                 const float* temb, const fm_step_noise* noise, const fm_dst* prev0, const fm_dst* dst_a,
                 const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst);

/* --- ABI 9: per-molecule time.  The molecules of the bound batch belong to n_groups <= 32 groups (mol_group: DEVICE (n_mols) int32, values in
 * [0, n_groups)); every group has its own time.  Time enters the network through the (atom type, charge) embedding table only, so group g's molecules
 * read the table built from row g of temb, and everything else is the arithmetic of fm_forward / fm_integrate: with canonical arithmetic and Philox
 * noise a molecule's bits are those of the molecule run alone on its own schedule.  CTMC models (has_mask) only: endpoint models return FM_ERR_INVALID,
 * as does n_groups > 32.  Neither call synchronises the stream or allocates device memory; workspace sizes are those of the existing calls.
 *
 * fm_forward_mixed: one evaluation; temb: device (n_groups, time_embedding_dim); prev / bootstrap / remove_com / out as in fm_forward. */
int fm_forward_mixed(fm_ctx* ctx, void* stream, const fm_state* state, const float* temb, int n_groups, const int32_t* mol_group,
                     const fm_dst* prev, int bootstrap, int remove_com, const fm_dst* out);

/* fm_integrate_mixed: n_steps steps; at call-step k group g takes the campbell step steps[k * n_groups + g] (its own t, dt, coefficients, last_step,
 * Philox step_index and seed) when active[k * n_groups + g] != 0, and is skipped otherwise: the state rows of its molecules stay bit-unchanged and no
 * draw of their streams is consumed.  A group that has finished its schedule waits inactive; its rows of steps / temb must still be readable (any
 * finite values).  A molecule's previous endpoint is carried from step to step only while its group stays active: groups go active -> inactive, not back.
 *   steps / active: HOST arrays (n_steps, n_groups), read for the launch decisions;  steps_dev / active_dev: the same arrays in DEVICE memory (the
 *   caller's; the fused CTMC kernel reads every molecule's scalars from them), which must stay untouched until the enqueued work has run;
 *   temb: device (n_steps, n_groups, time_embedding_dim); the embedding tables of floor(32 / n_groups) steps are built per launch;
 *   prev0, dst_a, dst_b, final_dst: as in fm_integrate.  Bootstrap follows the reference's `prev is None and (t == 0).all()` over the groups active at
 *   step 0: all of them at t == 0 -> the bootstrap evaluation runs; some at 0 and some later with prev0 == NULL -> FM_ERR_INVALID (start newcomers in a
 *   call of their own and pass their endpoint in);
 *   FM_ERR_INVALID also for: dfm_type FM_DFM_GAT or noise_mode FM_NOISE_TENSORS in an active step (the reference's tensor draw order depends on
 *   last_step, which differs between groups), and a non-NULL sink (trajectory frames are not recorded). */
int fm_integrate_mixed(fm_ctx* ctx, void* stream, const fm_state* state, int n_steps, int n_groups, const fm_step_scalars* steps,
                       const fm_step_scalars* steps_dev, const int32_t* active, const int32_t* active_dev, const int32_t* mol_group,
                       const float* temb, const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink,
                       int* final_dst);

/* --- ABI 10: the conditional path of a CTMC model (has_mask == 1) for given molecules: noise x1 back to an intermediate time with the model's own corruption
 * process, CTMCVectorField.sample_conditional_path (ctmc_vector_field.py:97-143, t of shape (B,)), in one launch on the bound batch with the ids of
 * fm_set_molecule_ids.  Molecule m belongs to time group mol_group[m] (DEVICE (n_mols) int32, values in [0, n_groups); NULL with n_groups == 1: group 0) and
 * reads row g of alpha: DEVICE (n_groups, 4) float32 = alpha_t of x, a, c, e at the group's time (interpolant_scheduler.py:97-153).
 *   positions (:112)      out->x_t = (1 - alpha_x) x_0 + alpha_x (x1->x_t - per-molecule mean): x_0 = fm_prior_philox's bits for this seed, the mean with
 *                         fm_remove_com's arithmetic, the three operations rounded separately like torch's
 *   tokens (:122-134)     out token = u < 1 - alpha ? mask token : x1 token, per atom (a, c) and per unordered pair (e); u = the row's uniform of the stream
 *                         entry "conditional path" (csrc/fm_device.h), disjoint from every draw of a sampling run
 * x1 must hold real categories (the kernel copies its tokens, it does not range-check them) and is only read; out must not alias it (no pointer of out may
 * equal the matching pointer of x1: FM_ERR_INVALID).  tape (may be NULL, as may any of its members) receives the draws the call consumed -- x0 (N,3), u_a, u_c
 * (N), u_e (U) -- the role fm_philox_tape plays for steps: the reference's sample_conditional_path fed with them in place of x_0 and torch.rand gives out.
 * Does not synchronise, allocates nothing and needs no workspace beyond the bind's.  FM_ERR_INVALID also for an endpoint model, n_groups < 1 and
 * n_groups > 1 with a NULL mol_group.  The state it writes continues through fm_integrate / fm_integrate_mixed with a first step at t > 0 and prev0 == NULL:
 * no bootstrap runs and the first evaluation is not self-conditioned (vector_field.py:269-289). */
typedef struct fm_cond_tape { float* x0; float* u_a; float* u_c; float* u_e; } fm_cond_tape;   /* optional outputs, any may be NULL */
int fm_conditional_path(fm_ctx* ctx, void* stream, uint64_t seed, const fm_state* x1, int n_groups, const int32_t* mol_group, const float* alpha,
                        const fm_state* out, const fm_cond_tape* tape);

/* --- ABI 11: the denoising loss of given molecules, FlowMol.forward (flowmol/models/flowmol.py:297-415) after its sample_conditional_path call.
 * fm_denoising_loss runs ONE evaluation of the bound batch on xt -- the launch plan of fm_forward_mixed(prev = NULL, bootstrap = 0, remove_com = 0), temb / n_groups /
 * mol_group as there (mol_group may be NULL with n_groups == 1) -- with the output heads in their loss variant, then one reduction launch.  The heads keep their logits
 * on chip (vector_field.py:217: apply_softmax=False) and write, per row, what CrossEntropyLoss(reduction='none') gives on them (flowmol.py:408):
 *   rows->a, rows->c (N), rows->e (U, upper-triangle order)   nll = (logf(sum_c expf(l_c - m)) + m) - l_target, m = max_c l_c: -log_softmax(l)[target] as torch evaluates it;
 *                         +0.0 for a row the ignore_index rule drops, i.e. whose token in xt is not the mask token (flowmol.py:378-384)
 *   rows->x (N)           se = ((dx dx) + dy dy) + dz dz, d = predicted x_1 (not COM-removed) - x1->x_t, separately rounded: MSELoss(reduction='none') summed over xyz
 *   mol_out (n_mols, 8)   {se_x, 3 n_atoms, nll_a, cnt_a, nll_c, cnt_c, nll_e, cnt_e}: the molecule's sums of the row terms in the canonical order documented at
 *                         fm_k_denoise_reduce (csrc/fm_kernels.h: 16-row chunks from the molecule's first row, rows in order, chunks in order) and the number of
 *                         rows that count.  The reference's batch values follow on the host: mean x = sum se_x / sum 3 n_atoms, categorical = sum nll / sum cnt
 *                         (flowmol.py:388-413; FlowMol.denoising_loss in flowmol_amd/model.py also restates the time-scaled variant).
 * x1 holds the targets: real-category tokens (the kernels index the logits with them, they do not range-check them), and x_t = the centred positions
 * x_1 - mean the conditional path used.  xt and x1 are only read.
 * temb == NULL skips the evaluation: rows then holds the CALLER's row terms (all four), xt's tokens say which rows count, and only the reduction runs.
 * It never bootstraps: the reference's eval-mode special case `prev is None and (t == 0).all()` (vector_field.py:269-272) depends on the whole batch and is the one
 * deliberate difference.  Does not synchronise, allocates nothing and needs no workspace beyond the bind's.  FM_ERR_INVALID, with a message, for an endpoint model,
 * n_groups outside 1..32, a NULL member of rows, rows or mol_out aliasing an input or each other, and a molecule with more than 2^24 pair rows (cnt_e is a float). */
typedef struct fm_loss_rows { float* x; float* a; float* c; float* e; } fm_loss_rows;   /* caller-owned: (N) se, (N), (N), (U) nll; all required */
int fm_denoising_loss(fm_ctx* ctx, void* stream, const fm_state* xt, const fm_state* x1, const float* temb, int n_groups, const int32_t* mol_group,
                      const fm_loss_rows* rows, float* mol_out /* (n_mols, 8) */);
/* fm_distort_philox: flowmol.py:333-337 in place on x (N,3): every atom of a molecule whose group is switched on (group_on: DEVICE (n_groups) int32, non-zero where the
 * group's t > distort_t; mol_group as above) gets x += (z * [u < p]) * 0.5, three normals z and one uniform u per atom from the stream entry "distortion" (csrc/fm_device.h,
 * DESIGN.md section 6), disjoint from every other draw.  tape (may be NULL, as may its members): z (N,3) and u (N) of every atom, switched on or not.  Same conventions;
 * FM_ERR_INVALID for n_groups < 1, a NULL mol_group with n_groups > 1, p outside [0, 1] and a tape that aliases x. */
typedef struct fm_distort_tape { float* z; float* u; } fm_distort_tape;
int fm_distort_philox(fm_ctx* ctx, void* stream, uint64_t seed, float p, int n_groups, const int32_t* mol_group,
                      const int32_t* group_on /* DEVICE (n_groups) */, float* x, const fm_distort_tape* tape);

/* --- ABI 12: frozen atoms (replacement conditioning) -- keep a scaffold or fragment of a given molecule exactly as given and let the model regenerate the rest.
 * A step of the calls below is EXACTLY the step of fm_ctmc_step / fm_integrate / fm_integrate_mixed on all rows: frozen rows take part in the purity counts like
 * any row, the sampled endpoint tokens (fm_sampled, the sink's a1 / c1 / e1 / x1 frames) and every draw are those of the plain step.  Then, inside the store
 * that writes the new state, every frozen row is set to the conditional path of the given molecule at the step's NEW time point:
 *   an atom row (x, a, c) is frozen iff keep_atom[atom] != 0; a pair row (e, upper-triangle order) iff BOTH its atoms are kept; a pair with one free atom is free;
 *   positions   x = (1 - ax) x0 + ax x1c, the three operations rounded separately (fm_conditional_path's arithmetic)
 *   tokens      tok = u < 1 - alpha ? mask token : tok1
 *   alpha_next = alpha_t of x, a, c, e at the time the step ARRIVES at (alpha_tables(linspace(0, 1, T))[0][i + 1] for step i of a T-point schedule).
 * x0, x1c, a1 / c1 / e1 and u_a / u_c / u_e are INPUTS: what fm_conditional_path(seed, x1, ..., tape) consumed (tape.x0, tape.u_*), x1's tokens, and x1's positions
 * after fm_remove_com.  The step kernels draw nothing new, so after step i the frozen rows equal the frozen rows of fm_conditional_path at alpha_next -- a monotone
 * unmasking, u being fixed per row -- and with alpha(1) = 1 the frozen atoms of the result are x1c bit for bit: the result is NOT re-centred, its frame is the given
 * molecule's.  The sink's frame of the new state (x, a, c, e) shows the overwritten rows.  With no atom kept the calls give the bits of the plain entry points.
 * keep_pair is caller-owned scratch of U bytes that every call fills from keep_atom with one small launch; everything else of the struct is only read.
 * Neither call synchronises or allocates, and no workspace beyond the bind's is needed.  FM_ERR_INVALID, with a message and before anything is enqueued, for an
 * endpoint model, a NULL member (keep_pair / e1 / u_e may be NULL only in a batch without pairs), and a member equal to a pointer of state, dst / dst_a / dst_b,
 * sampled or the sink. */
typedef struct fm_inpaint {
    const uint8_t* keep_atom;     /* (N) one flag per atom of the bound batch, fake atoms included */
    uint8_t* keep_pair;           /* (U) filled by the call */
    const float* x0;              /* (N,3) position prior of the path (fm_cond_tape.x0) */
    const float* x1c;             /* (N,3) given positions minus the whole molecule's mean (fm_remove_com) */
    const int32_t* a1; const int32_t* c1;      /* (N) given tokens, real categories */
    const int32_t* e1;            /* (U) */
    const float* u_a; const float* u_c;        /* (N) uniforms of the path (fm_cond_tape.u_a / u_c) */
    const float* u_e;             /* (U) */
} fm_inpaint;
/* fm_ctmc_step with frozen rows: one step, campbell or gat, either noise mode.  alpha_next: HOST, 4 floats. */
int fm_ctmc_step_inpaint(fm_ctx* ctx, void* stream, const fm_state* state, const fm_dst* dst, const fm_step_noise* noise, const fm_step_scalars* sc,
                         const fm_sampled* sampled, const fm_inpaint* inp, const float* alpha_next);
/* fm_integrate_mixed with frozen rows; alpha_next / alpha_next_dev: the (n_steps, n_groups, 4) alpha_next of every call-step and group on the HOST and in DEVICE
 * memory (the per-molecule-time kernel reads its group's row like the step scalars; an inactive group is skipped altogether, the overwrite included).
 * n_groups == 1 is fm_integrate with frozen rows instead: gat steps, FM_NOISE_TENSORS (noise: host array of n_steps fm_step_noise, else NULL) and a trajectory
 * sink are accepted, the single-schedule step kernels run, and steps_dev / active / active_dev / mol_group / alpha_next_dev are not read (may be NULL).
 * n_groups > 1 keeps fm_integrate_mixed's refusals (gat, tensor noise, a sink, prev0 == NULL with only some groups at t = 0) and does not read noise.
 * FM_ERR_INVALID also for n_groups outside 1..32. */
int fm_integrate_inpaint(fm_ctx* ctx, void* stream, const fm_state* state, int n_steps, int n_groups, const fm_step_scalars* steps,
                         const fm_step_scalars* steps_dev, const int32_t* active, const int32_t* active_dev, const int32_t* mol_group, const float* temb,
                         const fm_step_noise* noise, const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst,
                         const fm_inpaint* inp, const float* alpha_next, const float* alpha_next_dev);

/* --- ABI 13: frozen rows per modality -- fm_ctmc_step_inpaint / fm_integrate_inpaint with one keep array per modality in place of keep_atom: freeze every type, charge
 * and bond and let the positions run (conformers of a given graph), fix a pose and let the chemistry run, or freeze a bond between two free atoms.
 * A step is EXACTLY the step of fm_ctmc_step / fm_integrate / fm_integrate_mixed on all rows: every draw and every sampled endpoint token (fm_sampled, the sink's
 * a1 / c1 / e1 / x1 frames) is the plain step's.  Then, inside the store that writes the new state, the flagged rows are overwritten:
 *   a position row with keep_x[atom] != 0      x = (1 - ax) x0 + ax x1c, the three operations rounded separately (fm_conditional_path's arithmetic)
 *   an a / c / e row with ITS OWN flag set     tok = u < 1 - alpha ? mask token : tok1
 * The four flags are independent: a bond may be frozen between two free atoms, a type without the charge or the position.  alpha_next and the path inputs x0, x1c,
 * a1 / c1 / e1, u_a / u_c / u_e are those of fm_inpaint.  Everything in the struct is an INPUT: nothing is written, there is no pair scratch and no setup launch.
 * A NULL keep_* means nothing of that modality is frozen; that modality's path inputs (x0 and x1c for x, tok1 and u for a, c, e) are then not read and may be NULL too
 * -- the conformer case passes no x0 and no x1c.
 * Equivalence with ABI 12: keep_x = keep_a = keep_c = keep_atom and keep_e[u] = both atoms of pair u kept gives the bits of fm_*_inpaint(keep_atom), whose kernels these
 * are.  With every flag zero, or every keep pointer NULL, the calls give the bits of the plain entry points.
 * Neither call synchronises or allocates, and no workspace beyond the bind's is needed.  FM_ERR_INVALID, with a message and before anything is enqueued, for an
 * endpoint model; a member equal to a pointer of state, dst / dst_a / dst_b, sampled or the sink; a modality whose keep pointer is given while one of its path inputs
 * is NULL (the pair modality only in a batch that has pairs); and, in fm_integrate_freeze, what fm_integrate_inpaint refuses (n_groups outside 1..32; for n_groups > 1
 * fm_integrate_mixed's refusals). */
typedef struct fm_freeze {
    const uint8_t* keep_x; const uint8_t* keep_a; const uint8_t* keep_c;      /* (N) one flag per atom of the bound batch, fake atoms included; NULL = none */
    const uint8_t* keep_e;        /* (U) one flag per unordered pair, upper-triangle order: the order of e_t; NULL = none */
    const float* x0;              /* (N,3) position prior of the path (fm_cond_tape.x0) */
    const float* x1c;             /* (N,3) given positions minus the whole molecule's mean (fm_remove_com) */
    const int32_t* a1; const int32_t* c1;      /* (N) given tokens, real categories */
    const int32_t* e1;            /* (U) */
    const float* u_a; const float* u_c;        /* (N) uniforms of the path (fm_cond_tape.u_a / u_c) */
    const float* u_e;             /* (U) */
} fm_freeze;
/* argument lists of fm_ctmc_step_inpaint / fm_integrate_inpaint, const fm_freeze* in place of const fm_inpaint* */
int fm_ctmc_step_freeze(fm_ctx* ctx, void* stream, const fm_state* state, const fm_dst* dst, const fm_step_noise* noise, const fm_step_scalars* sc,
                        const fm_sampled* sampled, const fm_freeze* fz, const float* alpha_next);
int fm_integrate_freeze(fm_ctx* ctx, void* stream, const fm_state* state, int n_steps, int n_groups, const fm_step_scalars* steps,
                        const fm_step_scalars* steps_dev, const int32_t* active, const int32_t* active_dev, const int32_t* mol_group, const float* temb,
                        const fm_step_noise* noise, const fm_dst* prev0, const fm_dst* dst_a, const fm_dst* dst_b, const fm_traj_sink* sink, int* final_dst,
                        const fm_freeze* fz, const float* alpha_next, const float* alpha_next_dev);

/* Aligned RMSD of two coordinate sets xa, xb (N,3) of the bound batch, molecule by molecule over its selected atoms (select: (N) uint8, NULL = all), on the device:
 *   out (n_mols, 4) = {count of selected atoms, rmsd after centring both sets on their selected atoms, rmsd after the optimal PROPER rotation of xa onto xb, 0}
 *   xa_aligned (N,3), may be NULL: ALL atoms of xa moved by the transform fitted on the selected ones, R (xa - mean_a) + mean_b
 * The rotation maximises the overlap over det = +1 (no reflection: a mirror image is not a conformer): the eigenvector of the largest eigenvalue of Horn's 4x4
 * quaternion matrix, by a fixed number of cyclic Jacobi sweeps in float32; the aligned rmsd is summed from the explicit residuals R a - b, so near-identical
 * conformers do not cancel.  One wave per molecule and sums in a fixed per-molecule order: a molecule's bits do not depend on its batch.
 * A molecule with no selected atom gives {0, 0, 0, 0} and leaves its rows of xa_aligned equal to xa.  Does not synchronise, allocates nothing.
 * FM_ERR_INVALID if xa_aligned or out aliases an input or each other. */
int fm_align_rmsd(fm_ctx* ctx, void* stream, const float* xa, const float* xb, const uint8_t* select /* (N), may be NULL = all */, float* out /* (n_mols, 4) */,
                  float* xa_aligned /* (N,3), may be NULL */);

/* --- ABI 14: conformer ensembles -- the symmetry-aware RMSD of pairs of molecules of ONE coordinate set, and the greedy threshold pruning that consumes it.
 *
 * fm_pair_rmsd: x (N,3) of the bound batch; pair p = (ma, mb) names two of its molecules, of equal size n.
 *   n_pairs, pairs_host: HOST (n_pairs,2) int32, read here for the refusals only; pairs: the same array in DEVICE memory, read by the kernel
 *   select: DEVICE (N) uint8 or NULL = all atoms, read at the rows of the FIRST molecule of each pair (the caller gives both molecules of a pair the same flags)
 *   the permutation table, or three NULLs and n_sets = 0 for the identity only: perm_set DEVICE (n_mols) int32, a set id per molecule or -1 (identity);
 *     set_off DEVICE (n_sets + 1) int32 element offsets into perms; perms DEVICE int32, set s = the rows of n local atom indices between set_off[s] and
 *     set_off[s + 1].  The set of a pair is that of its first molecule; an empty set is the identity.  PRECONDITION (device data, not checked here): every
 *     row is a permutation of 0..n-1 that maps selected atoms onto selected atoms and is the identity on the rest.
 *   out DEVICE (n_pairs,2) float32 = {count of selected atoms, min over the rows q of rmsd_q}, rmsd_q after centring both molecules on the selected atoms and
 *     the optimal PROPER rotation (fm_align_rmsd's: no reflection) of a[i] onto b[q[i]], summed from the explicit residuals in float64 (the fit itself is float32)
 *   best_perm DEVICE (n_pairs) int32, may be NULL: the lowest row index, within the set, that attains the minimum
 * A pair without a selected atom gives {0, 0} and best_perm 0; n_pairs = 0 is legal.  One wave per pair, one lane per row, sums in ascending atom order: the two
 * numbers of a pair are a function of the two molecules, the selection and the SET of rows -- the same bits whatever else the batch holds, wherever the pair stands
 * and in whatever order the rows are given; only best_perm depends on that order.  Not bit-equal to fm_align_rmsd (another summation order).
 * Does not synchronise, allocates nothing.  FM_ERR_INVALID, before anything is enqueued, for an index outside the batch, a pair of unequal sizes, a partial
 * permutation table, and an output that aliases an input or the other output.
 *
 * fm_prune_rmsd: group g = the conformers group_off[g] .. group_off[g + 1] - 1 (DEVICE (n_groups + 1) int32), K of them; d + tri_off[g] (DEVICE float32, DEVICE
 * (n_groups + 1) int32) = its strict upper triangle, row-major (i < j), K (K - 1) / 2 values.  For i = 0, 1, ... in order: among the KEPT j < i the one with the
 * smallest d(j, i), ties to the lowest j; d < threshold drops i (keep[i] = 0, rep[i] = j), otherwise i is kept (keep[i] = 1, rep[i] = i) -- conformer 0 always, and
 * a NaN compares false and drops nothing.  keep DEVICE (group_off[n_groups]) uint8, rep the same in int32, both indexed like the conformers; rep holds
 * indices of the concatenated conformers (group_off[g] + j).  Groups of 0 or 1 conformers are legal.  Needs no bound batch; does not synchronise, allocates nothing; FM_ERR_INVALID for an output that aliases. */
int fm_pair_rmsd(fm_ctx* ctx, void* stream, const float* x, int n_pairs, const int32_t* pairs_host, const int32_t* pairs, const uint8_t* select,
                 const int32_t* perm_set, const int32_t* set_off, const int32_t* perms, int n_sets, float* out, int32_t* best_perm);
int fm_prune_rmsd(fm_ctx* ctx, void* stream, int n_groups, const int32_t* group_off, const float* d, const int32_t* tri_off, float threshold, uint8_t* keep,
                  int32_t* rep);

/* --- ABI 15: the stereo check -- do the conformers keep the handedness of the input's stereocentres and the cis/trans state of its double bonds?
 *
 * fm_stereo: x, x_ref (N,3) of the bound batch: the coordinates to check and the coordinates that define the stereo state.
 *   the element table, or three NULLs and n_sets = 0 for no element at all: elem_set DEVICE (n_mols) int32, a set id per molecule or -1 (none); set_off DEVICE
 *     (n_sets + 1) int32 ROW offsets into elems; elems DEVICE (rows,5) int32, a row = {kind, i0, i1, i2, i3} with local atom indices.  The layout mirrors
 *     fm_pair_rmsd's permutation sets; conformers of one graph share a set.  PRECONDITION (device data, not checked here): kind is 0 or 1 (anything else is read
 *     as 1) and the four indices lie inside every molecule that names the set (an index outside is read as 0: nothing is read out of the molecule).
 *   value of an element in one coordinate set, float32, every operation separately rounded:
 *     kind 0 (tetrahedral centre i0 with neighbours i1, i2, i3): (u1 x u2) . u3, u_k the unit vector from i0 to i_k
 *     kind 1 (double bond i1 = i2 with substituents i0, i3): the cosine of the dihedral i0-i1-i2-i3
 *     a vector or a normal of zero length gives the value +0, never a NaN
 *   an element is DEFINED in a set when |value| >= flat_tol, and a MISMATCH when it is defined in both x and x_ref and the two signs differ
 *   out DEVICE (n_mols,8) int32 = {kind-0 elements, of them defined in both, of them mismatches, kind-1 elements, defined in both, mismatches, match, mirror}:
 *     match = 1 when every element is defined in both sets and none mismatches (a molecule without elements matches); mirror = 1 when there is a kind-0
 *     element, every element is defined in both, every kind-0 element mismatches and no kind-1 element does -- what a point inversion of x_ref gives
 *   values DEVICE float32 with val_off DEVICE (n_mols + 1) int32, both may be NULL: the values of x of molecule m at val_off[m] .., in row order (the caller
 *     leaves room for the rows of the molecule's set)
 *   x_out DEVICE (N,3), may be NULL: -x (an exact sign flip) for the atoms of a molecule with mirror = 1, x for the others
 * One wave per molecule, lanes strided over its rows; the counts are integer sums: a molecule's outputs are a function of that molecule, its rows and
 * flat_tol -- the same bits whatever else the batch holds; the order of the rows changes the order of values only.
 * Does not synchronise, allocates nothing.  FM_ERR_INVALID (this call's status for every refusal), before anything is enqueued, for no bound batch, an output
 * that aliases an input or another output, values without val_off, a partial element table, and a flat_tol that is negative or NaN. */
int fm_stereo(fm_ctx* ctx, void* stream, const float* x, const float* x_ref, const int32_t* elem_set /* (n_mols), -1 = none */,
              const int32_t* set_off /* (n_sets+1), in rows */, const int32_t* elems /* (rows,5) */, int n_sets, float flat_tol, int32_t* out /* (n_mols,8) */,
              const int32_t* val_off /* (n_mols+1) or NULL */, float* values /* or NULL */, float* x_out /* (N,3) or NULL */);

/* --- ABI 16: the equivariant-OT coupling of the position prior -- the conditional path the network was TRAINED on starts from a prior that was assigned and
 * rigidly fitted to the molecule, not from an independent Gaussian.
 *
 * fm_ot_align: x0 (N,3) the prior (fm_prior_philox's output), x1c (N,3) the given positions after fm_remove_com, both of the bound batch and both used AS GIVEN
 * (nothing is re-centred for the cost: the reference's cost is between the dataset's COM-free x_1 and the prior).  Molecule by molecule, on the device:
 *   A  the assignment: perm minimises sum_i c(i, perm[i]) with c(i, j) = sqrtf(((dx dx) + (dy dy)) + (dz dz)), d = x1c[i] - x0[j], every operation float32 and
 *      separately rounded -- torch.cdist(x_1, x_0) (priors.py:113) up to rounding.  perm[i] is the LOCAL index of the prior row given to atom i (the reference's
 *      prior_idx, :114-115), x0p[i] = x0[perm[i]].  Solver: shortest augmenting paths (Jonker-Volgenant, the algorithm behind linear_sum_assignment), rows inserted
 *      in order, the next column the arg-min of the path costs with ties to the LOWEST column index.  Duals, path costs and minima are float64; a molecule's
 *      float32 costs span far fewer than 2^29, so sums and differences of up to n of them are exact: perm is exactly optimal for the float32 cost matrix
 *      above, and unique whenever that matrix has a unique optimum.  The matrix is never stored: LDS use is O(n).  Coordinates that are not numbers give the
 *      identity permutation (and NaN results), in bounded work.
 *   B  the rigid fit of x0p onto x1c (:128-169): means relative to the molecule's first atom, the 3x3 cross-covariance, Horn's 4x4 by fm_align_rmsd's fixed
 *      Jacobi sweeps -- fm_align_rmsd's rounds and summation order.  allow_reflection = 1 is the REFERENCE'S behaviour, the optimum over all orthogonal
 *      transforms (R = V U^T, no determinant correction): with lambda the eigenvalues of Horn's matrix, -lambda_min > lambda_max takes R = -R(q_min), otherwise
 *      (ties included) R(q_max).  allow_reflection = 0 is the optimal PROPER rotation, fm_align_rmsd's.  x0_aligned = R (x0p - mean0) + mean1.
 *   x0_aligned DEVICE (N,3); perm DEVICE (N) int32, may be NULL
 *   out DEVICE (n_mols,4) float32 = {n, sum_i c(i, perm[i]) added in float64 in atom order and rounded once, sqrt(mean |x0p - x1c|^2) (after the permutation
 *     only, nothing centred), sqrt(mean |x0_aligned - x1c|^2) from the explicit residuals}
 * n = 0 gives {0, 0, 0, 0}; n = 1 gives perm = {0} and x0_aligned = x1c's row.  One wave per molecule, every sum in a fixed per-molecule order: a molecule's
 * outputs are the same bits whatever else the batch holds.  Work is O(n^3 / 64) wave steps per molecule; FM_OT_MAX_ATOMS bounds it (GEOM-drugs' largest
 * molecule, 181 atoms, with the 54 fake atoms of fake_atom_p = 0.3 is 235 rows).  Does not synchronise, allocates nothing.
 * FM_ERR_INVALID (this call's status for every refusal), with a message and before anything is enqueued, for no bound batch, a bound molecule above
 * FM_OT_MAX_ATOMS (read from the bind's host-side sizes; the message names it), allow_reflection outside {0, 1}, and an output that aliases an input or another
 * output -- x0_aligned == x0 included, the kernel gathers from x0.
 *
 * fm_conditional_path_x0: fm_conditional_path's arguments and x0_in DEVICE (N,3): the position job reads x0_in[row] instead of drawing (one uniform branch).
 * x0_in = NULL is fm_conditional_path bit for bit, and so is x0_in = fm_prior_philox(seed)'s output; the tokens and the tape's uniforms never depend on x0_in.
 * tape->x0 receives the prior actually used, so the frozen-row structs (fm_inpaint / fm_freeze) carry a coupled path unchanged.  fm_conditional_path's
 * refusals, and FM_ERR_INVALID for x0_in equal to out->x_t or tape->x0. */
#define FM_OT_MAX_ATOMS 256
int fm_ot_align(fm_ctx* ctx, void* stream, const float* x0, const float* x1c, int allow_reflection, float* x0_aligned /* (N,3) */,
                int32_t* perm /* (N) or NULL */, float* out /* (n_mols,4) */);
int fm_conditional_path_x0(fm_ctx* ctx, void* stream, uint64_t seed, const fm_state* x1, int n_groups, const int32_t* mol_group, const float* alpha,
                           const fm_state* out, const fm_cond_tape* tape, const float* x0_in /* (N,3) or NULL */);

/* debugging / parity taps: copy an internal buffer to `dst` (device) after the next fm_forward stages.
 * name: "embed.s", "sc.s", "sc.ef", "conv<i>.s", "conv<i>.v", "conv<i>.agg.s", "conv<i>.agg.v",
 * "upd<i>.x", "upd<i>.ef", "conv0.msg.s", "conv0.msg.v"; internal layouts: v (N,3,V), ef (E,128) in the
 * internal edge order.  fm_batch_query copies an int32 descriptor array ("e_src","e_dst","e_pair",
 * "p_e0","p_e1","node_mol") to `dst`. */
int fm_set_tap(fm_ctx* ctx, const char* name, void* dst);
int fm_clear_taps(fm_ctx* ctx);
int fm_batch_query(fm_ctx* ctx, void* stream, const char* name, int32_t* dst);

/* Valence stability and connectivity of the molecules in `state` (tokens), computed on the device
 * (reference flowmol/analysis/metrics.py:96-117 + check_stability :333-363; SampledMolecule.compute_valencies,
 * molecule_builder.py:138-157).  table: device array of n_types * n_charges uint32 bit masks (bit v = valency v valid;
 * explicit aromaticity: bit n_arom*8+v); fake_atom_token: token of the fake atom or -1; out: device (n_mols,4) int32 =
 * {stable atoms, real atoms, connected components, largest component}. */
int fm_stability(fm_ctx* ctx, void* stream, const fm_state* state, const uint32_t* table, int n_types,
                 int fake_atom_token, int explicit_aromaticity, int32_t* out);

/* per-kernel timing of the last fm_forward / fm_integrate when enabled (HIP events on `stream`):
 * fm_profile_enable(ctx, 1); ... ; fm_profile_get(ctx, "edge_message", &total_ms, &launches).
 * While profiling, every CTMC step also times an EMPTY kernel under the name "event_overhead": what an event pair adds to a launch
 * (subtract its average from the other kernels' averages to compare with rocprofv3 kernel durations). */
int fm_profile_enable(fm_ctx* ctx, int on);
int fm_profile_get(fm_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* FLOWMOL_HIP_H */
