/*
 * nts_hip.h — C-ABI of the MI355X (gfx950) sampled-GNN hot path.
 *
 * This is the drop-in boundary: a plain-C interface (raw device pointers,
 * sizes, status codes; no torch types) that replaces the hot subset of the
 * reference's `Cuda_Stream` device layer (cuda/ntsCUDA.hpp:177-595) and its
 * NCCL wrapper (cuda/ntsCUDA.hpp:132-175).  Every entry point below names
 * the reference interface it replaces (file:line in AiX-im/Sample-based-GNN).
 *
 * Conventions
 *  - Vertex ids are uint32 (VertexId, dep/gemini/type.hpp:29; cuda/cuda_type.h:21).
 *  - Global CSC offsets are uint64 (the reference uses uint32 and overflows
 *    past 2^32 edges); per-batch sampled offsets are uint32.
 *  - Values are fp32 (ValueType, dep/gemini/type.hpp:31).
 *  - Sizes that are only known on the device (e_size, src_size of a sampled
 *    layer) are passed as device scalars plus a host-side capacity; kernels
 *    read the live size and never touch entries past it.  No entry point
 *    synchronises with the host.
 *  - All work is enqueued on the context's stream (async); buffers are owned
 *    by the caller.  Return value 0 = success; on failure the message is
 *    available from nts_hip_last_error() (thread-local).  The reference
 *    aborts instead (CHECK_CUDA_RESULT, cuda/ntsCUDAGraphOP.cu:21-28); the
 *    C++ host layer reproduces abort-on-error by throwing.
 *  - A context is re-entrant per stream and holds no global mutable state
 *    (unlike Cuda_Stream::total_*, cuda/ntsCUDAGraphOP.cu:64-66).
 */
#ifndef NTS_HIP_H
#define NTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTS_HIP_ABI_VERSION 11  /* 2: nts_sampcsc_dev gained dst_local_id, csr_edge_id;
                                  3: transform-first entry points, fused agg+GEMM removed,
                                     accuracy counts in the fused loss;
                                  4: PD cache entry points + omit fields, GEMM mode;
                                  5: two-piece f16 pair-table GEMMs (nts_hip_h2_*);
                                  6: nts_hip_spmm_csr_bwd_colmax + nts_hip_gemm_h2p_tn_gather_cm;
                                  7: the column maxima per part of rows (no row scales in
                                     the backward), nts_hip_csr_bwd_colmax_rows_per_part;
                                  8: nts_hip_comm_count; the CSR-backward column maxima scaled by
                                     the pair table's row scales (exact TN operand maxima);
                                  9: nts_sampcsc_dev::sizes_host;
                                  10: the activation's keep mask as bits (nts_hip_act_bits_words,
                                      nts_hip_spmm_csc_fwd_act_bits,
                                      nts_hip_spmm_csr_bwd_postmask_bits);
                                  11: MT19937 re-run of a short stream (nts_hip_mt_budget_scale,
                                      nts_hip_mt_checkpoint, nts_hip_mt_rewind);
                                      later entry points (nts_hip_lp_*, nts_hip_random_walk and
                                      nts_hip_induced_layer among them) are additions: no
                                      struct or existing signature changed */

/* status codes */
#define NTS_OK 0
#define NTS_ERR_INVALID 1
#define NTS_ERR_HIP 2
#define NTS_ERR_OOM 3
#define NTS_ERR_UNSUPPORTED 4
#define NTS_ERR_RCCL 5

/* Random stream used by the sampler.
 *  PHILOX          : counter-based Philox4x32-10 keyed by (seed), counter
 *                    (word block, dst id, layer, batch_seq) — every dst is
 *                    independent, fully parallel (the fast default).
 *  MT19937_LEMIRE  : the reference's stream, bit-exact: one
 *                    `static thread_local std::mt19937 generator(seed)`
 *                    consumed sequentially by std::uniform_int_distribution
 *                    (core/ntsFastSampler.hpp:200-205) in libstdc++ >= 11 form
 *                    (Lemire nearly-divisionless, uniform_int_dist.h:246-263).
 *  MT19937_DIV     : same stream, libstdc++ <= 10 form (2-division rejection).
 *  PHILOX_SHARED   : one Philox word r(s) per *source* s of a layer call
 *                    (counter (0, s, layer | 0x80000000, batch_seq)); a dst
 *                    with deg > fanout keeps the `fanout` positions p with the
 *                    smallest key (r(src_p) << 32) | p, in CSC order.  Each
 *                    dst's set is still a uniform fanout-subset, but dsts
 *                    sharing neighbours pick the same ones: a smaller
 *                    frontier (fixed-size LABOR).  Stateless like
 *                    PHILOX; any fanout.
 * The MT modes consume one generator shared by all layers/batches of a
 * context, exactly like the reference's thread_local generator. */
#define NTS_RNG_PHILOX 0
#define NTS_RNG_MT19937_LEMIRE 1
#define NTS_RNG_MT19937_DIV 2
#define NTS_RNG_PHILOX_SHARED 3

/* Edge weights, mirrors `enum class WeightType{Sum, Mean, None}`
 * (core/ntsFastSampler.hpp:27) with the CPU sampler's formulas
 * (core/ntsFastSampler.hpp:1111-1119, nts_norm_degree core/ntsBaseOp.hpp:652-657). */
#define NTS_WEIGHT_SUM 0
#define NTS_WEIGHT_MEAN 1  /* CPU sampler: norm / in_degree(dst) of the full graph (:1111-1113) */
#define NTS_WEIGHT_NONE 2
/* The reference GPU kernel get_mean_weight (cuda/ntsCUDATransferKernel.cuh:319-342):
 * norm / (sampled edge count of the dst).  Note the reference's GPU toolkits never
 * reach it: sample_gpu_fast(int, int, WeightType) drops the weight type
 * (core/ntsFastSampler.hpp:944-948), so GS_SAMPLE_ALLGPU
 * actually trains with SUM weights.  Offered for the kernel's semantics. */
#define NTS_WEIGHT_MEAN_SAMPLED 3
/* OR-ed into SUM / MEAN: UP_DEGREE — the degrees in the weights are the
 * sampled layer's own (in = sampled edges of the dst, out = sampled edges of
 * the src), SampledSubgraph::update_degrees(_GPU) (core/FullyRepGraph.hpp:189-217,
 * cfg key UP_DEGREE, core/ntsFastSampler.hpp:691-693,1107-1108). */
#define NTS_WEIGHT_UP_DEGREE 0x10

typedef struct nts_hip_ctx nts_hip_ctx;
typedef struct nts_hip_comm nts_hip_comm;

/* Replicated global graph resident in HBM (FullyRepGraph, core/FullyRepGraph.hpp:682-798
 * + Graph degrees core/graph.hpp:1157-1186,1420-1425,4525-4530). */
typedef struct {
  uint64_t n_vertices;
  uint64_t n_edges;
  const uint64_t *column_offset; /* [V+1] CSC keyed by dst                         */
  const uint32_t *row_indices;   /* [E] src ids, file order within each dst        */
  const uint32_t *in_degree;     /* [V] in_degree_for_backward  (clamped >= 1)     */
  const uint32_t *out_degree;    /* [V] out_degree_for_backward (clamped >= 1)     */
} nts_graph_dev;

/* One sampled layer (sampCSC, core/coocsc.hpp:417-460), device side.
 * Inputs: destination + v_size.  Everything else is written by
 * nts_hip_sample_layer.  CSR arrays may be NULL (no transpose built). */
typedef struct {
  uint32_t v_cap, e_cap, s_cap;    /* host capacities of the arrays below       */
  const uint32_t *destination;     /* [v_cap] global dst ids (input)           */
  const uint32_t *v_size;          /* device scalar: live dst count (input)    */
  uint32_t *column_offset;         /* [v_cap+1] local CSC offsets              */
  uint32_t *row_indices;           /* [e_cap] local src ids                    */
  uint32_t *sample_ans;            /* [e_cap] global src ids (sample_ans)      */
  uint32_t *edge_dst;              /* [e_cap] local dst of each edge (COO)     */
  uint32_t *source;                /* [s_cap] global src ids, ascending        */
  float *edge_weight_forward;      /* [e_cap] CSC order (NULL iff WEIGHT_NONE) */
  uint32_t *row_offset;            /* [s_cap+1] CSR offsets, or NULL           */
  uint32_t *column_indices;        /* [e_cap] CSR local dst ids, or NULL       */
  float *edge_weight_backward;     /* [e_cap] CSR order, or NULL               */
  uint32_t *sizes;                 /* device [4]: v_size, e_size, src_size,
                                      overflow flag (nonzero = a capacity was
                                      exceeded and the layer is truncated)     */
  uint32_t *dst_local_id;          /* [v_cap] or NULL.  Non-NULL: every dst is
                                      also put in the frontier (is_merge_src_dst,
                                      core/ntsFastSampler.hpp:1050-1052, the GAT
                                      drivers) and dst_local_id[d] = its local
                                      src id (:1095-1097; set_dst_local_index,
                                      cuda/ntsCUDAGraphOP.cu:1696).  s_cap must
                                      then allow e + v sources.               */
  uint32_t *csr_edge_id;           /* [e_cap] or NULL: CSC edge id of each CSR
                                      slot (with row_offset)                   */
  const uint32_t *omit_map;        /* [V] or NULL: a dst d with omit_map[d] ==
                                      omit_key samples no neighbours
                                      (sample_gpu_fast_omit, bottom layer of
                                      the PD-cache toolkits,
                                      core/ntsFastSampler.hpp:711-915)         */
  uint32_t omit_key;
  const uint32_t *omit_loc;        /* [V] with omit_map: the PD cache row of d */
  uint32_t *omit_row;              /* [v_cap] with omit_map: omit_loc[dst[i]]
                                      for an omitted dst i, else NTS_NOT_CACHED
                                      (the batch's own snapshot of the cache) */
  uint32_t *sizes_host;            /* NULL, or a device-visible pointer to host
                                      memory (hipHostMalloc mapped + coherent):
                                      the layer's last kernel also stores the 4
                                      sizes words there, so the host reads them
                                      after the stream's event without a D2H
                                      copy of its own                          */
} nts_sampcsc_dev;

/* ---- context ------------------------------------------------------------ */
int nts_hip_abi_version(void);
const char *nts_hip_last_error(void);
/* Replaces `new Cuda_Stream()` (cuda/ntsCUDAGraphOP.cu:201-212).  `stream` is
 * used as given; NULL is HIP's legacy default stream.  seed feeds PHILOX and
 * the MT19937 generator (reference: 2000, core/ntsFastSampler.hpp:202). */
int nts_hip_ctx_create(nts_hip_ctx **ctx, int device, void *stream, uint64_t seed);
int nts_hip_ctx_destroy(nts_hip_ctx *ctx);
/* Cuda_Stream::setNewStream (cuda/ntsCUDA.hpp:188). */
int nts_hip_ctx_set_stream(nts_hip_ctx *ctx, void *stream);
void *nts_hip_ctx_get_stream(nts_hip_ctx *ctx);
/* Pre-size the scratch arena so no allocation happens inside the hot loop
 * (keeps every call graph-capturable).  n_vertices: |V| of the graph;
 * max_items: largest e_cap / v_cap that will be passed. */
int nts_hip_ctx_reserve(nts_hip_ctx *ctx, uint64_t n_vertices, uint64_t max_items);
/* Arithmetic of the dense layer GEMMs issued through this context
 * (nts_hip_gemm_*, the bottom-layer transform): NTS_GEMM_F32 = the fp32-input
 * MFMA (one fp32 fma chain per output, the reference's fp32 GEMM semantics);
 * NTS_GEMM_SPLIT3 = fp32 operands split exactly into three bf16 pieces, the
 * six significant piece products on the bf16 MFMA with fp32 accumulation
 * (error vs fp64 of the same order as the fp32 path; csrc/gemm3.hip) for
 * the GEMMs whose reduction (NN) or output rows (TN) span >= 256 — narrower
 * ones run faster on the fp32 path and take it; NTS_GEMM_SPLIT3_ALL = the
 * split kernels for every shape they take (kernel tests).  Shapes the split
 * kernels do not take run on the fp32 path. */
#define NTS_GEMM_F32 0
#define NTS_GEMM_SPLIT3 1
#define NTS_GEMM_SPLIT3_ALL 2
int nts_hip_ctx_set_gemm_mode(nts_hip_ctx *ctx, int mode);
int nts_hip_ctx_get_gemm_mode(nts_hip_ctx *ctx);
/* Re-seed the MT19937 state (std::mt19937(seed)).  Enqueued on the stream. */
int nts_hip_rng_seed(nts_hip_ctx *ctx, uint64_t seed);
/* Copy the MT19937 state (624 words + position) to host; synchronises. */
int nts_hip_rng_state(nts_hip_ctx *ctx, uint32_t *host_state625);
/* MT19937 modes, recovery from a short stream (no reference counterpart: the
 * reference's CPU generator, core/ntsFastSampler.hpp:200-205, is unbounded;
 * the device replay generates each layer's words ahead up to a bound).
 * A layer whose draws pass its bound reports it (sizes[3] bit 2) and leaves
 * the generator where the layer began; the caller rewinds to the batch's
 * checkpoint, scales the bound up and samples the batch again — bit-exact,
 * the stream is the same.
 *   nts_hip_mt_budget_scale: multiply every later layer's word bound by
 *     `scale` (> 0; 1 = the coupon-collector mean x 1.05 + 131,072 words).
 *   nts_hip_mt_checkpoint: enqueue (on the context's stream) a copy of the
 *     generator state (625 u32: 624 words + position) into the DEVICE buffer
 *     `dev_state625` — taken before a batch's first layer.
 *   nts_hip_mt_rewind: synchronise the context's streams, make
 *     `dev_state625` the generator state and restart the word ring from it. */
int nts_hip_mt_budget_scale(nts_hip_ctx *ctx, double scale);
int nts_hip_mt_checkpoint(nts_hip_ctx *ctx, uint32_t *dev_state625);
int nts_hip_mt_rewind(nts_hip_ctx *ctx, const uint32_t *dev_state625);

/* ---- graph preprocessing ----------------------------------------------- */
/* Degrees from an edge list, clamped to >= 1:
 * Graph::load_directed (core/graph.hpp:1157-1186 out, :1420-1425 in) +
 * generate_backward_structure clamp (core/graph.hpp:4525-4530). */
int nts_hip_degrees(nts_hip_ctx *ctx, const uint32_t *src, const uint32_t *dst,
                    uint64_t n_edges, uint64_t n_vertices, uint32_t *out_degree,
                    uint32_t *in_degree);
/* Global CSC keyed by dst, src ids in edge-list (file) order within each dst:
 * FullyRepGraph::ReadRepGraphFromRawFile (core/FullyRepGraph.hpp:724-798). */
int nts_hip_build_csc(nts_hip_ctx *ctx, const uint32_t *src, const uint32_t *dst,
                      uint64_t n_edges, uint64_t n_vertices, uint64_t *column_offset,
                      uint32_t *row_indices);

/* ---- sampler ------------------------------------------------------------ */
/* One hop of FastSampler::sample_fast / sample_gpu_fast
 * (core/ntsFastSampler.hpp:962-1140, :648-709):
 *   num_d = min(deg(d), fanout) (fanout < 0: all), draw num_d distinct
 *   neighbour positions by rejection (deg > fanout) or take all in CSC order,
 *   frontier = distinct sampled ids in ascending global order (source),
 *   row_indices relabelled to local ids, CSR transpose (csc_to_csr,
 *   core/coocsc.hpp:82-111, stable = ascending dst) and edge weights
 *   (WeightCompute, core/coocsc.hpp:301-324).  Replaces
 *   sample_processing_get_co_gpu + sample_processing_traverse_gpu +
 *   sample_processing_update_ri_gpu + GetWeight (cuda/ntsCUDAGraphOP.cu:1246-1700).
 * batch_seq/layer key the PHILOX and PHILOX_SHARED streams; MT modes ignore
 * them.  PHILOX_SHARED replaces only the draw: the deg > fanout dsts keep the
 * positions with the smallest shared keys; everything else is the same. */
int nts_hip_sample_layer(nts_hip_ctx *ctx, const nts_graph_dev *graph, int fanout,
                         int layer, uint64_t batch_seq, int rng_mode, int weight_type,
                         nts_sampcsc_dev *out);
/* The same hop with edge-weighted neighbour selection (DGL
 * sample_neighbors(prob=), PyG NeighborLoader(weight_attr=)).  edge_prob holds
 * one fp32 value per edge of `graph` in CSC order, finite and in
 * [2^-60, 2^60] (the caller checks the range once, at load).  Position p of a
 * dst d with deg > fanout draws
 *   x   = word p of the Philox stream (d, layer | 0x40000000, batch_seq),
 *   u   = ((x >> 9) + 0.5f) * 2^-23      (exact in fp32, inside (0, 1)),
 *   key = -log2f(u) / edge_prob[beg + p] (fp32),
 * and d keeps the `fanout` positions with the smallest
 * (float_as_uint(key) << 32) | p, in CSC order: successive sampling without
 * replacement with probability proportional to edge_prob (Efraimidis-Spirakis).
 * Only the draw differs from NTS_RNG_PHILOX: counts (min(deg, fanout)),
 * frontier, relabel, CSR and the weight_type weights are the same code; this
 * entry does not use edge_prob as an aggregation coefficient
 * (nts_hip_sample_layer_coef does).  Stateless; any fanout.
 * NTS_ERR_INVALID, before any write: edge_prob == NULL, out->omit_map set. */
int nts_hip_sample_layer_weighted(nts_hip_ctx *ctx, const nts_graph_dev *graph,
                                  const float *edge_prob, int fanout, int layer,
                                  uint64_t batch_seq, int weight_type, nts_sampcsc_dev *out);
/* The same hop with per-edge aggregation coefficients (DGL
 * GraphConv(edge_weight=), PyG GCNConv(x, edge_index, edge_weight)): the
 * sampled convolution becomes Y[d] = sum_e c(e) a_e X[src(e)].  edge_coef holds
 * one fp32 value per edge of `graph` in CSC order.  The draw is today's:
 * edge_prob == NULL: nts_hip_sample_layer's with rng_mode NTS_RNG_PHILOX or
 * NTS_RNG_PHILOX_SHARED; edge_prob != NULL: nts_hip_sample_layer_weighted's
 * (rng_mode must then be NTS_RNG_PHILOX).  Counts, sample_ans, edge_dst,
 * frontier, relabel, CSR, csr_edge_id and sizes are the same code and bits.
 *   edge_weight_forward[k] = fl32(c(e_k) * edge_coef[q_k])
 * with q_k the CSC position of kept edge k in `graph` and c the weight_type
 * weight, fully formed (the MEAN / MEAN_SAMPLED division included) before the
 * one fp32 multiply.  Under NTS_WEIGHT_NONE the array is built all the same and
 * holds edge_coef[q_k] itself (a caller's own normalisation).
 * edge_weight_backward, where asked for, holds the same values in CSR order,
 * under NONE too.
 * NTS_ERR_INVALID, before any write: edge_coef == NULL, an MT19937 rng_mode,
 * the NTS_WEIGHT_UP_DEGREE bit, out->omit_map set, edge_prob != NULL with
 * NTS_RNG_PHILOX_SHARED, out->edge_weight_forward == NULL. */
int nts_hip_sample_layer_coef(nts_hip_ctx *ctx, const nts_graph_dev *graph,
                              const float *edge_prob, const float *edge_coef, int fanout,
                              int layer, uint64_t batch_seq, int rng_mode, int weight_type,
                              nts_sampcsc_dev *out);
/* Test and diagnostic entry: the key bits nts_hip_sample_layer_weighted gives
 * every position of the `v` destinations (device ids):
 * keys_out[out_offset[i] + p] = float_as_uint(key of position p of
 * destination[i]), p < deg(destination[i]).  All pointers on the device. */
int nts_hip_weighted_keys(nts_hip_ctx *ctx, const nts_graph_dev *graph, const float *edge_prob,
                          const uint32_t *destination, uint32_t v, int layer,
                          uint64_t batch_seq, uint32_t *keys_out, const uint64_t *out_offset);

/* ---- subgraph sampling ---------------------------------------- */
/* Random walks over in-neighbours (the CSC row of a vertex: the direction
 * messages come from), GraphSAINT-RW's node set.  roots[0 .. n) with
 * n = min(*n_roots, cap) (device ids, device count: the convention of
 * nts_sampcsc_dev::v_size); out receives cap * (walk_len + 1) ids, walk-major:
 * out[i (walk_len + 1)] = roots[i], and step t < walk_len of the walk rooted at
 * r, standing at u, moves to the neighbour at CSC position
 *   mulhi32(x, deg(u)),  x = word 0 of Philox4x32-10(counter = (0, r,
 *   0x10000000 | t, lo32(batch_seq)), keyed as the sampler's streams are).
 * The counter words in use are disjoint: the plain layer number (PHILOX),
 * layer | 0x80000000 (PHILOX_SHARED), layer | 0x40000000 (weighted),
 * 0x20000000 | t (link prediction's negatives) and 0x10000000 | t here
 * (walk_len < 2^28).  deg(u) == 0: the walk stays at u.  No rejection step:
 * the position's bias is at most deg / 2^32.  Two roots with the same id walk
 * the same path.  Slots of walks past the live count are not written.
 * Stateless; two calls give the same bytes. */
int nts_hip_random_walk(nts_hip_ctx *ctx, const nts_graph_dev *graph, const uint32_t *roots,
                        const uint32_t *n_roots, uint32_t cap, int walk_len, uint64_t batch_seq,
                        uint32_t *out);
/* The block a vertex set induces: out->destination / out->v_size are inputs as
 * for nts_hip_sample_layer, set_ids[0 .. min(*set_size, set_cap)) is the set
 * (device ids in any order, duplicates allowed, device count).  Every
 * destination must be a member of the set (the caller guarantees it; it is not
 * checked on the device).  Output, in nts_hip_sample_layer's layout:
 *   source       the distinct members of the set, ascending — the whole set,
 *                members that are nobody's neighbour included;
 *   column i     the neighbours of destination[i] that are in the set, in the
 *                graph's CSC order (a neighbour listed twice is kept twice);
 *   row_indices  local ids into source; sample_ans, edge_dst, the weight_type
 *                weights (NTS_WEIGHT_UP_DEGREE honoured), the CSR transpose with
 *                its weights, csr_edge_id, dst_local_id, sizes (overflow flag
 *                included) and sizes_host as nts_hip_sample_layer fills them —
 *                the same launches from the frontier compaction on.
 * A block above e_cap is cut at a destination boundary as a sampled layer is
 * (sizes[1] = the offset of the first destination that does not fit, flag bit
 * 0), and every column_offset entry is then clamped to sizes[1]: the cut
 * destinations are empty columns, so a consumer enqueued before the host reads
 * the flag stays inside the written edges.
 * Nothing is drawn: there is no rng_mode, layer or batch_seq argument and no
 * generator state is touched (an MT19937 caller has nothing to keep in step).
 * Integer work only apart from the weights, no atomics on floats: two calls
 * give the same bytes.  NTS_ERR_INVALID, before any write: set_ids == NULL,
 * set_size == NULL, out->omit_map set. */
int nts_hip_induced_layer(nts_hip_ctx *ctx, const nts_graph_dev *graph, const uint32_t *set_ids,
                          const uint32_t *set_size, uint32_t set_cap, int weight_type,
                          nts_sampcsc_dev *out);

/* ---- feature / label movement ------------------------------------------- */
/* out[i,:] = table[index[i],:] for i < *n (n == NULL: n_cap rows).
 * Replaces zero_copy_feature_move_gpu (cuda/ntsCUDAGraphOP.cu:1711-1729) and
 * nts::op::get_feature (core/ntsMiniBatchGraphOp.hpp:45-60); the table is
 * HBM-resident instead of pinned host memory; 64-bit row offsets. */
int nts_hip_gather_rows(nts_hip_ctx *ctx, const float *table, uint64_t ld_table,
                        const uint32_t *index, const uint32_t *n, uint32_t n_cap,
                        uint32_t feature_size, float *out, uint64_t ld_out);
/* out[i] = labels[index[i]]: global_copy_label_move_gpu (cuda/ntsCUDAGraphOP.cu,
 * kernel cuda/ntsCUDATransferKernel.cuh:203-212) / get_label (core/ntsMiniBatchGraphOp.hpp:36-43). */
int nts_hip_gather_labels(nts_hip_ctx *ctx, const int64_t *labels, const uint32_t *index,
                          const uint32_t *n, uint32_t n_cap, int64_t *out);

/* ---- HBM feature cache + host-pinned spill -------------------------------- */
/* The reference keeps the feature table in pinned host memory and caches the
 * rows of the highest-degree vertices on the GPU (GS_SAMPLE_PD_CACHE:
 * determine_cache_node_idx / cache_high_degree / mark_cache_node,
 * toolkits/GS_SAMPLE_PD_CACHE.hpp:1019-1112).  On MI355X every BASELINE
 * config fits HBM, so this two-tier table is the path for tables that do not.
 *
 * Selection: cache_map[v] = slot of v if v is among the n_cache vertices of
 * largest out_degree (ties: ascending id), else NTS_NOT_CACHED;
 * cache_ids[slot] = v (may be NULL when n_cache == 0).  Slots follow the
 * (degree descending, id ascending) order.  n_vertices < 2^31.  Fill the
 * cache with nts_hip_gather_rows(table, cache_ids -> cache). */
#define NTS_NOT_CACHED 0xFFFFFFFFu
int nts_hip_cache_select(nts_hip_ctx *ctx, const uint32_t *out_degree, uint64_t n_vertices,
                         uint64_t n_cache, uint32_t *cache_map, uint32_t *cache_ids);
/* Pinned host memory mapped into the device address space (coarse-grained),
 * for the spilled feature table (cudaMallocPinned, core/ntsDataloador.hpp:483). */
int nts_hip_host_alloc(uint64_t bytes, void **host_ptr);
int nts_hip_host_free(void *host_ptr);
int nts_hip_host_device_pointer(void *host_ptr, void **dev_ptr);
/* load_feature_gpu_cache (core/ntsFastSampler.hpp:263-317; kernels
 * cuda/ntsCUDATransferKernel.cuh:154-183) in one pass:
 *   out[i,:] = cache_map[index[i]] != NTS_NOT_CACHED ? cache[cache_map[index[i]],:]
 *                                                   : host_table[index[i],:]
 * host_table: device-visible pointer of the pinned host table (zero-copy). */
int nts_hip_gather_rows_cached(nts_hip_ctx *ctx, const float *cache, uint64_t ld_cache,
                               const uint32_t *cache_map, const float *host_table,
                               uint64_t ld_host, const uint32_t *index, const uint32_t *n,
                               uint32_t n_cap, uint32_t feature_size, float *out,
                               uint64_t ld_out);

/* ---- sampled aggregation ------------------------------------------------ */
/* Y[d,:] = sum_{e in [co[d],co[d+1])} w[e] * X[row(e),:], summed in CSC edge
 * order as (x*w)+acc with no FMA contraction — the exact arithmetic of
 * MiniBatchFuseOp::forward / nts_comp (core/ntsMiniBatchGraphOp.hpp:153-182,
 * core/ntsBaseOp.hpp:546-562).  row(e) = row_indices[e], or
 * x_row_map[row_indices[e]] when x_row_map != NULL (fused feature gather:
 * X is then the global feature table and x_row_map the layer's `source`).
 * Every row d < *v is written (no pre-zeroing needed).  Replaces
 * Gather_By_Dst_From_Src(_Spmm) (cuda/ntsCUDAGraphOP.cu:340-373,425-587). */
int nts_hip_spmm_csc_fwd(nts_hip_ctx *ctx, const uint32_t *column_offset,
                         const uint32_t *row_indices, const float *weight,
                         const uint32_t *v, uint32_t v_cap, const float *x, uint64_t ldx,
                         const uint32_t *x_row_map, uint32_t feature_size, float *y,
                         uint64_t ldy);
/* Full-neighbour aggregation over the GLOBAL CSC of `graph` (u64 offsets,
 * global ids on both sides) — layer-wise inference over the whole graph:
 *   Y[d,:] = (relu?)( sum_{e in [co[d],co[d+1])} w(e) * X[row_indices[e],:] )
 * for v_begin <= d < v_end, in nts_hip_spmm_csc_fwd's arithmetic (serial in
 * CSC edge order, (x*w)+acc, no contraction, from 0).  w(e) is the weight
 * nts_hip_sample_layer writes for that (src, dst) from the graph's degrees:
 * NTS_WEIGHT_SUM, NTS_WEIGHT_MEAN, or 1 for NTS_WEIGHT_NONE; MEAN_SAMPLED and
 * the UP_DEGREE bit are NTS_ERR_INVALID (they are properties of a sample).
 * No per-edge weight array is built.  An empty column writes a zero row; rows
 * outside [v_begin, v_end) are not touched; bit-identical from run to run.
 * Uses the context's scratch arena (2 V floats + 2 (v_end - v_begin) words).
 * The reference has no counterpart (its drivers score with sampled batches). */
int nts_hip_spmm_graph_fwd(nts_hip_ctx *ctx, const nts_graph_dev *graph,
                           uint64_t v_begin, uint64_t v_end, int weight_type, int relu,
                           const float *x, uint64_t ldx, uint32_t feature_size,
                           float *y, uint64_t ldy);
/* nts_hip_spmm_graph_fwd with per-edge coefficients: edge e uses
 * fl32(w(e) * edge_coef[e]), edge_coef one fp32 per edge of `graph` in CSC
 * order (under NTS_WEIGHT_NONE: edge_coef[e] itself).  The same contract
 * otherwise: order, hub columns by column slice, scratch, refused weight
 * types.  On the same destinations it gives, bit for bit, what
 * nts_hip_sample_layer_coef(fanout = -1) + nts_hip_spmm_csc_fwd give. */
int nts_hip_spmm_graph_fwd_coef(nts_hip_ctx *ctx, const nts_graph_dev *graph,
                                const float *edge_coef, uint64_t v_begin, uint64_t v_end,
                                int weight_type, int relu, const float *x, uint64_t ldx,
                                uint32_t feature_size, float *y, uint64_t ldy);
/* ---- f16 feature table (csrc/agghalf.hip; GCNConfig::feature_f16) ---------
 * The three gathers that read the feature table, over a table stored as IEEE
 * half: f16 storage, fp32 arithmetic.  xh / tableh hold the bits of the halves
 * (2-byte aligned at least), pitches of the half table are in halves, outputs
 * stay fp32.  Widening a half is exact, so each call gives, bit for bit, what
 * its fp32 sibling gives on the fp32 widening of the same table.  A lane loads
 * 16 bytes (8 halves) where the base is 16-byte aligned, the pitch a multiple
 * of 8 halves and the row, rounded up to 8, inside the pitch (the partial last
 * vector then reads pitch padding of its own row); 8-, 4- or 2-byte loads
 * otherwise.  A NULL table, feature_size == 0, a pitch below feature_size or
 * an odd table address: NTS_ERR_INVALID with a message, nothing written.
 *
 * nts_hip_spmm_csc_fwd over a half table:
 *   Y[d,:] = sum_{e in [co[d],co[d+1])} w[e] * float(Xh[row(e),:])
 * serial in CSC edge order as (x*w)+acc from 0, no FMA contraction; weight
 * NULL: w = 1; row(e) through x_row_map when non-NULL (fused feature gather).
 * Every row d < *v (v NULL: v_cap) is written, empty columns as zeros; rows
 * >= *v and the pitch padding of Y are not touched. */
int nts_hip_spmm_csc_fwd_h(nts_hip_ctx *ctx, const uint32_t *column_offset,
                           const uint32_t *row_indices, const float *weight,
                           const uint32_t *v, uint32_t v_cap, const uint16_t *xh, uint64_t ldxh,
                           const uint32_t *x_row_map, uint32_t feature_size, float *y,
                           uint64_t ldy);
/* nts_hip_spmm_graph_fwd over a half table (layer 0 of the full-neighbour
 * pass): the same weights (SUM, MEAN, NONE; MEAN_SAMPLED and the UP_DEGREE bit
 * are NTS_ERR_INVALID, as is a range outside the graph), the same order, hub
 * columns (more than 2,048 edges) split by column slice and never by edge
 * range, optional relu.  The same scratch. */
int nts_hip_spmm_graph_fwd_h(nts_hip_ctx *ctx, const nts_graph_dev *graph,
                             uint64_t v_begin, uint64_t v_end, int weight_type, int relu,
                             const uint16_t *xh, uint64_t ldxh, uint32_t feature_size,
                             float *y, uint64_t ldy);
/* nts_hip_spmm_graph_fwd_coef over a half table. */
int nts_hip_spmm_graph_fwd_coef_h(nts_hip_ctx *ctx, const nts_graph_dev *graph,
                                  const float *edge_coef, uint64_t v_begin, uint64_t v_end,
                                  int weight_type, int relu, const uint16_t *xh, uint64_t ldxh,
                                  uint32_t feature_size, float *y, uint64_t ldy);
/* out[i,:] = float(tableh[index[i],:]) for i < *n (n == NULL: n_cap rows):
 * nts_hip_gather_rows from a half table into fp32 rows. */
int nts_hip_gather_rows_h(nts_hip_ctx *ctx, const uint16_t *tableh, uint64_t ld_table,
                          const uint32_t *index, const uint32_t *n, uint32_t n_cap,
                          uint32_t feature_size, float *out, uint64_t ld_out);
/* Stage the NON-cached rows of a layer's sources once into HBM:
 *   stage[i,:] = host_table[index[i],:]  for every i with cache_map[index[i]] ==
 *   NTS_NOT_CACHED (other rows of stage are left untouched).
 * The host link then carries each distinct spilled row once per batch
 * instead of once per sampled edge. */
int nts_hip_stage_uncached_rows(nts_hip_ctx *ctx, const uint32_t *cache_map,
                                const float *host_table, uint64_t ld_host, const uint32_t *index,
                                const uint32_t *n, uint32_t n_cap, uint32_t feature_size,
                                float *stage, uint64_t ld_stage);
/* nts_hip_spmm_csc_fwd with the fused feature gather reading the two-tier
 * table: for local src r = row_indices[e] and g = x_row_map[r], the row comes
 * from cache[cache_map[g],:] when cached, else from spill[host_local ? r : g,:]
 * — the pinned host table (host_local = 0) or the rows staged by
 * nts_hip_stage_uncached_rows (host_local = 1).  load_feature_gpu_cache + the
 * bottom graph op; bit-identical to nts_hip_spmm_csc_fwd on the full table
 * for every cache content. */
int nts_hip_spmm_csc_fwd_cached(nts_hip_ctx *ctx, const uint32_t *column_offset,
                                const uint32_t *row_indices, const float *weight,
                                const uint32_t *v, uint32_t v_cap, const float *cache,
                                uint64_t ld_cache, const uint32_t *cache_map,
                                const float *spill, uint64_t ld_spill, int host_local,
                                const uint32_t *x_row_map, uint32_t feature_size, float *y,
                                uint64_t ldy);
/* G_in[s,:] = sum_{j in [ro[s],ro[s+1])} w_b[j] * G_out[ci[j],:] (ascending dst
 * order, deterministic, atomic-free).  Replaces Gather_By_Src_From_Dst_Spmm
 * (cuda/ntsCUDAGraphOP.cu:901-1042) and MiniBatchFuseOp::backward
 * (core/ntsMiniBatchGraphOp.hpp:214-268). */
int nts_hip_spmm_csr_bwd(nts_hip_ctx *ctx, const uint32_t *row_offset,
                         const uint32_t *column_indices, const float *weight_backward,
                         const uint32_t *s, uint32_t s_cap, const float *g_out,
                         uint64_t ld_gout, uint32_t feature_size, float *g_in,
                         uint64_t ld_gin);
/* nts_hip_spmm_csr_bwd that also leaves its output's column maxima per part
 * of R = nts_hip_csr_bwd_colmax_rows_per_part(feature_size) rows:
 * part_max[p * feature_size + c] = the float bits of max |rs(s) G_in[s, c]|
 * over s in [p R, (p+1) R) (0 past the live rows; exact — an unordered max),
 * ceil(s_cap / R) parts, with the row scale rs(s) = row_scale[row_map[s]]
 * (row_map NULL: row_scale[s]; row_scale NULL: 1).  With the pair table's row
 * scales and the GEMM's row map these are exactly the operand maxima
 * nts_hip_gemm_h2p_tn_gather_cm takes when G_in is its B, so that GEMM reads
 * G_in once.  feature_size <= 512, G rows 16-byte aligned with ld % 4 == 0. */
uint32_t nts_hip_csr_bwd_colmax_rows_per_part(uint32_t feature_size);
int nts_hip_spmm_csr_bwd_colmax(nts_hip_ctx *ctx, const uint32_t *row_offset,
                                const uint32_t *column_indices, const float *weight_backward,
                                const uint32_t *s, uint32_t s_cap, const float *g_out,
                                uint64_t ld_gout, uint32_t feature_size, float *g_in,
                                uint64_t ld_gin, uint32_t *part_max, const float *row_scale,
                                const uint32_t *row_map);
/* Transform-first bottom layer: when the layer narrows the rows
 * (F_in > F_out), A (X W) replaces (A X) W — the reference aggregates first
 * (SingleGPUAllSampleGraphOp::forward then Parameter::forward,
 * toolkits/GCN_SAMPLE_GPU.hpp:252-266); both are linear, so they agree up to
 * fp32 summation order.  The aggregation then runs over F_out-wide rows and
 * vertexForward's activation moves into its epilogue:
 *   y = dropout(relu(A x), p) with the Philox keep bits of
 *   nts_hip_gemm_relu_dropout_f32 (same seed/offset/(row, col) keys, so both
 *   orders drop the same elements); p == 0: relu only.  A, weights, v as in
 *   nts_hip_spmm_csc_fwd (no row map). */
int nts_hip_spmm_csc_fwd_act(nts_hip_ctx *ctx, const uint32_t *column_offset,
                             const uint32_t *row_indices, const float *weight, const uint32_t *v,
                             uint32_t v_cap, const float *x, uint64_t ldx, uint32_t feature_size,
                             float *y, uint64_t ldy, float p, uint64_t seed, uint64_t offset);
/* Its backward through the CSR, the activation's backward fused into the loads:
 *   G_in[s,:] = sum_j w_b[j] * (G_out[ci[j],:] ⊙ [X_act[ci[j],:] > 0] * scale)
 * (X_act = the forward output of nts_hip_spmm_csc_fwd_act, scale = 1/(1-p));
 * ascending dst order, deterministic. */
int nts_hip_spmm_csr_bwd_masked(nts_hip_ctx *ctx, const uint32_t *row_offset,
                                const uint32_t *column_indices, const float *weight_backward,
                                const uint32_t *s, uint32_t s_cap, const float *g_out,
                                uint64_t ld_gout, const float *x_act, uint64_t ld_act, float scale,
                                uint32_t feature_size, float *g_in, uint64_t ld_gin);
/* A graph-op backward whose result feeds that activation's backward:
 *   G_in[s,:] = (sum_j w_b[j] * G_out[ci[j],:]) ⊙ [X_act[s,:] > 0] * scale
 * — nts_hip_spmm_csr_bwd followed by nts_hip_act_backward on its output, in
 * one pass, the same arithmetic (the mask is read once per output row). */
int nts_hip_spmm_csr_bwd_postmask(nts_hip_ctx *ctx, const uint32_t *row_offset,
                                  const uint32_t *column_indices, const float *weight_backward,
                                  const uint32_t *s, uint32_t s_cap, const float *g_out,
                                  uint64_t ld_gout, const float *x_act, uint64_t ld_act, float scale,
                                  uint32_t feature_size, float *g_in, uint64_t ld_gin);
/* The same pair with the activation's keep mask [X_act > 0] carried as bits
 * instead of re-read from X_act's rows (16 bytes a 128-float row instead of
 * 512): nts_hip_act_bits_words(F) words per row (0: F unsupported — F must be
 * a multiple of 4 from 68 to 2048; the caller then uses the float forms),
 * 16-byte aligned.
 * nts_hip_spmm_csc_fwd_act_bits = nts_hip_spmm_csc_fwd_act that also writes
 * mask_bits[v_cap rows]; nts_hip_spmm_csr_bwd_postmask_bits =
 * nts_hip_spmm_csr_bwd_postmask reading those bits (X_act's rows = g_in's
 * rows).  Results identical to the float forms. */
uint32_t nts_hip_act_bits_words(uint32_t feature_size);
int nts_hip_spmm_csc_fwd_act_bits(nts_hip_ctx *ctx, const uint32_t *column_offset,
                                  const uint32_t *row_indices, const float *weight,
                                  const uint32_t *v, uint32_t v_cap, const float *x, uint64_t ldx,
                                  uint32_t feature_size, float *y, uint64_t ldy, float p,
                                  uint64_t seed, uint64_t offset, uint32_t *mask_bits);
int nts_hip_spmm_csr_bwd_postmask_bits(nts_hip_ctx *ctx, const uint32_t *row_offset,
                                       const uint32_t *column_indices,
                                       const float *weight_backward, const uint32_t *s,
                                       uint32_t s_cap, const float *g_out, uint64_t ld_gout,
                                       const uint32_t *mask_bits, float scale,
                                       uint32_t feature_size, float *g_in, uint64_t ld_gin);
/* The activation's backward alone: out = g ⊙ [x_act > 0] * scale ([rows x
 * feature_size], each with its leading dimension) — what libtorch's relu and
 * dropout backward compute for vertexForward (toolkits/GCN_SAMPLE_GPU.hpp:252-266),
 * in one pass; followed by nts_hip_spmm_csr_bwd it equals
 * nts_hip_spmm_csr_bwd_masked (same arithmetic per element). */
int nts_hip_act_backward(nts_hip_ctx *ctx, uint32_t rows, uint32_t feature_size, const float *g,
                         uint64_t ldg, const float *x_act, uint64_t ldx, float scale, float *out,
                         uint64_t ldo);
/* G_in[row_indices[e],:] += w[e] * G_out[d,:] with float atomics over the CSC
 * (g_in must be zeroed by the caller; summation order is not deterministic).
 * Replaces Push_From_Dst_To_Src_Spmm (cuda/ntsCUDAGraphOP.cu:621-770). */
int nts_hip_spmm_csc_bwd_atomic(nts_hip_ctx *ctx, const uint32_t *column_offset,
                                const uint32_t *row_indices, const float *weight,
                                const uint32_t *v, uint32_t v_cap, const float *g_out,
                                uint64_t ld_gout, uint32_t feature_size, float *g_in,
                                uint64_t ld_gin);

/* ---- NeutronOrch PD cache (toolkits/GCN_SAMPLE_PD_CACHE.hpp) -------------- */
/* preSample's hot-vertex count (get_most_neighbor, core/ntsBaseOp.hpp:330-404):
 * old[seeds[i]] = 1; then (layers - 1) times new[u] += old[v] for every
 * in-neighbour u of v in the CSC (column_offset[v] .. [v+1]); counts = the
 * last `new` (all zeros when layers == 1, as the reference's).  tmp: [V]. */
int nts_hip_presample_counts(nts_hip_ctx *ctx, const nts_graph_dev *graph, const uint32_t *seeds,
                             uint32_t n_seeds, int layers, uint32_t *counts, uint32_t *tmp);
/* ... and its selection: total = (number of non-zero counts) + 1 (V when none
 * is zero), n = (uint32)((float)total * cache_rate) (clamped to V), pivot =
 * the n-th largest count (0-based, descending), out_ids = the first n vertex
 * ids in ascending order whose count >= pivot (the reference's single-thread
 * order), *out_n = n (device scalar).  out_ids: [V]. */
int nts_hip_presample_select(nts_hip_ctx *ctx, const uint32_t *counts, uint64_t n_vertices,
                             float cache_rate, uint32_t *out_ids, uint32_t *out_n);
/* set_cache_index for one super-batch: cache_map[ids[i]] = key,
 * cache_location[ids[i]] = i for i < n (gnndatum->set_cache_index). */
int nts_hip_pd_set_cache(nts_hip_ctx *ctx, const uint32_t *ids, uint32_t n, uint32_t key,
                         uint32_t *cache_map, uint32_t *cache_location);
/* load_share_embedding (dev_load_share_embedding_kernel,
 * cuda/ntsCUDATransferKernel.cuh:454-500): for the bottom layer's dsts
 * i < *v, emb[i,:] = share[omit_row[i],:] when omit_row[i] != NTS_NOT_CACHED
 * (omit_row: written by nts_hip_sample_layer with omit_map; rows of other dsts
 * untouched).  The reference tests cache_map[dst[i]] == super_batch_id at
 * this point; the sampled layer's own record is the same decision, taken when
 * it was sampled, so a later super-batch may already reuse cache_map. */
int nts_hip_pd_load_share(nts_hip_ctx *ctx, const uint32_t *omit_row, const uint32_t *v,
                          uint32_t v_cap, const float *share, uint64_t ld_share,
                          uint32_t feature_size, float *emb, uint64_t ld_emb);
/* vertexForward's activation alone, y = dropout(relu(x), p) with the keep
 * bits of nts_hip_gemm_relu_dropout_f32 (same seed/offset/(row, col) keys):
 * after a GEMM whose rows are replaced by the PD cache. */
int nts_hip_relu_dropout_f32(nts_hip_ctx *ctx, uint32_t rows, uint32_t feature_size,
                             const float *x, uint64_t ldx, float p, uint64_t seed,
                             uint64_t offset, float *y, uint64_t ldy);

/* ---- LayerNorm + relu + dropout of a hidden layer (no reference counterpart) */
/* y = dropout(relu(LayerNorm(z)), p) over [rows x feature_size] in one pass:
 * per row r, mu = mean_c z[r,c], var = mean_c (z[r,c] - mu)^2 (the centred,
 * two-pass form on the row held in registers, never E[z^2] - mu^2; the centred
 * row is re-centred once, d -= mean_c d, which takes the rounding of the float
 * mu out of it), rstd = 1 / sqrt(var + eps),
 *   n = gamma[c] (z - mu) rstd + beta[c],  y = keep ? relu(n) / (1 - p) : 0,
 * with the keep bits, the 1 / (1 - p) float scale and the p >= 1 rule of
 * nts_hip_relu_dropout_f32 / nts_hip_gemm_relu_dropout_f32 for the same (seed,
 * offset, row, col): the masks are interchangeable.  mean / rstd [rows] receive
 * mu and rstd for the backward; both may be NULL (eval / inference: nothing
 * saved, the same y).  One wave per row, four rows per 256-thread block, the
 * row read once and written once; wave reductions are butterflies in a fixed
 * lane order and there are no atomics: two calls give the same bytes.
 * 1 <= feature_size <= 1024.  float4 where feature_size % 4 == 0, z, y, gamma
 * and beta are 16-byte aligned and both pitches are multiples of 4; scalar
 * otherwise, over the same range.  A wider row returns NTS_ERR_INVALID and
 * writes nothing; rows == 0 succeeds and writes nothing. */
int nts_hip_ln_act_fwd(nts_hip_ctx *ctx, uint64_t rows, uint32_t feature_size, const float *z,
                       uint64_t ldz, const float *gamma, const float *beta, float eps, float p,
                       uint64_t seed, uint64_t offset, float *y, uint64_t ldy, float *mean,
                       float *rstd);
/* Its backward, from the forward's y, z, mean and rstd (scale = 1 / (1 - p),
 * 0 for p >= 1):  xh = (z - mean) rstd (re-centred as the forward's: the same
 * bits),  g = dy [y > 0] scale,  t = g gamma,
 *   dz = rstd (t - mean_c t - xh mean_c (t xh)),
 *   dbeta[c] = sum_r g,  dgamma[c] = sum_r g xh.
 * dz: one wave per row.  dgamma / dbeta: each block owns a contiguous run of
 * rows whose length depends on `rows` alone (never on the device or on
 * timing); a wave walks its quarter of the run in row order, the block adds
 * its four waves in order and writes a [2 feature_size] partial into the
 * context's scratch; a second kernel sums the partials in block order (four
 * contiguous segments, then the segments in order).  No float atomics: two
 * calls give the same bytes.  rows == 0 writes zeros to dgamma / dbeta.  The
 * width limit, the float4 rule (over dy, y, z, dz and gamma) and the refusal
 * are the forward's; the refusal comes before any write. */
int nts_hip_ln_act_bwd(nts_hip_ctx *ctx, uint64_t rows, uint32_t feature_size, const float *dy,
                       uint64_t lddy, const float *y, uint64_t ldy, const float *z, uint64_t ldz,
                       const float *mean, const float *rstd, const float *gamma, float scale,
                       float *dz, uint64_t lddz, float *dgamma, float *dbeta);

/* ---- BatchNorm + relu + dropout of a hidden layer (no reference counterpart) */
/* Training forward, torch.nn.BatchNorm1d's semantics over [rows x feature_size]:
 * per column c, n = rows,
 *   mu = mean_r z[r,c],  var = mean_r (z[r,c] - mu)^2 (biased),
 *   rstd = 1 / sqrt(var + eps),  xh = (z - mu) rstd,
 *   y = keep ? relu(gamma[c] xh + beta[c]) / (1 - p) : 0,
 *   running_mean[c] <- (1 - momentum) running_mean[c] + momentum mu,
 *   running_var[c]  <- (1 - momentum) running_var[c]  + momentum var n / (n - 1),
 * with the keep bits, the float scale and the p >= 1 rule of
 * nts_hip_relu_dropout_f32 for the same (seed, offset, row, col).  mean / rstd
 * [feature_size] receive mu and rstd for the backward.  running_mean /
 * running_var may be NULL (no update); rows == 1 leaves them untouched (the
 * unbiased variance does not exist) and gives var = 0, xh = 0.
 * The variance is never E[z^2] - mu^2: z is read once by a statistics kernel in
 * which a block owns a contiguous run of rows whose length depends on `rows`
 * alone, each thread keeps a Welford (count, mean, M2) over its rows in row
 * order, and the partials are merged by Chan's formula in a fixed order (the
 * threads of a column, then the blocks, by a second kernel whose one thread
 * per column also updates the running statistics).  A third, elementwise
 * kernel reads z and writes y: 12 feature_size bytes per row in all.  No
 * atomics: two calls give the same bytes.  A column constant over the rows has
 * var = 0 and xh = 0 exactly.
 * 1 <= feature_size <= 1024.  float4 where feature_size % 4 == 0, every
 * pointer is 16-byte aligned and both pitches are multiples of 4; scalar
 * otherwise.  A wider row returns NTS_ERR_INVALID and writes nothing;
 * rows == 0 succeeds and writes nothing. */
int nts_hip_bn_act_fwd(nts_hip_ctx *ctx, uint64_t rows, uint32_t feature_size, const float *z,
                       uint64_t ldz, const float *gamma, const float *beta, float eps,
                       float momentum, float p, uint64_t seed, uint64_t offset, float *y,
                       uint64_t ldy, float *mean, float *rstd, float *running_mean,
                       float *running_var);
/* Eval mode, one elementwise pass that updates nothing:
 *   y = relu(gamma (z - running_mean) / sqrt(running_var + eps) + beta). */
int nts_hip_bn_act_eval(nts_hip_ctx *ctx, uint64_t rows, uint32_t feature_size, const float *z,
                        uint64_t ldz, const float *gamma, const float *beta,
                        const float *running_mean, const float *running_var, float eps, float *y,
                        uint64_t ldy);
/* The training forward's backward, from its y, z, mean and rstd (scale =
 * 1 / (1 - p), 0 for p >= 1):  g = dy [y > 0] scale,
 *   dbeta[c] = sum_r g,  dgamma[c] = sum_r g xh,
 *   dz = gamma rstd (g - dbeta / n - xh dgamma / n).
 * One reduction pass over (dy, y, z) in the statistics kernel's tiling writes
 * per-block partials (sum g, sum g (z - mean) rstd, sum (z - mean)), which a
 * second kernel sums in block order (nts_hip_ln_act_bwd's order); one
 * elementwise pass then writes dz: 28 feature_size bytes per row.  The third
 * sum recovers what rounding the saved mean to a float dropped, d = mean_r
 * (z - mean): forward and backward centre with it, xh = ((z - mean) - d) rstd.  No atomics: two calls give the same bytes.
 * rows == 0 writes zeros to dgamma / dbeta and nothing else.  Width limit,
 * float4 rule and refusal as the forward's. */
int nts_hip_bn_act_bwd(nts_hip_ctx *ctx, uint64_t rows, uint32_t feature_size, const float *dy,
                       uint64_t lddy, const float *y, uint64_t ldy, const float *z, uint64_t ldz,
                       const float *mean, const float *rstd, const float *gamma, float scale,
                       float *dz, uint64_t lddz, float *dgamma, float *dbeta);

/* ---- GAT layer on a merged src/dst sampled block ------------------------- */
/* The GAT_SAMPLE_ALL_GPU layer (toolkits/GAT_SAMPLE_ALL_GPU.hpp:308-391:
 * BatchGPUSrcDstScatterOp -> leaky_relu(msg . W_att, 0.2) -> BatchGPUEdgeSoftMax
 * -> e_msg * a -> BatchGPUAggregateDst -> relu; core/ntsPushdownGraphOp.hpp:490-748)
 * without materialising the [e, 2F] messages.  H = X W [src_size x F] is the
 * layer's transformed input (caller's GEMM); att = W_att [2F] (a1 = att[0:F]
 * for the source half, a2 = att[F:2F] for the destination half).  Forward:
 *   m[e] = leaky_relu(H[src_e].a1 + H[dst_local(d)].a2, 0.2),
 *   a[e] = softmax over the edges of d of m,  Y[d] = relu(sum_e a[e] H[src_e]).
 * One wave per destination, online softmax (running max/sum), edge order.
 * Width limit (a lane holds at most 4 vectors of a row): F <= 1024 when F is a
 * multiple of 4, every row pointer and att are 16-byte aligned and every
 * pitch is a multiple of 4 (float4 path); F <= 256 otherwise (scalar path).
 * The backward applies the same rule to all of its row operands, so it may
 * take the scalar path where the forward took float4.  A wider F returns
 * NTS_ERR_INVALID and writes nothing. */
int nts_hip_gat_forward(nts_hip_ctx *ctx, const uint32_t *column_offset,
                        const uint32_t *row_indices, const uint32_t *dst_local_id,
                        uint32_t v_size, const float *H, uint64_t ldh, uint32_t F,
                        const float *att, float *m_out, float *a_out, float *Y, uint64_t ldy);
/* Its backward for dL/dY = GY (deterministic: a per-destination pass and a
 * per-source pass over the CSR with csr_edge_id; no atomics):
 *   du[e] = dL/d(pre-leaky score of e), ds2[v] = dL/d(H[v].a2) (zero for
 *   non-destinations), GM [v_size x F] = GY masked by Y > 0 (scratch, ld ldm),
 *   dH [src_size x F] = dL/dH, dS [src_size x 2] =
 *   (dL/d(H[v].a1), dL/d(H[v].a2)) so that dW_att = H^T dS (caller's GEMM). */
int nts_hip_gat_backward(nts_hip_ctx *ctx, const uint32_t *column_offset,
                         const uint32_t *row_indices, const uint32_t *dst_local_id,
                         uint32_t v_size, const uint32_t *row_offset,
                         const uint32_t *column_indices, const uint32_t *csr_edge_id,
                         uint32_t src_size, const float *H, uint64_t ldh, uint32_t F,
                         const float *att, const float *a, const float *m, const float *Y,
                         uint64_t ldy, const float *GY, uint64_t ldg, float *du, float *ds2,
                         float *GM, uint64_t ldm, float *dH, uint64_t lddh, float *dS);
/* The multi-head layer: K = heads heads of D columns, F = K D.  Head h owns
 * columns [hD, (h+1)D) of H, of a1 = att[0:F] and of a2 = att[F:2F], and has a
 * softmax of its own over the edges of each destination:
 *   m[e,h] = leaky_relu(H[src_e]_h . a1_h + H[dst_local(d)]_h . a2_h, 0.2),
 *   a[e,h] = softmax over the edges of d of m[., h],  Z_h[d] = sum_e a[e,h] H[src_e]_h;
 *   mean == 0 (concat): Y[d] = relu([Z_0 | ... | Z_{K-1}])   (F wide)
 *   mean != 0:          Y[d] = relu((1/K) sum_h Z_h[d])      (D wide)
 * m_out / a_out / du are edge-major [e, K], ds2 is [src_size, K], dS is
 * [src_size, 2K] (ds1 of every head, then ds2 of every head: dW_att's a1 part
 * is sum_v H[v,hD+j] dS[v,h], its a2 part the same with dS[v,K+h]).  Y and GY
 * are F wide (concat) or D wide (mean); GM and dH are F wide, GM holding GY
 * (mean: GY / K, for every head) masked by Y > 0.  The neighbour row is read
 * once for all heads (one wave per destination / source, as above).  Width
 * limit: F <= 1024 on the float4 path, which needs D % 4 == 0 besides the
 * single-head rule on F, the pitches and the pointers; F <= 256 otherwise.
 * heads == 0, D == 0 or a wider F return NTS_ERR_INVALID and write nothing
 * (the backward's clearing of ds2 included).  heads == 1 computes the
 * single-head layer (both modes). */
int nts_hip_gat_forward_heads(nts_hip_ctx *ctx, const uint32_t *column_offset,
                              const uint32_t *row_indices, const uint32_t *dst_local_id,
                              uint32_t v_size, const float *H, uint64_t ldh, uint32_t heads,
                              uint32_t D, const float *att, float *m_out, float *a_out, float *Y,
                              uint64_t ldy, int mean);
int nts_hip_gat_backward_heads(nts_hip_ctx *ctx, const uint32_t *column_offset,
                               const uint32_t *row_indices, const uint32_t *dst_local_id,
                               uint32_t v_size, const uint32_t *row_offset,
                               const uint32_t *column_indices, const uint32_t *csr_edge_id,
                               uint32_t src_size, const float *H, uint64_t ldh, uint32_t heads,
                               uint32_t D, const float *att, const float *a, const float *m,
                               const float *Y, uint64_t ldy, const float *GY, uint64_t ldg,
                               float *du, float *ds2, float *GM, uint64_t ldm, float *dH,
                               uint64_t lddh, float *dS, int mean);
/* The dropout forms of the four entry points above (no reference counterpart:
 * the reference's GAT stores drop_rate and never uses it).  p_attn drops the
 * normalised attention coefficients, p_out the written Y:
 *   a[e,h]  = the softmax over ALL edges of d, as above (what a_out receives)
 *   a~[e,h] = keepA(e,h) ? a[e,h] / (1 - p_attn) : 0
 *   Z_h[d]  = sum_e a~[e,h] H[src_e]_h,   Y = relu(concat or mean of Z_h)
 *   Y[d,c] <- keepF(d,c) ? Y[d,c] / (1 - p_out) : 0.
 * Keep bits, the 1 / (1 - p) float scale and the p >= 1 rule are those of
 * nts_hip_relu_dropout_f32 under key `seed`: keepA(e,h) is the bit of element
 * (row = CSC edge position e, col = h) at offset off_attn, keepF(d,c) that of
 * element (d, c) of Y at offset off_out, so either mask is what
 * nts_hip_relu_dropout_f32 leaves of a ones tensor of that shape.  The
 * backward takes the forward's a (undropped), m and Y, regenerates keepA (no
 * mask is stored) and reads keepF off Y > 0:
 *   GM = GY [Y > 0] / (1 - p_out) (mean: / K),
 *   ga[e,h] = (GM[d]_h . H[src_e]_h) keepA(e,h) / (1 - p_attn),
 *   du = a (ga - sum_e a ga) leaky',  dH[v] = sum_e a~[e] GM[d_e] + ds1 a1 + ds2 a2.
 * Edge order and the absence of atomics are those of the plain forms: two
 * calls give the same bytes.  With both rates 0 the plain kernels run (the
 * same bytes as the plain entry points).  Width limits and refusals are the
 * plain forms'; a rate that is negative, above 1 or NaN returns
 * NTS_ERR_INVALID.  Every refusal comes before any write. */
int nts_hip_gat_forward_drop(nts_hip_ctx *ctx, const uint32_t *column_offset,
                             const uint32_t *row_indices, const uint32_t *dst_local_id,
                             uint32_t v_size, const float *H, uint64_t ldh, uint32_t F,
                             const float *att, float *m_out, float *a_out, float *Y, uint64_t ldy,
                             float p_attn, float p_out, uint64_t seed, uint64_t off_attn,
                             uint64_t off_out);
int nts_hip_gat_backward_drop(nts_hip_ctx *ctx, const uint32_t *column_offset,
                              const uint32_t *row_indices, const uint32_t *dst_local_id,
                              uint32_t v_size, const uint32_t *row_offset,
                              const uint32_t *column_indices, const uint32_t *csr_edge_id,
                              uint32_t src_size, const float *H, uint64_t ldh, uint32_t F,
                              const float *att, const float *a, const float *m, const float *Y,
                              uint64_t ldy, const float *GY, uint64_t ldg, float *du, float *ds2,
                              float *GM, uint64_t ldm, float *dH, uint64_t lddh, float *dS,
                              float p_attn, float p_out, uint64_t seed, uint64_t off_attn);
int nts_hip_gat_forward_heads_drop(nts_hip_ctx *ctx, const uint32_t *column_offset,
                                   const uint32_t *row_indices, const uint32_t *dst_local_id,
                                   uint32_t v_size, const float *H, uint64_t ldh, uint32_t heads,
                                   uint32_t D, const float *att, float *m_out, float *a_out,
                                   float *Y, uint64_t ldy, int mean, float p_attn, float p_out,
                                   uint64_t seed, uint64_t off_attn, uint64_t off_out);
int nts_hip_gat_backward_heads_drop(nts_hip_ctx *ctx, const uint32_t *column_offset,
                                    const uint32_t *row_indices, const uint32_t *dst_local_id,
                                    uint32_t v_size, const uint32_t *row_offset,
                                    const uint32_t *column_indices, const uint32_t *csr_edge_id,
                                    uint32_t src_size, const float *H, uint64_t ldh, uint32_t heads,
                                    uint32_t D, const float *att, const float *a, const float *m,
                                    const float *Y, uint64_t ldy, const float *GY, uint64_t ldg,
                                    float *du, float *ds2, float *GM, uint64_t ldm, float *dH,
                                    uint64_t lddh, float *dS, int mean, float p_attn, float p_out,
                                    uint64_t seed, uint64_t off_attn);
/* Plain inverted dropout with the same keep bits (no relu: the input pass of
 * gat_feat_drop, whose features may be negative): y = keep(row, col) ?
 * x / (1 - p) : 0 over [rows x feature_size]; y == x is allowed. */
int nts_hip_dropout_f32(nts_hip_ctx *ctx, uint32_t rows, uint32_t feature_size, const float *x,
                        uint64_t ldx, float p, uint64_t seed, uint64_t offset, float *y,
                        uint64_t ldy);
/* The GATv2 layer (Brody et al., ICLR 2022: "dynamic" attention; no reference
 * counterpart), K = heads heads of D columns, F = K D.  Hs [src_size, F] holds
 * the source rows X W_s (also the aggregated values), Hd [v_size, F] one row
 * X[dst] W_d per destination, in destination order (no dst_local_id), att [F]
 * the score vectors of the K heads:
 *   t[e]   = leaky_relu(Hs[src_e] + Hd[d_e], 0.2)        (F wide, never stored)
 *   u[e,h] = t[e]_h . att_h                               (u_out, edge-major [e, K])
 *   a[e,h] = softmax over the edges of d of u[., h]       (a_out, [e, K], undropped)
 *   a~[e,h] = keepA(e,h) ? a[e,h] / (1 - p_attn) : 0      (a itself when p_attn == 0)
 *   Z_h[d] = sum_e a~[e,h] Hs[src_e]_h
 *   mean == 0: Y[d] = relu([Z_0 | ... | Z_{K-1}]) (F wide);  mean != 0: relu((1/K) sum_h Z_h) (D wide)
 *   Y[d,c] <- keepF(d,c) ? Y[d,c] / (1 - p_out) : 0.
 * Empty columns give a zero row; edge order, the keep bits (element (e, h) at
 * off_attn, element (d, c) of Y at off_out, key `seed`), the 1 / (1 - p) float
 * scales and the p >= 1 rule are those of nts_hip_gat_forward_heads_drop; with
 * both rates 0 the plain kernels run.  Backward, for GY = dL/dY (Y / GY F or D
 * wide as in the forward; du [e, K]; GM, dHs, dHd F wide; datt [F]):
 *   GM[d]   = GY[d] [Y > 0] / (1 - p_out)                 (mean: / K, for every head)
 *   ga[e,h] = (GM[d]_h . Hs[src_e]_h) keepA(e,h) / (1 - p_attn)
 *   du[e,h] = a[e,h] (ga[e,h] - sum_e a ga)               (dL/du)
 *   q[e][c] = du[e, head(c)] att[c] leaky'(Hs[src_e][c] + Hd[d_e][c])
 *   dHd[d]  = sum_{e of d} q[e]                           (CSC order)
 *   dHs[v]  = sum_{e: src_e = v} (a~[e] GM[d_e] + q[e])   (CSR order, via csr_edge_id)
 *   datt[c] = sum_e du[e, head(c)] t[e][c]
 * with leaky' = 1 for a positive sum and 0.2 otherwise, recomputed from Hs and
 * Hd.  Nothing F wide per edge is written.  No float atomics: datt is summed
 * over fixed runs of destinations (their length a function of v_size alone),
 * the partial rows (in the context's scratch) then added in order, so two
 * calls give the same bytes for every output.  Width limit: F <= 1024 on the
 * float4 path (D % 4 == 0, every row pointer and att 16-byte aligned, every
 * pitch a multiple of 4, over all row operands of the call), F <= 256
 * otherwise.  A wider F, heads == 0, D == 0 or a rate that is negative, above
 * 1 or NaN return NTS_ERR_INVALID with a message that states the limits,
 * before any write. */
int nts_hip_gatv2_forward(nts_hip_ctx *ctx, const uint32_t *column_offset,
                          const uint32_t *row_indices, uint32_t v_size, const float *Hs,
                          uint64_t ldhs, const float *Hd, uint64_t ldhd, uint32_t heads,
                          uint32_t D, const float *att, float *u_out, float *a_out, float *Y,
                          uint64_t ldy, int mean, float p_attn, float p_out, uint64_t seed,
                          uint64_t off_attn, uint64_t off_out);
int nts_hip_gatv2_backward(nts_hip_ctx *ctx, const uint32_t *column_offset,
                           const uint32_t *row_indices, uint32_t v_size,
                           const uint32_t *row_offset, const uint32_t *column_indices,
                           const uint32_t *csr_edge_id, uint32_t src_size, const float *Hs,
                           uint64_t ldhs, const float *Hd, uint64_t ldhd, uint32_t heads,
                           uint32_t D, const float *att, const float *a, const float *Y,
                           uint64_t ldy, const float *GY, uint64_t ldg, float *du, float *GM,
                           uint64_t ldm, float *dHs, uint64_t lddhs, float *dHd, uint64_t lddhd,
                           float *datt, int mean, float p_attn, float p_out, uint64_t seed,
                           uint64_t off_attn);

/* ---- dense layer update (MFMA fp32) -------------------------------------- */
/* Row-major fp32 GEMM on the matrix cores (v_mfma_f32_16x16x4_f32 /
 * v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulate):
 *  trans_a == 0: C[M,N] = A[M,K] B[K,N]   — Parameter::forward x.matmul(W)
 *                (core/NtsScheduler.hpp:859-862)
 *  trans_a != 0: C[M,N] = A[K,M]^T B[K,N] — the weight gradient Y^T dZ that
 *                libtorch's matmul backward computes for it.
 * Long reductions are split over blocks and summed in a fixed order
 * (deterministic).  May grow the context's scratch arena. */
int nts_hip_gemm_f32(nts_hip_ctx *ctx, int trans_a, int M, int N, int K, const float *A,
                     uint64_t lda, const float *B, uint64_t ldb, float *C, uint64_t ldc);

/* Row-gathered forms for the transform-first bottom layer (A = the feature
 * table, a_rows = the layer's `source`, so the gathered rows never land in HBM
 * — the fused load_feature_gpu of core/ntsFastSampler.hpp:244-261):
 *   nts_hip_gemm_gather_f32:    C[i,:] = A[a_rows[i],:] B        (i < M; A rows of K floats)
 *   nts_hip_gemm_tn_gather_f32: C[M,N] = A[a_rows[0..K),:]^T B[K,N] (A rows of M floats)
 * Same kernels and summation order as nts_hip_gemm_f32 on the gathered matrix
 * (bit-identical to it). */
int nts_hip_gemm_gather_f32(nts_hip_ctx *ctx, int M, int N, int K, const float *A, uint64_t lda,
                            const uint32_t *a_rows, const float *B, uint64_t ldb, float *C,
                            uint64_t ldc);
int nts_hip_gemm_tn_gather_f32(nts_hip_ctx *ctx, int M, int N, int K, const float *A,
                               uint64_t lda, const uint32_t *a_rows, const float *B, uint64_t ldb,
                               float *C, uint64_t ldc);

/* Two-piece f16 forms of the two GEMMs above (csrc/gemmh2.hip), for a STATIC
 * A table pre-split once ("pair table"): row r is scaled by a power of two
 * rs[r] so that its largest |x| / rs[r] lies in [2^14, 2^15), and each
 * x / rs[r] is stored as one 32-bit word = f16 y0 (low half) + f16 y1 (high
 * half), y0 = f16(y), y1 = f16(y - y0): 22 significant bits.  Products run as
 * y0 b0 + y0 b1 + y1 b0 on the f16 MFMA with fp32 accumulation (three MFMAs
 * per k-slice where NTS_GEMM_SPLIT3 needs six), the scales applied exactly
 * to the fp32 result: error vs fp64 within a small factor of the fp32 GEMM's
 * (tests/test_gemm_h2.py).  Same operations as nts_hip_gemm_gather_f32 /
 * nts_hip_gemm_tn_gather_f32 on the transform-first bottom layer
 * (toolkits/GCN_SAMPLE_ALLGPU.hpp:247-266 x.matmul(W) and its weight gradient).
 *   nts_hip_h2_split_rows:  X [R x K] (ld ldx) -> P [R x Kp] words (ld ldp,
 *                           Kp % 32 == 0, zero past K) + rs [R]
 *   nts_hip_gemm_h2_gather: C[i,:] = act(X[a_rows[i],:] W) with X given as
 *                           (P, rs); W [K x N] fp32 (N % 16 == 0, N <= 1024);
 *                           relu_dropout != 0: the fused relu + inverted
 *                           dropout of nts_hip_gemm_relu_dropout_f32 (same
 *                           mask bits); a_rows NULL = rows 0..M-1
 *   nts_hip_gemm_h2_tn_gather: C[M,N] = X[a_rows[0..K),:M]^T op(B[K,N]),
 *                           op(B) = B, or B * bscale where Xm > 0 when Xm != NULL
 * May grow the context's scratch arena. */
int nts_hip_h2_split_rows(nts_hip_ctx *ctx, uint64_t R, uint32_t K, const float *X, uint64_t ldx,
                          uint32_t Kp, uint32_t *P, uint64_t ldp, float *rs);
int nts_hip_gemm_h2_gather(nts_hip_ctx *ctx, int relu_dropout, int M, int N, int Kp,
                           const uint32_t *P, uint64_t ldp, const float *rs, const uint32_t *a_rows,
                           const float *W, uint64_t ldw, int K, float *C, uint64_t ldc, float p,
                           uint64_t seed, uint64_t offset);
int nts_hip_gemm_h2_tn_gather(nts_hip_ctx *ctx, int M, int N, int K, const uint32_t *P, uint64_t ldp,
                              const float *rs, const uint32_t *a_rows, const float *B, uint64_t ldb,
                              const float *Xm, uint64_t ldx, float bscale, float *C, uint64_t ldc);
/* The same weight gradient on a "planar" pair table (per row the y0 plane of
 * Kp f16, then the y1 plane; row scales as above), whole rows streamed once by
 * LDS DMA, every output row in one block (csrc/gemmh2.hip k_h2_tn3):
 * N % 128 == 0, M <= 640, M <= Kp <= 640. */
int nts_hip_h2_split_rows_planar(nts_hip_ctx *ctx, uint64_t R, uint32_t K, const float *X,
                                 uint64_t ldx, uint32_t Kp, uint16_t *Q, uint64_t ldq, float *rs);
int nts_hip_gemm_h2p_tn_gather(nts_hip_ctx *ctx, int M, int N, int K, const uint16_t *Q, uint64_t ldq,
                               int Kp, const float *rs, const uint32_t *a_rows, const float *B,
                               uint64_t ldb, float *C, uint64_t ldc);
/* The same with per-part column maxima of |rs[a_rows[k]] B[k, c]| given
 * (part p = B rows [p R, (p+1) R), N words per part —
 * nts_hip_spmm_csr_bwd_colmax's output with row_scale = rs and row_map =
 * a_rows, R = rows_per_part): each k-chunk's column scales come from the
 * parts that cover its rows, with no pre-pass over B in the kernel. */
int nts_hip_gemm_h2p_tn_gather_cm(nts_hip_ctx *ctx, int M, int N, int K, const uint16_t *Q,
                                  uint64_t ldq, int Kp, const float *rs, const uint32_t *a_rows,
                                  const float *B, uint64_t ldb, float *C, uint64_t ldc,
                                  const uint32_t *part_max, uint32_t rows_per_part);
/* The forward GEMM on the planar table (k_h2_nn3: W's 16-column slices held
 * in registers, 16-row tiles of whole rows by LDS DMA): N % 128 == 0,
 * K <= Kp <= 640; arguments as nts_hip_gemm_h2_gather. */
int nts_hip_gemm_h2p_gather(nts_hip_ctx *ctx, int relu_dropout, int M, int N, int Kp, const uint16_t *Q,
                            uint64_t ldq, const float *rs, const uint32_t *a_rows, const float *W,
                            uint64_t ldw, int K, float *C, uint64_t ldc, float p, uint64_t seed,
                            uint64_t offset);

/* Layer forward on a dynamic fp32 input with at most 128 columns (the
 * aggregate-first layer of the products / papers-shaped configs, 100 or 128
 * -> 256): C = act(A W), A split into f16 pairs with power-of-two row scales
 * inside the kernel, W into pairs with column scales, 3 f16 MFMA products,
 * fp32 accumulate (the pair-table arithmetic of nts_hip_gemm_h2p_gather).
 * relu_dropout: the activation of nts_hip_gemm_relu_dropout_f32 (same Philox
 * keys, so the same elements are dropped).  K <= 128 with K % 4 == 0, A rows
 * 16-byte aligned, N 128 or 256.  Q != NULL: A's planar pair table
 * (rows of 2 Kp f16, Kp = K rounded up to 32) and row scales rs[M] are also
 * written (the weight gradient's operand). */
int nts_hip_gemm_h2d_act(nts_hip_ctx *ctx, int relu_dropout, int M, int N, int K, const float *A,
                         uint64_t lda, const float *W, uint64_t ldw, float *C, uint64_t ldc, float p,
                         uint64_t seed, uint64_t offset, uint16_t *Q, uint64_t ldq, float *rs);

/* Hidden-layer forward with its activation fused into the GEMM epilogue:
 *   C = dropout(relu(A B), p)   — vertexForward's
 *   torch::dropout(torch::relu(x.matmul(W)), drop_rate, training)
 *   (toolkits/GCN_SAMPLE_GPU.hpp:252-266).  Inverted dropout: kept elements
 *   are scaled by 1/(1-p); keep(row, col) comes from Philox4x32-10 keyed by
 *   `seed`, counter {row/4, col/2, offset}: 16 bits per element (word row%4,
 *   low half for even col, high half for odd col) >= floor(p*2^16), so the
 *   mask is reproducible and never stored.  p == 0: plain relu (eval). */
int nts_hip_gemm_relu_dropout_f32(nts_hip_ctx *ctx, int M, int N, int K, const float *A,
                                  uint64_t lda, const float *B, uint64_t ldb, float *C,
                                  uint64_t ldc, float p, uint64_t seed, uint64_t offset);

/* Its weight gradient: C[M,N] = A[K,M]^T (B ⊙ [X > 0] · scale), with B = dX
 * (the gradient of the layer output) and X the forward output, scale =
 * 1/(1-p): the relu and dropout backward fused into the operand load. */
int nts_hip_gemm_tn_masked_f32(nts_hip_ctx *ctx, int M, int N, int K, const float *A,
                               uint64_t lda, const float *B, uint64_t ldb, const float *X,
                               uint64_t ldx, float scale, float *C, uint64_t ldc);

/* ---- output layer + loss (fused) ------------------------------------------ */
/* Training forward of the last layer and the loss, in the reference's
 * arithmetic: logits = Y W, log_softmax (vertexForward,
 * toolkits/GCN_SAMPLE_ALLGPU.hpp:247-252), log_softmax again + mean
 * nll_loss (Loss, :214-222).  Y [n x K] (ld ldy), W [K x C] row-major,
 * labels int64 [n] in [0, C).  Writes the scalar loss (device).
 * Shapes (all three entry points): K % 16 == 0 and either C <= 64 with K x C
 * within the kernel's LDS (W resident), or 64 < C <= 512 with K <= 512 (the
 * wide form, W streamed from global memory); other shapes return
 * NTS_ERR_INVALID and launch nothing.
 * correct != NULL: *correct += the rows whose argmax (first index of the
 * largest log_softmax value) is the label — getCorrect
 * (toolkits/GCN_SAMPLE_ALLGPU.hpp:166-172) accumulated on the device.
 * Replaces the libtorch matmul/log_softmax/nll_loss kernels of those lines. */
int nts_hip_linear_xent_fwd(nts_hip_ctx *ctx, const float *Y, uint64_t ldy, int n, int K,
                            const float *W, int C, const int64_t *labels, float *loss,
                            uint32_t *correct);
/* Its backward for an upstream gradient *grad_loss (device scalar):
 * dY [n x K] (ld K) and dW [K x C] (row-major), i.e. what libtorch's
 * autograd produces through nll_loss, both log_softmaxes and the matmul.
 * Deterministic (fixed-order reductions). */
int nts_hip_linear_xent_bwd(nts_hip_ctx *ctx, const float *Y, uint64_t ldy, int n, int K,
                            const float *W, int C, const int64_t *labels,
                            const float *grad_loss, float *dY, float *dW);

/* Training call of the same layer: the loss AND its gradients dY, dW for an
 * upstream gradient of exactly 1 (Loss followed by loss.backward(),
 * toolkits/GCN_SAMPLE_ALLGPU.hpp:214-222 + core/ntsContext.hpp:436-440), in
 * one pass over Y.  Bit-identical to nts_hip_linear_xent_fwd followed by
 * nts_hip_linear_xent_bwd with *grad_loss == 1. */
int nts_hip_linear_xent_train(nts_hip_ctx *ctx, const float *Y, uint64_t ldy, int n, int K,
                              const float *W, int C, const int64_t *labels, float *loss,
                              float *dY, float *dW, uint32_t *correct);

/* Multi-label form of the same layer (no reference counterpart): logits
 * Z = Y W and the mean sigmoid binary cross-entropy over all n * C entries,
 *   loss = mean(max(z, 0) - z t + log1p(exp(-|z|)))      (finite for finite z)
 * i.e. binary_cross_entropy_with_logits(Y W, T) with mean reduction.
 * Y [n x K] (ld ldy), W [K x C] row-major, C <= 128, K % 16 == 0 and K x C
 * within the kernel's LDS; other shapes return NTS_ERR_INVALID
 * and launch nothing.  Targets are bit-packed: label_bits [V x wpr] uint32,
 * wpr >= ceil(C / 32) words per vertex, label c of vertex u = bit c & 31 of
 * label_bits[u * wpr + (c >> 5)]; bits at positions >= C are ignored.  Row r
 * takes the labels of vertex index[r] (the batch's seeds), or of vertex r
 * when index == NULL.  Writes the scalar loss (device).  counts != NULL:
 * counts[0..2] += the true positives, false positives and false negatives of
 * the prediction z > 0 over the n * C entries (micro-F1 = 2 tp / (2 tp + fp +
 * fn)), accumulated on the device. */
int nts_hip_linear_bce_fwd(nts_hip_ctx *ctx, const float *Y, uint64_t ldy, int n, int K,
                           const float *W, int C, const uint32_t *label_bits, uint32_t wpr,
                           const uint32_t *index, float *loss, uint32_t *counts);
/* Training call: the same loss and counts (bit-identical to
 * nts_hip_linear_bce_fwd) AND the gradients for an upstream gradient of
 * exactly 1: dZ = (sigmoid(z) - t) / (n C), dY [n x K] (ld K) = dZ W^T,
 * dW [K x C] = Y^T dZ.  Deterministic: fixed-order reductions, no
 * floating-point atomics. */
int nts_hip_linear_bce_train(nts_hip_ctx *ctx, const float *Y, uint64_t ldy, int n, int K,
                             const float *W, int C, const uint32_t *label_bits, uint32_t wpr,
                             const uint32_t *index, float *loss, float *dY, float *dW,
                             uint32_t *counts);

/* ---- link prediction (csrc/linkpred.hip; no counterpart in the reference) --
 * The semantics of DGL's as_edge_prediction_sampler with negative_sampler.Uniform
 * and of PyG's LinkNeighborLoader, on the device.
 *
 * nts_hip_lp_batch: the pairs and the seed set of one batch.  pos_src / pos_dst
 * [B] hold the global ids (< n_vertices) of the positive edges.  Negative
 * (i, k), k < K, keeps the head pos_src[i]; its tail is
 *   x    = word k % 4 of Philox4x32-10(counter = (k / 4, i, 0x20000000, lo32(batch_seq)),
 *                                      key = (lo32(seed), hi32(seed) ^ hi32(batch_seq)))
 *   tail = (uint64(x) * n_vertices) >> 32
 * i.e. the sampler's counter layout with a layer tag of its own beside
 * 0x80000000 (PHILOX_SHARED) and 0x40000000 (weighted).  Negatives are NOT
 * filtered against the graph's true edges (a negative may be a real edge or a
 * self pair); the tail's bias from uniform is at most n_vertices / 2^32.
 * Pairs are numbered p < B for the positives, then B + i K + k: P = B (1 + K).
 * Outputs (device, caller-owned):
 *   destination [v_cap]   the distinct endpoint ids, ascending; entries past
 *                         *v_size are not written
 *   v_size                device scalar: their count
 *   pair_u, pair_v [P]    the two ends of every pair as rows of destination
 *   inc_offset [v_cap+1], inc_slot [2 P]   the incidence CSR over those rows:
 *                         slot 2p is the u-end and 2p + 1 the v-end of pair p,
 *                         each row's slots ascending (a pair with u == v has both
 *                         slots on one row); rows past *v_size are empty
 *                         (offset 2 P).
 * destination / v_size are what nts_sampcsc_dev takes as a layer's input.
 * Scratch comes from the context arena; nts_hip_ctx_reserve(V, 8 P) beforehand
 * keeps the call allocation-free.
 * NTS_ERR_INVALID, before any write: a NULL pointer, K < 1, B == 0,
 * v_cap < 2 P, P > 2^30, n_vertices outside 1..2^32. */
int nts_hip_lp_batch(nts_hip_ctx *ctx, const uint32_t *pos_src, const uint32_t *pos_dst,
                     uint32_t B, uint32_t K, uint64_t n_vertices, uint64_t batch_seq,
                     uint32_t v_cap, uint32_t *destination, uint32_t *v_size, uint32_t *pair_u,
                     uint32_t *pair_v, uint32_t *inc_offset, uint32_t *inc_slot);
/* Dot-product scores and the mean sigmoid BCE of the P = B (1 + K) pairs:
 *   score[p] = <H[pair_u[p], 0:D], H[pair_v[p], 0:D]>   H fp32 [rows x ldh], 1 <= D <= 1024
 *   loss     = mean_p (max(s, 0) - s y + log1p(exp(-|s|))),   y = 1 for p < B, else 0.
 * mrr != NULL: a device pair of floats, mrr[0] += sum_i 1 / rank_i and
 * mrr[1] += B, with rank_i = 1 + #{k : score(neg i,k) >= score(pos i)} (ties
 * count against the positive); MRR = mrr[0] / mrr[1].  Both sums are fp32 in
 * a fixed order: consecutive runs of 16 positives summed ascending into one
 * partial each, the partials summed ascending.  NULL: no MRR counting.
 * 16-byte row loads when D % 4 == 0, ldh % 4 == 0 and H is 16-byte aligned,
 * scalar loads otherwise.
 * NTS_ERR_INVALID, before any write: a NULL pointer (mrr apart), D outside
 * 1..1024, ldh < D, B == 0, K == 0. */
int nts_hip_lp_bce_fwd(nts_hip_ctx *ctx, const float *H, uint64_t ldh, uint32_t D,
                       const uint32_t *pair_u, const uint32_t *pair_v, uint32_t B, uint32_t K,
                       float *score, float *loss, float *mrr);
/* Training call: the same scores, loss and counter (bit-identical to
 * nts_hip_lp_bce_fwd) AND the gradient for an upstream gradient of exactly 1:
 *   g_p = (sigmoid(s_p) - y_p) / P
 *   dH[r, 0:D] = sum over row r's incidence slots, in ascending slot order, of
 *                g_pair * H[other end of the pair, 0:D]        for r < *v_size
 * (inc_offset / inc_slot / v_size from nts_hip_lp_batch).  A gather over the
 * incidence CSR: no floating-point atomics, two runs give the same bits.  Rows
 * r >= *v_size of dH, and columns >= D, are not touched.
 * Also NTS_ERR_INVALID: lddh < D, v_cap == 0. */
int nts_hip_lp_bce_train(nts_hip_ctx *ctx, const float *H, uint64_t ldh, uint32_t D,
                         const uint32_t *pair_u, const uint32_t *pair_v, uint32_t B, uint32_t K,
                         const uint32_t *inc_offset, const uint32_t *inc_slot,
                         const uint32_t *v_size, uint32_t v_cap, float *score, float *loss,
                         float *dH, uint64_t lddh, float *mrr);

/* Target-edge exclusion and filtered negatives (DGL's
 * as_edge_prediction_sampler(exclude = 'self' | 'reverse_id')).
 *
 * nts_hip_lp_exclude_keys: the batch's excluded edges as a sorted table.  A
 * positive (pos_src[i], pos_dst[i]) is the graph edge src = pos_src[i] ->
 * dst = pos_dst[i] of the CSC keyed by destination, its key
 * (uint64(dst) << 32) | src; with reverse != 0 the key of the edge turned round
 * (dst = pos_src[i], src = pos_dst[i]) is added.  keys_out[0 .. *n_keys_dev)
 * receives the DISTINCT keys ascending (a repeated positive, a positive whose
 * reverse is in the batch too and a self pair under reverse collapse);
 * entries past the count are not written.  Ids must be < n_vertices <= 2^32:
 * the two stable radix sorts (low word, then high word) run over
 * ceil(log2 n_vertices) bits each.  Integer work only: two runs give the same
 * bytes.  Scratch from the context arena, never more than nts_hip_lp_batch
 * takes for the same B.
 * NTS_ERR_INVALID, before any write: a NULL pointer, B == 0, B > 2^30,
 * n_vertices outside 1..2^32, key_cap < (reverse ? 2 B : B). */
int nts_hip_lp_exclude_keys(nts_hip_ctx *ctx, const uint32_t *pos_src, const uint32_t *pos_dst,
                            uint32_t B, int reverse, uint64_t n_vertices, uint32_t key_cap,
                            uint64_t *keys_out, uint32_t *n_keys_dev);
/* Applies the table to one sampled block, after selection: the block's
 * structure is not touched.  With e = min(sizes[1], e_cap) read on the device:
 *   CSC edge k < e:  key (destination[edge_dst[k]], sample_ans[k]);
 *   CSR slot s < e (row_offset != NULL; column_indices, source and
 *                    edge_weight_backward are then needed):
 *                    key (destination[column_indices[s]], source[row of s]);
 * a key in the table sets the edge's coefficient (edge_weight_forward[k],
 * edge_weight_backward[s]) to exactly 0.0f; any other edge keeps its value when
 * had_weights != 0 and is set to 1.0f otherwise (the sampler writes no weights
 * under NTS_WEIGHT_NONE without coefficients).  *excluded_count_dev += the
 * number of CSC edges set to 0 (the caller zeroes it).  Edges and slots past
 * the live sizes, and every array of a block whose overflow flag (sizes[3])
 * is set, are neither read nor written.  keys / n_keys_dev as written by
 * nts_hip_lp_exclude_keys (*n_keys_dev == 0: nothing is excluded).
 * NTS_ERR_INVALID, before any write: a NULL pointer, a block without
 * edge_weight_forward, row_offset without the three CSR arrays. */
int nts_hip_lp_mask_block(nts_hip_ctx *ctx, const nts_sampcsc_dev *block, const uint64_t *keys,
                          const uint32_t *n_keys_dev, int had_weights,
                          uint32_t *excluded_count_dev);
/* nts_hip_lp_batch with negatives filtered against the graph.  sorted_rows
 * [E]: graph->row_indices sorted ascending within each destination's segment.
 * Negative (i, k) of head u = pos_src[i] tries t = 0 .. 15: the candidate is
 * nts_hip_lp_batch's tail with the counter word 0x20000000 | t (t = 0: the
 * unfiltered draw), rejected when it equals u or the graph holds an edge
 * between the two in either direction (a binary search of u in the
 * candidate's segment and of the candidate in u's).  The first accepted
 * candidate is taken; when all 16 are rejected the 16th is kept and
 * *unresolved_dev += 1 (the caller zeroes it).  Everything else is
 * nts_hip_lp_batch: a batch none of whose t = 0 candidates is rejected gives
 * the same bytes.
 * Also NTS_ERR_INVALID: graph, graph->column_offset, sorted_rows or
 * unresolved_dev NULL, graph->n_vertices != n_vertices. */
int nts_hip_lp_batch_filtered(nts_hip_ctx *ctx, const uint32_t *pos_src, const uint32_t *pos_dst,
                              uint32_t B, uint32_t K, uint64_t n_vertices, uint64_t batch_seq,
                              uint32_t v_cap, uint32_t *destination, uint32_t *v_size,
                              uint32_t *pair_u, uint32_t *pair_v, uint32_t *inc_offset,
                              uint32_t *inc_slot, const nts_graph_dev *graph,
                              const uint32_t *sorted_rows, uint32_t *unresolved_dev);
/* All-candidate ranking (csrc/lprank.hip).  Query i < M has the
 * head u = q_head[i] and the true tail v = q_tail[i]; its candidates are the
 * rows w = cand[j], j < n_cand, of H [n_rows, D] (pitch ldh), or every row
 * 0 .. n_rows - 1 when cand is NULL (n_cand is then not read).  With
 *   s(a, b) = the fp32 fmaf chain over k = 0 .. D-1 ascending, from 0,
 * which is what the f32 MFMA computes and what the positive's pre-pass
 * computes, a score depends on the two rows only.  A candidate is VALID iff
 * w != v and, with the filter (adj_offset [n_rows + 1] = the graph's
 * column_offset, adj_sorted = its row_indices ascending within each
 * destination's segment: nts_hip_lp_batch_filtered's arrays and test),
 * w != u and the graph holds neither u -> w nor w -> u.  Then
 *   n_valid[i] = the valid candidates,
 *   greater[i] = the valid candidates with s(u, w) >  s(u, v),
 *   equal[i]   = the valid candidates with s(u, w) == s(u, v),
 * a candidate id repeated in cand counting once per occurrence and the true
 * tail never, wherever it stands.  The three arrays ([M] each) are
 * overwritten.  The [n_cand, M] scores are never written: an LDS-tiled
 * product on v_mfma_f32_32x32x2_f32 (k past D zero-filled, the row pad never
 * read) whose epilogue compares and counts; integer atomics only, so two
 * calls give the same bytes.  The filter's binary searches run for a
 * candidate with s >= s(u, v) only; the filtered n_valid is a pass of its
 * own over every (query, candidate).  Ids are not validated on the device:
 * q_head, q_tail and cand entries must be < n_rows.  M floats of the
 * context's scratch.
 * NTS_ERR_INVALID, nothing written: a NULL ctx, H, q_head, q_tail or output,
 * D == 0, D > 1024, ldh < D, M == 0, n_rows == 0, exactly one of adj_offset /
 * adj_sorted, cand with n_cand == 0, more than 2^32 - 1 candidates. */
int nts_hip_lp_rank(nts_hip_ctx *ctx, const float *H, uint64_t ldh, uint32_t D, uint32_t n_rows,
                    const uint32_t *q_head, const uint32_t *q_tail, uint32_t M,
                    const uint32_t *cand, uint64_t n_cand, const uint64_t *adj_offset,
                    const uint32_t *adj_sorted, uint32_t *greater, uint32_t *equal,
                    uint32_t *n_valid);

/* ---- GraphSAGE root weight (csrc/aggregate.hip; no counterpart in the reference) --
 * The graph op of X' = act([A X | X_dst] W), W = [W_n; W_s] stacked on K.
 *
 * Forward, one launch: for every d < *v
 *   ycat[d, 0:F]  = sum_e w[e] x[row(e), :]   exactly nts_hip_spmm_csc_fwd's sum
 *   ycat[d, F:2F] = x[self(d), :]             a copy
 * row(e) = x_row_map ? x_row_map[row_indices[e]] : row_indices[e].  self(d) =
 * self_index[d], a row of x either way: a local source row (dst_local_id) when
 * x_row_map is NULL, a global table row (destination) when it is not.
 * ld_ycat >= 2 F; any F >= 1 (float4 / float2 / scalar by alignment).  Rows
 * >= *v are left untouched. */
int nts_hip_spmm_csc_fwd_root(nts_hip_ctx *ctx, const uint32_t *column_offset,
                              const uint32_t *row_indices, const float *weight,
                              const uint32_t *v, uint32_t v_cap, const float *x, uint64_t ldx,
                              const uint32_t *x_row_map, const uint32_t *self_index,
                              uint32_t feature_size, float *ycat, uint64_t ld_ycat);
/* src_dst[s] = the d < *v with dst_local_id[d] == s, else NTS_NOT_CACHED, for
 * s < *s (a merged layer: dst_local_id is one-to-one).  Two launches on the
 * context's stream: fill, scatter. */
int nts_hip_root_inverse_map(nts_hip_ctx *ctx, const uint32_t *dst_local_id, const uint32_t *v,
                             uint32_t v_cap, const uint32_t *s, uint32_t s_cap,
                             uint32_t *src_dst);
/* Backward of the forward above for an upstream g_ycat [n, 2F] (pitch ld_g):
 *   g_in[s, :] = m_s ⊙ ( sum_j w_b[j] g_ycat[ci[j], 0:F]
 *                        + (src_dst[s] != NTS_NOT_CACHED ? g_ycat[src_dst[s], F:2F] : 0) )
 * for s < *s.  The sum is nts_hip_spmm_csr_bwd's (order and arithmetic, its
 * long-row rule included) for the same operands, the self term one more fp32
 * add, and m_s = [x_act[s, :] > 0] scale when x_act != NULL
 * (nts_hip_spmm_csr_bwd_postmask's), else 1.  Deterministic, no atomics. */
int nts_hip_spmm_csr_bwd_root(nts_hip_ctx *ctx, const uint32_t *row_offset,
                              const uint32_t *column_indices, const float *weight_backward,
                              const uint32_t *s, uint32_t s_cap, const float *g_ycat,
                              uint64_t ld_g, const uint32_t *src_dst, const float *x_act,
                              uint64_t ld_act, float scale, uint32_t feature_size, float *g_in,
                              uint64_t ld_gin);

/* ---- GraphSAGE max aggregator (csrc/aggmax.hip, csrc/infer.hip; no
 * counterpart in the reference, whose graph ops are weighted sums) ----------
 * Forward: for every d < *v and column c < F
 *   y[d, c] = max over e in [co[d], co[d+1]) of x[row(e), c]
 * with row(e) as in nts_hip_spmm_csc_fwd (through x_row_map when non-NULL).
 * The column is scanned serially in CSC edge order: the first edge's value
 * starts the maximum (not 0, not -FLT_MAX) and a later one replaces it on a
 * strict >, so ties (+0 / -0 included) go to the earliest edge.  An empty
 * column gives 0.0f.  No weights.  NaN inputs are unspecified.
 * arg (nullable, uint32 [v_cap, F], row pitch F): arg[d, c] = the winning CSC
 * edge index, 0xFFFFFFFF for an empty column.  self_index (nullable): also
 * y[d, F:2F] = x[self_index[d], :] as nts_hip_spmm_csc_fwd_root's right half
 * (ldy >= 2 F).  Rows >= *v are left untouched; any F >= 1 (float4 / float2 /
 * scalar by alignment). */
int nts_hip_spmm_csc_fwd_max(nts_hip_ctx *ctx, const uint32_t *column_offset,
                             const uint32_t *row_indices, const uint32_t *v, uint32_t v_cap,
                             const float *x, uint64_t ldx, const uint32_t *x_row_map,
                             const uint32_t *self_index, uint32_t feature_size, float *y,
                             uint64_t ldy, uint32_t *arg);
/* Backward over the CSR transpose of a layer sampled with csr_edge_id: for s < *s
 *   g_in[s, c] = m_s[c] ( sum_{j in [ro[s], ro[s+1]), arg[ci[j], c] == csr_edge_id[j]} g_y[ci[j], c]
 *                         + (src_dst && src_dst[s] != NTS_NOT_CACHED ? g_y[src_dst[s], F + c] : 0) )
 * m_s = [x_act[s, :] > 0] scale when x_act != NULL (nts_hip_spmm_csr_bwd_postmask's
 * rule), else 1.  The sum runs in nts_hip_spmm_csr_bwd's order for the same
 * row_offset and F, its long-row rule included; a slot that did not win adds
 * nothing or an exact +0, so where every slot of a row won the result is
 * nts_hip_spmm_csr_bwd's with unit weights bit for bit.  Deterministic: no
 * float atomics, no grid barrier.  ld_g >= 2 F with src_dst. */
int nts_hip_spmm_csr_bwd_max(nts_hip_ctx *ctx, const uint32_t *row_offset,
                             const uint32_t *column_indices, const uint32_t *csr_edge_id,
                             const uint32_t *s, uint32_t s_cap, const float *g_y, uint64_t ld_g,
                             const uint32_t *arg, const uint32_t *src_dst, const float *x_act,
                             uint64_t ld_act, float scale, uint32_t feature_size, float *g_in,
                             uint64_t ld_gin);
/* The same maximum over the GLOBAL CSC of `graph` for v_begin <= d < v_end
 * (layer-wise inference, see nts_hip_spmm_graph_fwd): no arg, an empty column
 * writes a zero row, relu optional.  Hub columns are walked in a fixed order,
 * and a maximum does not depend on it: the result equals the serial one (only
 * the sign of a zero maximum is left open). */
int nts_hip_spmm_graph_fwd_max(nts_hip_ctx *ctx, const nts_graph_dev *graph, uint64_t v_begin,
                               uint64_t v_end, int relu, const float *x, uint64_t ldx,
                               uint32_t feature_size, float *y, uint64_t ldy);
/* The per-vertex scores of a GAT layer (heads K of D columns, F = K D, the
 * layout of nts_hip_gat_forward_heads): S [rows, 2K] contiguous,
 *   S[v, h] = H[v]_h . a1_h,  S[v, K + h] = H[v]_h . a2_h,
 * a1 = att[0:F], a2 = att[F:2F], head h owning columns [hD, (h+1)D).  One pass
 * over H in a fixed summation order; float4 where D % 4 == 0, ldh % 4 == 0 and
 * H and att are 16-byte aligned, scalar otherwise.  heads == 0 or D == 0:
 * NTS_ERR_INVALID. */
int nts_hip_gat_scores(nts_hip_ctx *ctx, const float *H, uint64_t ldh, uint64_t rows,
                       uint32_t heads, uint32_t D, const float *att, float *S);
/* The GAT layer over ALL in-edges of d in the GLOBAL CSC of `graph`, for
 * v_begin <= d < v_end (layer-wise inference, dst_local(d) = d), from H [V, F]
 * and the scores S of nts_hip_gat_scores over the same H:
 *   m[e,h] = leaky_relu(S[src_e, h] + S[d, K + h], 0.2), a = softmax over d's edges,
 *   Z_h[d] = sum_e a[e,h] H[src_e]_h,
 *   mean == 0: Y[d] = relu([Z_0 | .. | Z_{K-1}]) (F wide),
 *   mean != 0: Y[d] = relu((1/K) sum_h Z_h[d]) (D wide; heads added in order).
 * Nothing E-sized is written (no m, no a: there is no backward).  An online
 * softmax per (row, column slice) lane group in CSC edge order; hub columns
 * are split by column slice, never by edge range, so every output element is
 * one fixed sequence of operations and two calls give the same bytes.  An
 * empty column writes a zero row; rows outside the range and pitch padding
 * are not touched; any F (wider rows take more slices).  float4 needs
 * D % 4 == 0 besides 16-byte aligned rows.  No atomics, no grid barrier.
 * heads == 0, D == 0 or a range outside the graph: NTS_ERR_INVALID, nothing
 * written.  Mean mode keeps [v_end - v_begin, F] floats in the context's
 * scratch. */
int nts_hip_gat_graph_fwd(nts_hip_ctx *ctx, const nts_graph_dev *graph, uint64_t v_begin,
                          uint64_t v_end, const float *H, uint64_t ldh, uint32_t heads,
                          uint32_t D, const float *S, float *Y, uint64_t ldy, int mean);

/* ---- optimiser ---------------------------------------------------------- */
/* Fused Adam step on one parameter (n elements), element-wise identical to
 *  bias_correction != 0: Parameter::learnC2C_with_decay_Adam (core/NtsScheduler.hpp:863-880)
 *  bias_correction == 0: Parameter::learn_local_with_decay_Adam (core/NtsScheduler.hpp:937-945)
 * beta1_t/beta2_t are the running powers kept by Parameter::next(). */
int nts_hip_adam(nts_hip_ctx *ctx, float *w, const float *grad, float *m, float *v,
                 uint64_t n, float alpha, float beta1, float beta2, float epsilon,
                 float weight_decay, float beta1_t, float beta2_t, int bias_correction);

/* ---- RCCL over xGMI (replaces NCCL_Communicator, cuda/ntsCUDA.hpp:132-175,
 *      cuda/ntsCUDAGraphOP.cu:173-200) --------------------------------------- */
int nts_hip_comm_unique_id(uint8_t out_id[128]);
/* One communicator per process/GPU (ncclCommInitRank) instead of the
 * reference's single-process ncclCommInitAll clique. */
int nts_hip_comm_init(nts_hip_comm **comm, int nranks, int rank, const uint8_t id[128],
                      int device);
int nts_hip_comm_destroy(nts_hip_comm *comm);
/* Ranks in the communicator as RCCL itself reports them (ncclCommCount) and
 * this process's rank (ncclCommUserRank): the check that an N-process launch
 * really built one N-rank clique (the reference's ncclCommInitAll over
 * `device_num` GPUs, toolkits/GCN_SAMPLE_ALL_MULTI.hpp:89-113). */
int nts_hip_comm_count(nts_hip_comm *comm, int *nranks, int *rank);
/* In-place float SUM all-reduce (NCCL_Communicator::AllReduce, cuda/ntsCUDAGraphOP.cu:180-186). */
int nts_hip_allreduce_sum_f32(nts_hip_comm *comm, float *buf, uint64_t count, void *stream);
/* In-place broadcast from root (NCCL_Communicator::Bcast, cuda/ntsCUDAGraphOP.cu:188-193). */
int nts_hip_broadcast_f32(nts_hip_comm *comm, float *buf, uint64_t count, int root,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NTS_HIP_H */
