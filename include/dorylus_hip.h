/*
 * dorylus_hip.h -- C-ABI of the MI355X-native aggregation + transform engine.
 *
 * This is the drop-in boundary for the reference's "cpu"/"gpu" backends
 * (uclasystem/dorylus, src/graph-server).  Every entry point replaces one piece
 * of the reference's Engine / ResourceComm interface; the replaced code is cited
 * as file:line relative to src/graph-server/ (or src/ where noted).
 *
 * Conventions
 *   - plain C, no C++/torch types; all functions return 0 on success or a
 *     negative dory_status; dory_last_error() gives the message.  Nothing in the
 *     library aborts the host process (the reference assert()/exit()s,
 *     GPU-Computation/cu_matrix.cu:137-141).
 *   - one dory_ctx per GPU / per graph partition ("node" in the reference).
 *     Calls on one ctx are serialised internally (mutex), so they may come from
 *     the Engine's different stage threads (engine/engine.cpp:243-273).
 *   - all tensors are fp32 (FeatType/EdgeType = float, common/utils.hpp:28-29);
 *     host buffers are dense row-major rows x cols exactly as the Engine's
 *     savedNNTensors (engine/ops/gcn_ops.cpp:27-93); the device copy is
 *     authoritative between dory_tensor_upload and dory_tensor_download.
 *   - layer / dir arguments have the meaning of Chunk::layer / Chunk::dir
 *     (common/utils.hpp:64-75) at the call site they replace.
 */
#ifndef DORYLUS_HIP_H
#define DORYLUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dory_ctx dory_ctx;

enum dory_status {
    DORY_OK = 0,
    DORY_ERR_ARG = -1,     /* bad argument / unknown tensor / wrong state        */
    DORY_ERR_HIP = -2,     /* a HIP runtime call failed                          */
    DORY_ERR_NODEVICE = -3,/* no usable MI355X (gfx950) device                   */
    DORY_ERR_COMM = -4,    /* RCCL failure                                       */
    DORY_ERR_IO = -5       /* file format / IO problem (host-side helpers)       */
};

enum dory_dir { DORY_FORWARD = 0, DORY_BACKWARD = 1 }; /* PROP_TYPE, common/utils.hpp:46 */
enum dory_gnn { DORY_GCN = 0, DORY_GAT = 1,            /* GNN,       common/utils.hpp:48 */
                DORY_GATMH = 2 };  /* extension, not in the reference: multi-head GAT with per-edge
                                      attention softmax (BASELINE config 3 wording) */

/* ---- lifetime ---------------------------------------------------------------
 * Replaces ComputingUnit::getInstance / ComputingServer construction
 * (GPU-Computation/comp_unit.cu:23-46, engine/engine.cpp:141-163). */
int dory_create(int device, dory_ctx **out);
int dory_destroy(dory_ctx *ctx);
const char *dory_last_error(dory_ctx *ctx); /* ctx may be NULL: last create error */

/* Adopt caller-owned HIP streams (hipStream_t passed as void*); NULL keeps the
 * context's own.  compute: all kernels; comm: RCCL + pack/unpack. */
int dory_set_streams(dory_ctx *ctx, void *compute_stream, void *comm_stream);
int dory_sync(dory_ctx *ctx); /* wait for both streams (NodeManager::barrier's local half) */

/* ---- model / partition description -------------------------------------------
 * Replaces Engine::readLayerConfigFile + the Engine fields the backend reads
 * (engine/utils.cpp:460-479; gnn_type, numLayers, layerConfig, nodeId, numNodes,
 * graph.globalVtxCnt).  dims has num_layers+1 entries (run/reddit.config = 602 128 41). */
int dory_configure(dory_ctx *ctx, int gnn_type, uint32_t num_layers,
                   const uint32_t *dims, uint32_t global_vtx_cnt,
                   uint32_t node_id, uint32_t num_nodes);

/* Multi-head GAT extension only (gnn_type == DORY_GATMH): heads per layer (num_layers
 * entries; default 8 for hidden layers, 1 for the last).  Hidden layer l concatenates its
 * heads (dims[l+1] = K*D, D a power of two <= 64, K*D <= 256) and applies ELU; the last layer
 * averages its heads into dims[L] logits.  Call between dory_configure and dory_preallocate.
 * Tensors: h z el er m den o do dz t del der (+ logits grad lab at L-1), weights w a_l a_r.
 * Stage mapping: apply_vertex fwd = z=h*W; apply_edge fwd = el,er; aggregate fwd = edge softmax
 * + weighted sum (+ELU / head mean); predict_gat = softmax - label; aggregate bwd = attention
 * backward (dz, da_l, da_r); apply_vertex bwd = dW, dh.  Partitioned runs: dory_halo_exchange(layer, FORWARD) ships
 * "z" -> "fg_z" (the ghost sources' scores are recomputed from it); the backward sweep of dory_aggregate runs in two
 * phases and ships "do" -> "bg_do" and "st" -> "bg_st" (the packed (er, m, 1/den, t) rows) of the out-edges' ghost
 * destinations in between -- itself over RCCL, or, with option "gatmh_bwd_phase" = 1 / 2, one phase per call so that
 * the caller can move those rows (dory_halo_pack_tensor / dory_halo_unpack_tensor, or as one merged row
 * dory_gatmh_bwd_pack / dory_gatmh_bwd_unpack); dory_halo_exchange(layer, BACKWARD) is a no-op for this model.
 * dory_gatmh_bwd_merged_exchange (below; opt-in): a whole sweep ships ONE row [do[v, 0:w) | st[v, 0:4K)] per sent vertex in
 * one exchange (w = ld of do, or cols rounded up to 4 with halo_exact_rows) and, with dory_halo_fused_pack on and the sweep
 * forms running, the row-wise kernel that produces st writes the send rows itself.  Not taken (two exchanges as ever): the
 * scatter transport, a plan made with halo_direct_recv = 1, gatmh_bwd_phase = 1 / 2 (the caller's own transport).
 * Partitioned runs take the sweep forms, else the source-blocked kernels ("gatmh_blocked" = 1), else -- no layout, no partial
 * buffer, a head shape neither covers -- the row-gather kernels with ghost rows (dory_gatmh_row_gather, below).
 * Sweep forms (option "gatmh_sweep" = 1, default; round 5): where the K1s layouts apply and a head spans 2..16 lanes of a
 * 16-byte-per-lane row slab, the forward runs on K1s's skeleton with a single-pass softmax against an upper-bound shift
 * ("m" then holds that shift, "den" the matching denominator: alpha = exp(s - m) / den as before) and leaves two more
 * tensors, "op" (the part of "o" that came over edges on LeakyReLU's positive branch) and "dpos" (their attention mass);
 * the backward's destination side is then a row-wise kernel (t = <do, o>, der = 0.8 (<do, op> - t dpos)) and its source
 * side a sweep over the out-edges' layout.  Other shapes, or "gatmh_sweep" = 0, keep the blocked kernels; the named
 * tensors and the two-phase protocol are the same either way.  "gatmh_sweep_rows": rows per lane group of the layouts. */
int dory_gatmh_heads(dory_ctx *ctx, const uint32_t *heads);

/* Upload one partition's adjacency, exactly the arrays of Graph
 * (graph/graph.hpp:60-99): forwardAdj (CSC over destination columns, in-edges)
 * and backwardAdj (CSR over source rows, out-edges), 64-bit pointers, 32-bit
 * local indices (ghost ids = N + k), per-edge values, vtxDataVec norms.
 * Replaces the upload in Engine::init (engine/engine.cpp:105-125) and
 * CuMatrix::loadSpCSR/loadSpCSC (GPU-Computation/cu_matrix.cu:36-98), without
 * the 32-bit truncation of cu_matrix.cu:55-58. */
int dory_graph_upload(dory_ctx *ctx, uint32_t local_vtx_cnt,
                      uint32_t src_ghost_cnt, uint32_t dst_ghost_cnt,
                      uint64_t nnz_in, const uint64_t *column_ptrs,
                      const uint32_t *row_idxs, const float *csc_values,
                      uint64_t nnz_out, const uint64_t *row_ptrs,
                      const uint32_t *column_idxs, const float *csr_values,
                      const float *vtx_norms);

/* Allocate the named tensor table on the device: Engine::preallocateGCN /
 * preallocateGAT (engine/ops/gcn_ops.cpp:27-93, gat_ops.cpp:27-115).  GCN names:
 * x fg ah z h lab grad bg aTg; GAT names: h z az fg_z A ah grad dA aTg bg_d lab
 * (SURVEY.md Appendix B).  Requires configure + graph_upload. */
int dory_preallocate(dory_ctx *ctx);

/* ---- named tensors (savedNNTensors[layer][name]) ----------------------------- */
int dory_tensor_info(dory_ctx *ctx, uint32_t layer, const char *name,
                     uint64_t *rows, uint32_t *cols, uint32_t *ld, void **device_ptr);
/* host (dense rows x cols) -> device, and back; both synchronous w.r.t. the
 * compute stream.  Replace the per-op cublasSetMatrix/GetMatrix round trips
 * (cu_matrix.cu:101-120,149,173) with explicit, once-per-run transfers. */
int dory_tensor_upload(dory_ctx *ctx, uint32_t layer, const char *name, const float *host);
int dory_tensor_download(dory_ctx *ctx, uint32_t layer, const char *name, float *host);
/* fill a tensor on the device (synthetic inputs): uniform[lo,hi) from a counter
 * RNG keyed by (seed, global_row * cols + col).  global_row_ids (host, `rows`
 * entries, or NULL for identity) makes a vertex's row independent of the
 * partition that holds it (pass localToGlobalId / the ghost gvids). */
int dory_tensor_fill_uniform(dory_ctx *ctx, uint32_t layer, const char *name,
                             uint64_t seed, float lo, float hi,
                             const uint32_t *global_row_ids);
/* one-hot labels from u32 class ids (Engine::readLabelsFile, engine/utils.cpp:559-596) */
int dory_labels_upload(dory_ctx *ctx, const uint32_t *labels);

/* ---- weights (replaces MessageService weight fetch / push,
 * commmanager/message_service.cpp:142-242, and the weight server's store) ------
 * name is "w" (dims[l] x dims[l+1]) or "a_i" (dims[l+1] x 1, GAT). */
int dory_weight_set(dory_ctx *ctx, uint32_t layer, const char *name, const float *host);
int dory_weight_get(dory_ctx *ctx, uint32_t layer, const char *name, float *host);
int dory_weight_grad_get(dory_ctx *ctx, uint32_t layer, const char *name, float *host);
/* the weight server's side of a push (WeightTensor::localUpdate, weighttensor.cpp:131-150): overwrite the
 * gradient the next dory_weight_update applies -- for callers that sum the updates themselves */
int dory_weight_grad_set(dory_ctx *ctx, uint32_t layer, const char *name, const float *host);
/* WeightServer::xavierInitializer, seed 8888 (src/weight-server/weightserver.cpp:567-585) */
int dory_weights_init_xavier(dory_ctx *ctx);

/* ---- the hot path ---------------------------------------------------------------
 * dory_aggregate      = Engine::aggregateGCN / aggregateGAT (Chunk c) for the whole
 *                       local partition [0, N)  (gcn_ops.cpp:130-191, gat_ops.cpp:173-243)
 * dory_apply_vertex   = ResourceComm::NNCompute(chunk) with chunk.vertex == true
 *                       (CPU_comm.cpp:22-44 -> vtxNNForward / vtxNNBackward, :98-188)
 * dory_apply_edge     = NNCompute with chunk.vertex == false (CPU_comm.cpp:33-42 ->
 *                       edgNNForwardGAT / edgNNBackwardGAT, :190-242); `layer` is the
 *                       chunk's layer, the callee applies the reference's layer-1.
 * dory_predict_gat    = Engine::predictGAT (gat_ops.cpp:246-265)
 */
int dory_aggregate(dory_ctx *ctx, uint32_t layer, int dir);
int dory_apply_vertex(dory_ctx *ctx, uint32_t layer, int dir);
int dory_apply_edge(dory_ctx *ctx, uint32_t layer, int dir);
int dory_predict_gat(dory_ctx *ctx, uint32_t layer);

/* validation accuracy / loss sums of the last forward pass
 * (CPUComm::getTrainStat, CPU_comm.cpp:448-462; MessageService::sendAccloss) */
int dory_train_stat(dory_ctx *ctx, float *acc_sum, float *loss_sum, uint32_t *val_rows);
/* The same summed over all partitions -- what the weight servers do with the AccLoss records the graph servers send them
 * (WeightServer::updateLocalAccLoss / updateGlobalAccLoss, src/weight-server/weightserver.cpp:190-262: vtcsCnt, acc, loss
 * added up over the nodes, "Epoch %u, acc: %.4f, loss: %.4f" on node 0).  A collective: every rank calls it, every rank gets
 * the sums (RCCL all-reduce of three scalars, or the local / host transport).  num_nodes == 1: the local values. */
int dory_train_stat_global(dory_ctx *ctx, float *acc_sum, float *loss_sum, uint32_t *val_rows);

/* ---- ghost-vertex halo exchange (replaces Engine::scatterGCN/GAT +
 * verticesPushOut + ghostReceiver*, gcn_ops.cpp:204-362, engine/utils.cpp:623-650)
 * The plan is the per-peer send lists of graph.<id>.bin (forwardGhostsList /
 * backwardGhostsList, graph/dataloader.cpp:277-297) plus, per peer, the ghost
 * slots its rows land in (srcGhostVtcs / dstGhostVtcs order, dataloader.cpp:311-322).
 * counts arrays have num_nodes entries; lists are concatenated in peer order.
 * (With option "halo_direct_recv" = 1 received row r is stored at ghost row r and recv_slots names its caller-visible index:
 * see the option's comment below.) */
int dory_halo_plan(dory_ctx *ctx, int dir, const uint32_t *send_counts,
                   const uint32_t *send_lvids, const uint32_t *recv_counts,
                   const uint32_t *recv_slots);
/* RCCL communicator over xGMI: rank 0 makes an id (128 bytes), every rank passes
 * the same bytes.  With num_nodes == 1 none of this is needed. */
int dory_comm_unique_id(void *id128);
int dory_comm_init(dory_ctx *ctx, const void *id128, int rank, int nranks);
/* Host transport instead of RCCL: the exchange step and the gradient sum call back into the host program with
 * host buffers -- the seam where the reference's own CommManager / ZeroMQ data path (gcn_ops.cpp:204-362:
 * verticesPushOut + ghostReceiver*, weighttensor.cpp:131-166 for the update sum) or any MPI can carry the bytes.
 * Everything else of the multi-rank path (plan, pack, unpack, stream ordering, overlap with the local-source
 * aggregation, Adam) stays the library's.  alltoallv: floats, per-peer counts and offsets (num_nodes entries
 * each, self entry 0); allreduce: in-place sum over all ranks.  Callbacks return 0 on success and run on the
 * calling thread, between two stream synchronisations.  Passing NULLs returns to RCCL. */
typedef int (*dory_alltoallv_fn)(void *user, const float *send, const uint64_t *send_counts, const uint64_t *send_offsets,
                                 float *recv, const uint64_t *recv_counts, const uint64_t *recv_offsets, uint32_t num_nodes);
typedef int (*dory_allreduce_fn)(void *user, float *buf, uint64_t n);
int dory_comm_set_host_transport(dory_ctx *ctx, dory_alltoallv_fn alltoallv, dory_allreduce_fn allreduce_sum, void *user);
/* In-process device transport: the `n` contexts (rank i = ctxs[i], all configured with num_nodes == n, graphs and halo
 * plans uploaded, preallocated, on ONE device) become each other's peers.  An exchange is then pack -> hipMemcpyAsync
 * device -> device into every peer's receive buffer on the SENDER's comm stream -> cross-context events -> unpack on the
 * receiver's comm stream; the gradient sum reads the peers' gradients in rank order.  Same stream / event structure as the
 * RCCL path and no host synchronisation with the device: the overlapped schedule of Engine::scatterGCN + ghostReceiver
 * (gcn_ops.cpp:204-282 send, :284-362 receive) with copies that really run beside the aggregation, on one GPU.  Drive
 * every rank from its own host thread (as real ranks are), or stage by stage; a rank whose peer's host thread never
 * arrives fails with DORY_ERR_COMM after option local_timeout_ms (default 30 s).  Destroy the contexts only after all of
 * them are synchronised.  A host transport set on a context takes precedence; RCCL is not used. */
int dory_comm_init_local(dory_ctx *const *ctxs, uint32_t n);
/* pack -> grouped ncclSend/ncclRecv (all-to-all-v) -> unpack into fg / bg
 * (GCN: fwd sends h@(layer-1) into fg@layer, bwd sends grad@layer into bg@(layer-1);
 *  GAT: fwd z@(layer-1) -> fg_z@(layer-1), bwd grad@(layer-1) -> bg_d@(layer-1);
 *  `layer`/`dir` are the chunk's, as in Engine::scatter*).  */
int dory_halo_exchange(dory_ctx *ctx, uint32_t layer, int dir);
/* split entry points for callers that own the transport (tests, other MPI):
 * buffers are device pointers of total_send_rows x cols / total_recv_rows x cols */
int dory_halo_pack(dory_ctx *ctx, uint32_t layer, int dir, float *send_buf);
int dory_halo_unpack(dory_ctx *ctx, uint32_t layer, int dir, const float *recv_buf);
/* The same for any named tensor: rows of a per-local-vertex tensor listed in the plan of `dir` -> send_buf, and
 * recv_buf -> the rows of a ghost tensor of that direction (foreign transports; what the multi-head GAT extension's
 * backward sweep ships between its two phases: "do" -> "bg_do", "st" -> "bg_st"). */
int dory_halo_pack_tensor(dory_ctx *ctx, uint32_t layer, const char *name, int dir, float *send_buf);
int dory_halo_unpack_tensor(dory_ctx *ctx, uint32_t layer, const char *name, int dir, const float *recv_buf);

/* The feature switches of this header -- the ten entry points dory_<name>(ctx, int), each with a dory_<name>_stats beside it: the
 * halo and ghost-twin switches of the sections below, from dory_halo_fused_pack to dory_gatmh_bf16_ghosts, and among them the
 * row-gather pair dory_gatmh_row_gather / dory_gatmh_row_gather_bf16 -- are records of one table: dorylus_amd/host/switches.cpp, ids
 * in dorylus_amd/csrc/switches.hpp.  A record holds the switch's values, its refusals in the order they are checked, whether a set
 * waits for the halo in flight and drops the fused pack's stamp, and its counters; dory_switch_spec and dory_switch_check
 * (dorylus_host.h) enumerate and ask it without a context.  All are off after dory_create.  (dory_gat_bf16_gather takes two values
 * and dory_timing_enable is no feature: neither is in the table.) */

/* ---- fused halo pack: the GEMM epilogues write the send rows (opt-in, default off; nothing in the reference: an MI355X-side
 * addition) ----
 * An exchange's pack kernel re-reads rows a GEMM wrote just before and sits in front of the link.  With the feature on, a K2 GEMM
 * whose output (C, or the tanh output C2) is the tensor dory_halo_exchange would pack next -- GCN h@l (l < L-1, forward), grad@l
 * (l >= 1, backward), xw@l (l > 0 of a transform-first layer, forward); GAT z@l (forward), grad@(l-1) of dory_apply_vertex
 * backward (backward); multi-head GAT z@l (forward) -- stores every row once more from its epilogue into the row's slots of the
 * internal send buffer (the plan's send lists turned round: dory_halo_send_map of dorylus_host.h, kept on the device per direction,
 * 4 (N + 1) + 4 send_total bytes, built by dory_halo_plan while on or by this call for the plans that exist, freed with the plan;
 * nothing is allocated inside an epoch).  The row width is the exchange's own (halo_exact_rows: cols floats, else ld with the
 * padding zeroed): the buffer is byte for byte what the pack kernel leaves, every tensor keeps its bits.  The context then holds
 * ONE stamp {source tensor, direction, width, send buffer}; the exchange whose source, direction, width and buffer match it skips
 * its pack kernel and consumes the stamp (fused_exchanges += 1, fused_rows += send rows); with the feature on any other exchange
 * packs as ever and counts as a fallback.  The stamp is dropped by dory_tensor_upload / dory_tensor_fill_uniform of that tensor,
 * by any pack into the internal send buffer (another exchange; the multi-head GAT's "do" / "st"), by the buffer growing, by a new
 * plan, by dory_halo_fused_pack(ctx, 0), by any dory_comm_* call; a second producer of the same tensor replaces it.  Once
 * dory_tensor_info has handed out a source tensor's device pointer that tensor never fuses again on this context (its rows may
 * change behind the library's back).  Not taken, i.e. a counted fallback with the same results: sources no GEMM writes (h of a
 * transform-first layer, g, the GAT prototype's last-layer grad -- unless dory_halo_fused_pack_rowwise, below -- and the multi-head
 * GAT's do / st, always), a product with K == 0 or no local rows, the scatter
 * transport (another buffer layout), the in-process transport with halo_direct_recv = 1 (the peers read the send buffer on their
 * own streams), epoch-graph recording.  dory_halo_pack* always run the kernel into the caller's buffer and leave the stamp
 * alone.  The producer waits for the previous exchange (as dory_apply_vertex does anyway) before its epilogue writes the
 * buffer.  num_nodes == 1: accepted, nothing changes.
 * dory_halo_fused_pack: on = 0 / 1, any time after dory_configure, outside an exchange.
 * dory_halo_fused_pack_stats: exchanges that skipped the pack, their send rows, exchanges that packed although the feature was
 * on -- eager calls only, counted since dory_create; any pointer may be NULL. */
int dory_halo_fused_pack(dory_ctx *ctx, int on);
int dory_halo_fused_pack_stats(dory_ctx *ctx, uint64_t *fused_exchanges, uint64_t *fused_rows, uint64_t *fallback_exchanges);

/* ---- bf16 row gathers of the GAT prototype's aggregations (opt-in, default off; nothing in the reference) ----
 * GAT prototype (DORY_GAT) only.  mode 0 = off (default), 1 = the aggregations that gather z / fg_z read them rounded to bf16
 * (the forward's, and the backward's dA-weighted term, reused or recomputed), 2 = also the backward's A^T grad gather of
 * grad / bg_d.  wide = 1: K1s gathers bf16 rows of 128 floats or more eight features per lane (16-byte gathers), same bits.
 * One rule, that of gcn_bf16_gather: with the mode on every row such an aggregation reads -- local rows, ghost rows (rounded
 * after their exchange has landed) and the self row -- is rounded to bf16, round to nearest even, into a shadow buffer of
 * (N + ghosts) x the widest layer's ld x 2 bytes (reserved by this call after dory_preallocate, else by the first eager
 * aggregation; it cannot grow while an epoch graph is recorded).  Edge values, arow / drow, the sums and the outputs stay fp32 and
 * the sums are added in the fp32 path's order: ah and aTg are, bit for bit, what the same context gives with mode 0 on z / fg_z
 * (mode 2: and grad / bg_d) already rounded to bf16 -- for either setting of gat_reuse_nsum, each against its own fp32
 * counterpart.  The neighbour sum kept from the forward ("nsum") is reused by the backward only if it was summed under the
 * rounding the mode asks for then; otherwise the dA term is gathered again.  K1s and K1 have the bf16 forms, K1b has none: where
 * fp32 would take K1b the aggregation takes K1, and spmm_variant = 1 with mode != 0 is refused by dory_aggregate.  No requested
 * aggregation runs on fp32 rows unannounced (fp32_fallbacks counts any that would; there is no such path today).
 * Refused with DORY_ERR_ARG: a context configured as another model (here, and by dory_configure when the mode was set first),
 * mode outside 0..2, wide outside 0..1, wide without mode, a call while an epoch graph is being recorded.  Changing mode or wide
 * drops a recorded epoch.
 * dory_gat_bf16_gather_stats: aggregations that ran on bf16 rows since dory_create, per kernel family (k1s_wide: those of k1s
 * that took the wide form); any pointer may be NULL.
 * Measured on one MI355X (profiles/r18_gat_bf16_gather.txt, profiles/HISTORY.md section 19), Reddit-size uniform graph, dims
 * 602-128-41: epoch 9.78 ms off, 9.57 ms mode 2, 8.68 ms mode 2 with wide; the four conversions cost 0.09 ms of it.  The
 * per-aggregation table there says which launch gains what; a form that is not faster at a shape is named there. */
int dory_gat_bf16_gather(dory_ctx *ctx, int mode, int wide);
int dory_gat_bf16_gather_stats(dory_ctx *ctx, uint64_t *k1s, uint64_t *k1s_wide, uint64_t *k1, uint64_t *fp32_fallbacks);

/* ---- bf16 halo rows: exchanges whose consumer gathers bf16 ship bf16 (opt-in, default off; nothing in the reference) ----
 * With the bf16 gathers on (option gcn_bf16_gather, dory_gat_bf16_gather) the aggregation that reads a ghost tensor rounds every
 * ghost row to bf16 (nearest even) before it reads it: the lower 16 bits of every fp32 the exchange ships are dropped unseen.
 * Rounding is idempotent, so with this switch on the pack rounds (the same conversion, v_cvt_pk_bf16_f32), 16 bits per element
 * travel, and the unpack widens them (bits << 16) into the fp32 ghost tensor: the aggregation's own conversion reproduces the
 * same bf16 row, and every result keeps its bits relative to the fp32 payload under the same gather mode.
 * The rule -- decided per exchange from the settings at that moment (the switch, the gather mode), the same for every layer:
 *     model           forward exchange                        backward exchange
 *     GCN             h -> fg, xw -> fgxw: gcn_bf16_gather >= 1    grad -> bg, g -> bgg: gcn_bf16_gather == 2
 *     GAT prototype   z -> fg_z: dory_gat_bf16_gather mode >= 1    grad -> bg_d: mode == 2
 *     multi-head GAT  never, unless dory_gatmh_halo_bf16 (below) is on too: then option gatmh_bf16_gather >= 1 / == 2 (its own do)
 * (without that switch the multi-head GAT keeps fp32 rows: a caller who had gatmh_bf16_gather and this switch on before it existed
 * keeps the bytes they had).
 * Not taken, i.e. fp32 rows travel as without the switch, the results are the same and the pack is counted in
 * fp32_packs_while_on: the rule says no; the scatter-message transport (the reference's format); a plan made with
 * halo_direct_recv = 1 (a 16-bit row cannot land in an fp32 ghost tensor, and such a plan may have no receive buffer) -- unless
 * dory_halo_bf16_ghosts (below) gives the rows a bf16 tensor to land in;
 * dory_halo_pack_tensor / dory_halo_unpack_tensor (the consumer is unknown).  dory_halo_pack / dory_halo_unpack follow the rule
 * as they follow halo_exact_rows: the caller's buffer (8-byte aligned) then holds rows x row_elems x 2 bytes.  The fused halo
 * pack never serves an exchange that ships bf16 (no GEMM stores fp32 rows nobody sends; its statistics count a fallback) -- unless
 * dory_halo_fused_pack_bf16 (below) has the GEMM epilogue round the rows itself.
 * Wire format: a packed row holds row_elems bf16 values -- the tensor's ld, or with halo_exact_rows = 1 its cols rounded up to a
 * multiple of 4 with zeros in the trailing elements, which the pack writes itself (a one-column tensor, ld == 1: 4 elements).
 * Rows are multiples of 8 bytes.  The host transport's counts and offsets stay in floats: rows x row_elems / 2.  RCCL and the
 * in-process copies move the same bytes; no buffer is re-sized.  In the in-process transport ranks that disagree -- on the switch
 * or on the gather mode that drives the rule -- fail at once with DORY_ERR_COMM; for RCCL and host transports EVERY RANK MUST SET
 * THE SAME.  The read-only key halo_floats_packed counts a bf16 row as row_elems / 2.
 * Visible consequence: after a bf16 exchange the fp32 ghost tensor holds the owner's rows rounded to bf16 (and zeros in
 * [cols, ld)): dory_tensor_download of fg / fgxw / bg / bgg / fg_z / bg_d shows rounded rows.
 * Bytes per row on the link -- ARITHMETIC, nothing here has run on more than one GPU:
 *     row                                          fp32 padded  fp32 exact  bf16 padded  bf16 exact
 *     Reddit h / grad, 128 floats                     512 B       512 B       256 B       256 B
 *     Amazon, 64 floats                               256 B       256 B       128 B       128 B
 *     Friendster, 48 floats                           256 B       192 B       128 B        96 B
 *     41-float rows (GAT z, transform-first xw)       256 B       164 B       128 B        88 B
 * dory_halo_bf16_rows: on = 0 (default) / 1, any time after dory_configure, outside an exchange; accepted and inert with
 * num_nodes == 1; DORY_ERR_ARG for other values or while an epoch graph is being recorded.
 * dory_halo_bf16_rows_stats: packs that wrote bf16 rows, their bytes, packs (and fused or scatter-message exchanges) that shipped
 * fp32 while the switch was on -- eager calls only, since dory_create; any pointer may be NULL.  An exchange whose bf16 rows a GEMM
 * epilogue wrote (dory_halo_fused_pack_bf16) counts in bf16_packs and bf16_bytes like a pack: they say what travelled as bf16.
 * dory_halo_wire_row: what dory_halo_exchange(layer, dir) and dory_halo_pack(layer, dir, ...) would put on the wire with the
 * settings of this moment: bytes per element (4 or 2) and elements per row -- what a foreign transport sizes its buffers by.
 * Kernels (csrc/elementwise.hip): four elements per lane, one 16-byte access on the fp32 side and one 8-byte access on the
 * packed side.  Chosen by measurement against an 8-element form (two 16-byte accesses, one 16-byte access; stand-alone copies of
 * both, 3.15 M rows): the 8-element unpack is 15-18 % SLOWER at every width, the 8-element pack 2-7 % faster on padded rows and even
 * on exact ones, and rows of row_elems % 8 == 4 (41 exact: 44) have no 16-byte grid at all -- one form of four serves every row.
 * Measured on one MI355X (profiles/r19_halo_bf16_rows.txt, profiles/HISTORY.md section 20; NOTHING HERE CROSSED A LINK), 3.15 M
 * send rows and as many ghost rows, switch off / on alternated: pack 0.293 -> 0.210 ms (64 floats), 1.477 -> 1.105 (300), 0.599 ->
 * 0.437 (128), 0.284 -> 0.212 (48 padded), 0.246 -> 0.195 (48 exact), 0.285 -> 0.205 (41 padded), 0.322 -> 0.188 (41 exact); unpack
 * 0.315 -> 0.218, 1.610 -> 1.092, 0.668 -> 0.461, 0.330 -> 0.211, 0.393 -> 0.203, 0.304 -> 0.210, 0.433 -> 0.202.  No bf16 kernel is
 * slower than its fp32 counterpart at a measured shape.  The in-process-transport epoch (200 000 vertices, 4 M edges, 128-128-16,
 * gather mode 2) does not move beyond its run-to-run spread at P = 2 or 4; with the switch off the headline and 8-head GAT epochs
 * are inside the parent's ranges. */
int dory_halo_bf16_rows(dory_ctx *ctx, int on);
int dory_halo_bf16_rows_stats(dory_ctx *ctx, uint64_t *bf16_packs, uint64_t *bf16_bytes, uint64_t *fp32_packs_while_on);
int dory_halo_wire_row(dory_ctx *ctx, uint32_t layer, int dir, uint32_t *elem_bytes, uint32_t *row_elems);

/* ---- fused halo pack for bf16 rows: the GEMM epilogues write the bf16 send rows (opt-in, default off; nothing in the reference) ----
 * dory_halo_fused_pack and dory_halo_bf16_rows cancel each other where both apply: the GEMM writes fp32, and the bf16 pack kernel
 * reads it back to round it.  With this third switch on, the fused pack also serves the exchanges that ship bf16: the producing K2
 * GEMM (NN / NT of both tile shapes, or the split-K reduce; kernels of their own, gemm_dma_send16_kernel[_occ4] and
 * splitk_reduce_send16_kernel in csrc/gemm.hip -- every other kernel keeps its code object) rounds each element with the pack's own
 * conversion (v_cvt_pk_bf16_f32) and stores it into the row's slots of the send buffer: row_elems bf16 a row, zeros in
 * [cols, row_elems) -- byte for byte what gather_rows_bf16_kernel would leave; C and C2 keep their bits.  The exchange then runs no
 * pack kernel.  It has an effect only while dory_halo_fused_pack is 1, dory_halo_bf16_rows is 1 and the rule above says the
 * exchange ships bf16; off (default): everything as before, bf16 exchanges pack and count as fallbacks of the fused pack.
 * The stamp carries the element kind and, for bf16, the columns that hold values; the exchange takes it only if source,
 * direction, kind, columns, width and buffer are what its own wire -- computed at the exchange -- has: a gather mode, any of the three
 * halo switches or halo_exact_rows changed between producer and exchange is a counted fallback with the bytes of the moment.
 * Not taken (counted fallbacks, same bytes): everything the fused pack does not take (above); a one-column tensor (ld == 1: a wire
 * row of 4 elements is wider than the tensor's row); TN products, K == 0, no local rows.  The multi-head GAT's z ships bf16, and is fused here, only under
 * dory_gatmh_halo_bf16 (below).
 * Direct plans over RCCL or the host transport whose rows land in twins fuse like any other: only the send side changes.
 * Counters of a fused bf16 exchange: fused_exchanges / fused_rows of dory_halo_fused_pack_stats move as for an fp32 one, and the
 * two of this section; bf16_packs / bf16_bytes of dory_halo_bf16_rows_stats move too (what travelled as bf16: a foreign
 * transport sizes by them); halo_rows_packed / halo_floats_packed do not (no pack kernel ran).  Eager calls only, since dory_create.
 * dory_halo_fused_pack_bf16: on = 0 (default) / 1, any time after dory_configure, outside an exchange; drops the stamp; accepted
 * and inert with num_nodes == 1; DORY_ERR_ARG for other values, before dory_configure, or while an epoch graph is being recorded.
 * Epilogue form (tools/probes/gemm_send16_forms.hip; profiles/r21_halo_fused_pack_bf16.txt, profiles/HISTORY.md section 22): a lane
 * holds one column and its neighbour the next, so the value of the lane to the right comes by DPP (quad_perm) and the even lanes
 * store one cvt_pk dword -- 16 lanes x 4 bytes per row and tile -- against the plain form of one 2-byte store per lane:
 *     N (w)          128     64      48 (64)  48 (48)  41 (64)  41 (44)  300 (320)  300 (300)     [1.05 M rows, K = 128, ms, medians of 3]
 *     GEMM + pack    0.493   0.259   0.255    0.265    0.266    0.257    1.362      1.394
 *     DPP pair       0.474   0.253   0.255    0.260    0.249    0.243    1.345      1.375
 *     2-byte stores  0.468   0.251   0.255    0.255    0.251    0.242    1.341      1.374
 * NO FORM WON: they lie within 2 % of each other at every shape (the 2-byte form ahead by 0-1.8 % at seven, behind by 0.8 % at one),
 * inside the 2-6 % between rounds (a second session: the same, the pair form at 64 floats 1.3 % above GEMM + pack, inside its rounds'
 * spread).  The pair form is the one instantiated: half the store instructions for the same bytes.  Both spend
 * most of what the pack kernel took: the row's slot range and slots are loaded in the epilogue with nothing to hide them behind.
 * Measured on one MI355X (same files; NO LINK AND NO MULTI-RANK RCCL RUN IS BEHIND ANY NUMBER), baseline = the parent's pair, the
 * GEMM plus gather_rows_bf16_kernel, against the bf16 send GEMM alone:
 *     1.05 M local rows, every row to 1 peer / to 3 peers (3.15 M send rows); ms per call, medians of 3 alternating rounds
 *     NN+tanh 602->128        1.602 -> 1.571 / 1.854 -> 1.698        NN 128->41 padded   0.282 -> 0.263 / 0.403 -> 0.372
 *     NT 41->128              0.726 -> 0.732 / 0.988 -> 0.945        NN 128->41 exact    0.280 -> 0.264 / 0.376 -> 0.352
 *     NN 300->64              0.523 -> 0.476 / 0.626 -> 0.560        NN 128->300 padded  1.378 -> 1.357 / 2.121 -> 1.794
 *     NN 128->48 padded       0.287 -> 0.274 / 0.402 -> 0.374        NN 128->300 exact   1.383 -> 1.363 / 2.096 -> 1.851
 *     NN 128->48 exact        0.285 -> 0.266 / 0.381 -> 0.359
 * x0.85-0.99 of the pair; the first round of every series is its slowest (0.01-0.25 ms between rounds), so only six of the eighteen
 * differences exceed the spread of their own series.  ONE SHAPE IS A TIE ON THE WRONG SIDE: NT 41->128 with one peer per row, +0.006 ms
 * (+0.8 %), far inside its spread of 0.095 ms; it is taken like the others.  With every switch off the headline epoch of bench.py is
 * inside the parent's range (18.057-18.064 ms against 18.037-18.092); the GAT epochs read 0.1-0.3 % above it when the parent's
 * process ran first of each pair and inside or below it when it ran second (same file, section 3: the position, not the library). */
int dory_halo_fused_pack_bf16(dory_ctx *ctx, int on);   /* 0 (default) / 1 */
int dory_halo_fused_pack_bf16_stats(dory_ctx *ctx, uint64_t *fused_bf16_exchanges, uint64_t *fused_bf16_rows);

/* ---- fused halo pack for rows the row-wise kernels produce (opt-in, default off; nothing in the reference) ----
 * The fused pack removes the pack kernel only where a K2 GEMM wrote the rows that travel.  With gcn_transform_first = 2, the
 * fastest configuration, a 2-layer GCN makes three exchanges an epoch and two of them ship g, which no GEMM writes.  With this
 * switch on, the row-wise kernels that produce the source of an exchange run SEND FORMS (kernels of their own in
 * csrc/elementwise.hip -- tanh_backward_send_kernel, tanh_forward_send_kernel, softmax_rows_send_kernel; every other kernel keeps
 * its code object) that compute and store the tensor exactly as the plain kernel does and store every row once more into the row's
 * slots of the send buffer, in the wire format of the moment: fp32 padded (ld floats, the zeros of the padding behind cols), fp32
 * exact (cols floats, dense), or bf16 (row_elems elements rounded with the pack's conversion, zeros in [cols, row_elems)) -- byte
 * for byte what the pack kernel would leave; every tensor keeps its bits.  Fused:
 *     dory_apply_vertex, GCN backward            g@l         travels backward when layer l is transform-first   (tanh backward)
 *     dory_apply_vertex, GCN last layer forward  g@(L-1)     travels backward when the last layer is            (softmax + loss)
 *     dory_apply_vertex, GCN hidden transform-first layer    h@l travels forward when layer l + 1 is not        (tanh forward)
 *     dory_predict_gat, GAT prototype            grad@(L-1)  travels backward                                   (softmax - label)
 * Each asks the question the GEMMs ask (same target, width, element kind and capacity rule), waits for the previous exchange
 * before the buffer is written, and leaves the one stamp -- which now also records who made it.  The switch has an effect only
 * while dory_halo_fused_pack is 1; an exchange that ships bf16 rows is fused by a row-wise producer only if
 * dory_halo_fused_pack_bf16 is 1 too.  Everything that drops or mismatches a GEMM's stamp does so with these (upload, fill, another
 * exchange, a new plan, halo_exact_rows or a wire switch changed, the raw pointer handed out: counted fallbacks with the rows of the
 * moment); a producer that runs its plain kernel drops a stamp that names its tensor.
 * Not taken: the multi-head GAT's do / st (two exchanges in a row through one send buffer with one stamp, and no (layer, direction)
 * of dory_halo_exchange names them): they keep packing under this switch -- dory_gatmh_bwd_merged_exchange, below, is the switch
 * that has their producer write them.  A one-column tensor (ld == 1).  Everything the fused pack does not take.
 * Counters: a consumed stamp of a row-wise producer moves rowwise_exchanges / rowwise_rows IN ADDITION to fused_exchanges /
 * fused_rows, and for a bf16 wire to fused_bf16_* and bf16_packs / bf16_bytes, exactly as a GEMM-made one.  Eager calls only, since
 * dory_create; any pointer may be NULL.
 * dory_halo_fused_pack_rowwise: on = 0 (default) / 1, any time after dory_configure, outside an exchange; drops the stamp; accepted
 * and inert with num_nodes == 1; DORY_ERR_ARG for other values, before dory_configure, or while an epoch graph is being recorded.
 * Forms: tanh_backward keeps its parent's float4 per lane (bf16: one 8-byte store per slot); tanh_forward takes a float4 per lane
 * where its parent takes one element (the DPP pair form was not built: no probe compares the two); the softmax forms keep lane c on
 * columns c, c + LPR, ... and form bf16 pairs by DPP.  A row's slot range is loaded once per lane and quad (softmax: per lane and
 * row), outside every element loop, and the softmax forms fetch the first slot ahead of the arithmetic (before that they were
 * x1.01-1.09 on every bf16 line below).
 * Measured on one MI355X (profiles/r22_halo_fused_pack_rowwise.txt, profiles/HISTORY.md section 23; tools/halo_fused_rowwise_rate.py;
 * NO LINK AND NO MULTI-RANK RCCL RUN IS BEHIND ANY NUMBER), 1.05 M local rows, every row to 1 peer / to 3 peers, each step a child
 * process, the parent commit's library (plain producer + pack kernel) and this one (send producer alone) alternated over three
 * rounds; send / pair, medians:
 *                        padded 1 / 3     exact 1 / 3      bf16 1 / 3
 *     tanh_backward 128  x0.71 / x0.68    x0.71 / x0.68    x0.70 / x0.63         (0.537 -> 0.380 ms ... 0.743 -> 0.467)
 *     tanh_backward 64   x0.73 / x0.69    x0.72 / x0.71    x0.72 / x0.65
 *     tanh_backward 48   x0.69 / x0.68    x0.71 / x0.77    x0.68 / x0.68
 *     tanh_backward 41   x0.71 / x0.67    x0.66 / x0.74    x0.71 / x0.71
 *     tanh_forward 128   x0.66 / x0.67    x0.66 / x0.69    x0.60 / x0.56
 *     tanh_forward 64    x0.68 / x0.73    x0.66 / x0.74    x0.59 / x0.58
 *     tanh_forward 48    x0.75 / x0.78    x0.72 / x0.82    x0.64 / x0.67
 *     tanh_forward 41    x0.71 / x0.74    x0.75 / x0.89    x0.64 / x0.64
 *     softmax_xent 41    x0.92 / x0.88    x0.80 / x0.72    x0.95 / x0.97
 *     softmax_xent 16    x1.03 / x0.97    x0.99 / x0.90    x1.04 / x1.05
 *     softmax_xent 64    x1.03 / x0.98    x1.05 / x1.01    x1.09 / x1.08
 *     softmax_sub 41     x0.88 / x0.92    x0.75 / x0.82    x0.91 / x1.03
 *     softmax_sub 16     x1.00 / x0.94    x0.98 / x0.86    x1.03 / x1.03
 *     softmax_sub 64     x1.02 / x0.98    x1.04 / x1.01    x1.08 / x1.08
 * The tanh forms gain at every shape.  NOT FASTER, NAMED: the softmax forms at 64 classes (every line but the padded one with three
 * peers: +1-9 %), at 16 classes under a bf16 wire (+3-5 %) and padded with one peer (+0-3 %), and softmax_sub 41 bf16 with three
 * peers (+3 %): a softmax row is held by 8-64 lanes that store dwords, and the slot loads sit at the end of a latency-bound kernel.
 * They are TAKEN all the same -- one rule per switch, and these lines have every row travelling, where a partition sends a
 * fraction of its rows -- so a caller whose last layer is that wide and whose rows mostly travel should leave the switch off. */
int dory_halo_fused_pack_rowwise(dory_ctx *ctx, int on);   /* 0 (default) / 1 */
int dory_halo_fused_pack_rowwise_stats(dory_ctx *ctx, uint64_t *rowwise_exchanges, uint64_t *rowwise_rows);

/* ---- the multi-head GAT's backward exchange, merged (opt-in, default off; nothing in the reference) ---------------------------
 * A whole backward sweep of the 8-head GAT (dory_gatmh_heads, option gatmh_bwd_phase = 0) ships do -> bg_do and st -> bg_st between
 * its two phases: two exchanges back to back -- two packs, two unpacks, two all-to-all-v rounds (each a stream synchronisation under
 * the host transport), two event hand-overs -- and st travels at its padded width (32 floats for 4 K of data).  With this switch on
 * a sent vertex v of layer l travels as ONE merged row
 *     [ do[v, 0:w) | st[v, 0:4K) ]      R = w + 4K floats, fp32, rows in the order of the backward plan's send lists
 * with w = ld of do, or, with option halo_exact_rows = 1, its cols rounded up to a multiple of 4 (the columns past cols are the
 * tensor's zero padding, as in the bf16 rows' rule).  R is a multiple of 4: every row starts on a 16-byte boundary.  One pack (or
 * none), one all-to-all-v, one unpack, one hand-over; the host transport's callback sees counts and offsets in floats of R per row.
 * The unpack (scatter_rows_pair_kernel) writes whole ghost rows -- bg_do[slot, 0:w) and bg_st[slot, 0:4K) from the buffer, zeros
 * into [w, ld) and [4K, ld of st) -- so every float of both ghost tensors is what the two exchanges leave; every tensor, weight and
 * gradient keeps its bits.  Bytes per sent row for 602-128-41 with heads 8 / 1, as arithmetic: hidden layer 512 + 128 B -> 640 B
 * (the same bytes in one message), last layer 256 + 128 = 384 B -> 272 B, 192 B with halo_exact_rows.
 * Taken when the switch is on, gatmh_bwd_phase == 0, the transport is RCCL, the host callbacks or the in-process one, and the plan
 * was not made with halo_direct_recv = 1.  NOT TAKEN -- the two exchanges as ever, the same bits, one split_fallbacks per backward
 * pass: the scatter transport (its messages have their own layout); a plan made with halo_direct_recv = 1 (received rows land in
 * one tensor and there are two).
 * Producer-packed: where the merged exchange is taken, dory_halo_fused_pack is 1, the backward runs the sweep forms, the backward
 * plan has its send map, no epoch graph is being recorded and the send buffer holds send_total x R floats, the row-wise kernel that
 * produces st runs its send form (csrc/gat_mh_sweep.hip: gatmh_dst_rowwise_send_kernel -- the same arithmetic in the same order, and
 * each thread stores the do quad it has loaded, the head's leader lane its st record, into the row's slots of the send buffer) and
 * the exchange runs no pack kernel.  Producer and exchange sit inside one dory_aggregate call under the context's lock: no stamp
 * is involved and no caller can get between them.  It counts in dory_halo_fused_pack_stats as one fused exchange of send_total
 * rows; a merged exchange that packs by kernel (gather_rows_pair_kernel: the blocked forms, whose st comes out of an edge pass)
 * while dory_halo_fused_pack is on counts there as one fallback -- fused + fallback == exchanges made still holds.
 * Buffers: dory_halo_plan sizes them for the widest merged row while the switch is on; the setter grows those of plans that exist;
 * after dory_comm_init_local the peers hold the buffers' addresses, so a setter that would have to grow them fails with
 * DORY_ERR_ARG and leaves the switch off: call it before dory_comm_init_local.
 * ALL RANKS MUST SET THE SAME VALUE.  In-process ranks that disagree fail with DORY_ERR_COMM (both ranks named) before anything of
 * the backward pass's exchange is enqueued; under RCCL and the host transport a mismatch cannot be seen.
 * dory_gatmh_bwd_merged_exchange: on = 0 (default) / 1; DORY_ERR_ARG for a context that is not DORY_GATMH or not configured, other
 * values, or while an epoch graph is being recorded; accepted and inert with num_nodes == 1 (all counters stay 0).
 * dory_gatmh_bwd_merged_exchange_stats: eager calls since dory_create -- merged exchanges, their send rows, those of them whose rows
 * the producer wrote, backward passes that kept the two exchanges while the switch was on; any pointer may be NULL.
 * For callers that move the rows themselves (gatmh_bwd_phase = 1 / 2: the library exchanges nothing), whatever the switch says:
 * dory_gatmh_bwd_wire_row tells the row (R, w, 4K floats) of the tensors' layer `layer` (dory_halo_pack_tensor's layer) as the wire
 * stands now; dory_gatmh_bwd_pack writes the plan's send_total merged rows into a device buffer, dory_gatmh_bwd_unpack takes
 * recv_total of them out of one (16-byte aligned; on the compute stream).  DORY_ERR_ARG before dory_preallocate or without a
 * backward plan.  dory_halo_pack_tensor / dory_halo_unpack_tensor on do / st keep working.
 * Measured on one MI355X -- NO LINK AND NO SECOND GPU ARE BEHIND ANY NUMBER; the halved message count and the last layer's narrower
 * row are arithmetic until an RCCL run with more than one rank exists: profiles/r23_gatmh_bwd_merged_exchange.txt
 * (tools/gatmh_bwd_exchange_rate.py), which also names the shapes that are not faster. */
int dory_gatmh_bwd_merged_exchange(dory_ctx *ctx, int on);          /* 0 (default) / 1 */
int dory_gatmh_bwd_merged_exchange_stats(dory_ctx *ctx, uint64_t *merged_exchanges, uint64_t *merged_rows, uint64_t *producer_packed,
                                         uint64_t *split_fallbacks);
int dory_gatmh_bwd_wire_row(dory_ctx *ctx, uint32_t layer, uint32_t *row_floats, uint32_t *do_floats, uint32_t *st_floats);
int dory_gatmh_bwd_pack(dory_ctx *ctx, uint32_t layer, float *send_buf);
int dory_gatmh_bwd_unpack(dory_ctx *ctx, uint32_t layer, const float *recv_buf);

/* ---- bf16 halo rows for the 8-head GAT (opt-in, default off, on top of dory_halo_bf16_rows; nothing in the reference) -------------
 * With option gatmh_bf16_gather >= 1 the forward sweep gathers z / fg_z only from their rounded shadow copy (and the redo kernel rounds
 * what it re-reads: rounding a rounded row is the identity); with == 2 the source-side sweep gathers do / bg_do only from rounded copies
 * and nothing else reads bg_do; where the dispatch would take a blocked form, which reads fp32, the option already fails with
 * DORY_ERR_ARG.  So half of every fp32 ghost row shipped is thrown away on arrival.  With this switch AND dory_halo_bf16_rows on, the
 * rule of that section covers this model:
 *     dory_halo_exchange(layer, FORWARD)   z -> fg_z ships bf16 iff gatmh_bf16_gather >= 1 at that moment: the existing bf16 row (row_elems
 *                                          bf16 = ld, or with halo_exact_rows cols rounded up to 4, zeros behind cols; dory_halo_wire_row
 *                                          reports it; dory_halo_pack / _unpack follow)
 *     the backward sweep's do -> bg_do     ships bf16 iff gatmh_bf16_gather == 2 at the moment of that dory_aggregate call (read per call:
 *                                          a layer run with 1 ships fp32)
 *     st -> bg_st                          always fp32
 * Two exchanges (dory_gatmh_bwd_merged_exchange off): do through the bf16 pack / unpack, st through the fp32 ones.  Merged: one row
 *     [ do[v, 0:w) as bf16 | st[v, 0:4K) as fp32 ]      w = ld, or with halo_exact_rows cols rounded up to a multiple of 8
 * -- the multiple of 8 puts the st records on a 16-byte boundary and makes the row w / 2 + 4K floats, a multiple of 4; the elements
 * behind cols are zeros (the tensor's padding).  dory_gatmh_bwd_wire_row keeps answering in 4-byte units (do_floats = w / 2),
 * dory_gatmh_bwd_wire_do reports the element size and the count w; dory_gatmh_bwd_pack / _unpack follow the rule, so that a caller's own
 * transport (gatmh_bwd_phase 1 / 2) gets the same rows.  Rounding is round to nearest even (v_cvt_pk_bf16_f32), the conversion of every
 * bf16 path.  do, st, t, der and every local tensor keep their bits; raw bg_do rows hold the widened rounded values and zeros in
 * [w, ld), whatever they held before.  Kernels of their own beside the fp32 ones, whose code objects do not change:
 * gather_rows_pair_bf16_kernel / scatter_rows_pair_bf16_kernel (csrc/elementwise.hip) and gatmh_dst_rowwise_send_bf16_kernel
 * (csrc/gat_mh_sweep.hip: taken where the fp32 send form is taken, when the wire of that call is bf16 -- no stamp, no further switch).
 * Forward z: the K2 GEMM's send16 epilogue (dory_halo_fused_pack_bf16) writes exactly this row; without that switch the bf16 pack
 * kernel runs, a counted fallback of the fused pack as elsewhere.
 * KEEP FP32 (eager calls counted in fp32_packs_while_on): the scatter transport; plans made with halo_direct_recv = 1 (no twins for
 * this model: dory_halo_bf16_ghosts stays inert for it unless dory_gatmh_bf16_ghosts is on, below); dory_halo_pack_tensor / dory_halo_unpack_tensor (the consumer is unknown); st.
 * VISIBLE CONSEQUENCE: dory_apply_edge computes fg_el from fg_z after the exchange, so with a bf16 forward wire fg_el comes from rounded
 * rows.  The contract: every tensor, weight and gradient is bit for bit what a run with the switch off and the same options produces
 * in which every ghost row of fg_z is replaced by its rounded value between dory_halo_exchange and dory_apply_edge.  The backward under
 * value 2 changes no bit of any local result; only the raw bg_do shows rounded rows.  After a bf16 exchange the shadow-copy conversion
 * of the ghost rows still runs (it re-rounds rounded rows: correct, and wasted work; dory_gatmh_bf16_ghosts, below, removes it).
 * Counters: halo_floats_packed counts 4-byte units; bf16_packs / bf16_bytes of dory_halo_bf16_rows_stats count what travelled as bf16,
 * a merged row with all its bytes; the merged and fused counters move as for an fp32 exchange.  No buffer is re-sized: rows only get
 * narrower.  Bytes per sent vertex for 602-128-41, heads 8 / 1, AS ARITHMETIC (no RCCL run with more than one rank is behind them):
 * forward z 512 -> 256 B (hidden), 256 -> 128 B (last; 88 B exact); merged [do | st] 640 -> 384 B (hidden), 272 -> 144 B (last; 112 B exact).
 * ALL RANKS MUST SET THE SAME VALUES: in-process ranks that disagree on the switch or the gather value fail with DORY_ERR_COMM before
 * anything of the exchange is enqueued (the option is published in an atomic mirror when dory_set_option writes it).
 * dory_gatmh_halo_bf16: on = 0 (default) / 1, any time after dory_configure, outside an exchange; it has an effect only while
 * dory_halo_bf16_rows is 1; drops the fused pack's stamp; accepted and inert with num_nodes == 1; DORY_ERR_ARG for a context that is
 * not DORY_GATMH or not configured, other values, or while an epoch graph is being recorded.  With it off every byte and counter is as
 * before.  dory_gatmh_halo_bf16_stats: eager exchanges since dory_create -- forward ones that shipped bf16, backward ones whose do shipped
 * bf16 (merged or alone), their send rows, the merged ones of them whose rows the producer wrote; any pointer may be NULL.
 * Measured on one MI355X -- NO LINK AND NO SECOND GPU ARE BEHIND ANY NUMBER -- profiles/r24_gatmh_halo_bf16.txt
 * (tools/gatmh_halo_bf16_rate.py: 1.05 M local rows, every row to 1 / 3 peers, 8 x 16, 4 x 16, 4 x 64 and 1 x 41, padded and exact, the
 * parent's library and this one alternated over three rounds): pair pack -> bf16 pair pack x0.72-0.86 at all sixteen lines, pair unpack
 * -> bf16 pair unpack x0.75-0.86 at fourteen, row-wise send -> bf16 send x0.82-0.94 at fourteen.  NOT FASTER, NAMED: the bf16 pair
 * unpack at 1 x 41 with exact rows (x1.010 / x1.008).  A TIE: the bf16 send form at 4 x 64 with one peer per row (x0.977 / x0.978).
 * With the switch off the headline epoch reads 18.160 / 18.185 ms against the parent's 18.157-18.160 (the second 0.14 % above, as
 * the last process of the series) and the 8-head GAT epoch 16.055 against 16.051. */
int dory_gatmh_halo_bf16(dory_ctx *ctx, int on);     /* 0 (default) / 1 */
int dory_gatmh_halo_bf16_stats(dory_ctx *ctx, uint64_t *fwd_bf16_exchanges, uint64_t *bwd_bf16_exchanges, uint64_t *bwd_bf16_rows,
                               uint64_t *producer_packed_bf16);
int dory_gatmh_bwd_wire_do(dory_ctx *ctx, uint32_t layer, uint32_t *elem_bytes, uint32_t *elems);

/* ---- the multi-head GAT's row-gather kernels with ghost rows (csrc/gat_mh_rows.hip; nothing in the reference) ----------------
 * The sweep forms need a K1s layout (at most 512 source windows, N + ghosts < 2^24, 32-bit byte offsets into the gathered rows),
 * the source-blocked forms a K1b layout (at most 256 blocks, D % 4 == 0 or one head) and a partial buffer of nb x N x (ld + 64)
 * floats; the row-wise forms of round 1 read no ghost rows.  A partitioned dory_aggregate of a DORY_GATMH context that found none of
 * them used to fail.  It now runs a fourth family, written as K1 is for GCN: one lane group of 8 / 16 / 32 / 64 lanes per row, one
 * float4 per lane, a group's edge ids fetched with one coalesced load and broadcast, four gathered rows in flight, an id >= N
 * selecting row id - N of the ghost tensor, 64-bit addressing, nothing of size E x K stored, no atomics (same input, same bits), no
 * LDS and no wait between workgroups.  Any shape dory_preallocate accepts runs (32 heads x 2 and x 1 included).
 *   forward            waits for the exchange in flight, then one pass over the in-edges with online rescaling (self edge last);
 *                      writes "o", "m", "den" and "op" / "dpos" as the sweep forward does.  "m" holds the row's TRUE maximum per
 *                      head, as with the blocked forms.
 *   backward, phase 1  destination side: where this layer's forward left op / dpos and a head spans 2..16 lanes of a row slab (the
 *                      shapes of the sweep forms) the row-wise kernel t = <do, o>, der = 0.8 (<do, op> - t dpos) -- no edges;
 *                      every other shape an edge pass over the in-edges with ghost sources.  Both write "t", "der", "st".
 *   exchange           do / st as ever (two exchanges, or one merged with dory_gatmh_bwd_merged_exchange: pack kernels, the
 *                      producer-packed form does not apply); gatmh_bwd_phase 0 / 1 / 2 mean what they mean for the other forms.
 *   backward, phase 2  source side over the out-edges, destinations local or ghost: del = <z, 0.2 S + 0.8 S+> - (0.2 T + 0.8 T+),
 *                      dz with the finishing terms; the attention gradients' column sums follow unchanged.
 * mode 0 (default): the family runs where a partitioned dory_aggregate of a DORY_GATMH context would otherwise be refused (no sweep
 * layout, no blocked layout or partial buffer, a head shape neither covers); single partitions keep the row-wise forms.  mode 1: it
 * runs in place of every other family, single partitions included (tests, measurement).  DORY_GCN / DORY_GAT contexts reject 1;
 * other values and a call while an epoch graph is being recorded are DORY_ERR_ARG.  The family allocates nothing and waits for
 * nothing on the host: a single-partition epoch in mode 1 can be recorded as an epoch graph like any other.
 * bf16 rows: "gatmh_bf16_gather" >= 1 is refused where the sweep forms do not run, mode 1 included, and the message says so --
 * unless dory_gatmh_row_gather_bf16 (below) is on, which gives this family bf16 forms of its three edge passes.
 * NOT TAKEN: overlap of the interior rows with the forward exchange.  Hub rows: a row's edges are walked by its one lane group,
 * however long the row, unless dory_gatmh_row_gather_hub_split (below) cuts it.
 * Counters: passes since dory_create, eager calls and recordings (not replays): forward, destination side as an edge pass,
 * destination side as the row-wise kernel, source side; any pointer may be NULL. */
int dory_gatmh_row_gather(dory_ctx *ctx, int mode);   /* 0 (default) / 1 */
int dory_gatmh_row_gather_stats(dory_ctx *ctx, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *dst_rowwise, uint64_t *src);

/* ---- bf16 row gathers for the row-gather kernels (opt-in, default off; nothing in the reference) --------------------------------
 * The family above is the one form of the model that waits on HBM bytes: a 64-float row is 256 bytes gathered once per edge.  With
 * on = 1, wherever dory_aggregate selects that family (mode 1, or mode 0's fall-back on a partitioned call) option
 * "gatmh_bf16_gather" runs its bf16 forms instead of being refused: the gathered row chunk is ONE 8-byte load of four bf16 from the
 * context's shadow rows (rounded to nearest even by a conversion kernel, as for the sweep forms; a 64-float row is then one 128-byte
 * line), widened exactly; lane geometry, rows in flight, ghost addressing and every fp32 operation after the load are the fp32
 * kernels', in their order (one shared body per pass).  CONTRACT: a bf16 pass equals, bit for bit, the fp32 pass run on rows that
 * were rounded to bf16 beforehand.
 *   forward ("gatmh_bf16_gather" >= 1)   gathers z / fg_z from the shadow rows (local rows converted at once, ghost rows after the
 *                      exchange has landed).  Where the scores come from the gathered row (every shape but rows of 96, 160, 192, 224
 *                      floats, which gather "el" / "fg_el" as before) they are scores of the ROUNDED row.
 *   backward, phase 1  the row-wise kernel runs where it ran (it reads no rows).  The edge pass gathers bf16 rows iff this layer's
 *                      forward ran the family's bf16 form (a per-layer flag, cleared by every other forward form): its scores must be
 *                      the forward's.  Otherwise -- a forward that swept, the switch turned off since -- it runs in fp32.
 *   backward, phase 2 ("gatmh_bf16_gather" = 2)   gathers do / bg_do from the shadow rows, converted after the do / st exchange has
 *                      landed (at once under gatmh_bwd_phase = 2); the 16-byte records, el[u], z[u], der, a_l, a_r stay fp32.
 * The shadow rows are reserved before anything is launched and never grow inside a recording (DORY_ERR_ARG there: run one eager epoch
 * first).  Calls that would take the blocked family or the single-partition row-wise kernels are refused with the option set as
 * before, with the messages as before; with on = 0 nothing changes anywhere.  DORY_GCN / DORY_GAT contexts reject 1; other values
 * and a call while an epoch graph is being recorded are DORY_ERR_ARG.
 * The bf16 wire: halo_ships_bf16 reads switches and the option only, so dory_halo_bf16_rows + dory_gatmh_halo_bf16 now reach these
 * ranks (z forward, do backward); rounding is idempotent, so a rank's tensors are the same bits with the wire on and off wherever
 * no kernel of the family reads fg_el (dory_apply_edge's fg_el is formed from the rounded fg_z: documented above).
 * KNOWN CONSEQUENCE: where the forward's scores come from the gathered row, "m" / "den" are statistics of scores of ROUNDED rows,
 * while the source side forms its alpha from the fp32 "el" tensor: the backward's alpha differs from the forward's by the rounding
 * of a score, relative 2^-9 of a dot product's terms.  The sweep forms do not have this difference (they take scores from the
 * table).  Forming el[u] from the rounded z[u] in the source kernel would remove it; not done here.  Measured on one epoch it
 * does not show above the rounding of the rows: the family deviates from its fp32 run as the sweep forms do from theirs.
 * MEASURED (one MI355X, rank 0 of 8 of the Amazon-size graph, 3.2 edges per converted row, against the parent's library;
 * profiles/r26_gatmh_row_gather_bf16.txt): the kernels alone take x0.57-0.63 of their fp32 siblings' time on the forward and the edge
 * pass at 64 / 128 floats, x0.73-0.87 on the source side, x0.90 at 32 floats; WITH the conversion into the shadow rows NO pass is
 * faster (x1.00-1.13 at 64 / 128 floats, x1.15-1.44 at 32; epochs 18.6-18.9 -> 19.7-19.9 ms).  This switch is not a speed-up
 * until the rows arrive as bf16 and stay (ghost twins for this model) or a partition has clearly more than 3 edges per row.
 * Counters: passes that ran a bf16 form (forward, destination-side edge pass, source side); the read-only options
 * "gatmh_bf16_gathers_fwd" / "_src" and dory_gatmh_row_gather_stats count those passes too.  Any pointer may be NULL. */
int dory_gatmh_row_gather_bf16(dory_ctx *ctx, int on);   /* 0 (default) / 1 */
int dory_gatmh_row_gather_bf16_stats(dory_ctx *ctx, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *src);

/* ---- hub splitting for the row-gather kernels (opt-in, default off; nothing in the reference) -------------------------------------
 * In the three edge passes of the family above one lane group walks a row's entries alone, four gathered rows at a time: a
 * destination with tens of thousands of in-edges (a power-law partition) is one serial chain.  With chunk_entries != 0, wherever
 * dory_aggregate takes that family -- mode 1 or mode 0's fall-back, gatmh_bwd_phase 0 / 1 / 2, every transport, with or without the
 * merged exchange, bf16 rows, bf16 halo rows and ghost twins -- a HUB ROW is cut into chunks that run on lane groups of their own.
 *   entry              an ENTRY of a row is one stored entry of its adjacency: an in-edge of a destination (forward and the
 *                      destination-side edge pass), an out-edge of a source (source side).  The self edge, which the kernels
 *                      append as the last entry of the id stream, is NOT counted and belongs to the row's last chunk.
 *   hub row            a row with MORE than chunk_entries entries.  Its entries are cut, in order, into consecutive chunks of
 *                      chunk_entries entries; the last chunk is shorter.  A row of exactly chunk_entries entries is not cut.
 *   a split pass       two launches: (1) the chunks, one lane group each, with the unchanged per-entry arithmetic over their range,
 *                      each leaving its state in scratch, and in the same launch every row that is no hub row, whole; (2) one lane
 *                      group per hub row folds its chunks' states IN CHUNK ORDER and closes with the one-pass epilogue.
 *                        forward: (m_c, den_c, den+_c, acc_c, acc+_c) unnormalised; M = max m_c, sums scaled by exp(m_c - M)
 *                        destination side: partial (t, a1, a2) against the row's m / den; source side: partial S, S+, T, T+
 *                      Where the destination side runs the row-wise kernel no edges are walked and nothing changes.
 * CONTRACT: no atomics -- same input, same bits, run after run.  A row that is not cut keeps the bits it has with the feature off,
 * in every tensor; "m" keeps them on every row (a maximum is exact).  A row that is cut has its sums in another association and
 * differs from the one-pass row by rounding.  With no row over chunk_entries in an adjacency its passes launch exactly what they
 * launch with the feature off.  The bf16 forms (dory_gatmh_row_gather_bf16) are the same bodies over bf16 row chunks: a split bf16
 * pass equals the split fp32 pass on rows rounded beforehand, bit for bit.
 * chunk_entries: 0 (default) = off; else a multiple of 64 in 64..1048576.  DORY_ERR_ARG: any other value, a value other than 0 on a
 * context configured as DORY_GCN / DORY_GAT, a call while an epoch graph is being recorded.  The chunk plan of an adjacency is built when the value is
 * set (a graph being there) or by the first pass that needs it, kept per adjacency and dropped by dory_graph_upload; the chunk
 * states live in the context's scratch buffer, which cannot grow inside a recording (DORY_ERR_ARG there: run one eager epoch first).
 * dory_row_chunk_plan (dorylus_host.h) gives the same plan without a device.
 * Counters: forward passes, destination-side edge passes and source-side passes that ran split since dory_create (eager calls and
 * recordings, not replays); hub rows and chunks of the current plan of the in-edges, and of the out-edges (0 while no plan for
 * the current value is built).  Any pointer may be NULL.
 * MEASURED (one MI355X, compute only; rank 0 of 8 of an R-MAT graph at Amazon size, largest degree 101 152; the parent's library and
 * this one alternated over three rounds; profiles/r28_gatmh_row_gather_hubs.txt, tools/gatmh_row_gather_hubs_rate.py): the parent
 * takes 24-35 ms a pass; at 1 024 every pass takes x0.05-0.15 of that (forward 29.5 -> 3.1 ms at 128-float rows, source side 35.3 ->
 * 3.4), x0.06-0.15 at 2 048, x0.09-0.18 at 4 096 / 8 192.  RECOMMENDED on power-law partitions: 1 024.  The uniform rank of that size
 * (nothing cut) stays inside the spread of the rounds, switched off and on.  NOT FASTER, NAMED: switched off, the R-MAT rank's forward
 * at 1 x 25 is x1.046 of the parent's, the one switched-off line of ten outside the spread. */
int dory_gatmh_row_gather_hub_split(dory_ctx *ctx, uint32_t chunk_entries);   /* 0 (default) = off */
int dory_gatmh_row_gather_hub_split_stats(dory_ctx *ctx, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *src, uint64_t *in_hub_rows,
                                          uint64_t *in_chunks, uint64_t *out_hub_rows, uint64_t *out_chunks);

/* ---- the row-gather family: interior rows beside the exchange (opt-in, default off; nothing in the reference) ----------------
 * The row-gather kernels read ghost rows through plain pointers, so a pass waits for the exchange that fills them before it
 * launches anything: with option halo_overlap = 1 the exchange of a rank on this family is fully exposed.  A row whose every
 * adjacency entry is local needs nothing from the exchange.  With this switch on, a pass over an adjacency that has such rows
 * and others is two launches:
 *   interior row       every entry of the row is < local_vtx_cnt; a row without entries is interior (its only edge is the self edge).
 *                      In-edges: a destination whose sources are all local; out-edges: a source whose destinations are all local.
 *   boundary row       at least one entry names a ghost row.  dory_row_interior_plan (dorylus_host.h) gives both lists without a device.
 *   forward            (1) the interior rows, packed densely into lane groups, reading z (or the local shadow rows) alone; (2) the
 *                      wait for the exchange of z, the ghost rows' conversion or widening; (3) the boundary rows.
 *   backward, source   the LAST exchange of the pass -- the merged one under dory_gatmh_bwd_merged_exchange, else st's -- is issued
 *   side (phase 0)     DEFERRED where halo_overlap = 1 (do's, the first of two, never: one exchange can be pending); (1) the interior
 *                      sources, reading do / st alone; (2) the wait, bg_do's conversion or widening; (3) the boundary sources.  The
 *                      pending exchange never outlives the dory_aggregate call.  gatmh_bwd_phase = 2: the same two launches.
 *   not touched        the destination-side edge pass (it reads fg_z, which landed during the forward); the sweep and blocked forms.
 * The same two launches run whether an exchange is in flight or not (timing families "spmm_beside_halo" / "spmm_local_first").
 * With dory_gatmh_row_gather_hub_split a row the chunk plan cuts counts as a boundary row: it goes, whole, to the launch after the
 * wait, with its chunks and the merge.  Where one of the lists is empty -- no ghosts, every row boundary, no vertices -- the pass
 * launches exactly what it launches with the switch off.
 * CONTRACT: switch on = switch off, BIT FOR BIT, in every tensor, weight and weight gradient: every row is computed whole by the body
 * that computes it with the switch off; only the launch that holds it changes.  This holds for every transport, both halo schedules,
 * gatmh_bwd_phase 0 / 1 / 2, fp32 and bf16 rows, bf16 halo rows and ghost twins, the merged exchange, halo_direct_recv and hub
 * splitting at any chunk size.  The switch moves no bytes on the wire: the ranks of an in-process group may differ in it.
 * on: 0 (default) or 1.  DORY_ERR_ARG: any other value, 1 on a context configured as DORY_GCN / DORY_GAT, a call while an epoch
 * graph is being recorded.  The row lists of an adjacency are built when the switch is set (a graph being there) or by the first
 * pass that needs them, kept per adjacency, dropped by dory_graph_upload and rebuilt when the hub chunk size changes; they cannot be
 * built inside a recording (DORY_ERR_ARG there: run one eager epoch first).
 * Counters, in this order: forward passes and source-side passes that ran as two launches since dory_create (eager calls and
 * recordings, not replays); of those forward passes, and of those source-side passes, the ones with an exchange in flight beside the
 * first launch; interior rows of the current plan of the in-edges, and of the out-edges (0 while none is built); backward
 * exchanges issued deferred.  Any pointer may be NULL. */
int dory_gatmh_row_gather_overlap(dory_ctx *ctx, int on);   /* 0 (default) = off */
int dory_gatmh_row_gather_overlap_stats(dory_ctx *ctx, uint64_t *fwd_split, uint64_t *src_split, uint64_t *fwd_in_flight,
                                        uint64_t *src_in_flight, uint64_t *in_interior_rows, uint64_t *out_interior_rows,
                                        uint64_t *bwd_deferred);

/* ---- the row-gather family: local entries beside the exchange (opt-in, default off; nothing in the reference) -----------------
 * dory_gatmh_row_gather_overlap hides the exchange behind the interior ROWS only: about none on a uniform rank, a few per cent on a
 * community rank, where 98 % of the rows have a ghost entry but 85 % of the ENTRIES are local.  With this switch the forward and the
 * backward's source side walk every row's local entries before its ghost entries -- K1's local-first edge copy (halo_overlap, GCN),
 * for this family -- and carry the row's state across the wait.  Kernels gatmh_rows_{forward,src}_carry[_bf16]_kernel
 * (csrc/gat_mh_rows.hip) over a copy of the adjacency's ids regrouped local-first (dory_row_edge_split_plan, dorylus_host.h).
 *   range A            the row's entries < local_vtx_cnt, in their original order, then the self edge (a local row).
 *   range B            the row's entries >= local_vtx_cnt (ghost rows), in their original order; no self edge.
 *                      Each range ends with its own masked batch; the per-entry arithmetic is the one-pass kernels'.
 *   one launch         ("both") range A, then range B, the state in registers, then the one-pass epilogue.
 *   two launches       ("first") range A of every row: a row without ghost entries closes, any other leaves its state -- forward
 *                      (m, den, den+, acc, acc+), source side (S, S+, T, T+) -- in its slot of a buffer the context keeps for this
 *                      alone; the wait for the exchange, the ghost rows' conversion or widening; ("second") the rows with ghost
 *                      entries, packed densely into lane groups: state loaded, range B, epilogue.  Which ranges a launch walks is a
 *                      kernel ARGUMENT: the three walks are one body of machine code.
 *   value 1            with an exchange in flight when the pass starts: two launches around the wait (timing families
 *                      "spmm_beside_halo" / "spmm_local_first"); with nothing in flight: one launch, no state traffic.
 *   value 2            always two launches (tests; what the state round trip costs).
 *   deferrals          as dory_gatmh_row_gather_overlap's, whether or not that switch is on: dory_apply_edge leaves the ghost
 *                      sources' scores to the wait; the backward's LAST exchange (the merged one, or st's of two; never do's) is
 *                      issued deferred under halo_overlap = 1 and never outlives the dory_aggregate call.  Where both switches are on
 *                      and this one takes a pass, this one decides it.
 *   not taken          an adjacency whose hub chunk plan (dory_gatmh_row_gather_hub_split) has chunks: the pass runs as with value 0
 *                      and is counted (hub_fallbacks); an adjacency without ghosts, a rank without vertices: nothing to split, not
 *                      counted.  The destination-side edge pass (it reads fg_z, landed during the forward), the sweep and blocked
 *                      forms.  With dory_gatmh_row_gather_bf16_wide on, a bf16 pass that is taken runs the NARROW bf16 carry kernel
 *                      (there is no wide carry form) and is counted (wide_not_taken).
 * CONTRACT: one launch = two launches, BIT FOR BIT, in every tensor, weight and weight gradient -- value 1 with nothing in flight,
 * value 2, value 1 with the exchange in flight.  Against value 0: m keeps its bits on every row (a maximum does not depend on the
 * order of the entries); every other output changes association (ghost entries behind the local ones, the self edge between them) and
 * agrees within the family's tolerances.  A bf16 pass equals the fp32 pass on rows rounded beforehand, bit for bit.  Two runs give the
 * same bits (no atomics).  This holds for dory_gatmh_row_gather modes 0 / 1, gatmh_bwd_phase 0 / 1 / 2, every transport, the merged
 * exchange, bf16 rows, bf16 halo rows, ghost twins and halo_direct_recv (the copy is built from the ids as uploaded, renumbered or not).
 * The switch moves no bytes on the wire: the ranks of a group may differ in it.
 * value: 0 (default), 1 or 2.  DORY_ERR_ARG: any other value, 1 / 2 on a context configured as DORY_GCN / DORY_GAT, a call while an
 * epoch graph is being recorded.  The copy of an adjacency and the state buffer are built when the switch is set (a graph / the tensors
 * being there) or by the first pass that needs them, the copy dropped by dory_graph_upload; neither can be built or grown inside a
 * recording (DORY_ERR_ARG there: run one eager epoch first).
 * Counters, in this order: forward passes and source-side passes that ran the carry kernels since dory_create (eager calls and
 * recordings, not replays); of those forward passes, and of those source-side passes, the ones with an exchange in flight beside the
 * first launch; local entries of the current copy of the in-edges, and of the out-edges (0 while none is built); passes left to the
 * hub chunk plan; bf16 passes that ran the narrow carry kernel with the wide switch on.  Any pointer may be NULL.
 * NOT MEASURED YET: tools/gatmh_row_gather_edge_split_rate.py is written (it writes profiles/r31_gatmh_row_gather_edge_split.txt); no
 * output of it is on record and no gain is claimed.  As arithmetic, two launches cost a 0.9 KB slot written and read per boundary row
 * (64-float rows, ldk = 32) against 6.4 KB gathered by an fp32 row of 25 edges.  The default stays 0. */
int dory_gatmh_row_gather_edge_split(dory_ctx *ctx, int value);   /* 0 (default) = off */
int dory_gatmh_row_gather_edge_split_stats(dory_ctx *ctx, uint64_t *fwd_split, uint64_t *src_split, uint64_t *fwd_in_flight,
                                           uint64_t *src_in_flight, uint64_t *in_local_entries, uint64_t *out_local_entries,
                                           uint64_t *hub_fallbacks, uint64_t *wide_not_taken);

/* ---- the row-gather family: 16-byte bf16 row gathers (opt-in, default off; nothing in the reference) -------------------------
 * The family's bf16 form (dory_gatmh_row_gather_bf16) loads four bf16 -- 8 bytes -- per lane and edge: a 64-float row occupies 16
 * lanes, and every lane of a head recomputes the head's exponentials.  With this switch on, a bf16 pass of the family runs its WIDE
 * form where the shape has one: a lane keeps eight consecutive features (one 16-byte load per edge, two float4 accumulators), a row
 * takes half the lanes -- twice the rows in flight per wave, half the gather, address and broadcast instructions per row, half the
 * redundant per-head arithmetic.  Kernels gatmh_rows8_{forward,dst,src}[_list][_hub]_kernel (csrc/gat_mh_rows.hip).
 *   shape rule         dory_gatmh_row_gather_bf16_wide_form (dorylus_host.h): the family covers the shape, 64 <= ld <= 256 (ld a
 *                      multiple of 8), and K == 1 or D % 8 == 0.  Not taken: ld = 32 (four lanes per row), D = 1 / 2 / 4 with
 *                      several heads (no wide counterpart of two or four heads per lane).  Lanes per row 8 / 16 / 32.
 *   which passes       exactly the passes that run the family's bf16 form: the forward and the source side by option
 *                      gatmh_bf16_gather, the destination-side edge pass of a layer whose forward ran the bf16 form.  Where the shape
 *                      rule fails, or the shadow rows / the ghost twin handed to the launch are not 16-byte aligned, the narrow form
 *                      runs as with the switch off, and the pass is counted (narrow_while_on).
 *   everything else    as it is: shadow rows, ghost twins, hub splitting (the narrow merge kernels fold a wide launch's chunk
 *                      states: same layout), interior rows beside the exchange, the merged exchange, gatmh_bwd_phase 0 / 1 / 2.
 * CONTRACT: switch on = switch off, BIT FOR BIT, in every tensor, weight and weight gradient -- hence the fp32 family's bits on rows
 * rounded beforehand.  Per column the sums are the same fmaf chains in entry order; per head the values are the same scalar chains
 * over the same batches of four entries; a dot product is the narrow lanes' two four-term chains added inside the lane (the narrow
 * form's first butterfly step) and then the same butterfly over half as many lanes.
 * on: 0 (default) or 1.  DORY_ERR_ARG: any other value, 1 on a context configured as DORY_GCN / DORY_GAT, a call while an epoch
 * graph is being recorded.  1 is legal while dory_gatmh_row_gather_bf16 is off: it is then inert.  Option gatmh_bf16_wide (the
 * sweeps' wide form) is unrelated.  Counters, in this order: forward passes, destination-side edge passes and source-side passes
 * that ran the wide form since dory_create (eager calls and recordings, not replays); bf16 passes of the family that ran narrow with
 * the switch on.  Any pointer may be NULL.
 * MEASURED (profiles/r29_gatmh_row_gather_bf16_wide.txt; rank 0 of 8 at Amazon size, twins and bf16 wire on, parent / switch off / switch
 * on alternated over three rounds): uniform rank -- 4 of the 6 passes at 64- / 128-float rows faster outside the spread (x0.89-0.95 a
 * pass; compute epoch 8 x 16: 15.49 -> 14.93 ms), 2 inside it.  NOT FASTER: every wide pass of the R-MAT rank with
 * dory_gatmh_row_gather_hub_split(1024) -- forward x1.39-1.41, source side x1.18-1.22, compute epochs x1.19 / x1.11: its passes are the
 * serial chains of the hub rows' chunks, on which a wide lane does twice the arithmetic per batch.  Leave the switch off on a rank with
 * hub rows.  Switch off against the parent's library: inside the spread on 23 of 24 lines (the other: x1.006, same instructions). */
int dory_gatmh_row_gather_bf16_wide(dory_ctx *ctx, int on);   /* 0 (default) = off */
int dory_gatmh_row_gather_bf16_wide_stats(dory_ctx *ctx, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *src, uint64_t *narrow_while_on);

/* ---- K1, the row gather: 16-byte bf16 row gathers (opt-in, default off; nothing in the reference) ---------------------------------
 * K1 (csrc/spmm.hip) is the aggregation a partitioned rank of a large graph ends up on, and the one family bound by the bytes it
 * gathers.  On bf16 rows (gcn_bf16_gather; GAT prototype: dory_gat_bf16_gather) it loads four bf16 -- 8 bytes -- per lane, edge and
 * chunk.  With this switch on, an aggregation on bf16 rows that K1 runs takes its WIDE form where the rule has one: a lane keeps eight
 * consecutive features per chunk (one 16-byte load from the shadow rows or the ghost twin, two float4 accumulators), a row takes half
 * the lanes or half the chunks.  Kernel spmm_rows_bf16x8_kernel<lanes, chunks>.
 *   form rule          dory_k1_bf16_wide_form(ld, slab, &lanes, &chunks): 1 and the instantiation, or 0 (outputs 0; any pointer may be
 *                      NULL) where ld < 64, ld is no multiple of 8, or option spmm_slab makes a pass narrower than 64 floats.  By
 *                      ch8 = ceil(width / 8), width = ld or the slab where narrower: <= 8 (8, 1); <= 16 (16, 1); <= 32 (32, 1);
 *                      <= 64 (64, 1); <= 96 (32, 3); <= 128 (64, 2); <= 192 (64, 3); wider: gridDim.y slabs of (64, 3).  No context,
 *                      no device needed (dorylus_amd/host/k1_rows_wide.cpp, csrc/k1_shapes.hpp).
 *   which launches     every launch of the aggregation: the local-first edge-split copy in one launch and in two, the interior /
 *                      boundary row split, the plain launch, the clamped launch ahead of the long-row kernels.  The long-row kernels
 *                      themselves stay narrow (a hub chunk is a serial chain; wave-ordered partials do not depend on the lane width).
 *                      Where the rule has no form, or the shadow rows / the ghost rows handed to the launch are not 16-byte aligned,
 *                      the narrow form runs as with the switch off, and the aggregation is counted (narrow_while_on).
 *   everything else    as it is: K1s (its own wide form: gcn_bf16_wide, dory_gat_bf16_gather's `wide`), K1b, the multi-head families.
 * CONTRACT: switch on = switch off, BIT FOR BIT, in every tensor, weight and weight gradient, on finite inputs: per output element the
 * same fmaf chain in edge order, from the same start (zero, the self term, or the first pass's sum).
 * on: 0 (default) or 1.  DORY_ERR_ARG: any other value, 1 on a context configured as DORY_GATMH (dory_gatmh_row_gather_bf16_wide is its
 * switch), a call while an epoch graph is being recorded.  A change drops a recorded epoch graph.  1 is legal while no bf16 gather mode
 * is on: it is then inert.  Counters, in this order: aggregations that K1 ran wide since dory_create (eager calls and recordings, not
 * replays); aggregations on bf16 rows that K1 ran narrow with the switch on.  Any pointer may be NULL.
 * MEASURED (profiles/r30_k1_bf16_wide.txt; rank 0 of 8 at Amazon size, twins and bf16 wire on, conversion of the local rows included; fp32 /
 * parent / switch off / switch on alternated over three rounds): narrow against fp32 faster on all 8 lines (x0.56-0.64 on the uniform rank,
 * x0.80 on the R-MAT rank).  Wide against narrow, uniform rank: 64-float rows x0.962 / x0.964 (backward outside the spread); NOT FASTER: 128
 * floats x1.023 / x1.017 and 320 floats forward x1.017, all inside the spread (320 backward x0.950, inside it too).  NOT FASTER, outside the
 * spread: the R-MAT rank, x1.142 / x1.148 -- hub rows' clamped serial chains; leave the switch off on a rank with hub rows.  ld 320 on (16, 3)
 * against (64, 1): inside the spread, the rule keeps (64, 1).  Switch off against the parent's library: inside the spread on all 8 lines. */
int dory_k1_bf16_wide(dory_ctx *ctx, int on);   /* 0 (default) = off */
int dory_k1_bf16_wide_stats(dory_ctx *ctx, uint64_t *wide, uint64_t *narrow_while_on);
int dory_k1_bf16_wide_form(uint32_t ld, uint32_t slab, uint32_t *lanes, uint32_t *chunks);

/* ---- bf16 ghost twins: bf16 halo rows land where they are read (opt-in, default off; nothing in the reference) -------------
 * With dory_halo_bf16_rows alone a bf16 row is widened into the fp32 ghost tensor on arrival and rounded back into the shadow rows
 * by the aggregation that reads it: two conversions that cancel (the argument above), 1536 bytes of memory traffic and two kernels
 * for a 128-float row, the second one on the compute stream between the wait for the exchange and the ghost-block launch.  With
 * this second switch on too, every ghost tensor the rule above can ever cover has a bf16 TWIN -- rows x ld bf16 in the tensor's own
 * row order (wire order under halo_direct_recv), owned by the tensor -- the received rows stay bf16 in it, and the aggregation on
 * bf16 rows gathers its ghost rows from it: no widening, no conversion of ghost rows (the N local rows are converted as ever).
 * Twins: GCN fg of layers >= 1, fgxw, bg, bgg; GAT prototype fg_z, bg_d; the multi-head GAT only with dory_gatmh_bf16_ghosts (below) on
 * top -- without it this switch is inert for that model: with dory_gatmh_halo_bf16 its bf16 rows are widened on arrival and its plans
 * made with halo_direct_recv = 1 keep fp32; never a tensor of ld < 4 (one
 * column: as without the switch).  Allocated by the setter for the tensors that exist (it needs dory_preallocate: DORY_ERR_ARG
 * before it) and by dory_preallocate while the switch is on; never inside an exchange or an aggregation; freed with the tensor, or
 * by on = 0 after any twin that holds the only current copy has been widened.
 * Every such tensor has a state, which dory_halo_bf16_ghost_peek reports next to the twin's device pointer (NULL: no twin):
 * DORY_GHOST_FP32 only the fp32 rows are current, DORY_GHOST_TWIN only the twin is, DORY_GHOST_BOTH both are.
 * The exchange.  The wire is what dory_halo_bf16_rows makes it (same rule, same row_elems), with one addition: a plan made with
 * halo_direct_recv = 1 now ships bf16 too where the tensor has ld >= 4 -- dory_halo_wire_row says so; in-process ranks that
 * disagree on what they would ship fail at once with DORY_ERR_COMM as above; over RCCL and host transports EVERY RANK MUST SET THE
 * SAME.  On arrival, where the wire is bf16 and the tensor has a twin:
 *   - a direct plan and row_elems == ld: the rows land in the twin itself (ncclRecv target, the host transport's H2D copy, the
 *     in-process pull); no kernel, no receive buffer; counted in landed_direct and in the read-only key halo_direct_recvs;
 *   - anything else (a plan that is not direct; exact rows narrower than ld, e.g. 41 -> 44 elements in an ld of 64): receive
 *     buffer, then one kernel copies the bf16 rows into the twin rows the plan names, zeros in [row_elems, ld) whatever the twin
 *     held -- the bits rounding today's fp32 ghost row would give; counted in landed_by_kernel.  Under a direct plan that buffer
 *     exists only if halo_exact_rows was 1 before dory_halo_plan (the refusal of halo_direct_recv, unchanged).
 * State afterwards: TWIN; or, for a tensor whose raw pointer dory_tensor_info has handed out, the fp32 rows are widened behind the
 * twin at once on the comm stream and the state is BOTH (the caller reads fp32 rows behind the library's back and keeps seeing
 * them; an aggregation on bf16 rows of such a tensor converts its fp32 rows as ever -- the caller may have written them).
 * dory_halo_unpack follows the same rule (its kernel always copies: landed_by_kernel).  Everything else that writes a ghost tensor
 * writes fp32 rows and sets FP32: an exchange that ships fp32, dory_halo_unpack_tensor, the scatter messages,
 * dory_tensor_upload, dory_tensor_fill_uniform.
 * The readers.  An aggregation on bf16 rows whose ghost tensor is TWIN or BOTH reads the twin (conversions_skipped); in state FP32
 * everything is as without the switch (layer 0's file-loaded fg always).  Whoever reads fp32 rows -- an aggregation on fp32 rows
 * (the gather mode changed after the exchange), dory_tensor_download, dory_tensor_info handing out the device pointer -- finds a
 * TWIN tensor widened first: the exchange is waited for, one dense kernel on the compute stream writes all rows x ld floats
 * (bits << 16), the state becomes BOTH, `widened` counts it.  Visible contract: that of dory_halo_bf16_rows -- a download of fg /
 * fgxw / bg / bgg / fg_z / bg_d shows the owner's rows rounded to bf16, zeros in [cols, ld); every local tensor, weight and gradient
 * keeps its bits.  With dory_halo_bf16_rows off, or where its rule says fp32, this switch changes nothing and no twin is written.
 * dory_halo_bf16_ghosts: on = 0 (default) / 1, after dory_preallocate, outside an exchange; DORY_ERR_ARG for other values, before
 * dory_preallocate, or while an epoch graph is being recorded (which more than one partition never is).
 * dory_halo_bf16_ghosts_stats: eager calls since dory_create -- exchanges / unpacks that landed in a twin itself, that a kernel
 * copied into one, aggregations that read a twin, widenings -- and the bytes of all twins now; any pointer may be NULL.
 * Kernels (csrc/elementwise.hip): scatter_rows_bf16_keep_kernel, a lane per 8-byte quad of a twin row (one 8-byte load or zeros,
 * one 8-byte store) -- chosen by measurement over a lane per 16-byte chunk (two 8-byte loads, one 16-byte store), which is 4-10 %
 * SLOWER at every measured shape -- and widen_rows_bf16_kernel (one 16-byte load, two 16-byte stores); no LDS, no scratch.
 * Measured on one MI355X (profiles/r20_halo_bf16_ghosts.txt, profiles/HISTORY.md section 21), 3.15 M ghost rows, switch off / on
 * alternated: unpack, widening -> keep, 0.221 -> 0.150 ms (64 floats), 1.153 -> 0.803 (300), 1.131 -> 0.745 (300 exact), 0.455 -> 0.308
 * (128), 0.216 -> 0.148 / 0.207 -> 0.129 (48 padded / exact), 0.214 -> 0.147 / 0.207 -> 0.127 (41): faster at every measured shape.  In the
 * in-process-transport epoch (200 000 vertices, 4 M edges, 128-128-16, gather mode 2) the ghost half of the timing key bf16_convert is
 * gone (launches 600 -> 400 per 50 epochs at P = 2, 1200 -> 800 at P = 4) and the epoch stays inside its run-to-run spread, direct 0
 * and 1; with both switches off the headline and the GAT prototype epoch are at the parent's level (one headline reading of seven
 * 0.5 % above the parent's highest of its session).  NO RCCL CALL WITH MORE THAN ONE RANK HAS RUN AND NO LINK IS MEASURED. */
enum { DORY_GHOST_FP32 = 0, DORY_GHOST_TWIN = 1, DORY_GHOST_BOTH = 2 };
int dory_halo_bf16_ghosts(dory_ctx *ctx, int on);
int dory_halo_bf16_ghosts_stats(dory_ctx *ctx, uint64_t *landed_direct, uint64_t *landed_by_kernel, uint64_t *conversions_skipped,
                                uint64_t *widened, uint64_t *twin_bytes);
int dory_halo_bf16_ghost_peek(dory_ctx *ctx, uint32_t layer, const char *name, const void **twin, int *state);

/* ---- bf16 ghost twins for the multi-head GAT (opt-in, default off; on top of dory_halo_bf16_ghosts; nothing in the reference) -----
 * dory_halo_bf16_ghosts leaves the multi-head GAT out: the model has readers of fg_z's fp32 rows the other models do not have
 * (dory_apply_edge forms fg_el / fg_er from them; the sweep forward's finish and redo kernels; the fp32 and the blocked forms) and it
 * exchanges do / st itself.  With this switch on, "fg_z" and "bg_do" of every layer get a twin as well (allocated by the setter and by
 * a later dory_preallocate; dory_halo_bf16_ghost_peek and twin_bytes report them); "bg_st", "fg_el" and "fg_er" never do.
 * LANDING.  Wherever the wire of an exchange is bf16 by the rule of dory_gatmh_halo_bf16 (dory_halo_bf16_rows + dory_gatmh_halo_bf16 +
 * option "gatmh_bf16_gather" at that call) the rows stay bf16 in the twin, states DORY_GHOST_TWIN / _BOTH exactly as for the other
 * models: in the RCCL, host and in-process transports and in the split entry points -- dory_halo_unpack, and dory_gatmh_bwd_unpack for
 * the merged row, whose do part goes into bg_do's twin while st goes into bg_st as fp32.  A plan made with halo_direct_recv = 1 now
 * ships bf16 for this model too and lands in the twin itself (forward z -> fg_z, and the do -> bg_do exchange of an unmerged
 * backward; the merged exchange is not taken under direct plans, as before).  There the switch changes what travels, fp32 -> bf16, so
 * the visible consequence of dory_gatmh_halo_bf16 (fg_el from rounded rows) now holds under direct plans too.
 * GATHERS.  The bf16 edge passes -- the row-gather family's three and the sweep forms' two -- gather their ghost rows from the twin
 * and convert only the N local rows into the shadow rows; those are reserved for N rows where a twin serves.
 * SCORES.  Where fg_z's twin alone is current, dory_apply_edge forms fg_el / fg_er from the twin (launch_gatmh_scores_bf16: one
 * 8-byte load of four bf16 per lane where the fp32 kernel loads a float4, the same lane mapping, fmaf chain and shuffle butterfly):
 * the fp32 kernel's result on the widened rows, bit for bit -- the contract of dory_gatmh_halo_bf16 (fg_el from rounded rows).
 * READERS OF FP32 ROWS find a twin that alone is current widened first (ghost_fp32_current: one dense kernel, state BOTH, counted
 * here and in dory_halo_bf16_ghosts_stats' `widened`).  CORRECT, AND NOT A GAIN: the sweep forward's finish and redo kernels, which
 * read fg_z's fp32 rows after every forward of a layer that sweeps (twin-reading forms of them are not built: with the sweep forms
 * this switch trades the conversion of the ghost rows for a widening of the same rows); the family's fp32 forms when
 * "gatmh_bf16_gather" was lowered between exchange and aggregation; the fp32 destination-side edge pass of a layer whose forward
 * swept; the blocked forms; dory_tensor_download; dory_tensor_info handing out a raw pointer (then BOTH after every later exchange).
 * CONTRACT: with dory_halo_bf16_rows, dory_gatmh_halo_bf16 and dory_halo_bf16_ghosts on, every local tensor, weight and gradient
 * has the same bits with this switch on and off, and a download of fg_z / bg_do shows the same (rounded) rows.
 * Kernels beside their siblings, whose code objects do not change: gatmh_scores4_bf16_kernel / gatmh_scores_bf16_kernel
 * (csrc/gat_mh.hip) and scatter_rows_pair_bf16_keep_kernel (csrc/elementwise.hip: the keep form of the merged unpack -- 16-byte
 * chunks, zeros in [w, ld) of the twin row, 32-bit indices, the launcher slices at 2^31 chunks; no LDS, no scratch).
 * dory_gatmh_bf16_ghosts: on = 0 (default) / 1; a DORY_GATMH context after dory_preallocate, outside an exchange, with
 * dory_halo_bf16_ghosts already on -- anything else, other values and a call while an epoch graph is being recorded are DORY_ERR_ARG
 * with a message naming what is missing.  dory_halo_bf16_ghosts(ctx, 0) turns this switch off too and frees these twins with the
 * others (the only current copies widened first).  ALL RANKS MUST SET THE SAME VALUE: in-process ranks that disagree fail with
 * DORY_ERR_COMM before anything of an exchange is enqueued.  With it off every byte and counter is as before.
 * dory_gatmh_bf16_ghosts_stats: eager calls since dory_create (not recordings) -- forward exchanges / unpacks whose rows stayed in
 * fg_z's twin; backward ones for bg_do, alone and through a merged row; bf16 passes that read a twin instead of converting ghost
 * rows, of the row-gather family and of the sweep forms; dory_apply_edge calls that formed fg_el from a twin; widenings for a reader
 * of fp32 rows.  dory_halo_bf16_ghosts_stats keeps moving as for the other models.  Any pointer may be NULL.
 * MEASURED on one MI355X -- NO LINK, NO SECOND GPU AND NO RCCL RUN WITH MORE THAN ONE RANK ARE BEHIND ANY NUMBER --
 * profiles/r27_gatmh_bf16_ghosts.txt (tools/gatmh_bf16_ghosts_rate.py: rank 0 of 8 of the Amazon-size graph, 3.2 edges per row, 87 % of
 * the rows ghosts, delivered as bf16 through dory_halo_unpack / dory_gatmh_bwd_unpack; rows of 32 / 64 / 128 floats, heads 8 x 16, 8 x 8,
 * 32 x 2; the parent's library and this one alternated over three rounds, each pass with the conversion that belongs to it).  The
 * row-gather family: against the parent (N + ghosts rows converted) forward and edge pass x0.63-0.69, source side x0.71-0.81, a compute
 * epoch x0.80-0.81 (19.5 -> 15.7, 12.3 -> 10.0, 15.7 -> 12.6 ms); against the fp32 pass, which r26 lost at every line, forward
 * x0.61-0.71 at 64 / 128 floats and x0.89-0.90 at 32, edge pass x0.64 / x0.88-0.90, source side x0.75-0.83 / x0.91-0.95, the compute
 * epoch x0.84-0.86.  The keep unpacks x0.66-0.75 (fg_z) and x0.75-0.90 (merged); dory_apply_edge x0.92-0.97 where the four-element
 * kernel runs.  NOT FASTER, NAMED: dory_apply_edge at 32 x 2 (the scalar kernel; x1.012 against the parent, a tie).  NOT FASTER, NAMED:
 * the SWEEP forms' Reddit-size epoch over the in-process transport at P = 2 (off 26.9-27.5 ms, on 27.4-28.4): bf16_convert falls
 * 6.3-6.6 -> 2.0 ms per 10 epochs, and the widening for the finish kernel takes it back. */
int dory_gatmh_bf16_ghosts(dory_ctx *ctx, int on);   /* 0 (default) / 1 */
int dory_gatmh_bf16_ghosts_stats(dory_ctx *ctx, uint64_t *fwd_kept, uint64_t *bwd_kept, uint64_t *bwd_kept_merged, uint64_t *twin_reads_rows,
                                 uint64_t *twin_reads_sweep, uint64_t *scores_from_twin, uint64_t *widened);

/* ---- scatter messages: the reference's own graph-server <-> graph-server wire, packed and unpacked on the device ----------
 * What Engine::verticesPushOut puts on a socket and ghostReceiver* takes apart (include/dorylus_wire.h: the format table with
 * its citations): messages of an 8-character receiver topic, five unsigned header fields and (global vertex id, featDim floats)
 * records, at most max_msg_bytes each.  With these entry points a HIP graph server hands an unmodified reference graph server
 * the very bytes it expects, and takes its messages as a socket leaves them, with no work on the rows by the host.  The sockets,
 * the per-message ACK, the barrier and async mode stay the caller's.  max_msg_bytes: 0 = the reference's
 * 1 MiB; below 2^32.  name == NULL: the tensors dory_halo_exchange(layer, dir) would move; otherwise any per-vertex tensor
 * (pack) / ghost tensor of that direction (deliver) at `layer`, as in dory_halo_pack_tensor.  Rows of at most 8185 floats.
 * Not executed against a reference binary and not measured over any link: DESIGN.md sections 4 and 5. */

/* The global ids the records carry: local_to_global[N] (localToGlobalId), and the ghosts' global ids of both directions in slot
 * order (srcGhostVtcs / dstGhostVtcs; what dory_partition_view holds) -- ascending, anything else is refused.  After
 * dory_graph_upload; dory_partition_upload calls it itself when `parts` is given.  Off the epoch's path: it uploads the tables,
 * clears the round stamps and allocates the fixed staging area of dory_scatter_msgs_deliver (two pinned host slots and two
 * device slots of max(1 MiB, the widest record) bytes). */
int dory_halo_wire_ids(dory_ctx *ctx, const uint32_t *local_to_global, const uint32_t *src_ghost_gvids, const uint32_t *dst_ghost_gvids);

/* one message of an exchange inside one buffer: `rows` records for `peer`, the entries first_row .. first_row + rows - 1 of the
 * plan's send list (dory_halo_plan's send_lvids, all peers concatenated), at byte `offset` (a multiple of 16), `bytes` =
 * 28 + rows x (4 + 4 cols) long */
struct dory_scatter_msg {
    uint32_t peer, first_row, rows;
    uint64_t offset, bytes;
};
/* The messages of one exchange, as the reference's sender loop cuts them (per peer in rank order the send list in consecutive
 * batches of dory_wire_scatter_batch(cols, max_msg_bytes) rows, the last one short, none for a peer without rows), laid out in
 * ONE buffer of *total_bytes bytes, every message 16-byte aligned.  msgs may be NULL (sizes only); otherwise max_msgs entries
 * are available, and fewer than *n_msgs is DORY_ERR_ARG.  Host only. */
int dory_scatter_msgs_layout(dory_ctx *ctx, uint32_t layer, int dir, const char *name, uint64_t max_msg_bytes,
                             struct dory_scatter_msg *msgs, uint32_t max_msgs, uint32_t *n_msgs, uint64_t *total_bytes);
/* Writes every message of that layout, headers included, into the device buffer dev_buf (16-byte aligned, total_bytes bytes; not
 * one byte beyond is touched) on the compute stream: each message is byte for byte what the reference sends for the same
 * tensor, the bytes between messages are zero.  The header's layer is the ghost tensor's (name: `layer` itself). */
int dory_scatter_msgs_pack(dory_ctx *ctx, uint32_t layer, int dir, const char *name, uint64_t max_msg_bytes, void *dev_buf);
/* n >= 1 whole messages in host memory (msgs[i] of bytes[i] bytes), from any senders, in any order and batching.  The headers
 * are parsed on the host; every message names its ghost tensor by (layer, dir) -- GCN "fg"@layer / "bg"@layer, GAT and GATMH
 * "fg_z"@layer / "bg_d"@layer -- or `name` names it at the header's layer.  Before anything is enqueued the call refuses
 * (DORY_ERR_ARG, the text names the field) a malformed or truncated message, a featDim other than the tensor's cols, a receiver
 * other than this rank, a dir other than 0 / 1 and a layer out of range.  The records then go through the staging area to the
 * device and an unpack kernel on the comm stream finds each record's ghost slot by binary search of the ids, and writes the
 * whole stored row ([0, cols) from the record, zeros into [cols, ld); under halo_direct_recv at the slot's wire-order row):
 * the raw rows are the bits dory_halo_exchange leaves.  Every ghost slot carries a round stamp: an unknown id and an id that
 * arrives twice in a round are counted on the device and never written.  Writing "fg"@0 / "fg_z" drops the cached ah@0 / the
 * kept neighbour sum, as dory_halo_exchange does.  Allocates nothing. */
int dory_scatter_msgs_deliver(dory_ctx *ctx, const char *name, const void *const *msgs, const uint64_t *bytes, uint32_t n);
/* The unpack alone, for records that are in device memory already (a transport that lands payloads there; what
 * tools/scatter_msgs_rate.py times): `count` records of (id, cols floats), no header, at the 16-byte aligned dev_records, into
 * the ghost tensor of the exchange (layer, dir) or the named one -- the same kernel, stamps and counters as the deliver's, on
 * the comm stream; dory_scatter_msgs_finish ends the round. */
int dory_scatter_msgs_unpack(dory_ctx *ctx, uint32_t layer, int dir, const char *name, const void *dev_records, uint32_t count);
/* Ends a round of direction `dir`: waits for the unpacks, reports the ghost rows written and the records refused, opens the next
 * round.  DORY_ERR_COMM unless every ghost slot of the direction was written exactly once (rows == ghost count, unknown ==
 * duplicate == 0): the reference's ghostVtcsRecvd == totalGhostCnt (gcn_ops.cpp:339-347).  Outputs may be NULL. */
int dory_scatter_msgs_finish(dory_ctx *ctx, uint32_t layer, int dir, const char *name, uint32_t *rows, uint32_t *unknown,
                             uint32_t *duplicate);
/* The same as a transport, next to dory_comm_set_host_transport (setting one clears the other; NULLs return to RCCL):
 * dory_halo_exchange and the multi-head GAT backward's "do" / "st" exchanges pack the messages on the device, copy the buffer
 * to pinned host memory and call exchange(user, ctx, host_buf, msgs, n_msgs) on the calling thread: message i is host_buf +
 * msgs[i].offset.  The callee sends them and, before it returns, hands every message that arrived for this rank to
 * dory_scatter_msgs_deliver(ctx, NULL, ...) (from this thread; NULL = the exchange's own ghost tensor); the library then runs
 * dory_scatter_msgs_finish.  Scheduling around the aggregation (halo_overlap, the timing families) is the host transport's, and
 * dory_weight_update / dory_train_stat_global use allreduce_sum as that arm does. */
typedef int (*dory_scatter_exchange_fn)(void *user, dory_ctx *ctx, const void *host_buf, const struct dory_scatter_msg *msgs, uint32_t n_msgs);
int dory_comm_set_scatter_transport(dory_ctx *ctx, dory_scatter_exchange_fn exchange, dory_allreduce_fn allreduce_sum, void *user,
                                    uint64_t max_msg_bytes);

/* ---- weight-gradient reduction + optimiser (replaces the weight server's
 * PUB/SUB all-gather-and-sum + Adam, src/weight-server/weightserver.cpp:89-187,
 * weighttensor.cpp:131-166,246-328, AdamOptimizer.cpp:29-51) ---------------------
 * dory_weight_update: all-reduce(sum) of the layer's gradient over the
 * communicator (no-op when alone), then one Adam step.  Layer 0 advances the
 * optimiser's iteration count like AdamOptimizer::update. */
int dory_adam_config(dory_ctx *ctx, float learning_rate);
int dory_weight_update(dory_ctx *ctx, uint32_t layer);

/* ---- introspection -------------------------------------------------------------- */
/* what dory_configure / dory_graph_upload recorded (any pointer may be NULL) */
int dory_ctx_describe(dory_ctx *ctx, int *gnn_type, uint32_t *num_layers, uint32_t *node_id,
                      uint32_t *num_nodes, uint32_t *local_vtx_cnt);
/* average device time (ms) and launch count of a kernel family since the last
 * reset, measured with HIP events on the stream the kernel runs on; names:
 * "spmm", "gemm", "loss", "edge", "halo", "allreduce", "adam".  Overlap of an exchange with the aggregation that runs beside
 * it ("halo_overlap"): "halo_deferred" = exchanges the compute stream did not wait for at once, "spmm_beside_halo" = the
 * launches that ran beside them (local-source blocks / interior rows), "halo_hidden" = the part of each such exchange that
 * lies inside its launch's interval on the device clock (total_ms; hidden / deferred = the overlap fraction). */
int dory_timing_enable(dory_ctx *ctx, int on);
int dory_timing_get(dory_ctx *ctx, const char *family, double *total_ms, uint64_t *launches);
int dory_timing_reset(dory_ctx *ctx);
/* tuning knobs (e.g. "spmm_variant", "spmm_slab"); unknown keys are an error (DORY_ERR_ARG).  Read-only keys of dory_get_option:
 * "spmm_gate_timeouts" (K1s sweeps whose workgroups were not co-resident within the polling bound: the launch and the
 * context's next 16 K1s launches ran without gates -- same results, unsynchronised gather rate) and
 * "spmm_ungated_launches"; "epoch_graph_recorded".  dory_timing_get("spmm_gate_timeouts") returns the same pair
 * (launches = timeouts, total_ms = ungated launches).  Write-only key "spmm_gates_rearm": ends a gate back-off at once
 * (a caller that has just changed its cause, e.g. another "spmm_sweep_reserve_cus"); the counters stay (refused while an
 * epoch graph is being recorded; read back: 1 while a back-off is pending).  K1s's placement assumption -- workgroups
 * with equal id & 7 share an XCD, eight XCDs -- is checked once per context at dory_create with HW_REG_XCC_ID probes:
 * read-only "spmm_xcd_mapping_ok", "spmm_xcd_count"; when it does not hold, the first repeatable K1s launch is timed with
 * and without gates and the faster form kept ("spmm_xcd_policy": -1 nothing to decide, 0 gated, 8 ungated;
 * "spmm_xcd_gated_us" / "spmm_xcd_ungated_us"); "spmm_xcd_assume_mismatch" = 1 forces that path (tests).
 * Every key -- the options with their defaults, accepted values, model and when the library reads them (every call, at
 * dory_graph_upload, at dory_preallocate, when a layout is built, by the engine), the read-only keys and the action -- is a
 * record of one table: dorylus_amd/host/options.cpp, ids in dorylus_amd/csrc/options.hpp; dory_option_spec and
 * dory_option_check (dorylus_host.h) enumerate and ask it without a context.  Two options are refused once a graph is uploaded
 * ("spmm_sweep_cus", "halo_direct_recv"); the others that the table marks as read at the upload or at a layout's build are
 * accepted later and reach what is built from then on.  The timing family "spmm_local_first" is the first launch of a
 * two-launch aggregation when no exchange is in flight ("spmm_blk_force_split"). */
int dory_set_option(dory_ctx *ctx, const char *key, int64_t value);
int dory_get_option(dory_ctx *ctx, const char *key, int64_t *value);
/* Diagnostic (no reference counterpart): hold `workgroups` whole CUs for `usec` microseconds with a sleeping kernel on
 * the context's comm stream -- what an exchange's RCCL kernels or a co-tenant's kernels do to the aggregation that runs
 * beside them.  Lets a single-GPU test exercise "spmm_sweep_reserve_cus" and the gate timeouts. */
int dory_debug_occupy_cus(dory_ctx *ctx, uint32_t workgroups, uint64_t usec);

/* Transform-first order of GCN layer 0 (option "gcn_transform_first" = 1; no reference counterpart): when the
 * input is wider than the first hidden layer, z0 = A (X W0) instead of (A X) W0, i.e. the aggregation gathers
 * dims[1]-wide rows, and dW0 = X^T (A^T g0).  Same z0, h0, dW0 within fp32 rounding; "ah"@0 is not produced.
 * Stage meaning in this mode: dory_aggregate(0, FORWARD) writes "z"@0; dory_apply_vertex(0, FORWARD) only applies
 * tanh; dory_apply_vertex(0, BACKWARD) only forms g0; dory_halo_exchange(0, BACKWARD) ships g0's ghost rows;
 * dory_aggregate(0, BACKWARD) forms dW0 -- call dory_weight_update(0) after it.  dory_engine_run follows this
 * order by itself.  Precondition: the backward adjacency values are the forward ones transposed, which holds for
 * partitions built from directed records (the reference datasets are stored symmetrised and run with
 * --undirected 0, run/run-onnode:46); with --undirected 1 the reference counts ghost degrees from file records
 * only (dataloader.cpp:192-218) and the two owners of an edge disagree on its value: dory_partition_upload then
 * sets the option "adjacency_values_asymmetric" and the mode stays off (a direct dory_graph_upload caller sets it
 * itself).  Returns 1 when the mode applies to the configured model and graph, else 0. */
int dory_transform_first_active(dory_ctx *ctx);
/* With "gcn_transform_first" = 2 every layer whose input is wider than its output runs in this order (Reddit: both
 * layers -- aggregations of 128, 41, 41 and 128 floats per edge instead of 602, 128, 128).  For such a layer l > 0:
 * dory_apply_vertex(l-1, FORWARD) also leaves "xw"@l = h_{l-1} W_l, the forward exchange of layer l ships those
 * (narrower) rows, dory_aggregate(l, FORWARD) writes "z"@l, the backward exchange of layer l ships g_l, and
 * dory_aggregate(l, BACKWARD) forms u_l = A^T g_l, dW_l = h_{l-1}^T u_l and "aTg"@(l-1) = u_l W_l^T; the weight
 * update of layer l follows that call.  dory_transform_first_active reports whether any layer is in this mode,
 * dory_transform_first_layer a particular one. */
int dory_transform_first_layer(dory_ctx *ctx, uint32_t layer);

/* Cached layer-0 aggregate (option "gcn_cache_ah0" = 1, default 0; no reference counterpart -- Engine::aggregateGCN
 * recomputes A_hat x every epoch, gcn_ops.cpp:139-148, and so does the default here).  In full-graph training "ah"@0 is a
 * constant of the run: "x" and "fg"@0 come from files and the adjacency never changes.  With the option on,
 * dory_aggregate(0, DORY_FORWARD) returns at once while "ah"@0 still holds the aggregate of the current inputs: it is
 * recomputed after any dory_tensor_upload / dory_tensor_fill_uniform / dory_halo_unpack* of a layer-0 tensor, a
 * dory_halo_exchange(0, DORY_FORWARD) (it rewrites "fg"@0: a peer may hold a new "x"), dory_graph_upload,
 * dory_preallocate or dory_set_option.  (A caller that writes "x" through the device pointer of
 * dory_tensor_info must invalidate by one of those calls itself.)  Results are bit-identical to the uncached run: the
 * same kernel produced the kept tensor.  Not combined with a recorded epoch (the recording always contains the
 * aggregation).  dory_get_option "gcn_cache_ah0_skips" counts the aggregations answered from the kept tensor. */

/* bf16 row gathers (option "gcn_bf16_gather", default 0; GCN contexts only, no reference counterpart).  1: every forward
 * GCN aggregation reads its source rows as bf16 -- "x"/"fg"@0, "h"@(l-1)/"fg"@l, and in the transform-first order
 * "xw"/"fgxw"; 2: as 1, and the backward aggregations too ("grad"/"bg" -> "aTg", transform-first "g"/"bgg" -> "u").
 * Every row an aggregation reads -- the self row norm[v]*x[v], local rows and ghost rows -- is rounded to bf16, round to
 * nearest even (fp32 subnormals stay bf16 subnormals); the edge values, norm, the sums (in the order of the fp32 path) and
 * the output stay fp32: the result is bit for bit the fp32 path's on the rounded rows.  The stored tensors stay fp32; the
 * bf16 rows are a per-call copy inside the library (ghost rows are converted only once their exchange has landed), never
 * kept across calls.  That copy grows lazily on first eager use and cannot grow while an epoch is recorded (DORY_ERR_ARG).
 * Kernels: K1s and K1 have bf16 forms; K1b has none -- where the fp32 dispatch would take K1b, the bf16 path runs K1, and
 * dory_aggregate fails with DORY_ERR_ARG for spmm_variant = 1 together with a nonzero value.  A GAT / multi-head GAT context
 * rejects values other than 0, as do values outside {0, 1, 2}.  Read-only "gcn_bf16_gathers_k1s" / "gcn_bf16_gathers_k1"
 * count the aggregations that ran on bf16 rows per kernel family (eager calls and recordings, not replays); timing family
 * "bf16_convert" times the conversions. */

/* 16-byte gathers of those bf16 rows (option "gcn_bf16_wide", default 0; GCN contexts only; read by every call).  1 changes
 * the lane mapping of the K1s launches on bf16 rows of 128 floats or more: 16-lane groups on slabs of 128 features, a lane
 * holding eight consecutive features and fetching them with one 16-byte load -- half the gather instructions per row of the
 * 8-byte form.  It changes no bit of any result: the same rounded rows, the same fp32 sums in the same order (bit for bit the
 * 8-byte form's on finite rows), the same layout, gates, schedule around a halo exchange and shadow copy; nothing new is
 * allocated, so it may be switched inside and outside an epoch-graph recording.  It does not apply -- the aggregation runs
 * as with 0 -- while "gcn_bf16_gather" is 0 (or 1, for the backward aggregations), to rows narrower than 128 floats, to K1
 * (and where K1 runs in K1b's place), to lane groups of 8 ("spmm_blk_group"), and where "spmm_sweep_rows" forces 6 or 8 rows
 * per lane group (the form is built for the 2 .. 5 rows a 16-lane launch takes of a layout).  Values outside {0, 1} are
 * rejected, 1 also by GAT / multi-head GAT contexts and by dory_configure for them.  Read-only "gcn_bf16_gathers_k1s_wide"
 * counts the aggregations that ran this form (eager calls and recordings, not replays); "gcn_bf16_gathers_k1s" and
 * "spmm_launches_k1s" count them too.  Measured: DESIGN.md section 3, profiles/r09_bf16_wide_ab.txt. */

/* Which kernel family ran.  Read-only "spmm_launches_k1s" / "spmm_launches_k1b" / "spmm_launches_k1" count the aggregations
 * (GCN's, and the GAT prototype's) per kernel family, at the point where the family commits to running one: K1s the gated
 * sweep, K1b the partial rows per source block, K1 the row gather.  One aggregation moves exactly one of them by one, however
 * many launches it is made of (eager calls and recordings, not replays).  The multi-head GAT's edge passes are not counted. */

/* bf16 row gathers in the multi-head GAT sweeps (option "gatmh_bf16_gather", default 0; DORY_GATMH contexts only, no reference
 * counterpart; "gcn_bf16_gather" keeps refusing these contexts).  1: the forward edge pass of every layer reads the rows of
 * "z" / "fg_z" rounded to bf16.  2: as 1, and the backward's source-side pass reads the rows of "do" / "bg_do" rounded to bf16.
 * Rounding is round to nearest even (fp32 subnormals stay bf16 subnormals), the conversion "gcn_bf16_gather" uses.  The
 * stored tensors stay fp32; "el", "er", the shift "m", the statistics records "st", a_l, every sum, "den", "dpos" and all
 * outputs stay fp32, and the sums run in the fp32 kernels' order:
 *   forward   dory_aggregate(layer, DORY_FORWARD) produces bit for bit what the call with the option off produces after
 *             "z" (and "fg_z") have been replaced by their rounded values between dory_apply_edge and dory_aggregate.  That
 *             covers the gathered rows, the score a 128-float launch forms from the gathered row, the self edge's row and the
 *             rows re-read for underflowed denominators.  Where the fp32 path takes el[u] from the table "el" / "fg_el", it
 *             still does: dory_apply_edge wrote the table from the unrounded "z".
 *   backward  with "gatmh_bwd_phase" = 2 the call produces bit for bit what the call with the option off produces after "do"
 *             (and "bg_do") have been replaced by their rounded values between phase 1 and phase 2: the rows gathered over
 *             the out-edges and the self edge's do[u].  The destination side (t, der, "st") keeps the fp32 "do", and z[u]
 *             stays fp32.  "gatmh_bwd_phase" = 0 equals phases 1 and 2 in turn.
 * The bf16 rows are the per-call copy "gcn_bf16_gather" uses ((N + ghosts) x ld, ghost rows converted only once their
 * exchange has landed, never kept across calls); it grows lazily in eager calls and cannot grow while an epoch is recorded
 * (DORY_ERR_ARG: run one eager epoch with the option first).
 * Only the sweep forms (gat_mh_sweep.hip) have bf16 kernels.  Where the dispatch would leave them -- "gatmh_sweep" = 0,
 * "spmm_variant" other than 2, heads x features outside the sweep's shapes, no sweep layout for the graph (a graph whose rows
 * fit the L2, unless "spmm_blk_nb" asks for one), and for value 2 a layer whose backward takes the blocked kernels (its
 * forward did not run the sweep form; a single head of at most 32 features) -- dory_aggregate fails with DORY_ERR_ARG and
 * names the condition; it never runs fp32 in silence.  The option is read by every call: a caller may run such a layer's
 * backward with value 1.  Values outside {0, 1, 2} and nonzero values on DORY_GCN / DORY_GAT contexts are rejected.
 * Read-only "gatmh_bf16_gathers_fwd" / "gatmh_bf16_gathers_src" count the passes that ran on bf16 rows (eager calls and
 * recordings, not replays); timing family "bf16_convert" times the conversions.  Measured: profiles/r08_gatmh_bf16_ab.txt. */

/* 16-byte gathers of those bf16 rows (option "gatmh_bf16_wide", default 0; DORY_GATMH contexts only; read by every call).  1
 * changes the lane mapping of the sweep launches that run on bf16 rows: 16-lane groups on the same slabs of 128 features, a
 * lane holding eight consecutive features and fetching them with one 16-byte load, a head of D features spanning D / 8 lanes
 * instead of D / 4 -- half the gather instructions per row and half the lanes that repeat a head's exponential, branch test
 * and statistics update per edge.  It changes no bit of any result: the same rounded rows, the score formed from the gathered
 * row with the sums in the 8-byte form's order, every later sum per feature in the same entry order, the same layout, gates,
 * two launches around an exchange, pieces of split rows and shadow copy; nothing new is allocated, so it may be switched
 * inside and outside an epoch-graph recording.  It takes effect on a pass that already runs on bf16 rows ("gatmh_bf16_gather"
 * >= 1 for the forward edge pass, 2 for the backward's source-side pass) of a layer whose rows are 128 floats or wider with
 * more than one head of 16, 32 or 64 features.  Everywhere else -- heads of 8 features, a single head, narrower rows,
 * "gatmh_bf16_gather" too small for the pass -- the pass runs exactly as with 0, and no error is raised.  Values outside
 * {0, 1} are rejected, 1 also by configured DORY_GCN / DORY_GAT contexts and by dory_configure for them.  Read-only
 * "gatmh_bf16_gathers_fwd_wide" / "gatmh_bf16_gathers_src_wide" count the passes that ran this form (eager calls and
 * recordings, not replays); "gatmh_bf16_gathers_fwd" / "_src" count them too.  Measured: DESIGN.md section 3,
 * profiles/r10_gatmh_bf16_wide_ab.txt. */

/* Exact-width halo rows (option "halo_exact_rows", default 0; every gnn_type; read by every call).  0: every packed halo row
 * holds the padded `ld` floats of its tensor (41 -> 64, 48 -> 64, 25 -> 32), the owner's zero padding included.  1: it holds
 * exactly `cols` floats, the logical width of the tensor that travels -- what the reference ships (featDim floats per row,
 * engine/utils.cpp:623-650, verticesPushOut).  Layout: rows are dense, row i at float offset i * cols, peer q's segment at
 * send_off[q] * cols / recv_off[q] * cols (row offsets of the plan, in peer order).  This holds for the library's own send /
 * receive buffers in all three arms of an exchange (dory_halo_exchange and the multi-head GAT backward's "do" / "st"
 * exchanges) and for the caller's buffers of dory_halo_pack / dory_halo_unpack / dory_halo_pack_tensor /
 * dory_halo_unpack_tensor (total_send_rows x cols / total_recv_rows x cols floats, not one more).
 *   host transport  the counts and offsets handed to dory_alltoallv_fn are rows x cols and row offset x cols floats: the
 *                   reference's own wire format, no re-packing on the host.
 *   unpack          writes the whole ghost row: [0, cols) from the buffer, zeros into [cols, ld).  The raw ld-wide ghost rows
 *                   are the bits the padded form leaves; no result of any later call changes by a bit.
 *   widths          source and ghost tensor must agree in cols as well as ld (DORY_ERR_ARG).
 *   alignment       with 1 and cols % 4 != 0 the caller's pointer of the four split entry points must be 16-byte aligned
 *                   (DORY_ERR_ARG otherwise): the buffer is addressed in 16-byte quads of the whole stream of rows x cols
 *                   floats.  (The padded form has always assumed that alignment without checking; 0 stays as it is.)
 *   agreement       all ranks must use the same value.  The in-process device transport checks it against every peer before
 *                   anything of the exchange is enqueued or counted and fails at once with DORY_ERR_COMM, naming both ranks;
 *                   the call may be repeated after the option is fixed.  Over RCCL and over a host transport agreement is
 *                   the caller's contract: a rank with another value sends and expects other counts.
 *   buffers         nothing new is allocated: what dory_halo_plan sized for the widest padded row is large enough, and the
 *                   option may be switched between calls.  num_nodes == 1 keeps exchanging nothing.
 * Values outside {0, 1} are rejected.  Read-only "halo_rows_packed" / "halo_floats_packed": rows and floats the eager packs
 * (exchanges and dory_halo_pack*) wrote into send buffers since dory_create, one step per pack; "halo_exact_packs": the packs
 * that ran the exact form on rows narrower than their padding (cols < ld).  Kernels: widths that are multiples of 4 keep
 * gather_rows_kernel / scatter_rows_kernel at the exact width (plus a kernel that zeroes the padding); other widths take
 * gather_rows_exact_kernel / scatter_rows_exact_kernel (csrc/elementwise.hip).  The RCCL arm takes its counts and offsets from
 * the same width variable as the other two, but no run with more than one RCCL rank has ever executed it (two ranks cannot
 * share one GPU under RCCL): the link bytes saved -- 41/64, 48/64, 25/32 of the padded form's -- are arithmetic, not a
 * measurement.  Pack / unpack cost measured on one GPU: DESIGN.md section 5, profiles/r11_halo_exact_rows.txt. */

/* Wire-ordered ghosts (option "halo_direct_recv", default 0; every gnn_type; set before dory_graph_upload and refused with
 * DORY_ERR_ARG once a graph is uploaded: the adjacency's ghost numbering depends on it; read by dory_graph_upload's callers and
 * by dory_halo_plan).  0: a halo exchange packs, transports into a receive buffer, and unpacks that buffer into the ghost tensor
 * by recv_slots.  1: ghost rows are stored in the order they arrive on the wire -- peer by peer, each peer's rows in the order
 * of its send list -- so the received row r IS ghost row r, the receive targets the ghost tensor itself, and the unpack kernel
 * and the receive buffer disappear.  Every gather already reads ghost rows through an index (a source id >= N is row id - N of
 * the ghost tensor), so nothing changes on the epoch's path but the ids.
 *   adjacency       the caller of dory_graph_upload promises index arrays whose ghost ids are already in wire order: id N + r
 *                   names the r-th received row.  dory_partition_upload does this itself (dory_partition_wire_order,
 *                   dorylus_host.h: renumbered copies, the partition object is not modified) and needs the parts vector.
 *   recv_slots      dory_halo_plan's recv_slots no longer says where a received row is stored -- row r is stored at ghost row r
 *                   -- but names the caller-visible ghost index of that row: the reference's slot k of local id N + k
 *                   (srcGhostVtcs / dstGhostVtcs order).  It must still be a permutation of the ghost slots.
 *   ghost tensors   dory_tensor_upload, dory_tensor_download and dory_tensor_fill_uniform of fg, fgxw, fg_z, fg_el, fg_er (plan
 *                   of DORY_FORWARD) and bg, bgg, bg_d, bg_do, bg_st (DORY_BACKWARD) keep the caller-visible order: host row k
 *                   is the reference's ghost k, global_row_ids[k] its id.  The rows are permuted on the device on the way in
 *                   and out (a row kernel on the compute stream, not on the epoch's path), so they need that direction's plan
 *                   (DORY_ERR_ARG before it).  The raw device_ptr of dory_tensor_info points at WIRE-ordered rows.
 *   exchange        where the wire's width is the tensor's ld (always with halo_exact_rows = 0; with 1 for tensors whose cols
 *                   equal ld): RCCL -- ncclRecv targets the ghost tensor at recv_off[peer] * ld; host transport -- the
 *                   host-to-device copy of the received floats targets the ghost tensor; in-process transport -- the RECEIVER
 *                   pulls: once its peers' "sent" events are recorded it copies each peer's segment out of that peer's send
 *                   buffer into its own ghost tensor on its own comm stream and records "consumed", and a sender waits for the
 *                   "consumed" of the ranks that read its send buffer in the previous exchange before it packs the next one (the
 *                   same counters and events, waited for in the same place as the push form's; no host-side wait is added).
 *                   The multi-head GAT backward's "do" / "st" exchanges land the same way.
 *   exact rows      with halo_exact_rows = 1 a tensor with cols < ld cannot land (its rows are strided): such an exchange keeps
 *                   the receive buffer and the unpack kernels, which scatter by an identity list; results are unchanged.
 *   receive buffer  dory_halo_plan allocates none unless halo_exact_rows is 1 at that moment.  A later exchange that needs it
 *                   fails with DORY_ERR_ARG and says so (set halo_exact_rows = 1 before dory_halo_plan); nothing is allocated
 *                   and no device-wide synchronisation happens inside an epoch.
 *   split calls     dory_halo_unpack / dory_halo_unpack_tensor (the caller's buffer in plan order) copy row r to ghost row r at
 *                   the wire's width; dory_halo_pack* are unchanged.
 *   agreement       all ranks must use the same value.  The in-process transport checks it against every peer before anything
 *                   of the exchange is enqueued or counted (DORY_ERR_COMM, naming both ranks); over RCCL and over a host
 *                   transport it is the caller's contract, as for halo_exact_rows.
 *   numbers         K1 walks a row's edges in edge order: its sums are bit-identical with 0 and 1.  K1s and K1b spread source
 *                   rows over blocks by id; renumbered ghosts fall into other blocks, the order of additions inside a row
 *                   changes, and results hold to the parity criteria, not to the bits of option 0.
 * Values outside {0, 1} are rejected.  Read-only "halo_direct_recvs" / "halo_staged_recvs": the exchanges (eager calls and
 * recordings, one step per exchange) whose rows landed in the ghost tensor / went through the receive buffer and an unpack;
 * "halo_recv_buf_bytes": the bytes of that buffer.  The bf16 shadow rows, the kept neighbour sum of the GAT prototype, the
 * invalidation of a cached ah@0 and the timing families "halo", "halo_deferred", "halo_waited" behave as with 0.  Not executed:
 * the RCCL arm with more than one rank (two ranks cannot share one GPU under RCCL).  Measured on one GPU: DESIGN.md section 5,
 * profiles/r12_halo_direct_recv.txt. */

/* Epoch graph (MI355X-side addition, no reference counterpart): record the calls of one
 * epoch -- dory_aggregate / dory_apply_vertex / dory_apply_edge / dory_predict_gat /
 * dory_weight_update, exactly as Engine::runEpoch issues them -- into a hipGraph and replay
 * it, so a launch-bound epoch costs one graph launch.  Single partition only; one eager epoch
 * must have run before (lazy allocations).  Between begin and end the calls record instead of
 * executing; dory_epoch_graph_launch(n) replays n epochs (asynchronously: dory_sync waits) and
 * advances Adam's iteration count exactly as n eager epochs would (AdamOptimizer.cpp:29-34).
 * dory_engine_run does all of this itself when the option "epoch_graph" is 1. */
int dory_epoch_graph_begin(dory_ctx *ctx);
int dory_epoch_graph_end(dory_ctx *ctx);
int dory_epoch_graph_launch(dory_ctx *ctx, uint32_t epochs);
int dory_epoch_graph_drop(dory_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* DORYLUS_HIP_H */
