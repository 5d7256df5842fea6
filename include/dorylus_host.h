/*
 * dorylus_host.h -- C-ABI of the host-side pieces either side of the hot path:
 * the partition builder / graph.<id>.bin reader-writer (the data format the
 * kernels consume) and the synchronous-epoch Engine driver.  Same library as
 * dorylus_hip.h (libdorylus_hip.so).  Reference citations are relative to
 * src/graph-server/ of uclasystem/dorylus.
 */
#ifndef DORYLUS_HOST_H
#define DORYLUS_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "dorylus_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one partition of the graph on the host: every field of graph.<id>.bin ---- */
typedef struct dory_partition dory_partition;

/* DataLoader::preprocess (graph/dataloader.cpp:225-330) on in-memory edge records:
 * local ids ascend with global id, ghost ids are N + rank in ascending global id,
 * edges inside a column/row keep record order (duplicates kept, self loops dropped),
 * edge values (indeg(src)+1)^-1/2 (indeg(dst)+1)^-1/2 computed like
 * setEdgeNormalizations (:153-185), ghost degrees like findGhostDegrees (:192-218).
 * parts[v] = partition of global vertex v.  Index-identical to the reference. */
int dory_partition_build(const uint32_t *src, const uint32_t *dst, uint64_t num_records,
                         const int32_t *parts, uint32_t global_vtx_cnt, uint32_t node_id,
                         uint32_t num_nodes, int undirected, dory_partition **out);
/* same, reading <dataset_dir>graph.bsnap.edges and graph.bsnap.parts
 * (dataloader.cpp:8-10; dataset_dir ends with '/') */
int dory_partition_build_from_files(const char *dataset_dir, uint32_t node_id, uint32_t num_nodes,
                                    int undirected, dory_partition **out);
/* Graph::init (graph/graph.cpp:7-115) / RawGraph::dump (graph.cpp:200-273) */
int dory_partition_load(const char *graph_bin_path, dory_partition **out);
int dory_partition_save(const dory_partition *p, const char *graph_bin_path);
int dory_partition_free(dory_partition *p);
const char *dory_host_last_error(void);

struct dory_partition_view {
    uint32_t local_vtx_cnt, global_vtx_cnt, src_ghost_cnt, dst_ghost_cnt, num_nodes;
    uint64_t local_in_edge_cnt, local_out_edge_cnt, global_edge_cnt;
    const uint32_t *local_to_global; /* N */
    const float *norms;              /* N   vtxDataVec */
    const uint32_t *src_ghosts;      /* Gsrc global ids, ascending (local id = N + k) */
    const uint32_t *dst_ghosts;      /* Gdst */
    const uint32_t *fwd_counts;      /* num_nodes: forwardGhostsList sizes */
    const uint32_t *fwd_lists;       /* concatenated local ids */
    const uint32_t *bwd_counts;
    const uint32_t *bwd_lists;
    const uint64_t *column_ptrs;     /* N+1  forwardAdj  */
    const uint32_t *row_idxs;
    const float *csc_values;
    const uint64_t *row_ptrs;        /* N+1  backwardAdj */
    const uint32_t *column_idxs;
    const float *csr_values;
};
int dory_partition_get(const dory_partition *p, struct dory_partition_view *view);

/* receive side of the halo plan for direction dir (0 forward / 1 backward): for each
 * peer q, recv_counts[q] rows arrive (in the sender's list order) and land in ghost
 * slots recv_slots[off_q .. off_q + recv_counts[q]) -- the ghost slots owned by q in
 * ascending global id.  recv_counts has num_nodes entries, recv_slots src/dst_ghost_cnt. */
int dory_partition_recv_plan(const dory_partition *p, const int32_t *parts, int dir,
                             uint32_t *recv_counts, uint32_t *recv_slots);

/* Wire order of a partition's ghosts for direction dir (no GPU needed; option "halo_direct_recv" of dorylus_hip.h):
 * order[r] = the ghost slot k (local id N + k in the partition) of the r-th row that arrives -- peers in rank order, a peer's
 * rows in the order of its send list -- which is the list dory_partition_recv_plan emits; idxs = a copy of that direction's index
 * array (row_idxs for dir 0, column_idxs for dir 1) in which every ghost id N + k is replaced by N + r with order[r] == k, local
 * ids, edge order, values and pointers untouched.  order has src/dst_ghost_cnt entries, idxs local_in/out_edge_cnt.  The
 * partition itself is not modified (dory_partition_get and dory_partition_save keep giving the reference's numbering). */
int dory_partition_wire_order(const dory_partition *p, const int32_t *parts, int dir, uint32_t *order, uint32_t *idxs);

/* The inverse of a halo plan's send side (pure host code, no context, no device; nothing in the reference: an MI355X-side
 * addition for dory_halo_fused_pack of dorylus_hip.h).  send_counts (num_nodes entries) and send_lvids (all peers' lists
 * concatenated) are dory_halo_plan's: entry s of send_lvids is the local row that travels as row s -- "slot" s -- of the packed send
 * buffer.  Out: row_ptr (local_vtx_cnt + 1 entries) and row_slots (sum of the counts), a CSR of row -> slots: the slots of row r are
 * row_slots[row_ptr[r] .. row_ptr[r + 1]), ascending.  A row has one slot per peer that needs it (at most num_nodes - 1, maybe
 * none); a list that names a row twice gives it two.  Every slot appears exactly once.  DORY_ERR_ARG for an id >=
 * local_vtx_cnt. */
int dory_halo_send_map(uint32_t local_vtx_cnt, uint32_t num_nodes, const uint32_t *send_counts, const uint32_t *send_lvids,
                       uint32_t *row_ptr, uint32_t *row_slots);

/* The chunk plan of an adjacency's hub rows (pure host code, no context, no device; the plan dory_gatmh_row_gather_hub_split of
 * dorylus_hip.h builds for the row-gather kernels).  ptr: rows + 1 ascending offsets (column_ptrs or row_ptrs of a partition); an
 * entry of row v is one of ptr[v] .. ptr[v + 1] - 1.  A row with MORE than chunk_entries entries is a hub row: its entries, in order,
 * are cut into consecutive chunks of chunk_entries entries, the last one shorter; a row of exactly chunk_entries entries is not cut.
 * Out: *hub_rows_out, *chunks_out the counts; hub_rows (ascending), row_first_chunk (hub rows + 1 entries: the chunks of hub row i
 * are row_first_chunk[i] .. row_first_chunk[i + 1] - 1), and per chunk its row and its entries [chunk_e0, chunk_e1).  Every output may
 * be NULL: call once for the counts, once more with arrays of that size.  DORY_ERR_ARG: ptr NULL or not ascending, chunk_entries 0. */
int dory_row_chunk_plan(const uint64_t *ptr, uint32_t rows, uint32_t chunk_entries, uint32_t *hub_rows_out, uint32_t *chunks_out,
                        uint32_t *hub_rows, uint32_t *row_first_chunk, uint32_t *chunk_row, uint64_t *chunk_e0, uint64_t *chunk_e1);

/* The interior rows of a partition's adjacency (pure host code, no context, no device; the plan dory_gatmh_row_gather_overlap of
 * dorylus_hip.h builds for the row-gather kernels).  ptr as above, idx: the ptr[rows] entries, local ids -- an entry >= rows names a
 * ghost row.  A row is INTERIOR when every entry is < rows (a row without entries is: its only edge is the self edge) and BOUNDARY
 * when at least one is >= rows.  With column_ptrs / the in-edges this sorts destinations by their sources, with row_ptrs / the
 * out-edges sources by their destinations; the ids dory_partition_wire_order renumbers stay >= rows, so the lists do not depend on it.
 * Out: *interior_out, *boundary_out the counts (their sum is rows); interior_rows, boundary_rows ascending.  Every output may be NULL:
 * call once for the counts, once more with arrays of that size.  DORY_ERR_ARG: ptr NULL or not ascending, idx NULL with entries. */
int dory_row_interior_plan(const uint64_t *ptr, const uint32_t *idx, uint32_t rows, uint32_t *interior_out, uint32_t *boundary_out,
                           uint32_t *interior_rows, uint32_t *boundary_rows);

/* Every row's entries regrouped local ids first (pure host code, no context, no device; the copy dory_gatmh_row_gather_edge_split of
 * dorylus_hip.h builds per adjacency for the row-gather kernels).  ptr, idx as above; N: the ids < N are local, the ids >= N name ghost
 * rows (the partition's local vertex count; rows is that count too for a partition's adjacency).  Out: idx_out (ptr[rows] entries,
 * another array than idx) -- within every row the entries < N first, in their original order, then the entries >= N, in their original
 * order: a stable partition, so every row keeps its ids as a multiset; mid_out (rows entries) -- the position of the row's first ghost
 * entry, ptr[v + 1] where it has none.  ptr is not changed.  DORY_ERR_ARG: ptr NULL or not ascending, an array NULL that has entries,
 * idx_out == idx. */
int dory_row_edge_split_plan(const uint64_t *ptr, const uint32_t *idx, uint32_t rows, uint32_t N, uint32_t *idx_out, uint64_t *mid_out);

/* upload adjacency (dory_graph_upload) and, when parts is given, both halo plans
 * (dory_halo_plan): recv slots of peer q = ghost slots whose owner is q, ascending.  On a context with option
 * "halo_direct_recv" = 1 the index arrays uploaded are the renumbered copies of dory_partition_wire_order (parts is then
 * required for a partition with ghosts); the plans are the same lists. */
int dory_partition_upload(dory_ctx *ctx, const dory_partition *p, const int32_t *parts);

/* ---- input files of the reference graph server (engine/utils.cpp:460-596) ------------- */
/* run/<dataset>.config: one layer width per line */
int dory_read_layer_config(const char *path, uint32_t *dims, uint32_t max_dims, uint32_t *count);
/* features.bsnap {u32 F} + V x F floats -> rows of this partition's local vertices
 * (N x F) and source ghosts (Gsrc x F); cache_dir (may be NULL) enables the reference's
 * feats<F>.<node>.bin cache in the dataset directory */
int dory_read_features(const char *path, const dory_partition *p, uint32_t expect_dim, uint32_t node_id,
                       const char *cache_dir, float *local, float *ghost);
/* labels.bsnap {u32 kinds} + V x u32 -> class id per local vertex */
int dory_read_labels(const char *path, const dory_partition *p, uint32_t expect_kinds, uint32_t *labels);
const char *dory_formats_last_error(void);

/* ---- synchronous-epoch Engine (the reference's stage order, one chunk per
 * partition: engine/engine.cpp:223-314, ops/pipeline.cpp, resource_comm.cpp) ------ */
typedef struct dory_engine dory_engine;
int dory_engine_create(dory_ctx *ctx, dory_engine **out);
int dory_engine_destroy(dory_engine *e);
/* run `epochs` epochs back to back; per-epoch wall time (ms, host clock around a
 * stream sync, as pipeline.cpp:118-127 measures consecutive epoch starts) is
 * written to epoch_ms[epochs] when non-NULL. */
int dory_engine_run(dory_engine *e, uint32_t epochs, double *epoch_ms);
/* single stages with the reference's Chunk semantics (for tests / foreign drivers) */
struct dory_chunk { /* common/utils.hpp:64-75 */
    uint32_t localId, globalId, lowBound, upBound, layer;
    int32_t dir;
    uint32_t epoch;
    uint8_t vertex;
};
int dory_engine_nn_compute(dory_engine *e, struct dory_chunk *chunk);   /* ResourceComm::NNCompute */
int dory_engine_inc_layer(dory_engine *e, const struct dory_chunk *in, struct dory_chunk *out); /* incLayerGCN/GAT */
int dory_engine_is_last_layer(dory_engine *e, const struct dory_chunk *c);
/* The same state machine without an engine or a device (engine/utils.cpp:707-753): next chunk of `in`. */
int dory_chunk_inc_layer(int gnn_type, uint32_t num_layers, const struct dory_chunk *in, struct dory_chunk *out);
/* Dry run of one synchronous epoch: the stages Engine::runEpoch would issue, as space-separated names
 * "<stage><layer><F|B>" with stage GA (aggregate), AV (applyVertex -> NNCompute), AE (applyEdge), SC (scatter),
 * plus "WU<layer>" (weight update sent, CPU_comm.cpp:131,147,178) and "PR<layer>" (predictGAT); no device needed.
 * The order is the one a chunk takes through the reference's queues (ops/pipeline.cpp:170-342,
 * resource_comm.cpp:17-90). */
int dory_engine_trace_epoch(int gnn_type, uint32_t num_layers, char *buf, size_t buflen);
/* "<EM>: ..." style report of the last run into buf (engine/utils.cpp:219-291) */
int dory_engine_report(dory_engine *e, char *buf, size_t buflen);

/* Layout introspection (tests): the destination side of the K1s layout -- dorylus_amd/host/sweep_deal.cpp.  `items` rows
 * (sorted by descending edge count) are dealt over 8 XCDs x S sweeps x sweep_tiles workgroups x 32 lane groups x
 * rows_per_group positions; groups of the last sweep carry fewer rows so that every sweep is whole.  positions_out: total
 * positions; group_rows_out (positions / rows_per_group entries, may be NULL): rows of every group; item_position
 * (`items` entries, may be NULL): the position of item i.  0 = ok. */
int dory_sweep_deal(uint32_t items, uint32_t rows_per_group, uint32_t sweep_tiles, uint32_t *positions_out,
                    uint32_t *group_rows_out, uint32_t *item_position);
/* The layout of the 32-lane launches with a loader wave (csrc/spmm.hip, LOADER): lane groups 0 and 1 of every workgroup --
 * the wave that also copies the next step's entries for the other fifteen -- get `loader_relief` rows fewer per sweep
 * (proportionally fewer in a shorter last sweep; never so many that a sweep more would be needed: then less or none), and
 * the items (sorted by descending weight = edge count, `weights` given) are dealt by weight, each to the group with the
 * smallest load per row slot, so that every group carries edges in proportion to its rows whatever the degree
 * distribution.  Outputs as dory_sweep_deal. */
int dory_sweep_deal_weighted(uint32_t items, const uint64_t *weights, uint32_t rows_per_group, uint32_t sweep_tiles,
                             uint32_t loader_relief, uint32_t *positions_out, uint32_t *group_rows_out,
                             uint32_t *item_position);
/* Launch introspection (tests): the geometry of one launch on the sweep skeleton -- dorylus_amd/host/sweep_geometry.cpp.  The
 * launch walks `rows` rows per lane group (the actual count, never an option value: < 1 is refused) over `positions` positions
 * of a layout, on rows of ld floats with `group` (16 | 32) lanes per row (wide: 16 lanes of eight features, whatever group) and
 * `cus` workgroups per sweep and XCD.  out, 11 words: slabs, rows per XCD, workgroups per XCD and slab, sweeps per slab,
 * sweeps, workgroups, gate counter words per source block; [7] the counter words a launch over nblocks blocks clears, [8] the
 * bound callers size the counters by (any launch of this shape over nblocks blocks, whatever it leaves to concurrent kernels).
 * Separately, K1s's row rule: [9] the rows a launch of this lane-group width walks on a layout dealt for layout_rows rows per
 * group under option spmm_sweep_rows = rows_option, [10] whether its 16-lane row count has a wide form.  0 = ok. */
int dory_sweep_geometry(uint32_t positions, uint32_t ld, int group, int rows, int wide, uint32_t cus, uint32_t nblocks,
                        uint32_t layout_rows, int rows_option, uint64_t *out);
/* Option introspection (tests, tools; no context needed): the table of the keys of dory_set_option / dory_get_option --
 * dorylus_amd/host/options.cpp, dorylus_amd/csrc/options.hpp.  dory_option_spec: record `index` (0, 1, ... until DORY_ERR_ARG;
 * options first, then the read-only keys, then the action "spmm_gates_rearm"); any pointer may be NULL.  kind: 0 option, 1
 * read-only, 2 action.  def: the value dory_create gives an option.  lo..hi: the accepted values (lo > hi: any int64_t).
 * gnn: -1, or the dory_gnn a nonzero value needs.  fixed_by_graph: refused once a graph is uploaded.  read: when the library
 * reads it -- 0 every call, 1 dory_graph_upload, 2 dory_preallocate (and the calls after it), 3 when a blocked / sweep layout
 * is built (dory_preallocate or the first aggregation that needs one), 4 dory_engine_run. */
int dory_option_spec(uint32_t index, const char **name, int *kind, int64_t *def, int64_t *lo, int64_t *hi, int *gnn,
                     int *fixed_by_graph, int *read);
/* What dory_set_option(name, value) answers on a context of model gnn that is / is not configured and has / has no graph:
 * DORY_OK, or DORY_ERR_ARG and the refusal in msg (n bytes).  "spmm_sweep_cus" is the exception: its range, 0..CUs per XCD, is
 * the device's and only the context checks it. */
int dory_option_check(const char *name, int64_t value, int gnn, int configured, int has_graph, char *msg, size_t n);
/* Switch introspection (tests, tools; no context needed): the table of the feature switches dory_<name>(ctx, int) of dorylus_hip.h --
 * dorylus_amd/host/switches.cpp, dorylus_amd/csrc/switches.hpp.  dory_switch_spec: record `index` (0, 1, ... until DORY_ERR_ARG); any pointer
 * may be NULL.  hi: the values are 0..hi.  refusals: how many its setter has.  waits_halo / drops_stamp: what a set does first.  parent: -1, or the
 * index of the switch it lives on top of.  counters: the values dory_<name>_stats reports.  dory_switch_check: what dory_<name>(ctx, value) answers on a
 * context of model gnn in that state -- DORY_OK, or DORY_ERR_ARG and in msg (n bytes) its setter's first refusal (a hook's refusal only a context knows). */
int dory_switch_spec(uint32_t index, const char **name, int *hi, int *refusals, int *waits_halo, int *drops_stamp, int *parent, int *counters);
int dory_switch_check(const char *name, int value, int gnn, int configured, int prealloc, int recording, int parent_on, char *msg, size_t n);
/* Shape introspection (tests, tools; no context or device needed): the wide bf16 form of the multi-head GAT's row-gather kernels
 * (dory_gatmh_row_gather_bf16_wide, dorylus_hip.h) -- dorylus_amd/host/gatmh_rows_wide.cpp, csrc/gat_mh_shapes.hpp.  Returns 1 where a
 * pass over K heads of D features on rows of ld floats takes the wide form: the family covers the shape (K*D <= ld <= 256, ld a
 * multiple of 4, a head shape of the model), 64 <= ld and ld a multiple of 8, and K == 1 or D % 8 == 0; else 0 (the narrow form runs).
 * Then lanes_per_row: 8 / 16 / 32 for ld / 8 <= 8, <= 16, more; lanes_per_head: the lanes a head's dot products are reduced over (the
 * row's lanes for K == 1, else D / 8); scores_from_row: 1 where the sources' scores are formed from the gathered row (ld / 4 a power of
 * two), 0 where el / fg_el are gathered.  Any pointer may be NULL; where 0 is returned the outputs are 0. */
int dory_gatmh_row_gather_bf16_wide_form(uint32_t K, uint32_t D, uint32_t ld, uint32_t *lanes_per_row, uint32_t *lanes_per_head,
                                         int *scores_from_row);

#ifdef __cplusplus
}
#endif
#endif /* DORYLUS_HOST_H */
