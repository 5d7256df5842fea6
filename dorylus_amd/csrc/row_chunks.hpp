// row_chunks.hpp -- rows of an adjacency cut into chunks of consecutive entries (pure host code: dorylus_amd/host/row_chunks.cpp).
// The plan record is K1's (LongRowsHost; spmm.hip's plan_long_rows fills it for the part of a row beyond LONG_ROW_CLAMP edges, in chunks
// of LONG_ROW_CHUNK); plan_row_chunks is the general rule -- which rows, from which entry on, in chunks of what size -- and serves the hub
// rows of the multi-head GAT's row-gather family (gat_mh_rows.hip, dory_gatmh_row_gather_hub_split: the whole row, the caller's size).
#pragma once
#include <cstdint>
#include <vector>

namespace dory {

struct LongRowsHost {                    // plan_long_rows / plan_row_chunks output
    std::vector<uint32_t> rows;          // the rows that are cut, ascending
    std::vector<uint32_t> row_chunk_ptr; // rows+1: first chunk of each
    std::vector<uint32_t> chunks;        // 6 words per chunk: row, flag, e0 (lo, hi), e1 (lo, hi); flag: plan_long_rows 0, plan_row_chunks
};                                       // 1 on the row's last chunk (else 0)
// Rows with more than `over` entries (entries = ptr[v + 1] - ptr[v]) are cut: their entries from the `skip`-th on, in order, into
// consecutive chunks of `chunk` entries, the last one shorter.  A row of exactly `over` entries is not cut.  chunk >= 1, skip <= over.
void plan_row_chunks(const uint64_t *ptr, uint32_t N, uint64_t over, uint64_t skip, uint64_t chunk, LongRowsHost *out);

// The rows of a partition's adjacency by what they read (dory_gatmh_row_gather_overlap; the C entry point: dory_row_interior_plan).  An
// entry >= N names a ghost row.  interior: every entry of the row is < N -- a row without entries too (its only edge is the self edge);
// boundary: at least one entry is >= N.  Both ascending; together they are [0, N).  The in-edge adjacency sorts destinations by their
// sources, the out-edge adjacency sources by their destinations; option halo_direct_recv renumbers the ghosts among themselves, so it
// changes neither list.
void plan_row_interior(const uint64_t *ptr, const uint32_t *idx, uint32_t N, std::vector<uint32_t> *interior, std::vector<uint32_t> *boundary);

// Every row's entries regrouped local-first (dory_gatmh_row_gather_edge_split; the C entry point: dory_row_edge_split_plan): within
// [ptr[v], ptr[v + 1]) of idx_out the entries < N come first, in their original order, the entries >= N follow, in their original order
// (a stable partition; ptr is unchanged, only ids move -- the multi-head GAT's adjacencies carry no per-edge values).  mid_out[v]: the
// position of the row's first entry >= N, ptr[v + 1] where it has none.  idx_out: as many entries as idx, another array.
void plan_row_edge_split(const uint64_t *ptr, const uint32_t *idx, uint32_t rows, uint32_t N, uint32_t *idx_out, uint64_t *mid_out);

}  // namespace dory
