// row_chunks.cpp -- plan_row_chunks (csrc/row_chunks.hpp) and its C entry point dory_row_chunk_plan (include/dorylus_host.h): the
// chunk plan of an adjacency's long rows, on the host, without a context or a device.  Likewise plan_row_interior /
// dory_row_interior_plan: the rows that read no ghost row, and the others; plan_row_edge_split / dory_row_edge_split_plan: every
// row's entries regrouped local ids first.
#include "../csrc/row_chunks.hpp"

#include "../../include/dorylus_host.h"

namespace dory {

void plan_row_chunks(const uint64_t *ptr, uint32_t N, uint64_t over, uint64_t skip, uint64_t chunk, LongRowsHost *out) {
    out->rows.clear(); out->row_chunk_ptr.assign(1, 0); out->chunks.clear();
    for (uint32_t v = 0; v < N; ++v) {
        const uint64_t beg = ptr[v], end = ptr[v + 1];
        if (end - beg <= over) continue;
        out->rows.push_back(v);
        for (uint64_t e = beg + skip; e < end; e += chunk) {
            const uint64_t e1 = end - e > chunk ? e + chunk : end;
            out->chunks.push_back(v);                                  // row
            out->chunks.push_back(e1 == end ? 1u : 0u);                // the row's last chunk
            out->chunks.push_back((uint32_t)(e & 0xFFFFFFFFu)); out->chunks.push_back((uint32_t)(e >> 32));
            out->chunks.push_back((uint32_t)(e1 & 0xFFFFFFFFu)); out->chunks.push_back((uint32_t)(e1 >> 32));
        }
        out->row_chunk_ptr.push_back((uint32_t)(out->chunks.size() / 6));
    }
}

void plan_row_interior(const uint64_t *ptr, const uint32_t *idx, uint32_t N, std::vector<uint32_t> *interior, std::vector<uint32_t> *boundary) {
    interior->clear(); boundary->clear();
    for (uint32_t v = 0; v < N; ++v) {
        bool ghost = false;
        for (uint64_t e = ptr[v]; e < ptr[v + 1] && !ghost; ++e) ghost = idx[e] >= N;
        (ghost ? boundary : interior)->push_back(v);
    }
}

void plan_row_edge_split(const uint64_t *ptr, const uint32_t *idx, uint32_t rows, uint32_t N, uint32_t *idx_out, uint64_t *mid_out) {
    for (uint32_t v = 0; v < rows; ++v) {
        uint64_t w = ptr[v];
        for (uint64_t e = ptr[v]; e < ptr[v + 1]; ++e)
            if (idx[e] < N) idx_out[w++] = idx[e];
        mid_out[v] = w;
        for (uint64_t e = ptr[v]; e < ptr[v + 1]; ++e)
            if (idx[e] >= N) idx_out[w++] = idx[e];
    }
}

}  // namespace dory

extern "C" int dory_row_edge_split_plan(const uint64_t *ptr, const uint32_t *idx, uint32_t rows, uint32_t N, uint32_t *idx_out,
                                        uint64_t *mid_out) {
    if (!ptr) return DORY_ERR_ARG;
    for (uint32_t v = 0; v < rows; ++v)
        if (ptr[v] > ptr[v + 1]) return DORY_ERR_ARG;
    const bool entries = rows && ptr[rows] > ptr[0];
    if (entries && (!idx || !idx_out || idx == idx_out)) return DORY_ERR_ARG;
    if (rows && !mid_out) return DORY_ERR_ARG;
    dory::plan_row_edge_split(ptr, idx, rows, N, idx_out, mid_out);
    return DORY_OK;
}

extern "C" int dory_row_interior_plan(const uint64_t *ptr, const uint32_t *idx, uint32_t rows, uint32_t *interior_out, uint32_t *boundary_out,
                                      uint32_t *interior_rows, uint32_t *boundary_rows) {
    if (!ptr) return DORY_ERR_ARG;
    for (uint32_t v = 0; v < rows; ++v)
        if (ptr[v] > ptr[v + 1]) return DORY_ERR_ARG;
    if (!idx && rows && ptr[rows] > ptr[0]) return DORY_ERR_ARG;
    std::vector<uint32_t> in, bd;
    dory::plan_row_interior(ptr, idx, rows, &in, &bd);
    if (interior_out) *interior_out = (uint32_t)in.size();
    if (boundary_out) *boundary_out = (uint32_t)bd.size();
    for (size_t i = 0; i < in.size() && interior_rows; ++i) interior_rows[i] = in[i];
    for (size_t i = 0; i < bd.size() && boundary_rows; ++i) boundary_rows[i] = bd[i];
    return DORY_OK;
}

extern "C" int dory_row_chunk_plan(const uint64_t *ptr, uint32_t rows, uint32_t chunk_entries, uint32_t *hub_rows_out, uint32_t *chunks_out,
                                   uint32_t *hub_rows, uint32_t *row_first_chunk, uint32_t *chunk_row, uint64_t *chunk_e0,
                                   uint64_t *chunk_e1) {
    if (!ptr || chunk_entries == 0) return DORY_ERR_ARG;
    for (uint32_t v = 0; v < rows; ++v)
        if (ptr[v] > ptr[v + 1]) return DORY_ERR_ARG;
    dory::LongRowsHost h;
    dory::plan_row_chunks(ptr, rows, chunk_entries, 0, chunk_entries, &h);
    const size_t nr = h.rows.size(), nc = h.chunks.size() / 6;
    if (hub_rows_out) *hub_rows_out = (uint32_t)nr;
    if (chunks_out) *chunks_out = (uint32_t)nc;
    for (size_t i = 0; i < nr && hub_rows; ++i) hub_rows[i] = h.rows[i];
    for (size_t i = 0; i <= nr && row_first_chunk; ++i) row_first_chunk[i] = h.row_chunk_ptr[i];
    for (size_t i = 0; i < nc; ++i) {
        const uint32_t *w = &h.chunks[6 * i];
        if (chunk_row) chunk_row[i] = w[0];
        if (chunk_e0) chunk_e0[i] = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
        if (chunk_e1) chunk_e1[i] = (uint64_t)w[4] | ((uint64_t)w[5] << 32);
    }
    return DORY_OK;
}
