// abi_context.hip -- C-ABI, part 1 (include/dorylus_hip.h): context, device tensor table, graph / tensor /
// weight uploads, options and timing.  The stage dispatch is in abi_stages.hip, the exchange and the weight update
// in abi_comm.hip.  Reference paths are relative to src/graph-server/ unless they start with src/.
#include "abi_internal.hpp"

namespace dory {

static std::string g_create_err;

int fail(dory_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

void drain_timing(dory_ctx *c) {
    const dory_ctx::Pending *halo = nullptr;   // the last deferred exchange seen: the next "spmm_beside_halo" ran beside it
    for (auto &p : c->pending) {
        (void)hipEventSynchronize(p.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->times[p.fam].total_ms += ms;
            c->times[p.fam].launches += 1;
        }
        if (p.fam == "halo_deferred") halo = &p;
        if (p.fam == "spmm_beside_halo" && halo) {
            // both intervals on the clock of the exchange's first event: [0, he] and [ss, se]
            float he = 0.f, ss = 0.f, se = 0.f;
            if (hipEventElapsedTime(&he, halo->a, halo->b) == hipSuccess && hipEventElapsedTime(&ss, halo->a, p.a) == hipSuccess &&
                hipEventElapsedTime(&se, halo->a, p.b) == hipSuccess) {
                const float hidden = std::max(0.f, std::min(he, se) - std::max(0.f, ss));
                c->times["halo_hidden"].total_ms += hidden;
                c->times["halo_hidden"].launches += 1;
            }
            halo = nullptr;
        }
    }
    for (auto &p : c->pending) c->ev_pool.push_back({p.a, p.b});
    c->pending.clear();
}

int alloc_tensor(dory_ctx *c, Tensor &t, uint64_t rows, uint32_t cols) {
    t.rows = rows;
    t.cols = cols;
    t.ld = pad_ld(cols);
    t.owned = true;
    t.d = nullptr;
    size_t b = t.bytes();
    if (b == 0) b = 256;  // keep a valid pointer for empty ghosts
    HIPCK(c, hipMalloc((void **)&t.d, b));
    HIPCK(c, hipMemsetAsync(t.d, 0, b, c->compute));
    return DORY_OK;
}

Tensor *find(dory_ctx *c, uint32_t layer, const char *name) {
    if (layer >= c->tensors.size()) return nullptr;
    auto it = c->tensors[layer].find(name);
    return it == c->tensors[layer].end() ? nullptr : &it->second;
}
Tensor *findw(std::vector<std::map<std::string, Tensor>> &tab, uint32_t layer, const char *name) {
    if (layer >= tab.size()) return nullptr;
    auto it = tab[layer].find(name);
    return it == tab[layer].end() ? nullptr : &it->second;
}

void free_table(std::vector<std::map<std::string, Tensor>> &tab) {
    for (auto &m : tab)
        for (auto &kv : m) {
            if (kv.second.owned && kv.second.d) (void)hipFree(kv.second.d);
            if (kv.second.twin) (void)hipFree(kv.second.twin);   // (dory_halo_bf16_ghosts: the bf16 twin of a ghost tensor)
        }
    tab.clear();
}

int ensure_scratch(dory_ctx *c, size_t bytes) {
    if (bytes <= c->scratch_bytes) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: scratch would have to grow while recording (run one eager epoch first)");
    if (c->scratch) {
        HIPCK(c, hipStreamSynchronize(c->compute));
        (void)hipFree(c->scratch);
        c->scratch = nullptr;
        c->scratch_bytes = 0;
    }
    HIPCK(c, hipMalloc((void **)&c->scratch, bytes));
    c->scratch_bytes = bytes;
    return DORY_OK;
}

int ensure_partial(dory_ctx *c, size_t bytes, const char *what) {
    if (bytes <= c->partial_bytes) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: %s would have to grow while recording", what);
    HIPCK(c, hipStreamSynchronize(c->compute));
    if (c->partial) (void)hipFree(c->partial);
    c->partial = nullptr;
    c->partial_bytes = 0;
    HIPCK(c, hipMalloc((void **)&c->partial, bytes));
    c->partial_bytes = bytes;
    return DORY_OK;
}

// longest-row-first schedule for skewed degree distributions
std::vector<uint32_t> degree_order(const uint64_t *ptr, uint32_t N) {
    std::vector<uint32_t> o(N);
    std::iota(o.begin(), o.end(), 0u);
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) {
        return (ptr[a + 1] - ptr[a]) > (ptr[b + 1] - ptr[b]);
    });
    return o;
}

// rows in the order of their MEDIAN source id (option spmm_order = 3, round 6 experiment): waves that run at the same time then
// read source rows from the same neighbourhood of the [local ; ghost] row space -- if the graph has one.  Per-row results are
// bit-identical whatever the schedule.
std::vector<uint32_t> median_source_order(const uint64_t *ptr, const uint32_t *idx, uint32_t N) {
    std::vector<uint32_t> med(N), o(N), tmp;
    for (uint32_t v = 0; v < N; ++v) {
        const uint64_t e0 = ptr[v], e1 = ptr[v + 1];
        if (e0 == e1) { med[v] = 0xFFFFFFFFu; continue; }
        tmp.assign(idx + e0, idx + e1);
        std::nth_element(tmp.begin(), tmp.begin() + (tmp.size() / 2), tmp.end());
        med[v] = tmp[tmp.size() / 2];
    }
    std::iota(o.begin(), o.end(), 0u);
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return med[a] < med[b]; });
    return o;
}

int gemm(dory_ctx *c, int ta, int tb, uint32_t M, uint32_t N, uint32_t K, const Tensor &A,
         const Tensor &B, Tensor &C, Tensor *C2) {
    GemmArgs g{};
    g.ta = ta; g.tb = tb; g.M = M; g.N = N; g.K = K;
    g.A = A.d; g.lda = A.ld; g.B = B.d; g.ldb = B.ld; g.C = C.d; g.ldc = C.ld;
    g.epilogue = C2 ? EPI_TANH : EPI_NONE;
    if (C2) { g.C2 = C2->d; g.ldc2 = C2->ld; }
    size_t need = gemm_scratch_bytes(M, N, K);
    if (need > ((size_t)256 << 20)) need = (size_t)256 << 20;
    int rc = ensure_scratch(c, need);
    if (rc) return rc;
    // the fused halo pack: a product that is the source of an exchange also goes into the send buffer -- once the previous
    // exchange has finished reading it (dory_apply_vertex has waited already; a producer reached by another route waits here)
    GemmSend sd{};
    int send_dir = 0;
    const Tensor *sent = nullptr;
    if (sw_on(c, SW_HALO_FUSED_PACK) && ta == 0) {
        if (C2 && fused_pack_target(c, C2, M, &sd, &send_dir)) { sent = C2; sd.which = 1; }
        else if (fused_pack_target(c, &C, M, &sd, &send_dir)) { sent = &C; sd.which = 0; }
    }
    if (sent && (rc = wait_halo(c))) return rc;
    ghost_wrote_fp32(&C);   // (dory_halo_bf16_ghosts: a product written into a ghost tensor -- fgxw@0 -- is fp32 rows)
    ghost_wrote_fp32(C2);
    Timed t(c, "gemm", c->compute);
    if (!sent) {
        fused_note_write(c, &C);
        fused_note_write(c, C2);
        HIPCK(c, launch_gemm(g, c->scratch, c->scratch_bytes, c->compute));
        return DORY_OK;
    }
    sd.cols = N;
    bool fused = false;
    HIPCK(c, launch_gemm_send(g, sd, c->scratch, c->scratch_bytes, c->compute, &fused));
    if (fused) fused_pack_stamp(c, sent, send_dir, sd);
    else if (c->fused_stamp.src == sent) fused_stamp_drop(c);   // (rewritten without its rows in the buffer: K == 0)
    return DORY_OK;
}

int gat_materialize(dory_ctx *c, uint32_t layer, int which) {
    if (c->gnn != DORY_GAT || !c->prealloc) return DORY_OK;
    if ((which & 1) && layer < c->gat_az_stale.size() && c->gat_az_stale[layer]) {
        Tensor *az = find(c, layer, "az"), *azrow = find(c, layer, "azrow");
        if (az && azrow) HIPCK(c, launch_expand_rows_to_edges(c->N, c->adj[ADJ_IN].ptr, azrow->d, az->d, c->compute));
        c->gat_az_stale[layer] = 0;
    }
    if ((which & 2) && c->gat_A_stale_layer >= 0) {
        Tensor *arow = find(c, (uint32_t)c->gat_A_stale_layer, "arow");
        if (arow) HIPCK(c, launch_expand_rows_to_edges(c->N, c->adj[ADJ_IN].ptr, arow->d, c->adj[ADJ_IN].val, c->compute));
        c->gat_A_stale_layer = -1;
    }
    if ((which & 4) && layer < c->gat_dA_stale.size() && c->gat_dA_stale[layer]) {
        Tensor *dA = find(c, layer, "dA"), *drow = find(c, layer, "drow");
        if (dA && drow) HIPCK(c, launch_expand_rows_to_edges(c->N, c->adj[ADJ_IN].ptr, drow->d, dA->d, c->compute));
        c->gat_dA_stale[layer] = 0;
    }
    return DORY_OK;
}
static int gat_edge_tensor_hook(dory_ctx *c, uint32_t layer, const char *name, bool overwrite) {
    if (c->gnn != DORY_GAT || !name) return DORY_OK;
    const int which = !strcmp(name, "az") ? 1 : !strcmp(name, "A") ? 2 : !strcmp(name, "dA") ? 4 : 0;
    if (!which) return DORY_OK;
    if (!overwrite) return gat_materialize(c, layer, which);
    // the caller's values replace the tensor: nothing of ours is pending any more, and the per-vertex copy no longer describes it
    if (which == 1 && layer < c->gat_az_stale.size()) { c->gat_az_stale[layer] = 0; c->gat_azrow_valid[layer] = 0; }
    if (which == 2) c->gat_A_stale_layer = -1;
    if (which == 4 && layer < c->gat_dA_stale.size()) c->gat_dA_stale[layer] = 0;
    return DORY_OK;
}

// Transform-first order for a GCN layer (opt-in, no reference counterpart): when a layer's input is wider than its
// output, z_l = A (in_l W_l) gathers d[l+1]-wide rows instead of the d[l]-wide rows of (A in_l) W_l -- 128 instead of
// 602 floats per edge on Reddit's layer 0, 41 instead of 128 on layer 1.  Backward: u_l = A^T g_l (d[l+1] wide),
// dW_l = in_l^T u_l, and the gradient handed down is u_l W_l^T (= A^T (g_l W_l^T), the reference's aTg).  "ah"@l is
// not produced for such a layer.  Option gcn_transform_first: 1 = layer 0 only, 2 = every layer that narrows.
bool tf_layer(dory_ctx *c, uint32_t layer) {
    const int64_t mode = c->opt[OPT_GCN_TRANSFORM_FIRST];
    if (c->gnn != DORY_GCN || c->L < 2 || layer >= c->L || mode == 0 || c->opt[OPT_ADJACENCY_VALUES_ASYMMETRIC] != 0) return false;
    if (mode == 1 && layer != 0) return false;
    return c->dims[layer] > c->dims[layer + 1];
}
bool tf_active(dory_ctx *c) { return tf_layer(c, 0); }

// dory_gatmh_row_gather_hub_split: the plan of one adjacency for the context's chunk size: built from the pointer array (read back from the device: the host copy is
// the caller's), cached in the adjacency, dropped with it (free_graph) or when the chunk size changes
int hub_plan_ensure(dory_ctx *c, Adjacency &A) {
    if (A.hub_chunk == c->gatmh_hub_chunk) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: the hub rows' chunk plan would have to be built while recording (run one eager epoch first)");
    LongRowsDev &L = A.hub_rows;
    if (L.rows || L.row_chunk_ptr || L.chunks) HIPCK(c, hipDeviceSynchronize());   // (a launch in flight may still read the old plan)
    for (void *p : {(void *)L.rows, (void *)L.row_chunk_ptr, (void *)L.chunks})
        if (p) (void)hipFree(p);
    L = LongRowsDev{};
    A.hub_chunk = 0;
    if (!c->gatmh_hub_chunk || !c->has_graph) return DORY_OK;
    std::vector<uint64_t> ptr((size_t)c->N + 1);
    HIPCK(c, hipMemcpy(ptr.data(), A.ptr, ptr.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    LongRowsHost h;
    plan_row_chunks(ptr.data(), c->N, c->gatmh_hub_chunk, 0, c->gatmh_hub_chunk, &h);
    int rc;
    if (!h.rows.empty()) {
        if ((rc = upload_array(c, &L.rows, h.rows.data(), h.rows.size()))) return rc;
        if ((rc = upload_array(c, &L.row_chunk_ptr, h.row_chunk_ptr.data(), h.row_chunk_ptr.size()))) return rc;
        if ((rc = upload_array(c, &L.chunks, h.chunks.data(), h.chunks.size()))) return rc;
    }
    L.nrows = (uint32_t)h.rows.size();
    L.nchunks = (uint32_t)(h.chunks.size() / 6);
    A.hub_chunk = c->gatmh_hub_chunk;
    return DORY_OK;
}

// dory_gatmh_row_gather_overlap: the rows of one adjacency in launch order -- plan_row_interior's interior rows that the hub plan of the
// context's chunk size does not cut (a row that is cut goes whole to the launch after the wait, with its chunks and the merge), then all
// other rows.  Built from the pointer and index arrays (read back from the device, as hub_plan_ensure does), cached in the adjacency,
// dropped with it (free_graph) and rebuilt when the chunk size changes
int interior_plan_ensure(dory_ctx *c, Adjacency &A) {
    if (A.rows_split_built && A.rows_hub_chunk == c->gatmh_hub_chunk) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: the interior rows' plan would have to be built while recording (run one eager epoch first)");
    if (A.rows_split) {
        HIPCK(c, hipDeviceSynchronize());   // (a launch in flight may still read the old list)
        (void)hipFree(A.rows_split);
        A.rows_split = nullptr;
    }
    A.rows_split_built = false;
    A.rows_first = A.rows_interior = 0;
    if (!c->has_graph) return DORY_OK;
    std::vector<uint64_t> ptr((size_t)c->N + 1, 0);
    std::vector<uint32_t> idx((size_t)A.nnz), in, bd, order;
    if (A.ptr) HIPCK(c, hipMemcpy(ptr.data(), A.ptr, ptr.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (A.nnz) HIPCK(c, hipMemcpy(idx.data(), A.idx, idx.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ptr[c->N] > A.nnz) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_overlap: the adjacency's pointers run past its %llu entries", (unsigned long long)A.nnz);
    plan_row_interior(ptr.data(), idx.data(), c->N, &in, &bd);
    A.rows_interior = (uint32_t)in.size();
    const uint64_t chunk = c->gatmh_hub_chunk;
    std::vector<uint32_t> rest;
    for (uint32_t v : in) (chunk && ptr[v + 1] - ptr[v] > chunk ? rest : order).push_back(v);   // (plan_row_chunks' rule: more than `chunk` entries)
    A.rows_first = (uint32_t)order.size();
    order.resize((size_t)c->N);
    std::merge(rest.begin(), rest.end(), bd.begin(), bd.end(), order.begin() + A.rows_first);
    if (c->N) { int rc = upload_array(c, &A.rows_split, order.data(), order.size()); if (rc) return rc; }
    A.rows_hub_chunk = c->gatmh_hub_chunk;
    A.rows_split_built = true;
    return DORY_OK;
}

// dory_gatmh_row_gather_edge_split: the local-first copy of one adjacency (RowsEdgeSplit) -- plan_row_edge_split over the pointer and
// index arrays as they were uploaded (read back from the device, as interior_plan_ensure does: under halo_direct_recv these are the
// renumbered ids), and the rows that have a ghost entry.  Cached in the adjacency, dropped with it (free_graph)
int rows_edge_ensure(dory_ctx *c, Adjacency &A) {
    if (A.rows_edge.built) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: the local-first copy of the edges would have to be built while recording (run one eager epoch first)");
    if (!c->has_graph) return DORY_OK;
    std::vector<uint64_t> ptr((size_t)c->N + 1, 0), mid((size_t)c->N);
    std::vector<uint32_t> idx((size_t)A.nnz), lf((size_t)A.nnz), brows;
    if (A.ptr) HIPCK(c, hipMemcpy(ptr.data(), A.ptr, ptr.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (A.nnz) HIPCK(c, hipMemcpy(idx.data(), A.idx, idx.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ptr[c->N] > A.nnz) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_edge_split: the adjacency's pointers run past its %llu entries", (unsigned long long)A.nnz);
    for (uint32_t v = 0; v < c->N; ++v)
        if (ptr[v] > ptr[v + 1]) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_edge_split: the adjacency's pointers do not ascend at row %u", v);
    plan_row_edge_split(ptr.data(), idx.data(), c->N, c->N, lf.data(), mid.data());
    RowsEdgeSplit &R = A.rows_edge;
    R.local = 0;
    for (uint32_t v = 0; v < c->N; ++v) {
        R.local += mid[v] - ptr[v];
        if (mid[v] < ptr[v + 1]) brows.push_back(v);
    }
    int rc;
    if (A.nnz && (rc = upload_array(c, &R.idx, lf.data(), lf.size()))) return rc;
    if (c->N && (rc = upload_array(c, &R.mid, mid.data(), mid.size()))) return rc;
    if (!brows.empty() && (rc = upload_array(c, &R.brows, brows.data(), brows.size()))) return rc;
    R.nbrows = (uint32_t)brows.size();
    R.built = true;
    return DORY_OK;
}
// ... and the buffer the rows' states wait in between the two launches of a pass: only ever grows, never while recording
int carry_state_ensure(dory_ctx *c, size_t bytes) {
    if (bytes <= c->gatmh_carry_bytes) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: the row states of gatmh_row_gather_edge_split would have to grow while recording (run one eager epoch first)");
    if (c->gatmh_carry_state) {
        HIPCK(c, hipStreamSynchronize(c->compute));
        (void)hipFree(c->gatmh_carry_state);
        c->gatmh_carry_state = nullptr;
        c->gatmh_carry_bytes = 0;
        epoch_graph_drop_locked(c);   // (a recorded epoch would write the freed buffer)
    }
    HIPCK(c, hipMalloc((void **)&c->gatmh_carry_state, bytes));
    c->gatmh_carry_bytes = bytes;
    return DORY_OK;
}

}  // namespace dory

using namespace dory;

extern "C" {

// ---------------------------------------------------------------------------------------
int dory_create(int device, dory_ctx **out) {
    if (!out) return DORY_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(nullptr, DORY_ERR_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(nullptr, DORY_ERR_ARG, "device %d out of range (%d)", device, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(nullptr, DORY_ERR_HIP, "hipGetDeviceProperties failed");
    if (!strstr(prop.gcnArchName, "gfx950"))
        return fail(nullptr, DORY_ERR_NODEVICE, "device %d is %s; kernels are built for gfx950 only", device,
                    prop.gcnArchName);
    dory_ctx *c = new dory_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->comm, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_a, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_b, hipEventDisableTiming) != hipSuccess ||
        hipMalloc((void **)&c->d_stat, 2 * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&c->sweep_stat, SWEEP_STAT_WORDS * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void **)&c->d_stat3, 256) != hipSuccess) {
        delete c;
        return fail(nullptr, DORY_ERR_HIP, "stream/event creation failed");
    }
    (void)hipMemset(c->d_stat, 0, 2 * sizeof(float));
    (void)hipMemset(c->sweep_stat, 0, SWEEP_STAT_WORDS * sizeof(uint32_t));
    c->own_compute = c->own_comm = true;
    for (int i = 0; i < OPT_COUNT; ++i) c->opt[i] = option_spec(i)->def;   // every option at the table's default (host/options.cpp)
    c->gcn_bf16_mode.store((int)c->opt[OPT_GCN_BF16_GATHER], std::memory_order_release);
    c->cus_per_xcd = (uint32_t)std::max(1, prop.multiProcessorCount / 8);
    {   // K1s's placement assumption (ctx.hpp): workgroup id & 7 = XCD, eight XCDs
        const uint32_t PG = 2048;
        uint32_t *dx = nullptr;
        std::vector<uint32_t> hx(PG, 0xFFu);
        if (hipMalloc((void **)&dx, PG * sizeof(uint32_t)) == hipSuccess) {
            bool ran = launch_xcd_probe(dx, PG, c->compute) == hipSuccess && hipStreamSynchronize(c->compute) == hipSuccess &&
                       hipMemcpy(hx.data(), dx, PG * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
            (void)hipFree(dx);
            // what K1s needs: workgroups with the same id & 7 share an XCD, the eight residues sit on eight different XCDs
            // (the dispatcher's round robin may start anywhere: the residue -> XCD map is a rotation, not the identity)
            uint32_t seen = 0, match = 0;
            for (uint32_t i = 0; i < PG; ++i) { if (hx[i] < 16) seen |= 1u << hx[i]; match += hx[i] == hx[i & 7u]; }
            uint32_t firsts = 0;
            for (uint32_t r = 0; r < 8; ++r) if (hx[r] < 16) firsts |= 1u << hx[r];
            c->xcd_count = (uint32_t)__builtin_popcount(seen);
            c->xcd_mapping_ok = ran && match == PG && c->xcd_count == 8 && __builtin_popcount(firsts) == 8;
        } else {
            c->xcd_mapping_ok = false;
        }
    }
    *out = c;
    return DORY_OK;
}

static void free_graph(dory_ctx *c) {
    if (c->norm) (void)hipFree(c->norm);
    c->norm = nullptr;
    for (Adjacency &A : c->adj) {
        for (void *p : {(void *)A.ptr, (void *)A.idx, (void *)A.val, (void *)A.order, (void *)A.split, (void *)A.edge_split.idx,
                        (void *)A.edge_split.val, (void *)A.edge_split.mid, (void *)A.long_rows.rows, (void *)A.long_rows.row_chunk_ptr,
                        (void *)A.long_rows.chunks, (void *)A.hub_rows.rows, (void *)A.hub_rows.row_chunk_ptr, (void *)A.hub_rows.chunks,
                        (void *)A.rows_split, (void *)A.rows_edge.idx, (void *)A.rows_edge.mid, (void *)A.rows_edge.brows})
            if (p) (void)hipFree(p);
        for (BlockedAdj *B : {(BlockedAdj *)&A.blk, (BlockedAdj *)&A.blk16, (BlockedAdj *)&A.swp}) free_blocked(B);
        A = Adjacency{};   // every schedule, layout and flag of the direction at once
    }
    c->has_graph = false;
}

int dory_destroy(dory_ctx *c) {
    if (!c) return DORY_ERR_ARG;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    drain_timing(c);
    for (auto &p : c->ev_pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    if (c->nccl) ncclCommDestroy((ncclComm_t)c->nccl);
    if (c->local) {   // leave the group: peers find a null entry, not a dangling pointer
        std::lock_guard<std::mutex> lk(c->local->mu);
        for (auto &q : c->local->ctx) if (q == c) q = nullptr;
    }
    for (hipEvent_t e : {c->ev_sent[0], c->ev_sent[1], c->ev_cons[0], c->ev_cons[1], c->ev_gready[0], c->ev_gready[1], c->ev_gdone[0], c->ev_gdone[1]})
        if (e) (void)hipEventDestroy(e);
    if (c->ar_tmp) (void)hipFree(c->ar_tmp);
    free_table(c->tensors);
    free_table(c->weights);
    free_table(c->wgrads);
    free_table(c->adam_m);
    free_table(c->adam_v);
    free_graph(c);
    for (int d = 0; d < 2; ++d) {
        if (c->plan[d].d_send_lvids) (void)hipFree(c->plan[d].d_send_lvids);
        if (c->plan[d].d_unpack_slots && c->plan[d].d_unpack_slots != c->plan[d].d_recv_slots) (void)hipFree(c->plan[d].d_unpack_slots);
        if (c->plan[d].d_recv_slots) (void)hipFree(c->plan[d].d_recv_slots);
        if (c->plan[d].d_send_map) (void)hipFree(c->plan[d].d_send_map);
    }
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->bf16_rows) (void)hipFree(c->bf16_rows);
    if (c->gatmh_carry_state) (void)hipFree(c->gatmh_carry_state);
    if (c->partial) (void)hipFree(c->partial);
    if (c->epoch_exec) (void)hipGraphExecDestroy(c->epoch_exec);
    if (c->epoch_graph) (void)hipGraphDestroy(c->epoch_graph);
    if (c->d_lr_table) (void)hipFree(c->d_lr_table);
    if (c->d_replay_idx) (void)hipFree(c->d_replay_idx);
    if (c->send_buf) (void)hipFree(c->send_buf);
    if (c->recv_buf) (void)hipFree(c->recv_buf);
    scatter_free(c);
    if (c->d_stat) (void)hipFree(c->d_stat);
    if (c->sweep_stat) (void)hipFree(c->sweep_stat);
    if (c->d_stat3) (void)hipFree(c->d_stat3);
    if (c->ev_a) (void)hipEventDestroy(c->ev_a);
    if (c->ev_b) (void)hipEventDestroy(c->ev_b);
    if (c->own_compute && c->compute) (void)hipStreamDestroy(c->compute);
    if (c->own_comm && c->comm) (void)hipStreamDestroy(c->comm);
    delete c;
    return DORY_OK;
}

const char *dory_last_error(dory_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int dory_set_streams(dory_ctx *c, void *compute_stream, void *comm_stream) {
    CHECK_CTX(c);
    HIPCK(c, hipDeviceSynchronize());
    if (compute_stream) {
        if (c->own_compute) (void)hipStreamDestroy(c->compute);
        c->compute = (hipStream_t)compute_stream;
        c->own_compute = false;
    }
    if (comm_stream) {
        if (c->own_comm) (void)hipStreamDestroy(c->comm);
        c->comm = (hipStream_t)comm_stream;
        c->own_comm = false;
    }
    return DORY_OK;
}

int dory_sync(dory_ctx *c) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }   // (a deferred exchange nobody consumed yet: its ghosts land first)
    HIPCK(c, hipStreamSynchronize(c->compute));
    HIPCK(c, hipStreamSynchronize(c->comm));
    c->halo_pending = false;   // everything has landed
    return DORY_OK;
}

int dory_configure(dory_ctx *c, int gnn_type, uint32_t num_layers, const uint32_t *dims,
                   uint32_t global_vtx_cnt, uint32_t node_id, uint32_t num_nodes) {
    CHECK_CTX(c);
    if (!dims || num_layers == 0 || (gnn_type != DORY_GCN && gnn_type != DORY_GAT && gnn_type != DORY_GATMH) || num_nodes == 0 ||
        node_id >= num_nodes)
        return fail(c, DORY_ERR_ARG, "dory_configure: bad arguments");
    for (uint32_t i = 0; i <= num_layers; ++i)
        if (dims[i] == 0) return fail(c, DORY_ERR_ARG, "dory_configure: zero layer width");
    char msg[256];
    if (option_model_conflict(c->opt, gnn_type, msg, sizeof(msg))) return fail(c, DORY_ERR_ARG, "%s", msg);
    if (c->gat_bf16_mode && gnn_type != DORY_GAT)
        return fail(c, DORY_ERR_ARG, "dory_configure: dory_gat_bf16_gather mode %d is set, which serves the GAT prototype (DORY_GAT) only", c->gat_bf16_mode);
    c->gnn = gnn_type;
    c->L = num_layers;
    c->dims.assign(dims, dims + num_layers + 1);
    c->globalV = global_vtx_cnt;
    c->nodeId = node_id;
    c->numNodes = num_nodes;
    c->heads.assign(num_layers, 8);   // multi-head GAT extension defaults: 8 hidden heads, 1 output head
    c->heads[num_layers - 1] = 1;
    c->configured = true;
    return DORY_OK;
}

// ---- the GAT prototype's bf16 row gathers: switch and counters (include/dorylus_hip.h; the dispatch: abi_stages.hip) ----
int dory_gat_bf16_gather(dory_ctx *c, int mode, int wide) {
    CHECK_CTX(c);
    if (c->configured && c->gnn != DORY_GAT)
        return fail(c, DORY_ERR_ARG, "gat_bf16_gather: this context is configured as %s; the feature serves the GAT prototype (DORY_GAT) only",
                    c->gnn == DORY_GCN ? "DORY_GCN (its option: gcn_bf16_gather)" : "DORY_GATMH (its option: gatmh_bf16_gather)");
    if (mode < 0 || mode > 2) return fail(c, DORY_ERR_ARG, "gat_bf16_gather: mode %d outside 0..2", mode);
    if (wide < 0 || wide > 1) return fail(c, DORY_ERR_ARG, "gat_bf16_gather: wide %d outside 0..1", wide);
    if (wide && !mode) return fail(c, DORY_ERR_ARG, "gat_bf16_gather: wide = 1 needs mode 1 or 2 (nothing gathers bf16 rows with mode 0)");
    if (c->capturing) return fail(c, DORY_ERR_ARG, "gat_bf16_gather: not while an epoch graph is being recorded");
    if (mode != c->gat_bf16_mode || (wide == 1) != c->gat_bf16_wide) epoch_graph_drop_locked(c);   // (a recorded epoch holds the other mode's kernels)
    c->gat_bf16_mode = mode;
    c->gat_bf16_mode_pub.store(mode, std::memory_order_release);   // (dory_halo_bf16_rows: the peers of the local transport read the rule's inputs)
    c->gat_bf16_wide = wide == 1;
    return gat_bf16_reserve_all(c);   // (before dory_preallocate: nothing yet -- the first eager aggregation reserves)
}

int dory_gat_bf16_gather_stats(dory_ctx *c, uint64_t *k1s, uint64_t *k1s_wide, uint64_t *k1, uint64_t *fp32_fallbacks) {
    CHECK_CTX(c);
    if (k1s) *k1s = c->gat_bf16_gathers_k1s;
    if (k1s_wide) *k1s_wide = c->gat_bf16_gathers_k1s_wide;
    if (k1) *k1 = c->gat_bf16_gathers_k1;
    if (fp32_fallbacks) *fp32_fallbacks = c->gat_bf16_fp32_fallbacks;
    return DORY_OK;
}

// ---- dory_gatmh_row_gather_hub_split: hub rows of the row-gather family cut into chunks (gat_mh_rows.hip; include/dorylus_hip.h) ----
int dory_gatmh_row_gather_hub_split(dory_ctx *c, uint32_t chunk_entries) {
    CHECK_CTX(c);
    if (chunk_entries && c->configured && c->gnn != DORY_GATMH)
        return fail(c, DORY_ERR_ARG, "gatmh_row_gather_hub_split: this context is configured as %s; the feature serves the multi-head GAT (DORY_GATMH) only",
                    c->gnn == DORY_GCN ? "DORY_GCN (K1 cuts its long rows itself)" : "DORY_GAT");
    if (chunk_entries && ((chunk_entries & 63u) || chunk_entries > (1u << 20)))
        return fail(c, DORY_ERR_ARG, "gatmh_row_gather_hub_split: chunk_entries %u is neither 0 nor a multiple of 64 in 64..1048576", chunk_entries);
    if (c->capturing) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_hub_split: not while an epoch graph is being recorded");
    if (chunk_entries != c->gatmh_hub_chunk) epoch_graph_drop_locked(c);   // (a recorded epoch holds the other value's launches)
    c->gatmh_hub_chunk = chunk_entries;
    if (!c->has_graph) return DORY_OK;   // (before dory_graph_upload: the first aggregation plans)
    for (Adjacency &A : c->adj) {
        const int rc = hub_plan_ensure(c, A);
        if (rc) return rc;
    }
    return DORY_OK;
}

int dory_gatmh_row_gather_hub_split_stats(dory_ctx *c, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *src, uint64_t *in_hub_rows,
                                          uint64_t *in_chunks, uint64_t *out_hub_rows, uint64_t *out_chunks) {
    CHECK_CTX(c);
    if (fwd) *fwd = c->gatmh_hub_fwd;
    if (dst_edge_pass) *dst_edge_pass = c->gatmh_hub_dst;
    if (src) *src = c->gatmh_hub_src;
    const bool in = c->adj[ADJ_IN].hub_chunk && c->adj[ADJ_IN].hub_chunk == c->gatmh_hub_chunk;
    const bool out = c->adj[ADJ_OUT].hub_chunk && c->adj[ADJ_OUT].hub_chunk == c->gatmh_hub_chunk;
    if (in_hub_rows) *in_hub_rows = in ? c->adj[ADJ_IN].hub_rows.nrows : 0;
    if (in_chunks) *in_chunks = in ? c->adj[ADJ_IN].hub_rows.nchunks : 0;
    if (out_hub_rows) *out_hub_rows = out ? c->adj[ADJ_OUT].hub_rows.nrows : 0;
    if (out_chunks) *out_chunks = out ? c->adj[ADJ_OUT].hub_rows.nchunks : 0;
    return DORY_OK;
}

// ---- dory_gatmh_row_gather_overlap: the row-gather family's interior rows beside the exchange (abi_stages.hip; include/dorylus_hip.h) ----
int dory_gatmh_row_gather_overlap(dory_ctx *c, int on) {
    CHECK_CTX(c);
    if (on != 0 && on != 1) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_overlap: value %d is neither 0 nor 1", on);
    if (on && c->configured && c->gnn != DORY_GATMH)
        return fail(c, DORY_ERR_ARG, "gatmh_row_gather_overlap: this context is configured as %s; the feature serves the multi-head GAT (DORY_GATMH) only",
                    c->gnn == DORY_GCN ? "DORY_GCN (K1 runs its local part first itself: halo_overlap)" : "DORY_GAT");
    if (c->capturing) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_overlap: not while an epoch graph is being recorded");
    if ((on == 1) != c->gatmh_rows_overlap) epoch_graph_drop_locked(c);   // (a recorded epoch holds the other value's launches)
    c->gatmh_rows_overlap = on == 1;
    if (!on || !c->has_graph) return DORY_OK;   // (before dory_graph_upload: the first aggregation plans)
    for (Adjacency &A : c->adj) {
        const int rc = interior_plan_ensure(c, A);
        if (rc) return rc;
    }
    return DORY_OK;
}

int dory_gatmh_row_gather_overlap_stats(dory_ctx *c, uint64_t *fwd_split, uint64_t *src_split, uint64_t *fwd_in_flight, uint64_t *src_in_flight,
                                        uint64_t *in_interior_rows, uint64_t *out_interior_rows, uint64_t *bwd_deferred) {
    CHECK_CTX(c);
    if (fwd_split) *fwd_split = c->gatmh_ovl_fwd;
    if (src_split) *src_split = c->gatmh_ovl_src;
    if (fwd_in_flight) *fwd_in_flight = c->gatmh_ovl_fwd_flight;
    if (src_in_flight) *src_in_flight = c->gatmh_ovl_src_flight;
    if (in_interior_rows) *in_interior_rows = c->adj[ADJ_IN].rows_split_built ? c->adj[ADJ_IN].rows_interior : 0;
    if (out_interior_rows) *out_interior_rows = c->adj[ADJ_OUT].rows_split_built ? c->adj[ADJ_OUT].rows_interior : 0;
    if (bwd_deferred) *bwd_deferred = c->gatmh_ovl_deferred;
    return DORY_OK;
}

// ---- dory_gatmh_row_gather_edge_split: the row-gather family's local entries beside the exchange (abi_stages.hip; include/dorylus_hip.h) ----
int dory_gatmh_row_gather_edge_split(dory_ctx *c, int value) {
    CHECK_CTX(c);
    if (value < 0 || value > 2) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_edge_split: value %d is neither 0, 1 nor 2", value);
    if (value && c->configured && c->gnn != DORY_GATMH)
        return fail(c, DORY_ERR_ARG, "gatmh_row_gather_edge_split: this context is configured as %s; the feature serves the multi-head GAT (DORY_GATMH) only",
                    c->gnn == DORY_GCN ? "DORY_GCN (K1 runs its local part first itself: halo_overlap)" : "DORY_GAT");
    if (c->capturing) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_edge_split: not while an epoch graph is being recorded");
    if (value != c->gatmh_edge_split) epoch_graph_drop_locked(c);   // (a recorded epoch holds the other value's launches)
    c->gatmh_edge_split = value;
    if (!value || !c->has_graph) return DORY_OK;   // (before dory_graph_upload: the first aggregation plans)
    for (Adjacency &A : c->adj) {
        if (!A.ghosts || !c->N) continue;
        const int rc = rows_edge_ensure(c, A);
        if (rc) return rc;
    }
    // the states of the widest layer, where the tensors exist already (else: at first use)
    size_t need = 0;
    for (uint32_t l = 0; l < c->L && c->prealloc; ++l) {
        Tensor *z = find(c, l, "z"), *el = find(c, l, "el");
        if (z && el) need = std::max(need, (size_t)c->N * gatmh_rows_hub_state_floats(0, z->ld, el->ld) * sizeof(float));
    }
    return need && (c->adj[ADJ_IN].ghosts || c->adj[ADJ_OUT].ghosts) ? carry_state_ensure(c, need) : (int)DORY_OK;
}

int dory_gatmh_row_gather_edge_split_stats(dory_ctx *c, uint64_t *fwd_split, uint64_t *src_split, uint64_t *fwd_in_flight, uint64_t *src_in_flight,
                                           uint64_t *in_local_entries, uint64_t *out_local_entries, uint64_t *hub_fallbacks,
                                           uint64_t *wide_not_taken) {
    CHECK_CTX(c);
    if (fwd_split) *fwd_split = c->gatmh_es_fwd;
    if (src_split) *src_split = c->gatmh_es_src;
    if (fwd_in_flight) *fwd_in_flight = c->gatmh_es_fwd_flight;
    if (src_in_flight) *src_in_flight = c->gatmh_es_src_flight;
    if (in_local_entries) *in_local_entries = c->adj[ADJ_IN].rows_edge.built ? c->adj[ADJ_IN].rows_edge.local : 0;
    if (out_local_entries) *out_local_entries = c->adj[ADJ_OUT].rows_edge.built ? c->adj[ADJ_OUT].rows_edge.local : 0;
    if (hub_fallbacks) *hub_fallbacks = c->gatmh_es_hub_fallbacks;
    if (wide_not_taken) *wide_not_taken = c->gatmh_es_wide_not_taken;
    return DORY_OK;
}

// ---- dory_gatmh_row_gather_bf16_wide: the row-gather family's bf16 passes gather 16 bytes a lane (gat_mh_rows.hip; include/dorylus_hip.h) ----
int dory_gatmh_row_gather_bf16_wide(dory_ctx *c, int on) {
    CHECK_CTX(c);
    if (on != 0 && on != 1) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_bf16_wide: value %d is neither 0 nor 1", on);
    if (on && c->configured && c->gnn != DORY_GATMH)
        return fail(c, DORY_ERR_ARG, "gatmh_row_gather_bf16_wide: this context is configured as %s; the feature serves the multi-head GAT (DORY_GATMH) only",
                    c->gnn == DORY_GCN ? "DORY_GCN (its wide forms: gcn_bf16_wide for K1s, dory_k1_bf16_wide for K1)"
                                       : "DORY_GAT (its wide forms: dory_gat_bf16_gather's wide for K1s, dory_k1_bf16_wide for K1)");
    if (c->capturing) return fail(c, DORY_ERR_ARG, "gatmh_row_gather_bf16_wide: not while an epoch graph is being recorded");
    if ((on == 1) != c->gatmh_rows_wide) epoch_graph_drop_locked(c);   // (a recorded epoch holds the other value's launches)
    c->gatmh_rows_wide = on == 1;
    return DORY_OK;
}

int dory_gatmh_row_gather_bf16_wide_stats(dory_ctx *c, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *src, uint64_t *narrow_while_on) {
    CHECK_CTX(c);
    if (fwd) *fwd = c->gatmh_rows8_fwd;
    if (dst_edge_pass) *dst_edge_pass = c->gatmh_rows8_dst;
    if (src) *src = c->gatmh_rows8_src;
    if (narrow_while_on) *narrow_while_on = c->gatmh_rows8_narrow;
    return DORY_OK;
}

// ---- dory_k1_bf16_wide: K1's aggregations on bf16 rows gather 16 bytes a lane (spmm.hip: spmm_rows_bf16x8_kernel; include/dorylus_hip.h) ----
int dory_k1_bf16_wide(dory_ctx *c, int on) {
    CHECK_CTX(c);
    if (on != 0 && on != 1) return fail(c, DORY_ERR_ARG, "k1_bf16_wide: value %d is neither 0 nor 1", on);
    if (on && c->configured && c->gnn == DORY_GATMH)
        return fail(c, DORY_ERR_ARG, "k1_bf16_wide: this context is configured as DORY_GATMH (its wide form: dory_gatmh_row_gather_bf16_wide); "
                                     "the feature serves K1 of DORY_GCN and DORY_GAT only");
    if (c->capturing) return fail(c, DORY_ERR_ARG, "k1_bf16_wide: not while an epoch graph is being recorded");
    if ((on == 1) != c->k1_bf16_wide) epoch_graph_drop_locked(c);   // (a recorded epoch holds the other value's launches)
    c->k1_bf16_wide = on == 1;
    return DORY_OK;
}

int dory_k1_bf16_wide_stats(dory_ctx *c, uint64_t *wide, uint64_t *narrow_while_on) {
    CHECK_CTX(c);
    if (wide) *wide = c->k1_rows8_wide;
    if (narrow_while_on) *narrow_while_on = c->k1_rows8_narrow;
    return DORY_OK;
}

int dory_gatmh_heads(dory_ctx *c, const uint32_t *heads) {
    CHECK_CTX(c);
    if (!c->configured || c->gnn != DORY_GATMH || !heads) return fail(c, DORY_ERR_ARG, "gatmh_heads: configure with DORY_GATMH first");
    for (uint32_t l = 0; l < c->L; ++l)
        if (heads[l] == 0 || heads[l] > 64) return fail(c, DORY_ERR_ARG, "gatmh_heads: bad head count");
    c->heads.assign(heads, heads + c->L);
    return DORY_OK;
}

int dory_graph_upload(dory_ctx *c, uint32_t N, uint32_t Gsrc, uint32_t Gdst, uint64_t nnz_in,
                      const uint64_t *column_ptrs, const uint32_t *row_idxs, const float *csc_values,
                      uint64_t nnz_out, const uint64_t *row_ptrs, const uint32_t *column_idxs,
                      const float *csr_values, const float *vtx_norms) {
    CHECK_CTX(c);
    c->ah0_valid = false;
    if (!column_ptrs || !row_ptrs || (N && !vtx_norms) || (nnz_in && (!row_idxs || !csc_values)) ||
        (nnz_out && (!column_idxs || !csr_values)))
        return fail(c, DORY_ERR_ARG, "dory_graph_upload: null array");
    epoch_graph_drop_locked(c);   // a recorded epoch points at the adjacency (and its blocked copies) freed below
    if (column_ptrs[0] != 0 || column_ptrs[N] != nnz_in || row_ptrs[0] != 0 || row_ptrs[N] != nnz_out)
        return fail(c, DORY_ERR_ARG, "dory_graph_upload: pointer arrays do not match nnz");
    for (uint32_t v = 0; v < N; ++v)
        if (column_ptrs[v] > column_ptrs[v + 1] || row_ptrs[v] > row_ptrs[v + 1])
            return fail(c, DORY_ERR_ARG, "dory_graph_upload: pointer array not monotone at %u", v);
    for (uint64_t e = 0; e < nnz_in; ++e)
        if (row_idxs[e] >= (uint64_t)N + Gsrc) return fail(c, DORY_ERR_ARG, "row index %u out of range at %llu", row_idxs[e], (unsigned long long)e);
    for (uint64_t e = 0; e < nnz_out; ++e)
        if (column_idxs[e] >= (uint64_t)N + Gdst) return fail(c, DORY_ERR_ARG, "column index %u out of range at %llu", column_idxs[e], (unsigned long long)e);
    HIPCK(c, hipDeviceSynchronize());
    free_graph(c);
    c->N = N;
    int rc;
    if ((rc = upload_array(c, &c->norm, vtx_norms, (uint64_t)N))) return rc;
    const bool by_median = c->opt[OPT_SPMM_ORDER] == 3;    // (set before the upload: the schedule is built here)
    struct HostAdj { const uint64_t *ptr; const uint32_t *idx; const float *val; uint64_t nnz; uint32_t ghosts; };
    const HostAdj host[2] = {{column_ptrs, row_idxs, csc_values, nnz_in, Gsrc}, {row_ptrs, column_idxs, csr_values, nnz_out, Gdst}};
    for (int d = 0; d < 2; ++d) {   // ADJ_IN, ADJ_OUT: each direction on its own
        Adjacency &A = c->adj[d];
        const uint64_t *ptr = host[d].ptr;
        const uint32_t *idx = host[d].idx;
        const float *val = host[d].val;
        const uint64_t nnz = A.nnz = host[d].nnz;
        A.ghosts = host[d].ghosts;
        if ((rc = upload_array(c, &A.ptr, ptr, (uint64_t)N + 1))) return rc;
        if ((rc = upload_array(c, &A.idx, idx, nnz))) return rc;
        if ((rc = upload_array(c, &A.val, val, nnz))) return rc;
        const std::vector<uint32_t> ord = by_median ? median_source_order(ptr, idx, N) : degree_order(ptr, N);
        if ((rc = upload_array(c, &A.order, ord.data(), (uint64_t)N))) return rc;
        {   // is the degree distribution skewed enough for the longest-first row schedule to pay?  (Amazon-size uniform graph:
            // 129 ms per epoch in row order against 134 longest first; R-MAT of the same size: 118 against 104)
            uint64_t mx = 0;
            for (uint32_t v = 0; v < N; ++v) mx = std::max<uint64_t>(mx, ptr[v + 1] - ptr[v]);
            A.skew = N > 0 && mx * (uint64_t)N > 8ull * nnz + 8ull * N;
        }
        if (A.ghosts) {   // K1's interior / boundary row split (partitions with ghosts)
            std::vector<uint32_t> interior, boundary;
            for (uint32_t v : ord) {   // keeps the longest-row-first order inside both parts
                bool local = true;
                for (uint64_t e = ptr[v]; e < ptr[v + 1] && local; ++e) local = idx[e] < N;
                (local ? interior : boundary).push_back(v);
            }
            A.n_interior = (uint32_t)interior.size();
            interior.insert(interior.end(), boundary.begin(), boundary.end());
            if ((rc = upload_array(c, &A.split, interior.data(), (uint64_t)N))) return rc;
        }
        {   // K1's hub rows (spmm.hip: long rows)
            LongRowsHost h;
            plan_long_rows(ptr, N, &h);
            LongRowsDev &L = A.long_rows;
            L.nrows = (uint32_t)h.rows.size();
            L.nchunks = (uint32_t)(h.chunks.size() / 6);
            if (L.nchunks) {
                if ((rc = upload_array(c, &L.rows, h.rows.data(), h.rows.size()))) return rc;
                if ((rc = upload_array(c, &L.row_chunk_ptr, h.row_chunk_ptr.data(), h.row_chunk_ptr.size()))) return rc;
                if ((rc = upload_array(c, &L.chunks, h.chunks.data(), h.chunks.size()))) return rc;
            }
        }
        // K1's local-first edge order (ctx.hpp: EdgeSplit) for GCN partitions with ghosts and without hub rows
        if (c->gnn == DORY_GCN && c->opt[OPT_SPMM_EDGE_SPLIT] && A.ghosts && !A.long_rows.nchunks) {
            std::vector<uint32_t> i2(nnz);
            std::vector<float> v2(nnz);
            std::vector<uint64_t> mid(N);
#pragma omp parallel for schedule(dynamic, 4096)
            for (int64_t v = 0; v < (int64_t)N; ++v) {
                uint64_t w = ptr[v];
                for (uint64_t e = ptr[v]; e < ptr[v + 1]; ++e)
                    if (idx[e] < N) { i2[w] = idx[e]; v2[w] = val[e]; ++w; }
                mid[v] = w;
                for (uint64_t e = ptr[v]; e < ptr[v + 1]; ++e)
                    if (idx[e] >= N) { i2[w] = idx[e]; v2[w] = val[e]; ++w; }
            }
            EdgeSplit &E = A.edge_split;
            if ((rc = upload_array(c, &E.idx, i2.data(), nnz))) return rc;
            if ((rc = upload_array(c, &E.val, v2.data(), nnz))) return rc;
            if ((rc = upload_array(c, &E.mid, mid.data(), (uint64_t)N))) return rc;
        }
    }
    c->has_graph = true;
    return DORY_OK;
}

int dory_preallocate(dory_ctx *c) {
    CHECK_CTX(c);
    c->ah0_valid = false;
    if (!c->configured || !c->has_graph) return fail(c, DORY_ERR_ARG, "dory_preallocate: configure and graph_upload first");
    epoch_graph_drop_locked(c);   // a recorded epoch points at the tensors freed below
    HIPCK(c, hipDeviceSynchronize());
    free_table(c->tensors); free_table(c->weights); free_table(c->wgrads); free_table(c->adam_m); free_table(c->adam_v);
    const uint32_t L = c->L, N = c->N;
    Adjacency &In = c->adj[ADJ_IN], &Out = c->adj[ADJ_OUT];
    auto &d = c->dims;
    c->tensors.assign(L + 1, {});
    c->weights.assign(L, {}); c->wgrads.assign(L, {}); c->adam_m.assign(L, {}); c->adam_v.assign(L, {});
    int rc = 0;
    auto mk = [&](uint32_t layer, const char *name, uint64_t rows, uint32_t cols) {
        if (rc) return;
        rc = alloc_tensor(c, c->tensors[layer][name], rows, cols);
    };
    if (c->gnn == DORY_GCN) {  // Engine::preallocateGCN (engine/ops/gcn_ops.cpp:27-93)
        mk(0, "x", N, d[0]);
        mk(0, "fg", In.ghosts, d[0]);
        mk(L - 1, "lab", N, d[L]);
        for (uint32_t l = 0; l < L; ++l) {
            mk(l, "ah", N, d[l]);
            mk(l, "z", N, d[l + 1]);            // reference keeps z only for l < L-1; last-layer logits are a temporary there
            if (l < L - 1) {
                mk(l, "h", N, d[l + 1]);
                mk(l + 1, "fg", In.ghosts, d[l + 1]);
            }
            mk(l, "g", N, d[l + 1]);            // interGrad / d_output temporaries of CPU_comm.cpp:121,143
        }
        for (uint32_t l = L - 1; l > 0; --l) {
            mk(l, "grad", N, d[l]);
            mk(l - 1, "bg", Out.ghosts, d[l]);
            mk(l - 1, "aTg", N, d[l]);
        }
        for (uint32_t l = 0; l < L && L >= 2; ++l) {   // transform-first order (option gcn_transform_first)
            if (d[l] <= d[l + 1]) continue;
            mk(l, "xw", N, d[l + 1]);          // in_l W_l
            mk(l, "fgxw", In.ghosts, d[l + 1]);  // its ghost rows (layer 0: transformed locally from fg@0, else exchanged)
            mk(l, "u", N, d[l + 1]);           // A^T g_l
            mk(l, "bgg", Out.ghosts, d[l + 1]);   // ghost rows of g_l (backward exchange)
        }
    } else if (c->gnn == DORY_GATMH) {  // extension (no reference counterpart): see dory_gatmh_heads
        mk(0, "h", N, d[0]);
        mk(L - 1, "lab", N, d[L]);
        mk(L - 1, "logits", N, d[L]);
        mk(L - 1, "grad", N, d[L]);
        for (uint32_t l = 0; l < L; ++l) {
            const uint32_t K = c->heads[l];
            const bool last = l == L - 1;
            const uint32_t zw = last ? d[l + 1] * K : d[l + 1];
            const uint32_t D = zw / K;
            if (zw % K || zw > 256 || (K > 1 && ((D & (D - 1)) || D > 64)))
                return fail(c, DORY_ERR_ARG, "multi-head GAT: layer %u width %u does not split into %u heads (D power of two <= 64, K*D <= 256)", l, zw, K);
            mk(l, "z", N, zw);
            mk(l, "o", N, zw);
            mk(l, "do", N, zw);
            mk(l, "dz", N, zw);
            for (const char *nm : {"el", "er", "m", "den", "t", "del", "der"}) mk(l, nm, N, K);
            mk(l, "st", N, 4 * K);               // (er, m, 1/den, t) per (v,k): what the source-side sweep gathers per edge
            mk(l, "op", N, zw);                  // the part of "o" that came over edges on LeakyReLU's positive branch (sweep forward)
            mk(l, "dpos", N, K);                 // and the attention mass of those edges
            // partitioned runs: ghost sources of the in-edges (z exchanged forward, el/er recomputed from it) and
            // ghost destinations of the out-edges (dO and st exchanged between the two phases of the backward sweep)
            mk(l, "fg_z", In.ghosts, zw);
            mk(l, "fg_el", In.ghosts, K);
            mk(l, "fg_er", In.ghosts, K);
            mk(l, "bg_do", Out.ghosts, zw);
            mk(l, "bg_st", Out.ghosts, 4 * K);
            if (!last) mk(l + 1, "h", N, d[l + 1]);
            if (l > 0) mk(l, "dh", N, d[l]);
        }
    } else {  // Engine::preallocateGAT (engine/ops/gat_ops.cpp:27-115)
        mk(0, "h", N, d[0]);
        mk(L - 1, "lab", N, d[L]);
        for (uint32_t l = 0; l < L; ++l) {
            mk(l, "z", N, d[l + 1]);
            mk(l, "az", In.nnz, 1);
            mk(l, "fg_z", In.ghosts, d[l + 1]);
            Tensor A;  // "A" aliases forwardAdj.values (gat_ops.cpp:61-64)
            A.rows = In.nnz; A.cols = 1; A.ld = 1; A.d = In.val; A.owned = false;
            c->tensors[l]["A"] = A;
            mk(l, "ah", N, d[l + 1]);
            if (l < L - 1) mk(l + 1, "h", N, d[l + 1]);
            mk(l, "grad", N, d[l + 1]);
            mk(l, "dA", In.nnz, 1);
            mk(l, "aTg", N, d[l + 1]);
            mk(l, "bg_d", Out.ghosts, d[l + 1]);
        }
        mk(0, "cw", N, 1);  // column weights for the a_i gradient (K5)
        for (uint32_t l = 0; l < L; ++l) {
            mk(l, "arow", N, 1);   // per-destination value of "A"  (all edges of a column are equal)
            mk(l, "drow", N, 1);   // per-destination value of "dA"
        }
        for (uint32_t l = 0; l < L; ++l) mk(l, "azrow", N, 1);  // per-destination value of "az"
        c->gat_az_stale.assign(L, 0);
        c->gat_dA_stale.assign(L, 0);
        c->gat_azrow_valid.assign(L, 0);
        c->gat_A_stale_layer = -1;
        for (uint32_t l = 0; l < L; ++l) mk(l, "nsum", N, d[l + 1]);   // unweighted neighbour sum of z (kept from the forward for the backward aggregation)
        mk(0, "ones", N, 1);
        c->gat_arow_valid.assign(L, 0);
        c->gat_drow_valid.assign(L, 0);
        c->gat_nsum_valid.assign(L, 0);
        c->gat_nsum_bf16.assign(L, 0);
    }
    if (rc) return rc;
    for (uint32_t l = 0; l < L; ++l) {
        if (c->gnn == DORY_GATMH) {
            const uint32_t zw = l == L - 1 ? d[l + 1] * c->heads[l] : d[l + 1];
            for (auto *tab : {&c->weights, &c->wgrads, &c->adam_m, &c->adam_v}) {
                if ((rc = alloc_tensor(c, (*tab)[l]["w"], d[l], zw))) return rc;
                if ((rc = alloc_tensor(c, (*tab)[l]["a_l"], zw, 1))) return rc;
                if ((rc = alloc_tensor(c, (*tab)[l]["a_r"], zw, 1))) return rc;
            }
            continue;
        }
        if ((rc = alloc_tensor(c, c->weights[l]["w"], d[l], d[l + 1]))) return rc;
        if ((rc = alloc_tensor(c, c->wgrads[l]["w"], d[l], d[l + 1]))) return rc;
        if ((rc = alloc_tensor(c, c->adam_m[l]["w"], d[l], d[l + 1]))) return rc;
        if ((rc = alloc_tensor(c, c->adam_v[l]["w"], d[l], d[l + 1]))) return rc;
        if (c->gnn == DORY_GAT) {
            if ((rc = alloc_tensor(c, c->weights[l]["a_i"], d[l + 1], 1))) return rc;
            if ((rc = alloc_tensor(c, c->wgrads[l]["a_i"], d[l + 1], 1))) return rc;
            if ((rc = alloc_tensor(c, c->adam_m[l]["a_i"], d[l + 1], 1))) return rc;
            if ((rc = alloc_tensor(c, c->adam_v[l]["a_i"], d[l + 1], 1))) return rc;
        }
    }
    c->adam.epochs = 1;
    if ((rc = ghost_twins_alloc(c))) return rc;   // (dory_halo_bf16_ghosts is on: the new ghost tensors' twins, now)
    HIPCK(c, hipStreamSynchronize(c->compute));
    auto layer_ld = [&](uint32_t l) { return pad_ld(l == L - 1 ? d[l + 1] * c->heads[l] : d[l + 1]); };   // multi-head GAT: z / o of layer l
    const uint32_t G = std::min<uint32_t>(32u, c->cus_per_xcd);
    if (c->opt[OPT_SPMM_VARIANT] == 2 && N > 0 && c->gnn == DORY_GATMH && c->opt[OPT_GATMH_SWEEP]) {
        // the sweep layouts (K1s's even layout; the deal is made for the 32-lane launches) and the gate counters now
        uint32_t maxld = 0;
        for (uint32_t l = 0; l < L; ++l) maxld = std::max(maxld, layer_ld(l));
        const int group = blk_group_for(c, maxld);
        c->gatmh_fwd_swept.assign(L, 0);
        size_t need = 0;
        for (Adjacency &A : c->adj) {
            if ((rc = ensure_sweep(c, A, group))) return rc;
            for (uint32_t l = 0; l < L && A.swp.nb; ++l)   // every layer's own launch shape: its leading dimension (a 96-float layer runs 16-lane
                // groups on two slabs) and the group blk_group_for() gives it; launches walk fewer rows per group than the
                // layout deals (more sweeps, more counters): 2 is the least
                need = std::max(need, sweep_counter_bound(A.swp.npos, layer_ld(l), blk_group_for(c, layer_ld(l)), 2, false, G, A.swp.nb));
        }
        // (ensure_partial synchronises the compute stream before it frees; nothing in flight reads c->partial before `prealloc` is set)
        if ((rc = ensure_partial(c, need, "sweep counters"))) return rc;
    }
    if (c->opt[OPT_SPMM_VARIANT] >= 1 && N > 0 && c->gnn == DORY_GATMH && c->opt[OPT_GATMH_BLOCKED]) {
        // the extension's forward sum gathers through the same source-blocked copy of the in-edges
        uint32_t maxld = 0, minld = 0xFFFFFFFFu;
        for (uint32_t l = 0; l < L; ++l) { maxld = std::max(maxld, layer_ld(l)); minld = std::min(minld, layer_ld(l)); }
        if ((rc = ensure_blocked(c, In, blk_group_for(c, maxld)))) return rc;
        if ((rc = ensure_blocked(c, Out, blk_group_for(c, maxld)))) return rc;   // backward, source side
        if (maxld >= 128 && minld < 128 && !In.blk.na && !Out.blk.na) {   // narrow layers beside wide ones: their own copies (256-B slabs)
            if ((rc = ensure_blocked(c, In, 16, true))) return rc;
            if ((rc = ensure_blocked(c, Out, 16, true))) return rc;
        }
        const uint32_t nbmax = std::max(In.blk.nb, Out.blk.nb);
        size_t need = (size_t)nbmax * N * (maxld + 64) * sizeof(float);            // + per-(block,row,head) partials
        need = std::max(need, (size_t)std::max(In.blk16.nb, Out.blk16.nb) * N * (std::min<uint32_t>(maxld, 96u) + 64) * sizeof(float));
        if (nbmax && need <= ((size_t)48 << 30) && (rc = ensure_partial(c, need, "partial buffer"))) return rc;
    }
    if (c->opt[OPT_SPMM_VARIANT] >= 1 && N > 0 && c->gnn != DORY_GATMH) {   // K1b: regroup the edges now, not inside the first epoch
        uint32_t minld = 0xFFFFFFFFu;
        for (uint32_t l = 0; l < L; ++l) {
            const uint32_t w = c->gnn == DORY_GCN ? (l == 0 ? d[0] : d[l]) : d[l + 1];
            minld = std::min(minld, pad_ld(w));
        }
        uint32_t maxld = 0;
        for (uint32_t l = 0; l <= L; ++l) maxld = std::max(maxld, pad_ld(d[l]));
        const int group = blk_group_for(c, maxld);   // block size for the widest rows (most of the traffic)
        if (minld >= 32 && c->opt[OPT_SPMM_VARIANT] == 2) {
            // K1s: its layouts and the gate counters of the largest launch now, so that nothing is built or allocated
            // inside an epoch (a partition it does not take -- too small, too large -- keeps K1 / builds K1b on demand)
            size_t need = 0;
            for (Adjacency &A : c->adj) {
                if ((rc = ensure_sweep(c, A, group))) return rc;
                if (A.swp.nb) need = std::max(need, sweep_counter_bound(A.swp.npos, maxld, group, k1s_rows(c, A.swp, group), false, G, A.swp.nb));
                // (the wide launches of option gcn_bf16_wide / dory_gat_bf16_gather never need more, but for a forced row count that only
                //  16-lane groups take)
                if (A.swp.nb && sweep_wide_applies(maxld, group, k1s_rows(c, A.swp, 16)))
                    need = std::max(need, sweep_counter_bound(A.swp.npos, maxld, group, k1s_rows(c, A.swp, 16), true, G, A.swp.nb));
            }
            if ((rc = ensure_partial(c, need, "sweep counters"))) return rc;
            // the slots of the split rows' pieces too (skewed graphs): an epoch recorded into a hipGraph right after a
            // re-upload must not find anything left to allocate
            const uint32_t nslots = std::max(In.swp.nslots, Out.swp.nslots);
            if (nslots && (rc = ensure_scratch(c, (size_t)nslots * maxld * sizeof(float)))) return rc;
        } else if (minld >= 32) {
            if ((rc = ensure_blocked(c, In, group))) return rc;
            if ((rc = ensure_blocked(c, Out, group))) return rc;
            // the partial-sum buffer too, so that no allocation happens inside an epoch
            const uint32_t nbmax = std::max(In.blk.nb, Out.blk.nb);
            const size_t need = (size_t)nbmax * N * maxld * sizeof(float);
            if (nbmax && need <= ((size_t)48 << 30) && (rc = ensure_partial(c, need, "partial buffer"))) return rc;
        }
    }
    c->gat_ones_set = false;
    c->prealloc = true;
    return DORY_OK;
}

// ---------------------------------------------------------------------------------------
int dory_tensor_info(dory_ctx *c, uint32_t layer, const char *name, uint64_t *rows, uint32_t *cols,
                     uint32_t *ld, void **device_ptr) {
    CHECK_CTX(c);
    Tensor *t = name ? find(c, layer, name) : nullptr;
    if (!t) return fail(c, DORY_ERR_ARG, "no tensor '%s' at layer %u", name ? name : "(null)", layer);
    if (device_ptr) { int hrc = gat_edge_tensor_hook(c, layer, name, false); if (hrc) return hrc; }   // a raw pointer: the data behind it must be current
    // (dory_halo_bf16_ghosts: ... the fp32 rows too, now and -- raw_handed -- after every later exchange)
    if (device_ptr) { int grc = ghost_fp32_current(c, t); if (grc) return grc; }
    if (rows) *rows = t->rows;
    if (cols) *cols = t->cols;
    if (ld) *ld = t->ld;
    if (device_ptr) {   // (the fused halo pack: the caller may now write the rows itself -- this tensor's exchanges pack from here on)
        *device_ptr = t->d;
        t->raw_handed = true;
        fused_note_write(c, t);
    }
    return DORY_OK;
}

static int upload_dense(dory_ctx *c, Tensor &t, const float *host) {
    if (t.rows == 0 || t.cols == 0) return DORY_OK;
    if (t.ld == t.cols) {
        HIPCK(c, hipMemcpyAsync(t.d, host, t.bytes(), hipMemcpyHostToDevice, c->compute));
    } else {
        float *stage = nullptr;
        const size_t b = (size_t)t.rows * t.cols * sizeof(float);
        HIPCK(c, hipMalloc((void **)&stage, b));
        HIPCK(c, hipMemcpyAsync(stage, host, b, hipMemcpyHostToDevice, c->compute));
        HIPCK(c, launch_pad_copy(t.d, t.ld, stage, t.cols, t.rows, t.cols, c->compute));
        HIPCK(c, hipStreamSynchronize(c->compute));
        (void)hipFree(stage);
    }
    HIPCK(c, hipStreamSynchronize(c->compute));
    return DORY_OK;
}

static int download_dense(dory_ctx *c, const Tensor &t, float *host) {
    if (t.rows == 0 || t.cols == 0) return DORY_OK;
    HIPCK(c, hipStreamSynchronize(c->comm));
    if (t.ld == t.cols) {
        HIPCK(c, hipMemcpyAsync(host, t.d, t.bytes(), hipMemcpyDeviceToHost, c->compute));
    } else {
        HIPCK(c, hipMemcpy2DAsync(host, (size_t)t.cols * sizeof(float), t.d, (size_t)t.ld * sizeof(float),
                                  (size_t)t.cols * sizeof(float), t.rows, hipMemcpyDeviceToHost, c->compute));
    }
    HIPCK(c, hipStreamSynchronize(c->compute));
    return DORY_OK;
}

// Option halo_direct_recv: the plan whose wire order the rows of tensor `name` are stored in -- a ghost tensor of that direction
// with rows -- or null: row r of the tensor is the received row r, the caller's row order[r] (HaloPlan, ctx.hpp).
static int ghost_wire_plan(dory_ctx *c, const char *who, const char *name, const Tensor &t, const HaloPlan **out) {
    *out = nullptr;
    if (!c->halo_direct.load(std::memory_order_acquire) || t.rows == 0) return DORY_OK;
    int dir = -1;
    for (const char *nm : {"fg", "fgxw", "fg_z", "fg_el", "fg_er"}) if (!strcmp(name, nm)) dir = DORY_FORWARD;
    for (const char *nm : {"bg", "bgg", "bg_d", "bg_do", "bg_st"}) if (!strcmp(name, nm)) dir = DORY_BACKWARD;
    if (dir < 0) return DORY_OK;
    const HaloPlan &p = c->plan[dir];
    if (!p.set || !p.direct || p.recv_total != t.rows)
        return fail(c, DORY_ERR_ARG, "%s: halo_direct_recv keeps '%s' in wire order: dory_halo_plan of direction %d first", who, name, dir);
    *out = &p;
    return DORY_OK;
}
// host rows in the caller's order -> the tensor's rows in wire order: the dense rows are permuted, then padded as upload_dense pads
static int upload_ghost_wire(dory_ctx *c, Tensor &t, const float *host, const HaloPlan &p) {
    if (t.cols == 0) return DORY_OK;
    const size_t n = (size_t)t.rows * t.cols;
    float *stage = nullptr;
    HIPCK(c, hipMalloc((void **)&stage, 2 * n * sizeof(float)));
    hipError_t e = hipMemcpyAsync(stage, host, n * sizeof(float), hipMemcpyHostToDevice, c->compute);
    if (e == hipSuccess) e = launch_permute_rows(t.ld == t.cols ? t.d : stage + n, stage, t.cols, p.d_recv_slots, (uint32_t)t.rows, true, c->compute);
    if (e == hipSuccess && t.ld != t.cols) e = launch_pad_copy(t.d, t.ld, stage + n, t.cols, t.rows, t.cols, c->compute);
    if (e == hipSuccess) e = hipStreamSynchronize(c->compute);
    (void)hipFree(stage);
    HIPCK(c, e);
    return DORY_OK;
}
// and back: the rows return to the caller's order in a staging copy, which travels as download_dense moves a tensor
static int download_ghost_wire(dory_ctx *c, const Tensor &t, float *host, const HaloPlan &p) {
    if (t.cols == 0) return DORY_OK;
    Tensor st = t;
    st.d = nullptr;
    HIPCK(c, hipStreamSynchronize(c->comm));
    HIPCK(c, hipMalloc((void **)&st.d, t.bytes()));
    hipError_t e = launch_permute_rows(st.d, t.d, t.ld, p.d_recv_slots, (uint32_t)t.rows, false, c->compute);
    int rc = e == hipSuccess ? download_dense(c, st, host) : fail(c, DORY_ERR_HIP, "tensor_download: row permutation failed: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(c->compute);
    (void)hipFree(st.d);
    return rc;
}

int dory_tensor_upload(dory_ctx *c, uint32_t layer, const char *name, const float *host) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *t = name ? find(c, layer, name) : nullptr;
    if (!t || !host) return fail(c, DORY_ERR_ARG, "tensor_upload: no tensor '%s' at layer %u", name ? name : "(null)", layer);
    if (layer == 0) c->ah0_valid = false;                                    // x / fg@0 / ah@0 may have changed
    if (!strcmp(name, "A")) for (auto &f : c->gat_arow_valid) f = 0;          // caller-supplied edge weights: general path
    if (!strcmp(name, "dA") && layer < c->gat_drow_valid.size()) c->gat_drow_valid[layer] = 0;
    if ((!strcmp(name, "z") || !strcmp(name, "fg_z")) && layer < c->gat_nsum_valid.size()) c->gat_nsum_valid[layer] = 0;
    { int hrc = gat_edge_tensor_hook(c, layer, name, true); if (hrc) return hrc; }
    fused_note_write(c, t);
    const HaloPlan *wire = nullptr;
    { int prc = ghost_wire_plan(c, "tensor_upload", name, *t, &wire); if (prc) return prc; }
    ghost_wrote_fp32(t);   // (dory_halo_bf16_ghosts: the caller's fp32 rows are the current ones)
    return wire ? upload_ghost_wire(c, *t, host, *wire) : upload_dense(c, *t, host);
}

int dory_tensor_download(dory_ctx *c, uint32_t layer, const char *name, float *host) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *t = name ? find(c, layer, name) : nullptr;
    if (!t || !host) return fail(c, DORY_ERR_ARG, "tensor_download: no tensor '%s' at layer %u", name ? name : "(null)", layer);
    { int hrc = gat_edge_tensor_hook(c, layer, name, false); if (hrc) return hrc; }
    { int grc = ghost_fp32_current(c, t); if (grc) return grc; }   // (dory_halo_bf16_ghosts: a twin that alone is current is widened first)
    const HaloPlan *wire = nullptr;
    { int prc = ghost_wire_plan(c, "tensor_download", name, *t, &wire); if (prc) return prc; }
    return wire ? download_ghost_wire(c, *t, host, *wire) : download_dense(c, *t, host);
}

int dory_tensor_fill_uniform(dory_ctx *c, uint32_t layer, const char *name, uint64_t seed, float lo,
                             float hi, const uint32_t *global_row_ids) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *t = name ? find(c, layer, name) : nullptr;
    if (!t) return fail(c, DORY_ERR_ARG, "tensor_fill: no tensor '%s' at layer %u", name ? name : "(null)", layer);
    if (layer == 0) c->ah0_valid = false;
    // (as in dory_tensor_upload: the caller's values replace what the stages kept of the tensor)
    if (!strcmp(name, "A")) for (auto &f : c->gat_arow_valid) f = 0;
    if (!strcmp(name, "dA") && layer < c->gat_drow_valid.size()) c->gat_drow_valid[layer] = 0;
    if ((!strcmp(name, "z") || !strcmp(name, "fg_z")) && layer < c->gat_nsum_valid.size()) c->gat_nsum_valid[layer] = 0;
    { int hrc = gat_edge_tensor_hook(c, layer, name, true); if (hrc) return hrc; }
    fused_note_write(c, t);
    uint32_t *ids = nullptr;
    const HaloPlan *wire = nullptr;
    { int prc = ghost_wire_plan(c, "tensor_fill", name, *t, &wire); if (prc) return prc; }
    ghost_wrote_fp32(t);   // (dory_halo_bf16_ghosts: as dory_tensor_upload)
    if (wire) {   // option halo_direct_recv: stored row r is the caller's row order[r] -- it gets that row's values
        std::vector<uint32_t> wids(t->rows);
        for (uint64_t r = 0; r < t->rows; ++r) wids[r] = global_row_ids ? global_row_ids[wire->order[r]] : wire->order[r];
        int rc = upload_array(c, &ids, wids.data(), t->rows);
        if (rc) return rc;
    } else if (global_row_ids && t->rows) {
        int rc = upload_array(c, &ids, global_row_ids, t->rows);
        if (rc) return rc;
    }
    HIPCK(c, launch_fill_uniform_ids(t->d, t->rows, t->cols, t->ld, ids, seed, lo, hi, c->compute));
    HIPCK(c, hipStreamSynchronize(c->compute));
    if (ids) (void)hipFree(ids);
    return DORY_OK;
}

int dory_labels_upload(dory_ctx *c, const uint32_t *labels) {
    CHECK_CTX(c);
    if (!c->prealloc) return fail(c, DORY_ERR_ARG, "labels_upload: preallocate first");
    Tensor *t = find(c, c->L - 1, "lab");
    if (!t || (!labels && t->rows)) return fail(c, DORY_ERR_ARG, "labels_upload: bad arguments");
    for (uint64_t i = 0; i < t->rows; ++i)
        if (labels[i] >= t->cols) return fail(c, DORY_ERR_ARG, "label %u at row %llu exceeds %u classes", labels[i], (unsigned long long)i, t->cols);
    uint32_t *dl = nullptr;
    int rc = upload_array(c, &dl, labels, t->rows);
    if (rc) return rc;
    HIPCK(c, launch_onehot(t->d, t->rows, t->cols, t->ld, dl, c->compute));
    HIPCK(c, hipStreamSynchronize(c->compute));
    (void)hipFree(dl);
    return DORY_OK;
}

// ---------------------------------------------------------------------------------------
int dory_weight_set(dory_ctx *c, uint32_t layer, const char *name, const float *host) {
    CHECK_CTX(c);
    Tensor *t = name ? findw(c->weights, layer, name) : nullptr;
    if (!t || !host) return fail(c, DORY_ERR_ARG, "weight_set: no weight '%s' at layer %u", name ? name : "(null)", layer);
    return upload_dense(c, *t, host);
}
int dory_weight_get(dory_ctx *c, uint32_t layer, const char *name, float *host) {
    CHECK_CTX(c);
    Tensor *t = name ? findw(c->weights, layer, name) : nullptr;
    if (!t || !host) return fail(c, DORY_ERR_ARG, "weight_get: no weight '%s' at layer %u", name ? name : "(null)", layer);
    return download_dense(c, *t, host);
}
int dory_weight_grad_get(dory_ctx *c, uint32_t layer, const char *name, float *host) {
    CHECK_CTX(c);
    Tensor *t = name ? findw(c->wgrads, layer, name) : nullptr;
    if (!t || !host) return fail(c, DORY_ERR_ARG, "weight_grad_get: no gradient '%s' at layer %u", name ? name : "(null)", layer);
    return download_dense(c, *t, host);
}

int dory_weight_grad_set(dory_ctx *c, uint32_t layer, const char *name, const float *host) {
    CHECK_CTX(c);
    Tensor *t = name ? findw(c->wgrads, layer, name) : nullptr;
    if (!t || !host) return fail(c, DORY_ERR_ARG, "weight_grad_set: no gradient '%s' at layer %u", name ? name : "(null)", layer);
    return upload_dense(c, *t, host);
}

int dory_weights_init_xavier(dory_ctx *c) {
    CHECK_CTX(c);
    if (!c->prealloc) return fail(c, DORY_ERR_ARG, "weights_init: preallocate first");
    for (uint32_t l = 0; l < c->L; ++l) {
        // WeightServer::xavierInitializer (src/weight-server/weightserver.cpp:567-585):
        // every tensor restarts the engine at seed 8888.
        for (auto &kv : c->weights[l]) {
            Tensor &t = kv.second;
            const uint32_t d1 = (uint32_t)t.rows, d2 = t.cols;
            std::vector<float> w((size_t)d1 * d2);
            std::default_random_engine dre(8888);
            std::uniform_real_distribution<float> dist(-1, 1);
            for (auto &x : w) x = dist(dre);
            const float nf = std::sqrt(6.0 / (float(d1 + d2)));
            for (auto &x : w) x *= nf;
            int rc = upload_dense(c, t, w.data());
            if (rc) return rc;
        }
    }
    return DORY_OK;
}

// ---------------------------------------------------------------------------------------
int dory_ctx_describe(dory_ctx *c, int *gnn_type, uint32_t *num_layers, uint32_t *node_id, uint32_t *num_nodes,
                      uint32_t *local_vtx_cnt) {
    CHECK_CTX(c);
    if (!c->configured || !c->has_graph) return fail(c, DORY_ERR_ARG, "ctx_describe: configure and graph_upload first");
    if (gnn_type) *gnn_type = c->gnn;
    if (num_layers) *num_layers = c->L;
    if (node_id) *node_id = c->nodeId;
    if (num_nodes) *num_nodes = c->numNodes;
    if (local_vtx_cnt) *local_vtx_cnt = c->N;
    return DORY_OK;
}

int dory_timing_enable(dory_ctx *c, int on) {
    CHECK_CTX(c);
    drain_timing(c);
    c->timing = on != 0;
    return DORY_OK;
}
// the K1s gate words (dory_ctx::sweep_stat) on the host, for the keys that report them: reading synchronises the stream
static int read_sweep_stat(dory_ctx *c, const char *key, uint32_t (&st)[SWEEP_STAT_WORDS]) {
    if (c->capturing) return fail(c, DORY_ERR_ARG, "%s: not while an epoch graph is being recorded (reading synchronises the stream)", key);
    HIPCK(c, hipStreamSynchronize(c->compute));
    HIPCK(c, hipMemcpy(st, c->sweep_stat, sizeof(st), hipMemcpyDeviceToHost));
    return DORY_OK;
}
int dory_timing_get(dory_ctx *c, const char *family, double *total_ms, uint64_t *launches) {
    CHECK_CTX(c);
    if (!family) return DORY_ERR_ARG;
    if (!strcmp(family, "spmm_gate_timeouts")) {   // not a kernel family: launches = gate timeouts, total_ms = ungated launches
        uint32_t st[SWEEP_STAT_WORDS];
        if (int rc = read_sweep_stat(c, family, st)) return rc;
        if (total_ms) *total_ms = (double)st[2];
        if (launches) *launches = st[0];
        return DORY_OK;
    }
    drain_timing(c);
    auto it = c->times.find(family);
    if (total_ms) *total_ms = it == c->times.end() ? 0.0 : it->second.total_ms;
    if (launches) *launches = it == c->times.end() ? 0 : it->second.launches;
    return DORY_OK;
}
int dory_timing_reset(dory_ctx *c) {
    CHECK_CTX(c);
    drain_timing(c);
    c->times.clear();
    return DORY_OK;
}
int dory_transform_first_active(dory_ctx *c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!c->configured) return 0;
    for (uint32_t l = 0; l < c->L; ++l)
        if (tf_layer(c, l)) return 1;
    return 0;
}

int dory_transform_first_layer(dory_ctx *c, uint32_t layer) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    return c->configured && tf_layer(c, layer) ? 1 : 0;
}

int dory_get_option(dory_ctx *c, const char *key, int64_t *value) {
    CHECK_CTX(c);
    const int id = value ? option_find(key) : -1;
    if (id < 0) return fail(c, DORY_ERR_ARG, "unknown option '%s'", key ? key : "(null)");
    if (id < OPT_COUNT) { *value = c->opt[id]; return DORY_OK; }
    uint32_t st[SWEEP_STAT_WORDS];
    if (id == KEY_SPMM_GATES_REARM) {   // "is a back-off pending": the launch number is below a horizon
        if (int rc = read_sweep_stat(c, key, st)) return rc;
        *value = (st[4] < st[1] || st[4] < st[3]) ? 1 : 0;
        return DORY_OK;
    }
    switch ((ReadOnlyId)(id - OPT_COUNT)) {   // (no default: the compiler names a read-only key without a case)
    case RO_GCN_CACHE_AH0_SKIPS: *value = (int64_t)c->ah0_skips; break;
    case RO_GCN_BF16_GATHERS_K1S: *value = (int64_t)c->bf16_gathers_k1s; break;
    case RO_GCN_BF16_GATHERS_K1S_WIDE: *value = (int64_t)c->bf16_gathers_k1s_wide; break;
    case RO_GCN_BF16_GATHERS_K1: *value = (int64_t)c->bf16_gathers_k1; break;
    case RO_SPMM_LAUNCHES_K1S: *value = (int64_t)c->spmm_launches_k1s; break;
    case RO_SPMM_LAUNCHES_K1B: *value = (int64_t)c->spmm_launches_k1b; break;
    case RO_SPMM_LAUNCHES_K1: *value = (int64_t)c->spmm_launches_k1; break;
    case RO_GATMH_BF16_GATHERS_FWD: *value = (int64_t)c->gatmh_bf16_gathers_fwd; break;
    case RO_GATMH_BF16_GATHERS_SRC: *value = (int64_t)c->gatmh_bf16_gathers_src; break;
    case RO_GATMH_BF16_GATHERS_FWD_WIDE: *value = (int64_t)c->gatmh_bf16_gathers_fwd_wide; break;
    case RO_GATMH_BF16_GATHERS_SRC_WIDE: *value = (int64_t)c->gatmh_bf16_gathers_src_wide; break;
    case RO_HALO_ROWS_PACKED: *value = (int64_t)c->halo_rows_packed; break;
    case RO_HALO_FLOATS_PACKED: *value = (int64_t)c->halo_floats_packed; break;
    case RO_HALO_EXACT_PACKS: *value = (int64_t)c->halo_exact_packs; break;
    case RO_HALO_DIRECT_RECVS: *value = (int64_t)c->halo_direct_recvs; break;
    case RO_HALO_STAGED_RECVS: *value = (int64_t)c->halo_staged_recvs; break;
    case RO_HALO_RECV_BUF_BYTES: *value = (int64_t)c->recv_cap; break;
    case RO_EPOCH_GRAPH_RECORDED: *value = c->epoch_exec ? 1 : 0; break;
    case RO_SPMM_XCD_MAPPING_OK: *value = c->xcd_mapping_ok ? 1 : 0; break;
    case RO_SPMM_XCD_COUNT: *value = c->xcd_count; break;
    case RO_SPMM_XCD_POLICY: *value = c->xcd_policy; break;
    case RO_SPMM_XCD_GATED_US: *value = (int64_t)(c->xcd_gated_ms * 1e3f); break;
    case RO_SPMM_XCD_UNGATED_US: *value = (int64_t)(c->xcd_ungated_ms * 1e3f); break;
    case RO_SPMM_GATE_TIMEOUTS:
    case RO_SPMM_UNGATED_LAUNCHES:
        if (int rc = read_sweep_stat(c, key, st)) return rc;
        *value = id - OPT_COUNT == RO_SPMM_GATE_TIMEOUTS ? st[0] : st[2];
        break;
    case RO_COUNT: break;
    }
    return DORY_OK;
}

int dory_debug_occupy_cus(dory_ctx *c, uint32_t workgroups, uint64_t usec) {
    CHECK_CTX(c);
    if (usec > 2000000) return fail(c, DORY_ERR_ARG, "debug_occupy_cus: at most 2 s");
    HIPCK(c, launch_occupy_cus(workgroups, usec, c->comm));
    return DORY_OK;
}

int dory_set_option(dory_ctx *c, const char *key, int64_t value) {
    CHECK_CTX(c);
    const int id = option_find(key);
    if (id == KEY_SPMM_GATES_REARM) {   // write-only: end a K1s gate back-off now (both launch classes); the counters stay.
        // For a caller that has just changed what caused the timeouts (bench.py trying another spmm_sweep_reserve_cus).
        if (c->capturing) return fail(c, DORY_ERR_ARG, "spmm_gates_rearm: not while an epoch graph is being recorded (it synchronises the stream)");
        HIPCK(c, hipStreamSynchronize(c->compute));
        const uint32_t zero = 0;
        HIPCK(c, hipMemcpy(c->sweep_stat + 1, &zero, sizeof(zero), hipMemcpyHostToDevice));
        HIPCK(c, hipMemcpy(c->sweep_stat + 3, &zero, sizeof(zero), hipMemcpyHostToDevice));
        return DORY_OK;
    }
    if (id < 0 || id >= OPT_COUNT) return fail(c, DORY_ERR_ARG, "unknown option '%s'", key ? key : "(null)");
    char msg[256];
    if (option_check(id, value, c->gnn, c->configured, c->has_graph, msg, sizeof(msg))) return fail(c, DORY_ERR_ARG, "%s", msg);
    if (id == OPT_SPMM_SWEEP_CUS) {   // workgroups per sweep and XCD of K1s and the GAT sweeps (0: every CU of an XCD).  For several
        // contexts that SHARE a device (dory_comm_init_local: P ranks on one GPU): each takes its share of the CUs, so that
        // the ranks' gated sweeps are co-resident beside each other.  Before dory_graph_upload (the layouts are dealt for it).
        hipDeviceProp_t prop;
        HIPCK(c, hipGetDeviceProperties(&prop, c->device));
        const uint32_t all = (uint32_t)std::max(1, prop.multiProcessorCount / 8);
        if (value < 0 || value > (int64_t)all) return fail(c, DORY_ERR_ARG, "spmm_sweep_cus: 0..%u", all);
        c->cus_per_xcd = value == 0 ? all : (uint32_t)value;
    }
    c->opt[id] = value;
    // the copies the peers of the in-process transport read without this context's lock
    if (id == OPT_HALO_EXACT_ROWS) c->halo_exact.store((int)value, std::memory_order_release);
    if (id == OPT_HALO_DIRECT_RECV) c->halo_direct.store((int)value, std::memory_order_release);
    if (id == OPT_GCN_BF16_GATHER) c->gcn_bf16_mode.store((int)value, std::memory_order_release);   // (dory_halo_bf16_rows' rule)
    if (id == OPT_GATMH_BF16_GATHER) c->gatmh_bf16_mode_pub.store((int)value, std::memory_order_release);   // (dory_gatmh_halo_bf16's rule)
    c->ah0_valid = false;   // (another kernel variant sums in another order: a cached ah@0 is only kept across identical settings)
    return DORY_OK;
}

}  // extern "C"
