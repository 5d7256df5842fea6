// gat_mh_rows.hip -- the multi-head GAT's row-gather kernels WITH ghost rows: the family a partitioned dory_aggregate runs where
// neither the sweep layout (gat_mh_sweep.hip) nor the source-blocked layout (gat_mh_blocked.hip) applies -- more source windows or
// blocks than the layouts hold, ghost tensors past the 32-bit byte offsets of the sweep's buffer resources, a head shape neither
// family covers (D = 1, 2) -- and, with dory_gatmh_row_gather(ctx, 1), everywhere.  Written the way K1 (spmm_rows_body, spmm.hip) is
// written for GCN:
//
//   * one lane GROUP (8 / 16 / 32 / 64 lanes, by ld / 4) owns one row; every lane keeps ONE float4 of it (K*D <= 256: a wave always
//     covers a row), 256-thread workgroups, 16-byte loads;
//   * the group loads GROUP edge ids with one coalesced load and broadcasts them (bcast_u32<GROUP>); four gathered rows are in
//     flight per group (the source side with four heads per lane: two -- see gatmh_rows_src_kernel); the self edge is the last
//     entry of the id stream, and a row's tail is one masked batch, not single steps;
//   * an id s >= N selects row s - N of the ghost array (which may be null on a rank without ghosts); plain 64-bit addressing
//     throughout -- a ghost tensor of 14.7 GB is exactly what sends a partition here;
//   * nothing of size E x K is stored, no atomics (same input, same bits), no LDS, no gate, poll or inter-workgroup wait.
//
// Heads and lanes.  HPQ = heads per float4: 1 where D % 4 == 0 (the head's D / 4 lanes are reduced by DPP moves where a kernel
// needs a dot product: rows_allreduce) and for a single head of any width (K == 1: the whole group is the head); 2 for D == 2; 4 for D == 1 (heads
// inside a lane: no cross-lane step at all).  Columns past K*D are zero padding: they are masked out of every dot product and
// stored as zeros.
//
// Forward (in-edges, self edge last): ONE pass with online rescaling -- the running maximum moves once per batch of four edges, so
// a batch costs five exponentials per head, not eight; the two-pass form (scores first, as gatmh_forward_kernel) would gather every
// el row twice and was not built.  The sources' scores are formed from the gathered rows (rows_el: the el tensor's bits, without
// a second 128-byte line per edge); every lane of a head carries the head's (m, den, den+) itself.  It writes o, m, den and op,
// dpos (the positive-branch part of o and of the attention mass, self edge on its branch: gatmh_forward_redo_body's definition).
// m is the row's TRUE maximum per head, as in the blocked forms.
// Backward, destination side (in-edges): where the forward left op / dpos and launch_gatmh_dst_rowwise covers the shape that
// kernel runs (abi_stages.hip) -- no edges; otherwise gatmh_rows_dst_kernel: gatmh_backward_dst_kernel's arithmetic per edge.
// Backward, source side (out-edges; destinations local or ghost: do / bg_do, st / bg_st): the form without dot products,
//     del = <Z_u, 0.2 S + 0.8 S+> - (0.2 T + 0.8 T+),   dz = S + del a_l + der a_r      (sums of gatmh_src_finish_body)
// one reduction per row instead of one per edge.
//
// bf16 rows (dory_gatmh_row_gather_bf16 + option gatmh_bf16_gather; gatmh_rows_{forward,dst,src}_bf16_kernel): the family is bound by
// HBM bytes, and a gathered row chunk becomes ONE 8-byte load of four bf16 from the context's shadow rows, widened exactly
// (row_chunk) -- a 64-float row is one 128-byte line read by 16 lanes.  Geometry, rows in flight, ghost addressing and every fp32
// operation after the load are the fp32 kernels': each pass is one __device__ body over the chunk type, so a bf16 kernel gives its
// sibling's bits on rows rounded beforehand.  The forward and the edge pass gather z / fg_z (scores from the ROUNDED row where ELFLY
// holds; el / fg_el from the tensors elsewhere), the source side do / bg_do; records, el[u], the closing z[u], der, a_l, a_r stay
// fp32.  Known consequence: with ELFLY the forward's m / den come from scores of rounded rows while the source side takes el[u]
// from the fp32 tensor -- its alpha differs from the forward's by the rounding of a score (include/dorylus_hip.h).
//
// Hub splitting (dory_gatmh_row_gather_hub_split(ctx, chunk); the *_hub_kernel / *_merge_kernel below).  A row's entries are walked by
// its one lane group, four rows at a time: a destination with tens of thousands of in-edges is one serial chain.  With a chunk size
// set, a row with MORE than `chunk` adjacency entries (edges; the self edge is not counted) is a hub row: the adjacency's plan
// (row_chunks.hpp) cuts its entries into consecutive chunks of `chunk`, the last one shorter, and the self edge -- the last entry of
// the id stream -- goes with the last chunk.  A split pass is two launches.  The first covers nchunks + N units: the chunk units
// come first (the long work starts first), one lane group each, running the UNCHANGED per-entry arithmetic over their range and
// leaving their state in a scratch slot; the row units follow and skip the hub rows -- every other row is computed by the
// same body as without the feature, so it keeps its bits.  The second runs one lane group per hub row and folds the row's chunk states
// in chunk order, then closes with the one-pass epilogue:
//   forward   state (m_c, den_c, den+_c, acc_c, acc+_c), unnormalised;  M = max_c m_c;  f_c = exp(m_c - M);  den = sum_c f_c den_c
//             (likewise den+, acc, acc+), then o = acc / den, op = acc+ / den, m = M (the row's TRUE maximum, exact), den, dpos = den+ / den
//   dst       state (t_c, a1_c, a2_c) against the row's m / den: plain sums;  t, der = a1 - t a2, st = (er, m, 1 / den, t)
//   src       state (S_c, S+_c, T_c, T+_c): plain sums, then del and dz as in the one-pass form
// No atomics (chunk order is fixed: same input, same bits), no LDS, no gate or wait; 64-bit addressing; ghost ids as everywhere here.
// A row that is split does NOT keep its one-pass bits (other association of the sums) except m.  With no hub row in the plan the
// launchers launch exactly the kernels they launched before.  Measured (profiles/r28_gatmh_row_gather_hubs.txt): rank 0 of 8 of an
// Amazon-size R-MAT graph, largest degree 101 152 -- 24-35 ms a pass one-pass, x0.05-0.15 of that at chunk 1 024; a uniform rank unchanged.
//
// Interior rows beside the exchange (dory_gatmh_row_gather_overlap; the *_list_kernel forms below).  The kernels read ghost rows through
// plain pointers, so a pass used to wait for the exchange before it launched anything.  A row whose every entry is local (row_chunks.hpp:
// plan_row_interior) reads no ghost row.  With the switch on, the forward and the source side run as two launches of a list form -- the
// body with its row units named by a list (unit i = row list[i], rows packed densely into lane groups: no all-N launch that skips rows
// by flag, the family is latency-bound and a wave with one live group of four loses its rows in flight): first the interior rows, then
// -- after the wait for the ghost rows -- the hub rows' chunks, if any, and all other rows, with the merge launch as ever.  There is a
// list form of the one-pass kernel and one of the hub kernel (taken where the chunk plan has chunks): the compiler contracts the closing
// arithmetic of the two differently at four heads per lane, and a listed row has to have the code it has with the switch off.  A row the chunk plan cuts goes whole to the second launch.  Every row is computed whole by the body that
// computes it in the all-N launch, so every bit stays.  The one-pass, hub and merge kernels are untouched instruction for instruction
// (the list is a template parameter of RowsWork and a kernel argument of the list kernels alone).  The destination-side edge pass reads
// fg_z, which landed during the forward: no exchange to hide behind, no list form.  Its measurement: tools/gatmh_row_gather_overlap_rate.py.
//
// Local entries beside the exchange (dory_gatmh_row_gather_edge_split; the *_carry_kernel forms below).  On a rank of 8 of a community
// graph 98 % of the rows have a ghost entry and 85 % of the entries are local: the row lists above hide next to nothing there.  The
// carry kernels walk a row as two ranges of a local-first copy of the ids (row_chunks.hpp: plan_row_edge_split) -- A: the local entries,
// then the self edge (a local row: with the part that does not wait); B: the ghost entries -- each with its own masked tail batch, the
// per-entry arithmetic (the state structs' step) unchanged.  Which ranges a launch walks is a kernel ARGUMENT (RowsCarryArgs::walk):
// both (state in registers), first (A; a row with ghost entries parks its state in its slot, any other closes), second (the boundary
// rows, packed densely: state loaded, B, the one-pass epilogue).  One body of machine code for the three walks: one launch and two
// launches give the same bits by construction -- two kernels instantiated from one body need not (the list forms above).  Against the
// one-pass kernels only m keeps its bits: the ghost entries move behind the local ones and the self edge between them.  fp32 and narrow
// bf16, the forms the launchers select for the one-pass kernels; no hub form (a plan with chunks keeps the pass as it was), no wide form.
//
// The wide (16-byte) bf16 form (dory_gatmh_row_gather_bf16_wide): the gatmh_rows8_*_kernel section below.
#include "gat_mh.hpp"
#include "spmm_common.hpp"

namespace dory {

// what a lane knows of its place: row, float4 column, the heads of its float4 (clamped: loads stay in bounds), which of its four
// columns hold features
template <int GROUP, int HPQ>
struct RowsLane {
    uint32_t v, nchunk, col, li;
    bool row_ok, lane_ok;
    uint32_t hk[HPQ];
    bool cm[4];
    // rid: the group's row where ok holds (a launch's units: rows_unit; a hub launch names rows through its plan)
    __device__ __forceinline__ RowsLane(const GatMhArgs &a, uint32_t rid, bool ok) {
        li = (uint32_t)((threadIdx.x & 63) % GROUP);
        row_ok = ok;
        v = row_ok ? rid : 0;
        if constexpr (GROUP == 64) v = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);   // one row per wave: scalar row base
        nchunk = a.ld >> 2;
        const uint32_t KD = a.K * a.D;
        lane_ok = row_ok && li < nchunk && 4 * li < KD;
        col = li < nchunk ? li : 0;           // lanes past the row gather column 0 (valid memory) and never store
#pragma unroll
        for (int s = 0; s < HPQ; ++s) hk[s] = min((4 * col) / a.D + (uint32_t)s, a.K - 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) cm[c] = lane_ok && 4 * col + c < KD;
    }
    // the lane that stores a head's per-(v,k) values (HPQ == 1); with HPQ > 1 every lane stores its own heads (head_live)
    __device__ __forceinline__ bool leader(const GatMhArgs &a) const {
        return lane_ok && (a.K == 1 ? li == 0 : (col % (a.D >> 2)) == 0);
    }
    __device__ __forceinline__ bool head_live(const GatMhArgs &a, int s) const { return lane_ok && (4 * col) / a.D + (uint32_t)s < a.K; }
};
// the unit of a launch a lane group works on: 4 waves of 64 / GROUP groups per workgroup
template <int GROUP>
__device__ __forceinline__ uint32_t rows_unit() {
    constexpr int RPW = 64 / GROUP, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return blockIdx.x * RPB + wave * RPW + lane / GROUP;
}
// the hub rows of a launch (GatmhHubs, ctx.hpp): nchunks chunk records of 6 words (row, 1 on the row's last chunk, e0, e1 as lo / hi),
// nrows rows with their first chunks, and the chunk states -- one slot of rows_hub_stride floats per chunk
struct RowsHubArgs {
    uint32_t nchunks, nrows, chunk;
    const uint32_t *chunks, *rows, *row_chunk_ptr;
    float *state;
};
// floats of a chunk's slot: two rows of ld (16-byte aligned) and the per-head values in runs of ldk
__host__ __device__ __forceinline__ size_t rows_hub_stride(int pass, uint32_t ld, uint32_t ldk) {
    return ((size_t)(pass == 1 ? 0 : 2) * ld + (size_t)(pass == 0 ? 3 : pass == 1 ? 3 : 2) * ldk + 3) & ~(size_t)3;
}
// dory_gatmh_row_gather_overlap: the rows of a launch named by a list -- unit i is row rows[i], n units (the interior rows beside
// an exchange, the boundary rows after it: Adjacency::rows_split)
struct RowsListArgs {
    const uint32_t *rows;
    uint32_t n;
};
// dory_gatmh_row_gather_edge_split: what a carry launch walks of every row.  a.idx is the adjacency's local-first copy (row_chunks.hpp:
// plan_row_edge_split), mid[v] the position of row v's first ghost entry.  Range A = [ptr[v], mid[v]) and then the self edge (a local
// row: it goes with the part that does not wait), range B = [mid[v], ptr[v + 1]).  walk BOTH: units = all N rows, A then B, the state in
// registers; FIRST: all N rows, A alone -- a row with an empty B closes, any other leaves its state in slot v of `state`
// (rows_hub_stride floats a slot); SECOND: units = the n boundary rows `rows` names, packed densely -- state loaded, B, closed.
enum { ROWS_WALK_BOTH = 0, ROWS_WALK_FIRST = 1, ROWS_WALK_SECOND = 2 };
struct RowsCarryArgs {
    const uint64_t *mid;
    const uint32_t *rows;
    uint32_t n;
    float *state;
    int walk;
};
// What a lane group of a launch does.  HUBS false: row = unit, all of it.  HUBS true: the first H.nchunks units are the chunks of the
// hub rows (part: a range of the row's entries, the self edge with the last), the rest the rows, of which the hub rows are skipped.
// LIST: the row units are the R.n rows R.rows names, packed densely, not all N (with HUBS: after the chunk units).
template <int GROUP, bool HUBS, bool LIST>
struct RowsWork {
    uint32_t row, slot;
    bool ok, part, self;
    uint64_t ce0, cend;
    __device__ __forceinline__ RowsWork(const GatMhArgs &a, const RowsHubArgs &H, const RowsListArgs &R) {
        uint32_t unit = rows_unit<GROUP>();
        part = false; self = true; slot = 0; ce0 = cend = 0;
        if constexpr (HUBS) {
            part = unit < H.nchunks;
            if (part) {
                const uint32_t *w = H.chunks + (size_t)6 * unit;
                slot = unit; row = w[0]; ok = true; self = w[1] != 0;
                ce0 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
                cend = (uint64_t)w[4] | ((uint64_t)w[5] << 32);
            } else unit -= H.nchunks;
        }
        if constexpr (LIST) {
            if (!part) { ok = unit < R.n; row = ok ? R.rows[unit] : 0; }
        } else if (!part) { ok = unit < a.N; row = ok ? unit : 0; }
    }
    // the group's entries: [e0, end) of idx, then -- total counts it -- the self edge; false: nothing to walk and nothing to store
    template <class LANE>
    __device__ __forceinline__ bool entries(const GatMhArgs &a, const LANE &L, const RowsHubArgs &H, uint64_t &e0, uint64_t &end,
                                            uint64_t &total) const {
        if constexpr (HUBS)
            if (part) { e0 = ce0; end = cend; total = cend - ce0 + (self ? 1 : 0); return true; }
        e0 = L.row_ok ? a.ptr[L.v] : 0; end = L.row_ok ? a.ptr[L.v + 1] : 0;
        bool live = L.row_ok;
        if constexpr (HUBS) live = live && end - e0 <= (uint64_t)H.chunk;     // (a hub row: its chunks and the merge kernel do it)
        total = live ? end - e0 + 1 : 0;
        return live;
    }
};
template <int HPQ> __device__ __forceinline__ constexpr int rows_slot(int c) { return c * HPQ / 4; }   // the head slot of column c

__device__ __forceinline__ float4 rows_mask(const float4 &x, const bool (&cm)[4]) {
    return make_float4(cm[0] ? x.x : 0.f, cm[1] ? x.y : 0.f, cm[2] ? x.z : 0.f, cm[3] ? x.w : 0.f);
}
// per-slot dot product of two float4 (the caller has masked one of them)
template <int HPQ>
__device__ __forceinline__ void rows_dot(const float4 &g, const float4 &x, float (&p)[HPQ]) {
    if constexpr (HPQ == 1) p[0] = fmaf(g.x, x.x, fmaf(g.y, x.y, fmaf(g.z, x.z, g.w * x.w)));
    else if constexpr (HPQ == 2) { p[0] = fmaf(g.x, x.x, g.y * x.y); p[1] = fmaf(g.z, x.z, g.w * x.w); }
    else { p[0] = g.x * x.x; p[1] = g.y * x.y; p[2] = g.z * x.z; p[3] = g.w * x.w; }
}
// acc += w[slot(c)] * x[c]
template <int HPQ>
__device__ __forceinline__ float4 rows_axpy(const float (&w)[HPQ], const float4 &x, float4 acc) {
    acc.x = fmaf(w[rows_slot<HPQ>(0)], x.x, acc.x);
    acc.y = fmaf(w[rows_slot<HPQ>(1)], x.y, acc.y);
    acc.z = fmaf(w[rows_slot<HPQ>(2)], x.z, acc.z);
    acc.w = fmaf(w[rows_slot<HPQ>(3)], x.w, acc.w);
    return acc;
}
template <int HPQ>
__device__ __forceinline__ float4 rows_scale(const float (&w)[HPQ], const float4 &x) {
    return make_float4(w[rows_slot<HPQ>(0)] * x.x, w[rows_slot<HPQ>(1)] * x.y, w[rows_slot<HPQ>(2)] * x.z, w[rows_slot<HPQ>(3)] * x.w);
}

// sum over the HL lanes of a head (a power of two, aligned), result in every lane: DPP inside the VALU up to a row of 16 lanes
// (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: after the quad steps all lanes of a quad agree, so a mirror hands
// over the other half's sum), xor shuffles beyond -- the additions of a butterfly over offsets 1, 2, 4, ... in that order
__device__ __forceinline__ float rows_allreduce(float v, int HL) {
    if (HL > 1) v += dpp_mov<0xB1>(v);
    if (HL > 2) v += dpp_mov<0x4E>(v);
    if (HL > 4) v += dpp_mov<0x141>(v);
    if (HL > 8) v += dpp_mov<0x140>(v);
    if (HL > 16) v += __shfl_xor(v, 16, 64);
    if (HL > 32) v += __shfl_xor(v, 32, 64);
    return v;
}
// ELFLY: the source's scores el[u,k] = <Z[u,k,:], a_l[k,:]> formed from the gathered row instead of gathered from el / fg_el -- an
// el row is a 128-byte line of its own per edge, half as much again as a 64-float row.  The arithmetic is launch_gatmh_scores's,
// operation for operation (a float4's four fmaf in column order from zero, then the butterfly over the head's lanes; heads inside
// a lane: the scalar kernel's chain), so the value is the el tensor's to the bit and the backward passes, which read the tensor,
// see the same alpha.  Rows whose float4 count is no power of two (ld = 96, 160, 192, 224) get their scores from the scalar
// kernel's chain over D columns: those shapes (one head per float4 only) gather el as before.  al: a_l's four columns, padding zeroed.
template <int HPQ>
__device__ __forceinline__ void rows_el(const float4 &x, const float4 &al, int HL, float (&sc)[HPQ]) {
    if constexpr (HPQ == 1) sc[0] = rows_allreduce(fmaf(x.w, al.w, fmaf(x.z, al.z, fmaf(x.y, al.y, fmaf(x.x, al.x, 0.f)))), HL);
    else if constexpr (HPQ == 2) { sc[0] = fmaf(x.y, al.y, fmaf(x.x, al.x, 0.f)); sc[1] = fmaf(x.w, al.w, fmaf(x.z, al.z, 0.f)); }
    else { sc[0] = fmaf(x.x, al.x, 0.f); sc[1] = fmaf(x.y, al.y, 0.f); sc[2] = fmaf(x.z, al.z, 0.f); sc[3] = fmaf(x.w, al.w, 0.f); }
}
template <int GROUP, int HPQ>
__device__ __forceinline__ float4 rows_attn4(const RowsLane<GROUP, HPQ> &L, const GatMhArgs &a, const float *a_l) {
    const uint32_t KD = a.K * a.D;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = L.cm[c] ? a_l[min(4 * L.col + c, KD - 1)] : 0.f;
    return make_float4(v[0], v[1], v[2], v[3]);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// W: float4s per lane -- 1, or 2 in the wide bf16 form (gatmh_rows8_*_kernel below: a lane stands for two lanes of this form and
// keeps the second one's float4 in the *1 members, x[NB + u] beside x[u]; everything of it is behind `if constexpr (W == 2)`)
// the wide form's in-lane addition of its two float4s' dot-product chains: the butterfly's offset-1 step, kept off any contraction
// with the chains' own operations (the narrow form adds after a DPP move)
__device__ __forceinline__ float rows8_add(float x, float y) {
#pragma clang fp contract(off)
    return x + y;
}
template <int HPQ, int W = 1>
struct RowsFwdState {
    float erv[HPQ], mx[HPQ], den[HPQ], denp[HPQ];
    float4 acc, accp;
    float4 acc1, accp1;   // (W == 2)
    // NB edges at once: the maximum moves once, the sums are rescaled once
    template <int NB>
    __device__ __forceinline__ void step(const float4 (&x)[NB * W], const float (&sc)[NB][HPQ]) {
        float al[NB][HPQ], alp[NB][HPQ], f[HPQ];
#pragma unroll
        for (int s = 0; s < HPQ; ++s) {
            float pre[NB], sv[NB], mn = mx[s];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                pre[u] = sc[u][s] + erv[s];
                sv[u] = lrelu02(pre[u]);
                mn = fmaxf(mn, sv[u]);
            }
            f[s] = __expf(mx[s] - mn);            // (exp(-inf) = 0 on the first batch)
            float d = den[s] * f[s], dp = denp[s] * f[s];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                al[u][s] = __expf(sv[u] - mn);
                alp[u][s] = pre[u] > 0.f ? al[u][s] : 0.f;
                d += al[u][s];
                dp += alp[u][s];
            }
            den[s] = d; denp[s] = dp; mx[s] = mn;
        }
        acc = rows_scale<HPQ>(f, acc);
        accp = rows_scale<HPQ>(f, accp);
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            acc = rows_axpy<HPQ>(al[u], x[u], acc);
            accp = rows_axpy<HPQ>(alp[u], x[u], accp);
        }
        if constexpr (W == 2) {
            acc1 = rows_scale<HPQ>(f, acc1);
            accp1 = rows_scale<HPQ>(f, accp1);
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                acc1 = rows_axpy<HPQ>(al[u], x[NB + u], acc1);
                accp1 = rows_axpy<HPQ>(alp[u], x[NB + u], accp1);
            }
        }
    }
};

// the one-pass epilogue: normalise and store o, op, m, den, dpos of row L.v (also the hub rows' merge kernel's)
template <int GROUP, int HPQ, int W>
__device__ __forceinline__ void rows_fwd_store(const RowsLane<GROUP, HPQ> &L, const GatMhArgs &a, const RowsFwdState<HPQ, W> &S, float *o, float *op,
                                               float *m_out, float *den_out, float *dpos_out) {
    if (!L.lane_ok) return;
    float idn[HPQ];
#pragma unroll
    for (int s = 0; s < HPQ; ++s) idn[s] = 1.f / S.den[s];
    const size_t oi = (size_t)L.v * L.nchunk + L.col;
    reinterpret_cast<float4 *>(o)[oi] = rows_mask(rows_scale<HPQ>(idn, S.acc), L.cm);
    reinterpret_cast<float4 *>(op)[oi] = rows_mask(rows_scale<HPQ>(idn, S.accp), L.cm);
#pragma unroll
    for (int s = 0; s < HPQ; ++s)
        if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) {
            const size_t vk = (size_t)L.v * a.ldk + L.hk[s];
            m_out[vk] = S.mx[s];
            den_out[vk] = S.den[s];
            dpos_out[vk] = S.denp[s] * idn[s];
        }
}

// CHUNK: what a lane gathers of a row -- float4 (fp32 rows), or uint2 (four bf16 of the shadow rows, launch_bf16_rows, widened
// exactly by row_chunk).  Everything after the load is the same arithmetic in the same order, so a bf16 kernel gives its fp32
// sibling's bits on rows that were rounded beforehand; the bodies below are shared by both, the __global__ kernels only name them.
template <int GROUP, int HPQ, bool ELFLY, bool HUBS, bool LIST, class CHUNK>
__device__ __forceinline__ void gatmh_rows_forward_body(const GatMhArgs &a, int HL, const CHUNK *z4, const CHUNK *zg4, const float *el,
                                                        const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                        float *m_out, float *den_out, float *dpos_out, const RowsHubArgs &H,
                                                        const RowsListArgs &R = RowsListArgs{}) {
    const RowsWork<GROUP, HUBS, LIST> W(a, H, R);
    const RowsLane<GROUP, HPQ> L(a, W.row, W.ok);
    const float4 al4 = ELFLY ? rows_attn4(L, a, a_l) : make_float4(0.f, 0.f, 0.f, 0.f);
    RowsFwdState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        S.erv[s] = er[(size_t)L.v * a.ldk + L.hk[s]];
        S.mx[s] = -INFINITY;
        S.den[s] = S.denp[s] = 0.f;
    }
    S.acc = S.accp = make_float4(0.f, 0.f, 0.f, 0.f);
    // the row's entries: its in-edges, then the self edge (id v, a local row like any other); batches of four, the dead slots of the
    // last batch gather the last entry's row again and are masked by a score of -inf (alpha = exp(-inf) = 0)
    uint64_t e0, end, total;
    const bool live = W.entries(a, L, H, e0, end, total);
    for (uint64_t done = 0; done < total; done += GROUP) {                     // GROUP == 64: wave-uniform
        const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
        const uint64_t ee = e0 + done + L.li;
        const uint32_t my_idx = ee < end ? a.idx[ee] : L.v;
        for (int j = 0; j < n; j += 4) {
            float4 x[4];
            float sc[4][HPQ];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                const bool loc = s < a.N;
                const size_t r = loc ? s : s - a.N;
                x[u] = row_chunk((loc ? z4 : zg4)[r * L.nchunk + L.col]);
                if constexpr (!ELFLY) {
                    const float *ep = (loc ? el : elg) + r * a.ldk;
#pragma unroll
                    for (int h = 0; h < HPQ; ++h) sc[u][h] = ep[L.hk[h]];
                }
            }
            if constexpr (ELFLY)
#pragma unroll
                for (int u = 0; u < 4; ++u) rows_el<HPQ>(x[u], al4, HL, sc[u]);
#pragma unroll
            for (int u = 1; u < 4; ++u)
#pragma unroll
                for (int h = 0; h < HPQ; ++h) sc[u][h] = j + u < n ? sc[u][h] : -INFINITY;
            S.template step<4>(x, sc);
        }
    }
    if (!live) return;
    if constexpr (HUBS)
        if (W.part) {   // a chunk of a hub row: its unnormalised state, for gatmh_rows_forward_merge_kernel
            if (L.li >= L.nchunk) return;
            float *sp = H.state + (size_t)W.slot * rows_hub_stride(0, a.ld, a.ldk), *hp = sp + 2 * (size_t)a.ld;
            reinterpret_cast<float4 *>(sp)[L.col] = S.acc;
            reinterpret_cast<float4 *>(sp + a.ld)[L.col] = S.accp;
#pragma unroll
            for (int s = 0; s < HPQ; ++s)
                if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) {
                    hp[L.hk[s]] = S.mx[s];
                    hp[a.ldk + L.hk[s]] = S.den[s];
                    hp[2 * a.ldk + L.hk[s]] = S.denp[s];
                }
            return;
        }
    rows_fwd_store(L, a, S, o, op, m_out, den_out, dpos_out);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_kernel(GatMhArgs a, int HL, const float *z, const float *zg, const float *el,
                                                                 const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                                 float *m_out, float *den_out, float *dpos_out) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, false, false>(a, HL, reinterpret_cast<const float4 *>(z), reinterpret_cast<const float4 *>(zg), el, elg, er,
                                                      a_l, o, op, m_out, den_out, dpos_out, RowsHubArgs{});
}
// the launch of a split pass: the hub rows' chunks, then the rows that are no hub rows (RowsWork)
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_hub_kernel(GatMhArgs a, int HL, const float *z, const float *zg, const float *el,
                                                                     const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                                     float *m_out, float *den_out, float *dpos_out, RowsHubArgs H) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, true, false>(a, HL, reinterpret_cast<const float4 *>(z), reinterpret_cast<const float4 *>(zg), el, elg, er,
                                                     a_l, o, op, m_out, den_out, dpos_out, H);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_hub_bf16_kernel(GatMhArgs a, int HL, const uint2 *zb, const uint2 *zgb, const float *el,
                                                                          const float *elg, const float *er, const float *a_l, float *o,
                                                                          float *op, float *m_out, float *den_out, float *dpos_out,
                                                                          RowsHubArgs H) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, true, false>(a, HL, zb, zgb, el, elg, er, a_l, o, op, m_out, den_out, dpos_out, H);
}
// one lane group per hub row: the chunk states folded in chunk order against the maximum of the chunk maxima (exp(m_c - M) <= 1: chunks
// whose maxima lie far apart merge to a factor of zero, never to Inf or NaN -- every chunk has an entry, so every m_c is finite)
template <int GROUP, int HPQ>
__global__ __launch_bounds__(256) void gatmh_rows_forward_merge_kernel(GatMhArgs a, float *o, float *op, float *m_out, float *den_out,
                                                                       float *dpos_out, RowsHubArgs H) {
    const uint32_t h = rows_unit<GROUP>();
    const bool ok = h < H.nrows;
    const RowsLane<GROUP, HPQ> L(a, ok ? H.rows[h] : 0, ok);
    if (!L.row_ok) return;
    const uint32_t c0 = H.row_chunk_ptr[h], c1 = H.row_chunk_ptr[h + 1];
    const size_t stride = rows_hub_stride(0, a.ld, a.ldk);
    RowsFwdState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        S.mx[s] = -INFINITY;
        S.den[s] = S.denp[s] = 0.f;
    }
    S.acc = S.accp = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t c = c0; c < c1; ++c)
#pragma unroll
        for (int s = 0; s < HPQ; ++s) S.mx[s] = fmaxf(S.mx[s], H.state[c * stride + 2 * (size_t)a.ld + L.hk[s]]);
    for (uint32_t c = c0; c < c1; ++c) {
        const float *sp = H.state + c * stride, *hp = sp + 2 * (size_t)a.ld;
        float f[HPQ];
#pragma unroll
        for (int s = 0; s < HPQ; ++s) {
            f[s] = __expf(hp[L.hk[s]] - S.mx[s]);
            S.den[s] = fmaf(f[s], hp[a.ldk + L.hk[s]], S.den[s]);
            S.denp[s] = fmaf(f[s], hp[2 * a.ldk + L.hk[s]], S.denp[s]);
        }
        S.acc = rows_axpy<HPQ>(f, reinterpret_cast<const float4 *>(sp)[L.col], S.acc);
        S.accp = rows_axpy<HPQ>(f, reinterpret_cast<const float4 *>(sp + a.ld)[L.col], S.accp);
    }
    rows_fwd_store(L, a, S, o, op, m_out, den_out, dpos_out);
}
// zb / zgb: the shadow rows of z / fg_z (ld bf16 per row, one 8-byte load per lane and edge: a 64-float row is one 128-byte line).
// Where ELFLY holds the sources' scores come from the gathered, rounded row -- what the sibling does when handed rounded rows;
// elsewhere el / elg are gathered from the fp32 tensors as before
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_bf16_kernel(GatMhArgs a, int HL, const uint2 *zb, const uint2 *zgb, const float *el,
                                                                      const float *elg, const float *er, const float *a_l, float *o,
                                                                      float *op, float *m_out, float *den_out, float *dpos_out) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, false, false>(a, HL, zb, zgb, el, elg, er, a_l, o, op, m_out, den_out, dpos_out, RowsHubArgs{});
}
// dory_gatmh_row_gather_overlap: the rows of a list -- the interior rows of the in-edges beside the exchange (they read z / the local
// shadow rows alone), the boundary rows after it; every row by the body above.  Two forms, so that a listed row has the code of the
// kernel that computes it with the switch off: *_list_kernel is the one-pass kernel over listed rows, *_list_hub_kernel the hub kernel
// (the hub rows' chunk units first) over listed rows, taken where the adjacency's chunk plan has chunks.
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_list_kernel(GatMhArgs a, int HL, const float *z, const float *zg, const float *el,
                                                                      const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                                      float *m_out, float *den_out, float *dpos_out, RowsListArgs R) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, false, true>(a, HL, reinterpret_cast<const float4 *>(z), reinterpret_cast<const float4 *>(zg), el, elg,
                                                            er, a_l, o, op, m_out, den_out, dpos_out, RowsHubArgs{}, R);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_list_bf16_kernel(GatMhArgs a, int HL, const uint2 *zb, const uint2 *zgb, const float *el,
                                                                           const float *elg, const float *er, const float *a_l, float *o,
                                                                           float *op, float *m_out, float *den_out, float *dpos_out,
                                                                           RowsListArgs R) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, false, true>(a, HL, zb, zgb, el, elg, er, a_l, o, op, m_out, den_out, dpos_out, RowsHubArgs{}, R);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_list_hub_kernel(GatMhArgs a, int HL, const float *z, const float *zg, const float *el,
                                                                          const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                                          float *m_out, float *den_out, float *dpos_out, RowsHubArgs H,
                                                                          RowsListArgs R) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, true, true>(a, HL, reinterpret_cast<const float4 *>(z), reinterpret_cast<const float4 *>(zg), el, elg,
                                                           er, a_l, o, op, m_out, den_out, dpos_out, H, R);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_list_hub_bf16_kernel(GatMhArgs a, int HL, const uint2 *zb, const uint2 *zgb, const float *el,
                                                                               const float *elg, const float *er, const float *a_l, float *o,
                                                                               float *op, float *m_out, float *den_out, float *dpos_out,
                                                                               RowsHubArgs H, RowsListArgs R) {
    gatmh_rows_forward_body<GROUP, HPQ, ELFLY, true, true>(a, HL, zb, zgb, el, elg, er, a_l, o, op, m_out, den_out, dpos_out, H, R);
}
// dory_gatmh_row_gather_edge_split: the carry form -- a row walked as two ranges of the local-first ids (a.idx; C.mid), its state parked
// between them where the launch says so (RowsCarryArgs::walk: a runtime value, one body of machine code for the three walks).  The
// batches, the masked tail of each range, the gathers and S.step are the one-pass body's; the epilogue is rows_fwd_store.
template <int GROUP, int HPQ, bool ELFLY, class CHUNK>
__device__ __forceinline__ void gatmh_rows_forward_carry_body(const GatMhArgs &a, int HL, const CHUNK *z4, const CHUNK *zg4, const float *el,
                                                              const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                              float *m_out, float *den_out, float *dpos_out, const RowsCarryArgs &C) {
    const uint32_t unit = rows_unit<GROUP>();
    const bool second = C.walk == ROWS_WALK_SECOND;
    const bool ok = unit < (second ? C.n : a.N);
    const RowsLane<GROUP, HPQ> L(a, ok ? (second ? C.rows[unit] : unit) : 0, ok);
    const float4 al4 = ELFLY ? rows_attn4(L, a, a_l) : make_float4(0.f, 0.f, 0.f, 0.f);
    RowsFwdState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        S.erv[s] = er[(size_t)L.v * a.ldk + L.hk[s]];
        S.mx[s] = -INFINITY;
        S.den[s] = S.denp[s] = 0.f;
    }
    S.acc = S.accp = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint64_t p0 = L.row_ok ? a.ptr[L.v] : 0, p1 = L.row_ok ? a.ptr[L.v + 1] : 0, md = L.row_ok ? C.mid[L.v] : 0;
    // the row's slot (one per row): two rows of ld, then (m, den, den+) in runs of ldk -- the layout of a hub chunk's state
    float *sp = C.state + (size_t)L.v * rows_hub_stride(0, a.ld, a.ldk), *hp = sp + 2 * (size_t)a.ld;
    if (second && L.row_ok) {   // (every lane takes its column and its heads: what it held when range A ended -- a head's lanes agree)
        S.acc = reinterpret_cast<const float4 *>(sp)[L.col];
        S.accp = reinterpret_cast<const float4 *>(sp + a.ld)[L.col];
#pragma unroll
        for (int s = 0; s < HPQ; ++s) {
            S.mx[s] = hp[L.hk[s]];
            S.den[s] = hp[a.ldk + L.hk[s]];
            S.denp[s] = hp[2 * a.ldk + L.hk[s]];
        }
    }
    // range A: the local entries, then the self edge; range B: the ghost entries.  Each ends with its own masked batch
    const int r1 = C.walk == ROWS_WALK_FIRST ? 1 : 2;
    for (int r = second ? 1 : 0; r < r1; ++r) {
        const uint64_t e0 = r ? md : p0, end = r ? p1 : md;
        const uint64_t total = L.row_ok ? end - e0 + (r ? 0 : 1) : 0;
        for (uint64_t done = 0; done < total; done += GROUP) {                     // GROUP == 64: wave-uniform
            const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
            const uint64_t ee = e0 + done + L.li;
            const uint32_t my_idx = ee < end ? a.idx[ee] : L.v;
            for (int j = 0; j < n; j += 4) {
                float4 x[4];
                float sc[4][HPQ];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                    const bool loc = s < a.N;
                    const size_t rr = loc ? s : s - a.N;
                    x[u] = row_chunk((loc ? z4 : zg4)[rr * L.nchunk + L.col]);
                    if constexpr (!ELFLY) {
                        const float *ep = (loc ? el : elg) + rr * a.ldk;
#pragma unroll
                        for (int h = 0; h < HPQ; ++h) sc[u][h] = ep[L.hk[h]];
                    }
                }
                if constexpr (ELFLY)
#pragma unroll
                    for (int u = 0; u < 4; ++u) rows_el<HPQ>(x[u], al4, HL, sc[u]);
#pragma unroll
                for (int u = 1; u < 4; ++u)
#pragma unroll
                    for (int h = 0; h < HPQ; ++h) sc[u][h] = j + u < n ? sc[u][h] : -INFINITY;
                S.template step<4>(x, sc);
            }
        }
    }
    if (!L.row_ok) return;
    if (C.walk == ROWS_WALK_FIRST && md < p1) {   // ghost entries to come: the unnormalised state, for the launch after the wait
        if (L.li >= L.nchunk) return;
        reinterpret_cast<float4 *>(sp)[L.col] = S.acc;
        reinterpret_cast<float4 *>(sp + a.ld)[L.col] = S.accp;
#pragma unroll
        for (int s = 0; s < HPQ; ++s)
            if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) {
                hp[L.hk[s]] = S.mx[s];
                hp[a.ldk + L.hk[s]] = S.den[s];
                hp[2 * a.ldk + L.hk[s]] = S.denp[s];
            }
        return;
    }
    rows_fwd_store(L, a, S, o, op, m_out, den_out, dpos_out);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_carry_kernel(GatMhArgs a, int HL, const float *z, const float *zg, const float *el,
                                                                       const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                                       float *m_out, float *den_out, float *dpos_out, RowsCarryArgs C) {
    gatmh_rows_forward_carry_body<GROUP, HPQ, ELFLY>(a, HL, reinterpret_cast<const float4 *>(z), reinterpret_cast<const float4 *>(zg), el, elg, er,
                                                     a_l, o, op, m_out, den_out, dpos_out, C);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_forward_carry_bf16_kernel(GatMhArgs a, int HL, const uint2 *zb, const uint2 *zgb, const float *el,
                                                                            const float *elg, const float *er, const float *a_l, float *o,
                                                                            float *op, float *m_out, float *den_out, float *dpos_out,
                                                                            RowsCarryArgs C) {
    gatmh_rows_forward_carry_body<GROUP, HPQ, ELFLY>(a, HL, zb, zgb, el, elg, er, a_l, o, op, m_out, den_out, dpos_out, C);
}

// ---- backward, destination side: t[v,k] = sum a*da, der[v,k] = sum a*da*l' - t * sum a*l', st = (er, m, 1/den, t) -------------------
template <int HPQ, int W = 1>
struct RowsDstState {
    float erv[HPQ], mv[HPQ], idn[HPQ], t[HPQ], a1[HPQ], a2[HPQ];
    float4 g;   // dO[v], padding columns zeroed
    float4 g1;  // (W == 2)
    template <int NB>
    __device__ __forceinline__ void step(const float4 (&x)[NB * W], const float (&sc)[NB][HPQ], int HL) {
        float prod[NB][HPQ];
#pragma unroll
        for (int u = 0; u < NB; ++u) rows_dot<HPQ>(g, x[u], prod[u]);
        if constexpr (W == 2)
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                float p1[HPQ];
                rows_dot<HPQ>(g1, x[NB + u], p1);
                prod[u][0] = rows8_add(prod[u][0], p1[0]);
            }
        if constexpr (HPQ == 1)
#pragma unroll
            for (int u = 0; u < NB; ++u) prod[u][0] = rows_allreduce(prod[u][0], HL);
#pragma unroll
        for (int u = 0; u < NB; ++u)
#pragma unroll
            for (int s = 0; s < HPQ; ++s) {
                const float pre = sc[u][s] + erv[s];
                const float al = __expf(lrelu02(pre) - mv[s]) * idn[s];
                const float lp = pre > 0.f ? 1.f : GATMH_SLOPE;
                t[s] = fmaf(al, prod[u][s], t[s]);
                a1[s] = fmaf(al * prod[u][s], lp, a1[s]);
                a2[s] = fmaf(al, lp, a2[s]);
            }
    }
};

// the one-pass epilogue of the destination side: t, der, st of row L.v (also the hub rows' merge kernel's)
template <int GROUP, int HPQ, int W>
__device__ __forceinline__ void rows_dst_store(const RowsLane<GROUP, HPQ> &L, const GatMhArgs &a, const RowsDstState<HPQ, W> &S, float *t_out,
                                               float *der_out, float4 *st4, uint32_t lds4) {
#pragma unroll
    for (int s = 0; s < HPQ; ++s)
        if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) {
            const size_t vk = (size_t)L.v * a.ldk + L.hk[s];
            t_out[vk] = S.t[s];
            der_out[vk] = S.a1[s] - S.t[s] * S.a2[s];
            st4[(size_t)L.v * lds4 + L.hk[s]] = make_float4(S.erv[s], S.mv[s], S.idn[s], S.t[s]);
        }
}

template <int GROUP, int HPQ, bool ELFLY, bool HUBS, bool LIST, class CHUNK>
__device__ __forceinline__ void gatmh_rows_dst_body(const GatMhArgs &a, int HL, const CHUNK *z4, const CHUNK *zg4, const float *el,
                                                    const float *elg, const float *er, const float *a_l, const float *m_in,
                                                    const float *den_in, const float *d_o, float *t_out, float *der_out, float4 *st4,
                                                    uint32_t lds4, const RowsHubArgs &H) {
    const RowsWork<GROUP, HUBS, LIST> W(a, H, RowsListArgs{});
    const RowsLane<GROUP, HPQ> L(a, W.row, W.ok);
    const float4 al4 = ELFLY ? rows_attn4(L, a, a_l) : make_float4(0.f, 0.f, 0.f, 0.f);
    RowsDstState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        const size_t vk = (size_t)L.v * a.ldk + L.hk[s];
        S.erv[s] = er[vk];
        S.mv[s] = m_in[vk];
        S.idn[s] = 1.f / den_in[vk];
        S.t[s] = S.a1[s] = S.a2[s] = 0.f;
    }
    S.g = rows_mask(reinterpret_cast<const float4 *>(d_o)[(size_t)L.v * L.nchunk + L.col], L.cm);
    // the row's entries: its in-edges, then the self edge (id v, a local row like any other); batches of four, the dead slots of the
    // last batch gather the last entry's row again and are masked by a score of -inf (alpha = exp(-inf) = 0)
    uint64_t e0, end, total;
    const bool live = W.entries(a, L, H, e0, end, total);
    for (uint64_t done = 0; done < total; done += GROUP) {                     // GROUP == 64: wave-uniform
        const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
        const uint64_t ee = e0 + done + L.li;
        const uint32_t my_idx = ee < end ? a.idx[ee] : L.v;
        for (int j = 0; j < n; j += 4) {
            float4 x[4];
            float sc[4][HPQ];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                const bool loc = s < a.N;
                const size_t r = loc ? s : s - a.N;
                x[u] = row_chunk((loc ? z4 : zg4)[r * L.nchunk + L.col]);
                if constexpr (!ELFLY) {
                    const float *ep = (loc ? el : elg) + r * a.ldk;
#pragma unroll
                    for (int h = 0; h < HPQ; ++h) sc[u][h] = ep[L.hk[h]];
                }
            }
            if constexpr (ELFLY)
#pragma unroll
                for (int u = 0; u < 4; ++u) rows_el<HPQ>(x[u], al4, HL, sc[u]);
#pragma unroll
            for (int u = 1; u < 4; ++u)
#pragma unroll
                for (int h = 0; h < HPQ; ++h) sc[u][h] = j + u < n ? sc[u][h] : -INFINITY;
            S.template step<4>(x, sc, HL);
        }
    }
    if (!live) return;
    if constexpr (HUBS)
        if (W.part) {   // a chunk of a hub row: its partial (t, a1, a2) against the row's m / den, for gatmh_rows_dst_merge_kernel
            float *hp = H.state + (size_t)W.slot * rows_hub_stride(1, a.ld, a.ldk);
#pragma unroll
            for (int s = 0; s < HPQ; ++s)
                if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) {
                    hp[L.hk[s]] = S.t[s];
                    hp[a.ldk + L.hk[s]] = S.a1[s];
                    hp[2 * a.ldk + L.hk[s]] = S.a2[s];
                }
            return;
        }
    rows_dst_store(L, a, S, t_out, der_out, st4, lds4);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_dst_kernel(GatMhArgs a, int HL, const float *z, const float *zg, const float *el,
                                                             const float *elg, const float *er, const float *a_l, const float *m_in,
                                                             const float *den_in, const float *d_o, float *t_out, float *der_out, float4 *st4,
                                                             uint32_t lds4) {
    gatmh_rows_dst_body<GROUP, HPQ, ELFLY, false, false>(a, HL, reinterpret_cast<const float4 *>(z), reinterpret_cast<const float4 *>(zg), el, elg, er, a_l,
                                                  m_in, den_in, d_o, t_out, der_out, st4, lds4, RowsHubArgs{});
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_dst_hub_kernel(GatMhArgs a, int HL, const float *z, const float *zg, const float *el,
                                                                 const float *elg, const float *er, const float *a_l, const float *m_in,
                                                                 const float *den_in, const float *d_o, float *t_out, float *der_out,
                                                                 float4 *st4, uint32_t lds4, RowsHubArgs H) {
    gatmh_rows_dst_body<GROUP, HPQ, ELFLY, true, false>(a, HL, reinterpret_cast<const float4 *>(z), reinterpret_cast<const float4 *>(zg), el, elg, er, a_l,
                                                 m_in, den_in, d_o, t_out, der_out, st4, lds4, H);
}
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_dst_hub_bf16_kernel(GatMhArgs a, int HL, const uint2 *zb, const uint2 *zgb, const float *el,
                                                                      const float *elg, const float *er, const float *a_l, const float *m_in,
                                                                      const float *den_in, const float *d_o, float *t_out, float *der_out,
                                                                      float4 *st4, uint32_t lds4, RowsHubArgs H) {
    gatmh_rows_dst_body<GROUP, HPQ, ELFLY, true, false>(a, HL, zb, zgb, el, elg, er, a_l, m_in, den_in, d_o, t_out, der_out, st4, lds4, H);
}
// one lane group per hub row: the chunks' (t, a1, a2) added in chunk order, then the one-pass epilogue
template <int GROUP, int HPQ>
__global__ __launch_bounds__(256) void gatmh_rows_dst_merge_kernel(GatMhArgs a, const float *er, const float *m_in, const float *den_in,
                                                                   float *t_out, float *der_out, float4 *st4, uint32_t lds4, RowsHubArgs H) {
    const uint32_t h = rows_unit<GROUP>();
    const bool ok = h < H.nrows;
    const RowsLane<GROUP, HPQ> L(a, ok ? H.rows[h] : 0, ok);
    if (!L.row_ok) return;
    const uint32_t c0 = H.row_chunk_ptr[h], c1 = H.row_chunk_ptr[h + 1];
    const size_t stride = rows_hub_stride(1, a.ld, a.ldk);
    RowsDstState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        const size_t vk = (size_t)L.v * a.ldk + L.hk[s];
        S.erv[s] = er[vk];
        S.mv[s] = m_in[vk];
        S.idn[s] = 1.f / den_in[vk];
        S.t[s] = S.a1[s] = S.a2[s] = 0.f;
    }
    for (uint32_t c = c0; c < c1; ++c) {
        const float *hp = H.state + c * stride;
#pragma unroll
        for (int s = 0; s < HPQ; ++s) {
            S.t[s] += hp[L.hk[s]];
            S.a1[s] += hp[a.ldk + L.hk[s]];
            S.a2[s] += hp[2 * a.ldk + L.hk[s]];
        }
    }
    rows_dst_store(L, a, S, t_out, der_out, st4, lds4);
}
// the edge pass of a layer whose forward ran gatmh_rows_forward_bf16_kernel: the same rounded rows, hence the forward's scores
// (m / den are statistics of those); d_o, m, den and er stay fp32
template <int GROUP, int HPQ, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows_dst_bf16_kernel(GatMhArgs a, int HL, const uint2 *zb, const uint2 *zgb, const float *el,
                                                                  const float *elg, const float *er, const float *a_l, const float *m_in,
                                                                  const float *den_in, const float *d_o, float *t_out, float *der_out,
                                                                  float4 *st4, uint32_t lds4) {
    gatmh_rows_dst_body<GROUP, HPQ, ELFLY, false, false>(a, HL, zb, zgb, el, elg, er, a_l, m_in, den_in, d_o, t_out, der_out, st4, lds4, RowsHubArgs{});
}

// ---- backward, source side: rows = sources u (out-edges), entries = destinations v (local: do / st, ghost: bg_do / bg_st) ---------
template <int HPQ, int W = 1>
struct RowsSrcState {
    float elu[HPQ], T[HPQ], Tp[HPQ];
    float4 S, Sp;
    float4 S1, Sp1;   // (W == 2)
    template <int NB>
    __device__ __forceinline__ void step(const float4 (&x)[NB * W], const float4 (&rec)[NB][HPQ]) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            float al[HPQ], alp[HPQ];
#pragma unroll
            for (int s = 0; s < HPQ; ++s) {
                const float4 r = rec[u][s];                       // (er, m, 1/den, t) of (v, k)
                const float pre = elu[s] + r.x;
                al[s] = __expf(lrelu02(pre) - r.y) * r.z;
                alp[s] = pre > 0.f ? al[s] : 0.f;
                T[s] = fmaf(al[s], r.w, T[s]);
                Tp[s] = fmaf(alp[s], r.w, Tp[s]);
            }
            S = rows_axpy<HPQ>(al, x[u], S);
            Sp = rows_axpy<HPQ>(alp, x[u], Sp);
            if constexpr (W == 2) {
                S1 = rows_axpy<HPQ>(al, x[NB + u], S1);
                Sp1 = rows_axpy<HPQ>(alp, x[NB + u], Sp1);
            }
        }
    }
};

// NB: destination rows in flight per group.  Four; the instantiations with four heads per lane (D == 1) keep two -- a batch holds
// NB x HPQ statistics records of four registers each: 64 registers at NB = 4, 32 more than in the two-row form, which takes 111
// in all -- past the 128 that leave four waves per SIMD (what a latency-bound gather lives on; tests/test_gatmh_row_gather_resources.py)
// the one-pass closing arithmetic of the source side: del and dz of row L.v from its sums (also the hub rows' merge kernel's; every
// lane of a live group arrives: the head's lanes reduce the dot product)
// (W == 2, the wide bf16 form: L is the lane of its first float4, L1 that of its second -- the same row and head)
template <int GROUP, int HPQ, int W>
__device__ __forceinline__ void rows_src_close(const RowsLane<GROUP, HPQ> &L, const GatMhArgs &a, int HL, const RowsSrcState<HPQ, W> &S, const float *z,
                                               const float *der, const float *a_l, const float *a_r, float *del_out, float *dz,
                                               const RowsLane<GROUP, HPQ> *L1 = nullptr) {
    // del[u,k] = <Z[u,k,:], 0.2 S + 0.8 S+> - (0.2 T + 0.8 T+)
    const float lo = GATMH_SLOPE, hi = 1.f - GATMH_SLOPE;
    const float4 zz = rows_mask(reinterpret_cast<const float4 *>(z)[(size_t)L.v * L.nchunk + L.col], L.cm);
    const float4 mix = make_float4(fmaf(hi, S.Sp.x, lo * S.S.x), fmaf(hi, S.Sp.y, lo * S.S.y), fmaf(hi, S.Sp.z, lo * S.S.z),
                                   fmaf(hi, S.Sp.w, lo * S.S.w));
    float dd[HPQ];
    rows_dot<HPQ>(zz, mix, dd);
    if constexpr (W == 2) {
        const float4 zz1 = rows_mask(reinterpret_cast<const float4 *>(z)[(size_t)L1->v * L1->nchunk + L1->col], L1->cm);
        const float4 mix1 = make_float4(fmaf(hi, S.Sp1.x, lo * S.S1.x), fmaf(hi, S.Sp1.y, lo * S.S1.y), fmaf(hi, S.Sp1.z, lo * S.S1.z),
                                        fmaf(hi, S.Sp1.w, lo * S.S1.w));
        float d1[HPQ];
        rows_dot<HPQ>(zz1, mix1, d1);
        dd[0] = rows8_add(dd[0], d1[0]);
    }
    if constexpr (HPQ == 1) dd[0] = rows_allreduce(dd[0], HL);
    if (!L.lane_ok) return;
    const uint32_t KD = a.K * a.D;
    float del[HPQ], dr[HPQ];
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        del[s] = dd[s] - (lo * S.T[s] + hi * S.Tp[s]);
        dr[s] = der[(size_t)L.v * a.ldk + L.hk[s]];
    }
    float al4[4], ar4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t f = min(4 * L.col + c, KD - 1);
        al4[c] = a_l[f];
        ar4[c] = a_r[f];
    }
    float4 out = S.S;
    out = rows_axpy<HPQ>(del, make_float4(al4[0], al4[1], al4[2], al4[3]), out);
    out = rows_axpy<HPQ>(dr, make_float4(ar4[0], ar4[1], ar4[2], ar4[3]), out);
    reinterpret_cast<float4 *>(dz)[(size_t)L.v * L.nchunk + L.col] = rows_mask(out, L.cm);
#pragma unroll
    for (int s = 0; s < HPQ; ++s)
        if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) del_out[(size_t)L.v * a.ldk + L.hk[s]] = del[s];
    if constexpr (W == 2) {
        if (!L1->lane_ok) return;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t f = min(4 * L1->col + c, KD - 1);
            al4[c] = a_l[f];
            ar4[c] = a_r[f];
        }
        float4 out1 = S.S1;
        out1 = rows_axpy<HPQ>(del, make_float4(al4[0], al4[1], al4[2], al4[3]), out1);
        out1 = rows_axpy<HPQ>(dr, make_float4(ar4[0], ar4[1], ar4[2], ar4[3]), out1);
        reinterpret_cast<float4 *>(dz)[(size_t)L1->v * L1->nchunk + L1->col] = rows_mask(out1, L1->cm);
    }
}

template <int GROUP, int HPQ, int NB, bool HUBS, bool LIST, class CHUNK>
__device__ __forceinline__ void gatmh_rows_src_body(const GatMhArgs &a, int HL, const float *z, const float *el, const CHUNK *d4,
                                                    const CHUNK *dg4, const float4 *st4, const float4 *stg, uint32_t lds4, const float *der,
                                                    const float *a_l, const float *a_r, float *del_out, float *dz, const RowsHubArgs &H,
                                                    const RowsListArgs &R = RowsListArgs{}) {
    const RowsWork<GROUP, HUBS, LIST> W(a, H, R);
    const RowsLane<GROUP, HPQ> L(a, W.row, W.ok);
    RowsSrcState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        S.elu[s] = el[(size_t)L.v * a.ldk + L.hk[s]];
        S.T[s] = S.Tp[s] = 0.f;
    }
    S.S = S.Sp = make_float4(0.f, 0.f, 0.f, 0.f);
    // the row's entries: its out-edges, then the self edge (id u); batches of NB, the dead slots of the last batch masked by a
    // destination score of -inf (alpha = exp(-inf) = 0)
    uint64_t e0, end, total;
    const bool live = W.entries(a, L, H, e0, end, total);
    for (uint64_t done = 0; done < total; done += GROUP) {
        const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
        const uint64_t ee = e0 + done + L.li;
        const uint32_t my_idx = ee < end ? a.idx[ee] : L.v;
        for (int j = 0; j < n; j += NB) {
            float4 x[NB], rec[NB][HPQ];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                const bool loc = s < a.N;
                const size_t r = loc ? s : s - a.N;
                x[u] = row_chunk((loc ? d4 : dg4)[r * L.nchunk + L.col]);
                const float4 *sp = (loc ? st4 : stg) + r * lds4;
#pragma unroll
                for (int h = 0; h < HPQ; ++h) rec[u][h] = sp[L.hk[h]];
            }
#pragma unroll
            for (int u = 1; u < NB; ++u)
#pragma unroll
                for (int h = 0; h < HPQ; ++h) rec[u][h].x = j + u < n ? rec[u][h].x : -INFINITY;
            S.template step<NB>(x, rec);
        }
    }
    if (!live) return;
    if constexpr (HUBS)
        if (W.part) {   // a chunk of a hub row: its partial sums, for gatmh_rows_src_merge_kernel
            if (L.li >= L.nchunk) return;
            float *sp = H.state + (size_t)W.slot * rows_hub_stride(2, a.ld, a.ldk), *hp = sp + 2 * (size_t)a.ld;
            reinterpret_cast<float4 *>(sp)[L.col] = S.S;
            reinterpret_cast<float4 *>(sp + a.ld)[L.col] = S.Sp;
#pragma unroll
            for (int s = 0; s < HPQ; ++s)
                if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) {
                    hp[L.hk[s]] = S.T[s];
                    hp[a.ldk + L.hk[s]] = S.Tp[s];
                }
            return;
        }
    rows_src_close(L, a, HL, S, z, der, a_l, a_r, del_out, dz);
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_kernel(GatMhArgs a, int HL, const float *z, const float *el, const float *d_o,
                                                             const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                             const float *der, const float *a_l, const float *a_r, float *del_out,
                                                             float *dz) {
    gatmh_rows_src_body<GROUP, HPQ, NB, false, false>(a, HL, z, el, reinterpret_cast<const float4 *>(d_o), reinterpret_cast<const float4 *>(dog), st4, stg,
                                               lds4, der, a_l, a_r, del_out, dz, RowsHubArgs{});
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_hub_kernel(GatMhArgs a, int HL, const float *z, const float *el, const float *d_o,
                                                                 const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                 const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                 float *dz, RowsHubArgs H) {
    gatmh_rows_src_body<GROUP, HPQ, NB, true, false>(a, HL, z, el, reinterpret_cast<const float4 *>(d_o), reinterpret_cast<const float4 *>(dog), st4, stg,
                                              lds4, der, a_l, a_r, del_out, dz, H);
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_hub_bf16_kernel(GatMhArgs a, int HL, const float *z, const float *el, const uint2 *dob,
                                                                      const uint2 *dogb, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                      const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                      float *dz, RowsHubArgs H) {
    gatmh_rows_src_body<GROUP, HPQ, NB, true, false>(a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del_out, dz, H);
}
// one lane group per hub row: the chunks' sums added in chunk order, then the one-pass closing arithmetic
template <int GROUP, int HPQ>
__global__ __launch_bounds__(256) void gatmh_rows_src_merge_kernel(GatMhArgs a, int HL, const float *z, const float *der, const float *a_l,
                                                                   const float *a_r, float *del_out, float *dz, RowsHubArgs H) {
    const uint32_t h = rows_unit<GROUP>();
    const bool ok = h < H.nrows;
    const RowsLane<GROUP, HPQ> L(a, ok ? H.rows[h] : 0, ok);
    if (!L.row_ok) return;
    const uint32_t c0 = H.row_chunk_ptr[h], c1 = H.row_chunk_ptr[h + 1];
    const size_t stride = rows_hub_stride(2, a.ld, a.ldk);
    RowsSrcState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) S.elu[s] = S.T[s] = S.Tp[s] = 0.f;
    S.S = S.Sp = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t c = c0; c < c1; ++c) {
        const float *sp = H.state + c * stride, *hp = sp + 2 * (size_t)a.ld;
        const float4 p = reinterpret_cast<const float4 *>(sp)[L.col], q = reinterpret_cast<const float4 *>(sp + a.ld)[L.col];
        S.S = make_float4(S.S.x + p.x, S.S.y + p.y, S.S.z + p.z, S.S.w + p.w);
        S.Sp = make_float4(S.Sp.x + q.x, S.Sp.y + q.y, S.Sp.z + q.z, S.Sp.w + q.w);
#pragma unroll
        for (int s = 0; s < HPQ; ++s) {
            S.T[s] += hp[L.hk[s]];
            S.Tp[s] += hp[a.ldk + L.hk[s]];
        }
    }
    rows_src_close(L, a, HL, S, z, der, a_l, a_r, del_out, dz);
}
// dob / dogb: the shadow rows of do / bg_do (gatmh_bf16_gather = 2).  The 16-byte records, the row's own el[u], the closing z[u]
// row, der, a_l and a_r stay fp32
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_bf16_kernel(GatMhArgs a, int HL, const float *z, const float *el, const uint2 *dob,
                                                                  const uint2 *dogb, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                  const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                  float *dz) {
    gatmh_rows_src_body<GROUP, HPQ, NB, false, false>(a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del_out, dz, RowsHubArgs{});
}
// dory_gatmh_row_gather_overlap: as gatmh_rows_forward_list_kernel, over the out-edges -- the interior sources (every destination local:
// do / st alone) beside the backward's last exchange, the boundary sources after it
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_list_kernel(GatMhArgs a, int HL, const float *z, const float *el, const float *d_o,
                                                                  const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                  const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                  float *dz, RowsListArgs R) {
    gatmh_rows_src_body<GROUP, HPQ, NB, false, true>(a, HL, z, el, reinterpret_cast<const float4 *>(d_o), reinterpret_cast<const float4 *>(dog), st4,
                                                     stg, lds4, der, a_l, a_r, del_out, dz, RowsHubArgs{}, R);
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_list_bf16_kernel(GatMhArgs a, int HL, const float *z, const float *el, const uint2 *dob,
                                                                       const uint2 *dogb, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                       const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                       float *dz, RowsListArgs R) {
    gatmh_rows_src_body<GROUP, HPQ, NB, false, true>(a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del_out, dz, RowsHubArgs{}, R);
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_list_hub_kernel(GatMhArgs a, int HL, const float *z, const float *el, const float *d_o,
                                                                      const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                      const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                      float *dz, RowsHubArgs H, RowsListArgs R) {
    gatmh_rows_src_body<GROUP, HPQ, NB, true, true>(a, HL, z, el, reinterpret_cast<const float4 *>(d_o), reinterpret_cast<const float4 *>(dog), st4,
                                                    stg, lds4, der, a_l, a_r, del_out, dz, H, R);
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_list_hub_bf16_kernel(GatMhArgs a, int HL, const float *z, const float *el, const uint2 *dob,
                                                                           const uint2 *dogb, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                           const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                           float *dz, RowsHubArgs H, RowsListArgs R) {
    gatmh_rows_src_body<GROUP, HPQ, NB, true, true>(a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del_out, dz, H, R);
}
// dory_gatmh_row_gather_edge_split: the carry form of the source side, as gatmh_rows_forward_carry_body -- range A: the local
// destinations (do / st) and the self edge, range B: the ghost destinations (bg_do / bg_st); the state is (S, S+, T, T+), plain sums
template <int GROUP, int HPQ, int NB, class CHUNK>
__device__ __forceinline__ void gatmh_rows_src_carry_body(const GatMhArgs &a, int HL, const float *z, const float *el, const CHUNK *d4,
                                                          const CHUNK *dg4, const float4 *st4, const float4 *stg, uint32_t lds4, const float *der,
                                                          const float *a_l, const float *a_r, float *del_out, float *dz, const RowsCarryArgs &C) {
    const uint32_t unit = rows_unit<GROUP>();
    const bool second = C.walk == ROWS_WALK_SECOND;
    const bool ok = unit < (second ? C.n : a.N);
    const RowsLane<GROUP, HPQ> L(a, ok ? (second ? C.rows[unit] : unit) : 0, ok);
    RowsSrcState<HPQ> S;
#pragma unroll
    for (int s = 0; s < HPQ; ++s) {
        S.elu[s] = el[(size_t)L.v * a.ldk + L.hk[s]];
        S.T[s] = S.Tp[s] = 0.f;
    }
    S.S = S.Sp = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint64_t p0 = L.row_ok ? a.ptr[L.v] : 0, p1 = L.row_ok ? a.ptr[L.v + 1] : 0, md = L.row_ok ? C.mid[L.v] : 0;
    float *sp = C.state + (size_t)L.v * rows_hub_stride(2, a.ld, a.ldk), *hp = sp + 2 * (size_t)a.ld;
    if (second && L.row_ok) {
        S.S = reinterpret_cast<const float4 *>(sp)[L.col];
        S.Sp = reinterpret_cast<const float4 *>(sp + a.ld)[L.col];
#pragma unroll
        for (int s = 0; s < HPQ; ++s) {
            S.T[s] = hp[L.hk[s]];
            S.Tp[s] = hp[a.ldk + L.hk[s]];
        }
    }
    const int r1 = C.walk == ROWS_WALK_FIRST ? 1 : 2;
    for (int r = second ? 1 : 0; r < r1; ++r) {
        const uint64_t e0 = r ? md : p0, end = r ? p1 : md;
        const uint64_t total = L.row_ok ? end - e0 + (r ? 0 : 1) : 0;
        for (uint64_t done = 0; done < total; done += GROUP) {
            const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
            const uint64_t ee = e0 + done + L.li;
            const uint32_t my_idx = ee < end ? a.idx[ee] : L.v;
            for (int j = 0; j < n; j += NB) {
                float4 x[NB], rec[NB][HPQ];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                    const bool loc = s < a.N;
                    const size_t rr = loc ? s : s - a.N;
                    x[u] = row_chunk((loc ? d4 : dg4)[rr * L.nchunk + L.col]);
                    const float4 *rp = (loc ? st4 : stg) + rr * lds4;
#pragma unroll
                    for (int h = 0; h < HPQ; ++h) rec[u][h] = rp[L.hk[h]];
                }
#pragma unroll
                for (int u = 1; u < NB; ++u)
#pragma unroll
                    for (int h = 0; h < HPQ; ++h) rec[u][h].x = j + u < n ? rec[u][h].x : -INFINITY;
                S.template step<NB>(x, rec);
            }
        }
    }
    if (!L.row_ok) return;
    if (C.walk == ROWS_WALK_FIRST && md < p1) {   // ghost destinations to come: the partial sums, for the launch after the wait
        if (L.li >= L.nchunk) return;
        reinterpret_cast<float4 *>(sp)[L.col] = S.S;
        reinterpret_cast<float4 *>(sp + a.ld)[L.col] = S.Sp;
#pragma unroll
        for (int s = 0; s < HPQ; ++s)
            if (HPQ == 1 ? L.leader(a) : L.head_live(a, s)) {
                hp[L.hk[s]] = S.T[s];
                hp[a.ldk + L.hk[s]] = S.Tp[s];
            }
        return;
    }
    rows_src_close(L, a, HL, S, z, der, a_l, a_r, del_out, dz);
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_carry_kernel(GatMhArgs a, int HL, const float *z, const float *el, const float *d_o,
                                                                   const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                   const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                   float *dz, RowsCarryArgs C) {
    gatmh_rows_src_carry_body<GROUP, HPQ, NB>(a, HL, z, el, reinterpret_cast<const float4 *>(d_o), reinterpret_cast<const float4 *>(dog), st4, stg,
                                              lds4, der, a_l, a_r, del_out, dz, C);
}
template <int GROUP, int HPQ, int NB>
__global__ __launch_bounds__(256) void gatmh_rows_src_carry_bf16_kernel(GatMhArgs a, int HL, const float *z, const float *el, const uint2 *dob,
                                                                        const uint2 *dogb, const float4 *st4, const float4 *stg, uint32_t lds4,
                                                                        const float *der, const float *a_l, const float *a_r, float *del_out,
                                                                        float *dz, RowsCarryArgs C) {
    gatmh_rows_src_carry_body<GROUP, HPQ, NB>(a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del_out, dz, C);
}

// ---- the wide bf16 form (dory_gatmh_row_gather_bf16_wide; gatmh_rows8_*_kernel) -----------------------------------------------------
// A lane keeps EIGHT consecutive features: one 16-byte load of eight bf16 per edge, two float4 accumulators wherever the narrow form
// has one -- the lane stands for the narrow form's lanes 2 li and 2 li + 1 (Rows8Lane::lo / hi), so a row takes 8 / 16 / 32 lanes
// (gatmh_rows8_form, gat_mh_shapes.hpp), a wave has twice the rows in flight, and the heads' exponentials are computed by half as
// many lanes.  One head per lane (a single head, or D % 8 == 0).  Everything else is the narrow form's: units, id blocks (a
// multiple of four entries in both forms: batches, masked tails and the moments the maximum moves coincide), ghost ids, 64-bit
// addressing, hub chunks and row lists.  The contract is the narrow bf16 kernels' BITS in every tensor:
//   * the state structs and epilogues above are the narrow form's, W = 2: their `if constexpr (W == 2)` parts repeat, for the second
//     float4, the calls made for the first -- per column the same fmaf chains in entry order;
//   * per head, the values are the structs' one scalar chain, run once a lane;
//   * a dot product is, per float4, the narrow lane's four-term chain (rows_el / rows_dot with nothing reduced);
//     the two are added in the lane (rows8_add: the butterfly's offset-1 step, a + b where the narrow lanes form a + b and b + a, kept
//     off any contraction -- the narrow form adds after a DPP move) and reduced by rows_allreduce over half as many lanes, whose
//     offsets 1, 2, 4 are the narrow form's 2, 4, 8.
// A hub row's chunk states keep their layout (lane li writes what lanes 2 li and 2 li + 1 write): the narrow merge kernels follow a
// wide chunk launch.
// the narrow form's lane that keeps float4 `lane` of the row: RowsLane's values for that place
template <int GROUP>
__device__ __forceinline__ RowsLane<GROUP, 1> rows8_half(const GatMhArgs &a, uint32_t rid, bool ok, uint32_t lane) {
    RowsLane<GROUP, 1> L(a, rid, ok);
    const uint32_t KD = a.K * a.D;
    L.li = lane;
    L.lane_ok = L.row_ok && lane < L.nchunk && 4 * lane < KD;
    L.col = lane < L.nchunk ? lane : 0;
    L.hk[0] = min((4 * L.col) / a.D, a.K - 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) L.cm[c] = L.lane_ok && 4 * L.col + c < KD;
    return L;
}
template <int GROUP>
struct Rows8Lane {
    RowsLane<GROUP, 1> lo, hi;
    uint32_t li, nchunk8, col8;
    __device__ __forceinline__ Rows8Lane(const GatMhArgs &a, uint32_t rid, bool ok, uint32_t lane = (uint32_t)((threadIdx.x & 63) % GROUP))
        : lo(rows8_half<GROUP>(a, rid, ok, 2 * lane)), hi(rows8_half<GROUP>(a, rid, ok, 2 * lane + 1)), li(lane) {
        nchunk8 = a.ld >> 3;
        col8 = li < nchunk8 ? li : 0;         // lanes past the row gather column 0 (valid memory) and never store
    }
};
// the source's score of the lane's head from the gathered row: rows_el's value (al0 / al1: a_l's columns of the two float4s)
__device__ __forceinline__ float rows8_el(const float4 &x0, const float4 &x1, const float4 &al0, const float4 &al1, int HL) {
    float p0[1], p1[1];
    rows_el<1>(x0, al0, 1, p0);
    rows_el<1>(x1, al1, 1, p1);
    return rows_allreduce(rows8_add(p0[0], p1[0]), HL);
}

template <int GROUP, bool ELFLY, bool HUBS, bool LIST>
__device__ __forceinline__ void gatmh_rows8_forward_body(const GatMhArgs &a, int HL, const uint4 *z8, const uint4 *zg8, const float *el,
                                                         const float *elg, const float *er, const float *a_l, float *o, float *op,
                                                         float *m_out, float *den_out, float *dpos_out, const RowsHubArgs &H,
                                                         const RowsListArgs &R = RowsListArgs{}) {
    const RowsWork<GROUP, HUBS, LIST> W(a, H, R);
    const Rows8Lane<GROUP> L(a, W.row, W.ok);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 al0 = ELFLY ? rows_attn4(L.lo, a, a_l) : zero4, al1 = ELFLY ? rows_attn4(L.hi, a, a_l) : zero4;
    RowsFwdState<1, 2> S;
    S.erv[0] = er[(size_t)L.lo.v * a.ldk + L.lo.hk[0]];
    S.mx[0] = -INFINITY;
    S.den[0] = S.denp[0] = 0.f;
    S.acc = S.accp = S.acc1 = S.accp1 = zero4;
    uint64_t e0, end, total;
    const bool live = W.entries(a, L.lo, H, e0, end, total);
    for (uint64_t done = 0; done < total; done += GROUP) {
        const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
        const uint64_t ee = e0 + done + L.li;
        const uint32_t my_idx = ee < end ? a.idx[ee] : L.lo.v;
        for (int j = 0; j < n; j += 4) {
            float4 x[8];      // x[u], x[4 + u]: the two float4s of row u of the batch
            float sc[4][1];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                const bool loc = s < a.N;
                const size_t r = loc ? s : s - a.N;
                row_chunk((loc ? z8 : zg8)[r * L.nchunk8 + L.col8], x[u], x[4 + u]);
                if constexpr (!ELFLY) sc[u][0] = ((loc ? el : elg) + r * a.ldk)[L.lo.hk[0]];
            }
            if constexpr (ELFLY)
#pragma unroll
                for (int u = 0; u < 4; ++u) sc[u][0] = rows8_el(x[u], x[4 + u], al0, al1, HL);
#pragma unroll
            for (int u = 1; u < 4; ++u) sc[u][0] = j + u < n ? sc[u][0] : -INFINITY;
            S.template step<4>(x, sc);
        }
    }
    if (!live) return;
    if constexpr (HUBS)
        if (W.part) {   // a chunk of a hub row: its state where the narrow form's lanes leave it, for gatmh_rows_forward_merge_kernel
            if (L.lo.li >= L.lo.nchunk) return;
            float *sp = H.state + (size_t)W.slot * rows_hub_stride(0, a.ld, a.ldk), *hp = sp + 2 * (size_t)a.ld;
            reinterpret_cast<float4 *>(sp)[L.lo.col] = S.acc;
            reinterpret_cast<float4 *>(sp)[L.hi.col] = S.acc1;
            reinterpret_cast<float4 *>(sp + a.ld)[L.lo.col] = S.accp;
            reinterpret_cast<float4 *>(sp + a.ld)[L.hi.col] = S.accp1;
            if (L.lo.leader(a)) {
                hp[L.lo.hk[0]] = S.mx[0];
                hp[a.ldk + L.lo.hk[0]] = S.den[0];
                hp[2 * a.ldk + L.lo.hk[0]] = S.denp[0];
            }
            return;
        }
    // the narrow epilogue per float4 (the second one's lane is no head's leader: it stores its float4 of o and op alone)
    rows_fwd_store(L.lo, a, S, o, op, m_out, den_out, dpos_out);
    RowsFwdState<1> Sh;
    Sh.mx[0] = S.mx[0]; Sh.den[0] = S.den[0]; Sh.denp[0] = S.denp[0];
    Sh.acc = S.acc1; Sh.accp = S.accp1;
    rows_fwd_store(L.hi, a, Sh, o, op, m_out, den_out, dpos_out);
}
#define GATMH_ROWS8_FWD_PARAMS                                                                                                        \
    GatMhArgs a, int HL, const uint4 *zb, const uint4 *zgb, const float *el, const float *elg, const float *er, const float *a_l, float *o, \
        float *op, float *m_out, float *den_out, float *dpos_out
#define GATMH_ROWS8_FWD_ARGS a, HL, zb, zgb, el, elg, er, a_l, o, op, m_out, den_out, dpos_out
template <int GROUP, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows8_forward_kernel(GATMH_ROWS8_FWD_PARAMS) {
    gatmh_rows8_forward_body<GROUP, ELFLY, false, false>(GATMH_ROWS8_FWD_ARGS, RowsHubArgs{});
}
template <int GROUP, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows8_forward_hub_kernel(GATMH_ROWS8_FWD_PARAMS, RowsHubArgs H) {
    gatmh_rows8_forward_body<GROUP, ELFLY, true, false>(GATMH_ROWS8_FWD_ARGS, H);
}
template <int GROUP, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows8_forward_list_kernel(GATMH_ROWS8_FWD_PARAMS, RowsListArgs R) {
    gatmh_rows8_forward_body<GROUP, ELFLY, false, true>(GATMH_ROWS8_FWD_ARGS, RowsHubArgs{}, R);
}
template <int GROUP, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows8_forward_list_hub_kernel(GATMH_ROWS8_FWD_PARAMS, RowsHubArgs H, RowsListArgs R) {
    gatmh_rows8_forward_body<GROUP, ELFLY, true, true>(GATMH_ROWS8_FWD_ARGS, H, R);
}
#undef GATMH_ROWS8_FWD_PARAMS
#undef GATMH_ROWS8_FWD_ARGS

template <int GROUP, bool ELFLY, bool HUBS>
__device__ __forceinline__ void gatmh_rows8_dst_body(const GatMhArgs &a, int HL, const uint4 *z8, const uint4 *zg8, const float *el,
                                                     const float *elg, const float *er, const float *a_l, const float *m_in,
                                                     const float *den_in, const float *d_o, float *t_out, float *der_out, float4 *st4,
                                                     uint32_t lds4, const RowsHubArgs &H) {
    const RowsWork<GROUP, HUBS, false> W(a, H, RowsListArgs{});
    const Rows8Lane<GROUP> L(a, W.row, W.ok);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 al0 = ELFLY ? rows_attn4(L.lo, a, a_l) : zero4, al1 = ELFLY ? rows_attn4(L.hi, a, a_l) : zero4;
    RowsDstState<1, 2> S;     // (S.g / S.g1: dO[v]'s two float4s, padding columns zeroed)
    const size_t vk = (size_t)L.lo.v * a.ldk + L.lo.hk[0];
    S.erv[0] = er[vk];
    S.mv[0] = m_in[vk];
    S.idn[0] = 1.f / den_in[vk];
    S.t[0] = S.a1[0] = S.a2[0] = 0.f;
    S.g = rows_mask(reinterpret_cast<const float4 *>(d_o)[(size_t)L.lo.v * L.lo.nchunk + L.lo.col], L.lo.cm);
    S.g1 = rows_mask(reinterpret_cast<const float4 *>(d_o)[(size_t)L.hi.v * L.hi.nchunk + L.hi.col], L.hi.cm);
    uint64_t e0, end, total;
    const bool live = W.entries(a, L.lo, H, e0, end, total);
    for (uint64_t done = 0; done < total; done += GROUP) {
        const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
        const uint64_t ee = e0 + done + L.li;
        const uint32_t my_idx = ee < end ? a.idx[ee] : L.lo.v;
        for (int j = 0; j < n; j += 4) {
            float4 x[8];
            float sc[4][1];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                const bool loc = s < a.N;
                const size_t r = loc ? s : s - a.N;
                row_chunk((loc ? z8 : zg8)[r * L.nchunk8 + L.col8], x[u], x[4 + u]);
                if constexpr (!ELFLY) sc[u][0] = ((loc ? el : elg) + r * a.ldk)[L.lo.hk[0]];
            }
            if constexpr (ELFLY)
#pragma unroll
                for (int u = 0; u < 4; ++u) sc[u][0] = rows8_el(x[u], x[4 + u], al0, al1, HL);
#pragma unroll
            for (int u = 1; u < 4; ++u) sc[u][0] = j + u < n ? sc[u][0] : -INFINITY;
            S.template step<4>(x, sc, HL);
        }
    }
    if (!live) return;
    if constexpr (HUBS)
        if (W.part) {   // a chunk of a hub row: its partial (t, a1, a2), for gatmh_rows_dst_merge_kernel
            float *hp = H.state + (size_t)W.slot * rows_hub_stride(1, a.ld, a.ldk);
            if (L.lo.leader(a)) {
                hp[L.lo.hk[0]] = S.t[0];
                hp[a.ldk + L.lo.hk[0]] = S.a1[0];
                hp[2 * a.ldk + L.lo.hk[0]] = S.a2[0];
            }
            return;
        }
    rows_dst_store(L.lo, a, S, t_out, der_out, st4, lds4);
}
#define GATMH_ROWS8_DST_PARAMS                                                                                                        \
    GatMhArgs a, int HL, const uint4 *zb, const uint4 *zgb, const float *el, const float *elg, const float *er, const float *a_l,     \
        const float *m_in, const float *den_in, const float *d_o, float *t_out, float *der_out, float4 *st4, uint32_t lds4
#define GATMH_ROWS8_DST_ARGS a, HL, zb, zgb, el, elg, er, a_l, m_in, den_in, d_o, t_out, der_out, st4, lds4
template <int GROUP, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows8_dst_kernel(GATMH_ROWS8_DST_PARAMS) {
    gatmh_rows8_dst_body<GROUP, ELFLY, false>(GATMH_ROWS8_DST_ARGS, RowsHubArgs{});
}
template <int GROUP, bool ELFLY>
__global__ __launch_bounds__(256) void gatmh_rows8_dst_hub_kernel(GATMH_ROWS8_DST_PARAMS, RowsHubArgs H) {
    gatmh_rows8_dst_body<GROUP, ELFLY, true>(GATMH_ROWS8_DST_ARGS, H);
}
#undef GATMH_ROWS8_DST_PARAMS
#undef GATMH_ROWS8_DST_ARGS

// the source side: four destination rows in flight (one head per lane: a batch holds four statistics records)
template <int GROUP, bool HUBS, bool LIST>
__device__ __forceinline__ void gatmh_rows8_src_body(const GatMhArgs &a, int HL, const float *z, const float *el, const uint4 *d8,
                                                     const uint4 *dg8, const float4 *st4, const float4 *stg, uint32_t lds4, const float *der,
                                                     const float *a_l, const float *a_r, float *del_out, float *dz, const RowsHubArgs &H,
                                                     const RowsListArgs &R = RowsListArgs{}) {
    constexpr int NB = 4;
    const RowsWork<GROUP, HUBS, LIST> W(a, H, R);
    const Rows8Lane<GROUP> L(a, W.row, W.ok);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    RowsSrcState<1, 2> S;
    S.elu[0] = el[(size_t)L.lo.v * a.ldk + L.lo.hk[0]];
    S.T[0] = S.Tp[0] = 0.f;
    S.S = S.Sp = S.S1 = S.Sp1 = zero4;
    uint64_t e0, end, total;
    const bool live = W.entries(a, L.lo, H, e0, end, total);
    for (uint64_t done = 0; done < total; done += GROUP) {
        const int n = (total - done) < (uint64_t)GROUP ? (int)(total - done) : GROUP;
        const uint64_t ee = e0 + done + L.li;
        const uint32_t my_idx = ee < end ? a.idx[ee] : L.lo.v;
        for (int j = 0; j < n; j += NB) {
            float4 x[2 * NB], rec[NB][1];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const uint32_t s = bcast_u32<GROUP>(my_idx, min(j + u, n - 1));
                const bool loc = s < a.N;
                const size_t r = loc ? s : s - a.N;
                row_chunk((loc ? d8 : dg8)[r * L.nchunk8 + L.col8], x[u], x[NB + u]);
                rec[u][0] = ((loc ? st4 : stg) + r * lds4)[L.lo.hk[0]];
            }
#pragma unroll
            for (int u = 1; u < NB; ++u) rec[u][0].x = j + u < n ? rec[u][0].x : -INFINITY;
            S.template step<NB>(x, rec);
        }
    }
    if (!live) return;
    if constexpr (HUBS)
        if (W.part) {   // a chunk of a hub row: its partial sums where the narrow form's lanes leave them, for gatmh_rows_src_merge_kernel
            if (L.lo.li >= L.lo.nchunk) return;
            float *sp = H.state + (size_t)W.slot * rows_hub_stride(2, a.ld, a.ldk), *hp = sp + 2 * (size_t)a.ld;
            reinterpret_cast<float4 *>(sp)[L.lo.col] = S.S;
            reinterpret_cast<float4 *>(sp)[L.hi.col] = S.S1;
            reinterpret_cast<float4 *>(sp + a.ld)[L.lo.col] = S.Sp;
            reinterpret_cast<float4 *>(sp + a.ld)[L.hi.col] = S.Sp1;
            if (L.lo.leader(a)) {
                hp[L.lo.hk[0]] = S.T[0];
                hp[a.ldk + L.lo.hk[0]] = S.Tp[0];
            }
            return;
        }
    rows_src_close(L.lo, a, HL, S, z, der, a_l, a_r, del_out, dz, &L.hi);
}
#define GATMH_ROWS8_SRC_PARAMS                                                                                                        \
    GatMhArgs a, int HL, const float *z, const float *el, const uint4 *dob, const uint4 *dogb, const float4 *st4, const float4 *stg,  \
        uint32_t lds4, const float *der, const float *a_l, const float *a_r, float *del_out, float *dz
#define GATMH_ROWS8_SRC_ARGS a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del_out, dz
template <int GROUP>
__global__ __launch_bounds__(256) void gatmh_rows8_src_kernel(GATMH_ROWS8_SRC_PARAMS) {
    gatmh_rows8_src_body<GROUP, false, false>(GATMH_ROWS8_SRC_ARGS, RowsHubArgs{});
}
template <int GROUP>
__global__ __launch_bounds__(256) void gatmh_rows8_src_hub_kernel(GATMH_ROWS8_SRC_PARAMS, RowsHubArgs H) {
    gatmh_rows8_src_body<GROUP, true, false>(GATMH_ROWS8_SRC_ARGS, H);
}
template <int GROUP>
__global__ __launch_bounds__(256) void gatmh_rows8_src_list_kernel(GATMH_ROWS8_SRC_PARAMS, RowsListArgs R) {
    gatmh_rows8_src_body<GROUP, false, true>(GATMH_ROWS8_SRC_ARGS, RowsHubArgs{}, R);
}
template <int GROUP>
__global__ __launch_bounds__(256) void gatmh_rows8_src_list_hub_kernel(GATMH_ROWS8_SRC_PARAMS, RowsHubArgs H, RowsListArgs R) {
    gatmh_rows8_src_body<GROUP, true, true>(GATMH_ROWS8_SRC_ARGS, H, R);
}
#undef GATMH_ROWS8_SRC_PARAMS
#undef GATMH_ROWS8_SRC_ARGS

// ---- launchers -------------------------------------------------------------------------------------------------------------------
// lanes per row and heads per float4 of a shape; false: a shape the model does not allow (gatmh_shape_ok) or rows no float4 tiles
static bool gatmh_rows_form(uint32_t K, uint32_t D, uint32_t ld, int *group, int *hpq, int *HL) {
    if (!gatmh_rows_shape_ok(K, D, ld)) return false;
    const uint32_t nchunk = ld >> 2;
    *group = nchunk <= 8 ? 8 : nchunk <= 16 ? 16 : nchunk <= 32 ? 32 : 64;
    *hpq = (K == 1 || (D & 3) == 0) ? 1 : D == 2 ? 2 : 4;     // (K > 1: D is a power of two)
    *HL = K == 1 ? *group : (D & 3) == 0 ? (int)(D >> 2) : 1;
    return true;
}
bool gatmh_rows_ok(uint32_t K, uint32_t D, uint32_t ld) {
    int g, h, hl;
    return gatmh_rows_form(K, D, ld, &g, &h, &hl);
}

// F(group, hpq): the instantiations the launchers can select -- D == 2 means K*D <= 128 (K <= 64), D == 1 means K*D <= 64.
// The forward and the destination side: F(group, hpq, elfly) -- scores from the gathered row wherever that gives the el tensor's
// bits (rows_el): heads inside a lane, or a power-of-two float4 count
static bool gatmh_rows_elfly(int hpq, uint32_t ld) { return hpq > 1 || ((ld >> 2) & ((ld >> 2) - 1)) == 0; }
#define GATMH_ROWS_FORMS_EL(F)                                                                                                      \
    do {                                                                                                                            \
        if (hpq == 1 && elfly) { if (group == 8) F(8, 1, true); else if (group == 16) F(16, 1, true); else if (group == 32) F(32, 1, true); else F(64, 1, true); } \
        else if (hpq == 1) { if (group == 32) F(32, 1, false); else F(64, 1, false); }                                               \
        else if (hpq == 2) { if (group == 8) F(8, 2, true); else if (group == 16) F(16, 2, true); else F(32, 2, true); }             \
        else { if (group == 8) F(8, 4, true); else F(16, 4, true); }                                                                \
    } while (0)
#define GATMH_ROWS_FORMS(F)                                                                                                         \
    do {                                                                                                                            \
        if (hpq == 1) { if (group == 8) F(8, 1); else if (group == 16) F(16, 1); else if (group == 32) F(32, 1); else F(64, 1); }   \
        else if (hpq == 2) { if (group == 8) F(8, 2); else if (group == 16) F(16, 2); else F(32, 2); }                              \
        else { if (group == 8) F(8, 4); else F(16, 4); }                                                                            \
    } while (0)

size_t gatmh_rows_hub_state_floats(int pass, uint32_t ld, uint32_t ldk) { return rows_hub_stride(pass, ld, ldk); }
// a split pass (hubs with chunks in the plan): the grid of the first launch -- chunk units, then row units -- and of the merge launch
// dory_gatmh_row_gather_overlap: a launch over a row list -- the listed rows, after the hub rows' chunk units where the plan has any.
// *hubform: the list-hub form (the plan has chunks: the code the rows run with the switch off); *merge: with the chunk units, and the
// hub rows' merge launch follows (not for the launch before the wait: no chunk unit, a chunk size no row exceeds)
static void gatmh_rows_listed(const GatmhHubs *hubs, const GatmhRowList &list, uint32_t rpb, RowsHubArgs *H, RowsListArgs *R, dim3 *gl, dim3 *gm,
                              bool *hubform, bool *merge) {
    *hubform = hubs && hubs->plan.nchunks && hubs->state;
    *merge = *hubform && list.chunks;
    *H = RowsHubArgs{0, 0, 0xFFFFFFFFu, nullptr, nullptr, nullptr, nullptr};
    if (*merge) {
        const LongRowsDev &P = hubs->plan;
        *H = RowsHubArgs{P.nchunks, P.nrows, hubs->chunk, P.chunks, P.rows, P.row_chunk_ptr, hubs->state};
        *gm = dim3((P.nrows + rpb - 1) / rpb);
    }
    *R = RowsListArgs{list.rows, list.n};
    *gl = dim3((uint32_t)(((uint64_t)list.n + H->nchunks + rpb - 1) / rpb));
}
static bool gatmh_rows_split(const GatmhHubs *hubs, uint32_t N, uint32_t rpb, RowsHubArgs *H, dim3 *gr, dim3 *gm) {
    if (!hubs || !hubs->plan.nchunks || !hubs->state) return false;
    const LongRowsDev &P = hubs->plan;
    *H = RowsHubArgs{P.nchunks, P.nrows, hubs->chunk, P.chunks, P.rows, P.row_chunk_ptr, hubs->state};
    *gr = dim3((uint32_t)(((uint64_t)N + P.nchunks + rpb - 1) / rpb));
    *gm = dim3((P.nrows + rpb - 1) / rpb);
    return true;
}

// ---- the wide bf16 form's launches: what the launchers below do with GATMH_ROWS_BF16_WIDE.  `group` / HL: the narrow form's, for the
// hub rows' merge kernels (unchanged: the chunk states have the narrow layout)
bool gatmh_rows_wide_ok(uint32_t K, uint32_t D, uint32_t ld, const void *rows, const void *ghost_rows) {
    uint32_t lr, lh;
    int el;
    return gatmh_rows_ok(K, D, ld) && gatmh_rows8_form(K, D, ld, &lr, &lh, &el) && !(((uintptr_t)rows | (uintptr_t)ghost_rows) & 15);
}
struct Rows8Launch {
    int g8, hl8;
    bool elfly;
    uint32_t rpb8, rpb;
    dim3 bl{256};
    // false: not a shape of the wide form, or rows that are not 16-byte aligned (the callers ask gatmh_rows_wide_ok first)
    bool plan(const GatMhArgs &a, int group, const void *rows, const void *ghost_rows) {
        uint32_t lr, lh;
        int el;
        if (!gatmh_rows_wide_ok(a.K, a.D, a.ld, rows, ghost_rows) || !gatmh_rows8_form(a.K, a.D, a.ld, &lr, &lh, &el)) return false;
        g8 = (int)lr; hl8 = (int)lh; elfly = el != 0;
        rpb8 = 4 * (64 / lr); rpb = 4 * (64 / (uint32_t)group);
        return true;
    }
    dim3 merge_grid(uint32_t nrows) const { return dim3((nrows + rpb - 1) / rpb); }
};
#define GATMH_ROWS8_FORMS_EL(F)                                                                                                     \
    do {                                                                                                                            \
        if (W.elfly) { if (W.g8 == 8) F(8, true); else if (W.g8 == 16) F(16, true); else F(32, true); }                            \
        else { if (W.g8 == 16) F(16, false); else F(32, false); }                                                                   \
    } while (0)
#define GATMH_ROWS8_FORMS(F)                                                                                                        \
    do { if (W.g8 == 8) F(8); else if (W.g8 == 16) F(16); else F(32); } while (0)

static hipError_t launch_rows8_forward(const GatMhArgs &a, int group, int HL, const float *z, const float *zg, const float *el, const float *elg,
                                       const float *er, const float *a_l, float *o, float *op, float *m, float *den, float *dpos, hipStream_t s,
                                       const GatmhHubs *hubs, const GatmhRowList *list) {
    Rows8Launch W;
    if (!W.plan(a, group, z, zg)) return hipErrorInvalidValue;
    const uint4 *zb = reinterpret_cast<const uint4 *>(z), *zgb = reinterpret_cast<const uint4 *>(zg);
    const int hpq = 1;
    RowsHubArgs HA;
    RowsListArgs LA;
    dim3 gh, gm;
    bool hubform = false, merge = false;
    if (list) {
        gatmh_rows_listed(hubs, *list, W.rpb8, &HA, &LA, &gh, &gm, &hubform, &merge);
        if (gh.x == 0) return hipSuccess;
#define F(G, E)                                                                                                                     \
    do {                                                                                                                            \
        if (hubform) hipLaunchKernelGGL((gatmh_rows8_forward_list_hub_kernel<G, E>), gh, W.bl, 0, s, a, W.hl8, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos, HA, LA); \
        else hipLaunchKernelGGL((gatmh_rows8_forward_list_kernel<G, E>), gh, W.bl, 0, s, a, W.hl8, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos, LA); \
    } while (0)
        GATMH_ROWS8_FORMS_EL(F);
#undef F
    } else if ((merge = gatmh_rows_split(hubs, a.N, W.rpb8, &HA, &gh, &gm))) {
#define F(G, E) hipLaunchKernelGGL((gatmh_rows8_forward_hub_kernel<G, E>), gh, W.bl, 0, s, a, W.hl8, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos, HA)
        GATMH_ROWS8_FORMS_EL(F);
#undef F
    } else {
        const dim3 gr((a.N + W.rpb8 - 1) / W.rpb8);
#define F(G, E) hipLaunchKernelGGL((gatmh_rows8_forward_kernel<G, E>), gr, W.bl, 0, s, a, W.hl8, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos)
        GATMH_ROWS8_FORMS_EL(F);
#undef F
    }
    if (!merge) return hipGetLastError();
    gm = W.merge_grid(HA.nrows);
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_forward_merge_kernel<G, H>), gm, W.bl, 0, s, a, o, op, m, den, dpos, HA)
    GATMH_ROWS_FORMS(F);
#undef F
    (void)HL;
    return hipGetLastError();
}

static hipError_t launch_rows8_dst(const GatMhArgs &a, int group, const float *z, const float *zg, const float *el, const float *elg,
                                   const float *er, const float *a_l, const float *m, const float *den, const float *d_o, float *t, float *der,
                                   float4 *st4, uint32_t lds4, hipStream_t s, const GatmhHubs *hubs) {
    Rows8Launch W;
    if (!W.plan(a, group, z, zg)) return hipErrorInvalidValue;
    const uint4 *zb = reinterpret_cast<const uint4 *>(z), *zgb = reinterpret_cast<const uint4 *>(zg);
    const int hpq = 1;
    RowsHubArgs HA;
    dim3 gh, gm;
    if (!gatmh_rows_split(hubs, a.N, W.rpb8, &HA, &gh, &gm)) {
        const dim3 gr((a.N + W.rpb8 - 1) / W.rpb8);
#define F(G, E) hipLaunchKernelGGL((gatmh_rows8_dst_kernel<G, E>), gr, W.bl, 0, s, a, W.hl8, zb, zgb, el, elg, er, a_l, m, den, d_o, t, der, st4, lds4)
        GATMH_ROWS8_FORMS_EL(F);
#undef F
        return hipGetLastError();
    }
#define F(G, E) hipLaunchKernelGGL((gatmh_rows8_dst_hub_kernel<G, E>), gh, W.bl, 0, s, a, W.hl8, zb, zgb, el, elg, er, a_l, m, den, d_o, t, der, st4, lds4, HA)
    GATMH_ROWS8_FORMS_EL(F);
#undef F
    gm = W.merge_grid(HA.nrows);
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_dst_merge_kernel<G, H>), gm, W.bl, 0, s, a, er, m, den, t, der, st4, lds4, HA)
    GATMH_ROWS_FORMS(F);
#undef F
    return hipGetLastError();
}

static hipError_t launch_rows8_src(const GatMhArgs &a, int group, int HL, const float *z, const float *el, const float *d_o, const float *dog,
                                   const float4 *st4, const float4 *stg, uint32_t lds4, const float *der, const float *a_l, const float *a_r,
                                   float *del, float *dz, hipStream_t s, const GatmhHubs *hubs, const GatmhRowList *list) {
    Rows8Launch W;
    if (!W.plan(a, group, d_o, dog)) return hipErrorInvalidValue;
    const uint4 *dob = reinterpret_cast<const uint4 *>(d_o), *dogb = reinterpret_cast<const uint4 *>(dog);
    const int hpq = 1;
    RowsHubArgs HA;
    RowsListArgs LA;
    dim3 gh, gm;
    bool hubform = false, merge = false;
    if (list) {
        gatmh_rows_listed(hubs, *list, W.rpb8, &HA, &LA, &gh, &gm, &hubform, &merge);
        if (gh.x == 0) return hipSuccess;
#define F(G)                                                                                                                        \
    do {                                                                                                                            \
        if (hubform) hipLaunchKernelGGL((gatmh_rows8_src_list_hub_kernel<G>), gh, W.bl, 0, s, a, W.hl8, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz, HA, LA); \
        else hipLaunchKernelGGL((gatmh_rows8_src_list_kernel<G>), gh, W.bl, 0, s, a, W.hl8, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz, LA); \
    } while (0)
        GATMH_ROWS8_FORMS(F);
#undef F
    } else if ((merge = gatmh_rows_split(hubs, a.N, W.rpb8, &HA, &gh, &gm))) {
#define F(G) hipLaunchKernelGGL((gatmh_rows8_src_hub_kernel<G>), gh, W.bl, 0, s, a, W.hl8, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz, HA)
        GATMH_ROWS8_FORMS(F);
#undef F
    } else {
        const dim3 gr((a.N + W.rpb8 - 1) / W.rpb8);
#define F(G) hipLaunchKernelGGL((gatmh_rows8_src_kernel<G>), gr, W.bl, 0, s, a, W.hl8, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz)
        GATMH_ROWS8_FORMS(F);
#undef F
    }
    if (!merge) return hipGetLastError();
    gm = W.merge_grid(HA.nrows);   // (the narrow merge kernel: the narrow form's lanes per head reduce its closing dot product)
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_src_merge_kernel<G, H>), gm, W.bl, 0, s, a, HL, z, der, a_l, a_r, del, dz, HA)
    GATMH_ROWS_FORMS(F);
#undef F
    return hipGetLastError();
}
#undef GATMH_ROWS8_FORMS
#undef GATMH_ROWS8_FORMS_EL

hipError_t launch_gatmh_rows_forward(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr,
                                     const uint32_t *rowidx, const float *z, const float *zg, const float *el, const float *elg,
                                     const float *er, const float *a_l, float *o, float *op, float *m, float *den, float *dpos,
                                     hipStream_t s, int form, const GatmhHubs *hubs, const GatmhRowList *list) {
    if (N == 0) return hipSuccess;
    int group, hpq, HL;
    if (!gatmh_rows_form(K, D, ld, &group, &hpq, &HL) || (hpq == 2 && group > 32) || (hpq == 4 && group > 16)) return hipErrorInvalidValue;
    const bool bf16 = form != GATMH_ROWS_FP32;
    GatMhArgs a{N, K, D, ld, ldk, colptr, rowidx};
    if (form == GATMH_ROWS_BF16_WIDE) return launch_rows8_forward(a, group, HL, z, zg, el, elg, er, a_l, o, op, m, den, dpos, s, hubs, list);
    const uint32_t rpb = 4 * (64 / (uint32_t)group);
    const dim3 gr((N + rpb - 1) / rpb), bl(256);
    const bool elfly = gatmh_rows_elfly(hpq, ld);
    RowsHubArgs HA;
    dim3 gh, gm;
    if (list) {   // dory_gatmh_row_gather_overlap: the listed rows (with the hub rows' chunks and their merge, where the caller hands hubs)
        RowsListArgs LA;
        bool hubform, merge;
        gatmh_rows_listed(hubs, *list, rpb, &HA, &LA, &gh, &gm, &hubform, &merge);
        if (gh.x == 0) return hipSuccess;
        const uint2 *zb = reinterpret_cast<const uint2 *>(z), *zgb = reinterpret_cast<const uint2 *>(zg);
#define F(G, H, E)                                                                                                                  \
    do {                                                                                                                            \
        if (hubform && bf16) hipLaunchKernelGGL((gatmh_rows_forward_list_hub_bf16_kernel<G, H, E>), gh, bl, 0, s, a, HL, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos, HA, LA); \
        else if (hubform) hipLaunchKernelGGL((gatmh_rows_forward_list_hub_kernel<G, H, E>), gh, bl, 0, s, a, HL, z, zg, el, elg, er, a_l, o, op, m, den, dpos, HA, LA); \
        else if (bf16) hipLaunchKernelGGL((gatmh_rows_forward_list_bf16_kernel<G, H, E>), gh, bl, 0, s, a, HL, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos, LA); \
        else hipLaunchKernelGGL((gatmh_rows_forward_list_kernel<G, H, E>), gh, bl, 0, s, a, HL, z, zg, el, elg, er, a_l, o, op, m, den, dpos, LA); \
    } while (0)
        GATMH_ROWS_FORMS_EL(F);
#undef F
        if (!merge) return hipGetLastError();
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_forward_merge_kernel<G, H>), gm, bl, 0, s, a, o, op, m, den, dpos, HA)
        GATMH_ROWS_FORMS(F);
#undef F
        return hipGetLastError();
    }
    if (gatmh_rows_split(hubs, N, rpb, &HA, &gh, &gm)) {   // hub rows: their chunks and the other rows, then the merge
        const uint2 *zb = reinterpret_cast<const uint2 *>(z), *zgb = reinterpret_cast<const uint2 *>(zg);
#define F(G, H, E)                                                                                                                  \
    do {                                                                                                                            \
        if (bf16) hipLaunchKernelGGL((gatmh_rows_forward_hub_bf16_kernel<G, H, E>), gh, bl, 0, s, a, HL, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos, HA); \
        else hipLaunchKernelGGL((gatmh_rows_forward_hub_kernel<G, H, E>), gh, bl, 0, s, a, HL, z, zg, el, elg, er, a_l, o, op, m, den, dpos, HA); \
    } while (0)
        GATMH_ROWS_FORMS_EL(F);
#undef F
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_forward_merge_kernel<G, H>), gm, bl, 0, s, a, o, op, m, den, dpos, HA)
        GATMH_ROWS_FORMS(F);
#undef F
        return hipGetLastError();
    }
    if (bf16) {   // z / zg: the shadow rows
        const uint2 *zb = reinterpret_cast<const uint2 *>(z), *zgb = reinterpret_cast<const uint2 *>(zg);
#define F(G, H, E) hipLaunchKernelGGL((gatmh_rows_forward_bf16_kernel<G, H, E>), gr, bl, 0, s, a, HL, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos)
        GATMH_ROWS_FORMS_EL(F);
#undef F
        return hipGetLastError();
    }
#define F(G, H, E) hipLaunchKernelGGL((gatmh_rows_forward_kernel<G, H, E>), gr, bl, 0, s, a, HL, z, zg, el, elg, er, a_l, o, op, m, den, dpos)
    GATMH_ROWS_FORMS_EL(F);
#undef F
    return hipGetLastError();
}

hipError_t launch_gatmh_rows_dst(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr,
                                 const uint32_t *rowidx, const float *z, const float *zg, const float *el, const float *elg,
                                 const float *er, const float *a_l, const float *m, const float *den, const float *d_o, float *t, float *der,
                                 float4 *st4, uint32_t lds4, hipStream_t s, int form, const GatmhHubs *hubs) {
    if (N == 0) return hipSuccess;
    int group, hpq, HL;
    if (!gatmh_rows_form(K, D, ld, &group, &hpq, &HL) || (hpq == 2 && group > 32) || (hpq == 4 && group > 16)) return hipErrorInvalidValue;
    const bool bf16 = form != GATMH_ROWS_FP32;
    GatMhArgs a{N, K, D, ld, ldk, colptr, rowidx};
    if (form == GATMH_ROWS_BF16_WIDE) return launch_rows8_dst(a, group, z, zg, el, elg, er, a_l, m, den, d_o, t, der, st4, lds4, s, hubs);
    const uint32_t rpb = 4 * (64 / (uint32_t)group);
    const dim3 gr((N + rpb - 1) / rpb), bl(256);
    const bool elfly = gatmh_rows_elfly(hpq, ld);
    RowsHubArgs HA;
    dim3 gh, gm;
    if (gatmh_rows_split(hubs, N, rpb, &HA, &gh, &gm)) {
        const uint2 *zb = reinterpret_cast<const uint2 *>(z), *zgb = reinterpret_cast<const uint2 *>(zg);
#define F(G, H, E)                                                                                                                  \
    do {                                                                                                                            \
        if (bf16) hipLaunchKernelGGL((gatmh_rows_dst_hub_bf16_kernel<G, H, E>), gh, bl, 0, s, a, HL, zb, zgb, el, elg, er, a_l, m, den, d_o, t, der, st4, lds4, HA); \
        else hipLaunchKernelGGL((gatmh_rows_dst_hub_kernel<G, H, E>), gh, bl, 0, s, a, HL, z, zg, el, elg, er, a_l, m, den, d_o, t, der, st4, lds4, HA); \
    } while (0)
        GATMH_ROWS_FORMS_EL(F);
#undef F
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_dst_merge_kernel<G, H>), gm, bl, 0, s, a, er, m, den, t, der, st4, lds4, HA)
        GATMH_ROWS_FORMS(F);
#undef F
        return hipGetLastError();
    }
    if (bf16) {   // z / zg: the shadow rows
        const uint2 *zb = reinterpret_cast<const uint2 *>(z), *zgb = reinterpret_cast<const uint2 *>(zg);
#define F(G, H, E) hipLaunchKernelGGL((gatmh_rows_dst_bf16_kernel<G, H, E>), gr, bl, 0, s, a, HL, zb, zgb, el, elg, er, a_l, m, den, d_o, t, der, st4, lds4)
        GATMH_ROWS_FORMS_EL(F);
#undef F
        return hipGetLastError();
    }
#define F(G, H, E) hipLaunchKernelGGL((gatmh_rows_dst_kernel<G, H, E>), gr, bl, 0, s, a, HL, z, zg, el, elg, er, a_l, m, den, d_o, t, der, st4, lds4)
    GATMH_ROWS_FORMS_EL(F);
#undef F
    return hipGetLastError();
}

hipError_t launch_gatmh_rows_src(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *rowptr,
                                 const uint32_t *colidx, const float *z, const float *el, const float *d_o, const float *dog,
                                 const float4 *st4, const float4 *stg, uint32_t lds4, const float *der, const float *a_l, const float *a_r,
                                 float *del, float *dz, hipStream_t s, int form, const GatmhHubs *hubs, const GatmhRowList *list) {
    if (N == 0) return hipSuccess;
    int group, hpq, HL;
    if (!gatmh_rows_form(K, D, ld, &group, &hpq, &HL) || (hpq == 2 && group > 32) || (hpq == 4 && group > 16)) return hipErrorInvalidValue;
    const bool bf16 = form != GATMH_ROWS_FP32;
    GatMhArgs a{N, K, D, ld, ldk, rowptr, colidx};
    if (form == GATMH_ROWS_BF16_WIDE) return launch_rows8_src(a, group, HL, z, el, d_o, dog, st4, stg, lds4, der, a_l, a_r, del, dz, s, hubs, list);
    const uint32_t rpb = 4 * (64 / (uint32_t)group);
    const dim3 gr((N + rpb - 1) / rpb), bl(256);
    RowsHubArgs HA;
    dim3 gh, gm;
    if (list) {   // dory_gatmh_row_gather_overlap: as in launch_gatmh_rows_forward
        RowsListArgs LA;
        bool hubform, merge;
        gatmh_rows_listed(hubs, *list, rpb, &HA, &LA, &gh, &gm, &hubform, &merge);
        if (gh.x == 0) return hipSuccess;
        const uint2 *dob = reinterpret_cast<const uint2 *>(d_o), *dogb = reinterpret_cast<const uint2 *>(dog);
#define F(G, H)                                                                                                                     \
    do {                                                                                                                            \
        if (hubform && bf16) hipLaunchKernelGGL((gatmh_rows_src_list_hub_bf16_kernel<G, H, (H == 4 ? 2 : 4)>), gh, bl, 0, s, a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz, HA, LA); \
        else if (hubform) hipLaunchKernelGGL((gatmh_rows_src_list_hub_kernel<G, H, (H == 4 ? 2 : 4)>), gh, bl, 0, s, a, HL, z, el, d_o, dog, st4, stg, lds4, der, a_l, a_r, del, dz, HA, LA); \
        else if (bf16) hipLaunchKernelGGL((gatmh_rows_src_list_bf16_kernel<G, H, (H == 4 ? 2 : 4)>), gh, bl, 0, s, a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz, LA); \
        else hipLaunchKernelGGL((gatmh_rows_src_list_kernel<G, H, (H == 4 ? 2 : 4)>), gh, bl, 0, s, a, HL, z, el, d_o, dog, st4, stg, lds4, der, a_l, a_r, del, dz, LA); \
    } while (0)
        GATMH_ROWS_FORMS(F);
#undef F
        if (!merge) return hipGetLastError();
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_src_merge_kernel<G, H>), gm, bl, 0, s, a, HL, z, der, a_l, a_r, del, dz, HA)
        GATMH_ROWS_FORMS(F);
#undef F
        return hipGetLastError();
    }
    if (gatmh_rows_split(hubs, N, rpb, &HA, &gh, &gm)) {
        const uint2 *dob = reinterpret_cast<const uint2 *>(d_o), *dogb = reinterpret_cast<const uint2 *>(dog);
#define F(G, H)                                                                                                                     \
    do {                                                                                                                            \
        if (bf16) hipLaunchKernelGGL((gatmh_rows_src_hub_bf16_kernel<G, H, (H == 4 ? 2 : 4)>), gh, bl, 0, s, a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz, HA); \
        else hipLaunchKernelGGL((gatmh_rows_src_hub_kernel<G, H, (H == 4 ? 2 : 4)>), gh, bl, 0, s, a, HL, z, el, d_o, dog, st4, stg, lds4, der, a_l, a_r, del, dz, HA); \
    } while (0)
        GATMH_ROWS_FORMS(F);
#undef F
#define F(G, H) hipLaunchKernelGGL((gatmh_rows_src_merge_kernel<G, H>), gm, bl, 0, s, a, HL, z, der, a_l, a_r, del, dz, HA)
        GATMH_ROWS_FORMS(F);
#undef F
        return hipGetLastError();
    }
    if (bf16) {   // d_o / dog: the shadow rows
        const uint2 *dob = reinterpret_cast<const uint2 *>(d_o), *dogb = reinterpret_cast<const uint2 *>(dog);
#define F(G, H)                                                                                                                     \
    hipLaunchKernelGGL((gatmh_rows_src_bf16_kernel<G, H, (H == 4 ? 2 : 4)>), gr, bl, 0, s, a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, \
                       a_r, del, dz)
        GATMH_ROWS_FORMS(F);
#undef F
        return hipGetLastError();
    }
#define F(G, H)                                                                                                                     \
    hipLaunchKernelGGL((gatmh_rows_src_kernel<G, H, (H == 4 ? 2 : 4)>), gr, bl, 0, s, a, HL, z, el, d_o, dog, st4, stg, lds4, der, a_l, \
                       a_r, del, dz)
    GATMH_ROWS_FORMS(F);
#undef F
    return hipGetLastError();
}

// dory_gatmh_row_gather_edge_split: one launch of the carry form -- walk GATMH_WALK_BOTH / _FIRST over all N rows, _SECOND over the
// boundary rows of the copy (none: nothing to launch).  fp32 rows or the narrow bf16 form; a walk that parks or loads states needs cy.state
static bool gatmh_rows_carry_args(const GatmhCarry &cy, int walk, uint32_t N, uint32_t rpb, RowsCarryArgs *C, dim3 *g) {
    if (!cy.idx || !cy.mid || walk < GATMH_WALK_BOTH || walk > GATMH_WALK_SECOND) return false;
    if (walk != GATMH_WALK_BOTH && !cy.state) return false;
    if (walk == GATMH_WALK_SECOND && cy.nrows && !cy.rows) return false;
    *C = RowsCarryArgs{cy.mid, cy.rows, cy.nrows, cy.state,
                       walk == GATMH_WALK_BOTH ? ROWS_WALK_BOTH : walk == GATMH_WALK_FIRST ? ROWS_WALK_FIRST : ROWS_WALK_SECOND};
    const uint32_t units = walk == GATMH_WALK_SECOND ? cy.nrows : N;
    *g = dim3((units + rpb - 1) / rpb);
    return true;
}
hipError_t launch_gatmh_rows_forward_carry(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr, const float *z,
                                           const float *zg, const float *el, const float *elg, const float *er, const float *a_l, float *o,
                                           float *op, float *m, float *den, float *dpos, hipStream_t s, int form, const GatmhCarry &cy,
                                           int walk) {
    if (N == 0) return hipSuccess;
    int group, hpq, HL;
    if (!gatmh_rows_form(K, D, ld, &group, &hpq, &HL) || (hpq == 2 && group > 32) || (hpq == 4 && group > 16)) return hipErrorInvalidValue;
    if (form != GATMH_ROWS_FP32 && form != GATMH_ROWS_BF16) return hipErrorInvalidValue;   // (no wide carry form)
    const bool bf16 = form == GATMH_ROWS_BF16;
    GatMhArgs a{N, K, D, ld, ldk, colptr, cy.idx};
    const uint32_t rpb = 4 * (64 / (uint32_t)group);
    const dim3 bl(256);
    const bool elfly = gatmh_rows_elfly(hpq, ld);
    RowsCarryArgs CA;
    dim3 gc;
    if (!gatmh_rows_carry_args(cy, walk, N, rpb, &CA, &gc)) return hipErrorInvalidValue;
    if (gc.x == 0) return hipSuccess;
    const uint2 *zb = reinterpret_cast<const uint2 *>(z), *zgb = reinterpret_cast<const uint2 *>(zg);
#define F(G, H, E)                                                                                                                  \
    do {                                                                                                                            \
        if (bf16) hipLaunchKernelGGL((gatmh_rows_forward_carry_bf16_kernel<G, H, E>), gc, bl, 0, s, a, HL, zb, zgb, el, elg, er, a_l, o, op, m, den, dpos, CA); \
        else hipLaunchKernelGGL((gatmh_rows_forward_carry_kernel<G, H, E>), gc, bl, 0, s, a, HL, z, zg, el, elg, er, a_l, o, op, m, den, dpos, CA); \
    } while (0)
    GATMH_ROWS_FORMS_EL(F);
#undef F
    return hipGetLastError();
}
hipError_t launch_gatmh_rows_src_carry(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *rowptr, const float *z,
                                       const float *el, const float *d_o, const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                       const float *der, const float *a_l, const float *a_r, float *del, float *dz, hipStream_t s, int form,
                                       const GatmhCarry &cy, int walk) {
    if (N == 0) return hipSuccess;
    int group, hpq, HL;
    if (!gatmh_rows_form(K, D, ld, &group, &hpq, &HL) || (hpq == 2 && group > 32) || (hpq == 4 && group > 16)) return hipErrorInvalidValue;
    if (form != GATMH_ROWS_FP32 && form != GATMH_ROWS_BF16) return hipErrorInvalidValue;
    const bool bf16 = form == GATMH_ROWS_BF16;
    GatMhArgs a{N, K, D, ld, ldk, rowptr, cy.idx};
    const uint32_t rpb = 4 * (64 / (uint32_t)group);
    const dim3 bl(256);
    RowsCarryArgs CA;
    dim3 gc;
    if (!gatmh_rows_carry_args(cy, walk, N, rpb, &CA, &gc)) return hipErrorInvalidValue;
    if (gc.x == 0) return hipSuccess;
    const uint2 *dob = reinterpret_cast<const uint2 *>(d_o), *dogb = reinterpret_cast<const uint2 *>(dog);
#define F(G, H)                                                                                                                     \
    do {                                                                                                                            \
        if (bf16) hipLaunchKernelGGL((gatmh_rows_src_carry_bf16_kernel<G, H, (H == 4 ? 2 : 4)>), gc, bl, 0, s, a, HL, z, el, dob, dogb, st4, stg, lds4, der, a_l, a_r, del, dz, CA); \
        else hipLaunchKernelGGL((gatmh_rows_src_carry_kernel<G, H, (H == 4 ? 2 : 4)>), gc, bl, 0, s, a, HL, z, el, d_o, dog, st4, stg, lds4, der, a_l, a_r, del, dz, CA); \
    } while (0)
    GATMH_ROWS_FORMS(F);
#undef F
    return hipGetLastError();
}
#undef GATMH_ROWS_FORMS
#undef GATMH_ROWS_FORMS_EL

}  // namespace dory
