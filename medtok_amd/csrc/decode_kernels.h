// Decode: (token ids, soft-assignment weights) -> embedding, and its backward.  Included by medtok_vq.hip (uses ld4 / st4).
//
// What a forward stores per code and modality slot -- k region-local ids and k softmax weights -- determines the slot's e_dim block of
// the embedding: sum_j w_j * what[lo + idx_j] over the normalised codebook `what` (soft_assign_kernel's code mix with
// MEDTOK_ASSIGN_RAW).  No matrix work: per (row, slot) the kernel reads 12 k bytes of ids and weights, gathers k rows of the codebook
// (L2 / Infinity Cache: the whole table is 5 MB at the reference shape and 151 MB at n_e = 49152, D = 768) and writes 4 D bytes.
//
// Mapping: one item = one (row, slot).  LANES lanes own an item and stride its D axis in float4: LANES = 64 (a wavefront per item, four
// items per block) for wide rows, LANES = 16 (four items per wavefront, as rownorm16_kernel) for rows of at most 64 floats, where a
// whole wavefront would leave 48 lanes without an element.  Lane j < k of the group loads id j and weight j once; they reach the other
// lanes by a shuffle.  The k row gathers of a float4 column are issued before the first multiply-add.
//
// Arithmetic: per element ONE fp32 chain acc = +0; acc = fmaf(w_j, what[lo + idx_j][i], acc), j = 0 .. k-1 in list order: the same
// bits under either mapping and for any number of slots per call.
//
// Ids are validated here: an id outside [0, size_s) never forms an address.  The item's block is written as zeros and bit s of the
// caller's status word is set with an ordinary atomicOr from a vector lane (no assert, no trap: the caller turns the word into an error).
#pragma once

#define MEDTOK_DECODE_MAX_SLOTS 4

struct DecodeRegions {
    long lo[MEDTOK_DECODE_MAX_SLOTS], size[MEDTOK_DECODE_MAX_SLOTS];
};

// What both kernels start with: the item of this lane group, its k (code row, weight) pairs in every lane, whether any id is bad.
template <int LANES, int MAXK>
struct DecodeItem {
    long item, row, lo;
    int slot, own;                   // own: the codebook row of THIS lane's id (lanes sub < k)
    bool live, bad;
    int cj[MAXK];
    float wj[MAXK];

    __device__ __forceinline__ void load(const int64_t *__restrict__ tokens, const float *__restrict__ weights, long items, int slots, int topk,
                                         const DecodeRegions &reg, int *status)
    {
        const int lane = threadIdx.x & 63, sub = threadIdx.x & (LANES - 1), base = lane & ~(LANES - 1);
        item = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES;
        live = item < items;
        if (!live) item = 0;
        row = item / slots;
        slot = (int)(item - row * slots);
        lo = reg.lo[0];
        long size = reg.size[0];
#pragma unroll
        for (int s = 1; s < MEDTOK_DECODE_MAX_SLOTS; ++s)       // (selects on constant indices: the regions stay in scalar registers)
            if (slot == s) { lo = reg.lo[s]; size = reg.size[s]; }
        long id = 0;
        float wv = 0.f;
        if (live && sub < topk) { id = tokens[item * topk + sub]; wv = weights[item * topk + sub]; }
        const bool bad_lane = id < 0 || id >= size;             // (a lane without an id holds 0: in range, size >= 1)
        const unsigned long long votes = __ballot(bad_lane);
        if (LANES == 64) bad = votes != 0ull;
        else bad = ((votes >> base) & ((1ull << (LANES & 63)) - 1ull)) != 0ull;
        const int code = bad_lane ? 0 : (int)(lo + id);          // lo + size <= n_codes < 2^31 (checked on the host)
        own = code;
#pragma unroll
        for (int j = 0; j < MAXK; ++j) {
            cj[j] = __shfl(code, base + j, 64);
            wj[j] = __shfl(wv, base + j, 64);
        }
        if (bad && live && sub == 0 && status) atomicOr(status, 1 << slot);
    }
};

template <int LANES, int MAXK>
__global__ __launch_bounds__(256) void decode_tokens_kernel(const int64_t *__restrict__ tokens, const float *__restrict__ weights, long items,
                                                            int slots, int topk, const float *__restrict__ what, int d, DecodeRegions reg,
                                                            float *__restrict__ out, long out_stride, int *status)
{
    static_assert(MAXK <= LANES, "lane j of a group loads id j");
    const int sub = threadIdx.x & (LANES - 1);
    DecodeItem<LANES, MAXK> it;
    it.load(tokens, weights, items, slots, topk, reg, status);
    if (!it.live) return;
    float *dst = out + it.row * out_stride + (long)it.slot * d;
    for (int i = sub * 4; i < d; i += LANES * 4) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!it.bad) {
            float4 e[MAXK];
#pragma unroll
            for (int j = 0; j < MAXK; ++j)                       // the k gathers of this column: in flight together
                if (j < topk) e[j] = ld4(what + (long)it.cj[j] * d + i);
#pragma unroll
            for (int j = 0; j < MAXK; ++j)
                if (j < topk) {
                    a.x = fmaf(it.wj[j], e[j].x, a.x); a.y = fmaf(it.wj[j], e[j].y, a.y);
                    a.z = fmaf(it.wj[j], e[j].z, a.z); a.w = fmaf(it.wj[j], e[j].w, a.w);
                }
        }
        st4(dst + i, a);
    }
}

// Backward.  With g = g_out[row, slot block] and e_j = what[lo + idx_j]:
//   g_w[item, j]            = <g, e_j>       per lane one fmaf chain over its float4s in increasing i (x, y, z, w), joined by the xor
//                                            butterfly over the group's lanes (offsets LANES/2 .. 1): a fixed order
//   g_code[item * k + j, :] = w_j * g        the gradient w.r.t. the NORMALISED code, one row per (item, j)
//   g_ids[item * k + j]     = lo + idx_j     the row of the codebook it belongs to (what medtok_ema_stats_f32 sums per code)
// Either output may be NULL.  An item with a bad id contributes nothing: zeros, filed under the region's first code.
template <int LANES, int MAXK>
__global__ __launch_bounds__(256) void decode_tokens_backward_kernel(const float *__restrict__ g_out, long g_stride, const int64_t *__restrict__ tokens,
                                                                     const float *__restrict__ weights, long items, int slots, int topk,
                                                                     const float *__restrict__ what, int d, DecodeRegions reg,
                                                                     float *__restrict__ g_w, float *__restrict__ g_code, int64_t *__restrict__ g_ids,
                                                                     int *status)
{
    static_assert(MAXK <= LANES, "lane j of a group loads id j");
    const int sub = threadIdx.x & (LANES - 1);
    DecodeItem<LANES, MAXK> it;
    it.load(tokens, weights, items, slots, topk, reg, status);
    const bool work = it.live && !it.bad;
    float dot[MAXK];
#pragma unroll
    for (int j = 0; j < MAXK; ++j) dot[j] = 0.f;
    const float *g = g_out + it.row * g_stride + (long)it.slot * d;
    float *gc = g_code ? g_code + it.item * topk * d : nullptr;
    if (it.live) {
        for (int i = sub * 4; i < d; i += LANES * 4) {
            const float4 gv = work ? ld4(g + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (g_w && work) {
                float4 e[MAXK];
#pragma unroll
                for (int j = 0; j < MAXK; ++j)
                    if (j < topk) e[j] = ld4(what + (long)it.cj[j] * d + i);
#pragma unroll
                for (int j = 0; j < MAXK; ++j)
                    if (j < topk) {
                        dot[j] = fmaf(gv.x, e[j].x, dot[j]); dot[j] = fmaf(gv.y, e[j].y, dot[j]);
                        dot[j] = fmaf(gv.z, e[j].z, dot[j]); dot[j] = fmaf(gv.w, e[j].w, dot[j]);
                    }
            }
            if (gc) {
#pragma unroll
                for (int j = 0; j < MAXK; ++j)
                    if (j < topk) {
                        const float w = it.wj[j];
                        st4(gc + (long)j * d + i, work ? make_float4(w * gv.x, w * gv.y, w * gv.z, w * gv.w) : make_float4(0.f, 0.f, 0.f, 0.f));
                    }
            }
        }
    }
    if (g_w) {                                                   // (every lane of the wavefront takes part in the shuffles)
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < MAXK; ++j)
            if (j < topk) {
                float p = dot[j];
#pragma unroll
                for (int off = LANES / 2; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
                mine = (sub == j) ? p : mine;
            }
        if (it.live && sub < topk) g_w[it.item * topk + sub] = mine;
    }
    if (g_ids && it.live && sub < topk) g_ids[it.item * topk + sub] = it.bad ? it.lo : (long)it.own;
}
