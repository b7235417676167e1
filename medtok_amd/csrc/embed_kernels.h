// Embedding lookup over the stored token table: code indices -> embeddings, and the gradient of the "missing code" row.  Included by
// medtok_vq.hip behind decode_kernels.h (uses ld4 / st4, DecodeRegions).
//
// A downstream model indexes a [num_codes + 1, S * d] table with a [B, L] batch of code indices (row num_codes: the learned row of
// a code the table does not know; padded positions are masked).  The table's rows are what decode makes of tokens [num_codes, S, k]
// and weights [num_codes, S, k], so embed_codes_kernel is decode_tokens_kernel with one indirection in front: per (position, slot)
// it reads the position's code index, then the 12 k bytes of that code's ids and weights, gathers k rows of the codebook and writes
// the slot's d floats.  Neither the table nor gathered copies of the id / weight rows ever exist.
//
// Mapping, arithmetic and id validation are decode's (decode_kernels.h): one item = one (position, slot), LANES = 64 or 16 lanes per
// item, lane j < k loads id j and weight j, a shuffle hands them round, the k gathers of a float4 column are issued before the first
// fmaf, per element ONE fp32 chain acc = +0; acc = fmaf(w_j, e_j, acc) in list order -- the bits of decode_tokens_kernel on the
// gathered rows.  Per position p with c = index[p]:
//   pad[p] != 0               zeros; index[p] is not read, nor are the tables, and status is not touched
//   0 <= c < num_codes        the decoded row of code c (a slot with an id outside its region: zeros, bit `slot` of *status)
//   c == num_codes, miss      a copy of miss [S * d]
//   anything else             zeros, bit 4 of *status
// No index and no id forms an address before it has been checked; every product with c is 64-bit (num_codes * S * k > 2^31 at 600k
// codes x 4 x 5 and beyond).  OUT = float, _Float16 or __bf16: each element of the finished fp32 chain is rounded once, to nearest even.
#pragma once

#define MEDTOK_EMBED_BAD_INDEX_BIT 4

__device__ __forceinline__ void embed_store4(float *p, float4 v) { st4(p, v); }
__device__ __forceinline__ void embed_store4(_Float16 *p, float4 v)
{
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 h;
    h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
    *reinterpret_cast<h4 *>(p) = h;
}
__device__ __forceinline__ void embed_store4(__bf16 *p, float4 v)
{
    typedef __bf16 b4 __attribute__((ext_vector_type(4)));
    b4 h;
    h[0] = (__bf16)v.x; h[1] = (__bf16)v.y; h[2] = (__bf16)v.z; h[3] = (__bf16)v.w;
    *reinterpret_cast<b4 *>(p) = h;
}

template <int LANES, int MAXK, typename OUT>
__global__ __launch_bounds__(256) void embed_codes_kernel(const int64_t *__restrict__ index, const uint8_t *__restrict__ pad, long items,
                                                          const int64_t *__restrict__ tokens, const float *__restrict__ weights, long num_codes,
                                                          int slots, int topk, const float *__restrict__ what, int d, DecodeRegions reg,
                                                          const float *__restrict__ miss, OUT *__restrict__ out, long out_stride, int *status)
{
    static_assert(MAXK <= LANES, "lane j of a group loads id j");
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (LANES - 1), base = lane & ~(LANES - 1);
    long item = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES;
    const bool live = item < items;
    if (!live) item = 0;
    const long pos = item / slots;
    const int slot = (int)(item - pos * slots);
    long lo = reg.lo[0], size = reg.size[0];
#pragma unroll
    for (int s = 1; s < MEDTOK_DECODE_MAX_SLOTS; ++s)           // (selects on constant indices: the regions stay in scalar registers)
        if (slot == s) { lo = reg.lo[s]; size = reg.size[s]; }
    // what this position is: the lanes of a group agree (one address each), so every branch below is uniform over the group
    const bool padded = !live || (pad && pad[pos] != 0);
    const long c = padded ? 0 : index[pos];
    const bool is_code = !padded && c >= 0 && c < num_codes;
    const bool is_miss = !padded && miss && c == num_codes;
    if (!padded && !is_code && !is_miss && sub == 0 && slot == 0 && status) atomicOr(status, 1 << MEDTOK_EMBED_BAD_INDEX_BIT);
    long id = 0;
    float wv = 0.f;
    if (is_code && sub < topk) {
        const long at = (c * slots + slot) * topk + sub;          // 64-bit: c < num_codes was checked above
        id = tokens[at];
        wv = weights[at];
    }
    const bool bad_lane = id < 0 || id >= size;                 // (a lane without an id holds 0: in range, size >= 1)
    const unsigned long long votes = __ballot(bad_lane);
    bool bad;
    if (LANES == 64) bad = votes != 0ull;
    else bad = ((votes >> base) & ((1ull << (LANES & 63)) - 1ull)) != 0ull;
    const int code = bad_lane ? 0 : (int)(lo + id);              // lo + size <= n_codes < 2^31 (checked on the host)
    int cj[MAXK];
    float wj[MAXK];
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
        cj[j] = __shfl(code, base + j, 64);
        wj[j] = __shfl(wv, base + j, 64);
    }
    if (bad && sub == 0 && status) atomicOr(status, 1 << slot);  // (bad implies is_code: only such groups loaded an id)
    if (!live) return;
    OUT *dst = out + pos * out_stride + (long)slot * d;
    const float *mrow = is_miss ? miss + (long)slot * d : nullptr;
    const bool mix = is_code && !bad;
    for (int i = sub * 4; i < d; i += LANES * 4) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (mix) {
            float4 e[MAXK];
#pragma unroll
            for (int j = 0; j < MAXK; ++j)                       // the k gathers of this column: in flight together
                if (j < topk) e[j] = ld4(what + (long)cj[j] * d + i);
#pragma unroll
            for (int j = 0; j < MAXK; ++j)
                if (j < topk) {
                    a.x = fmaf(wj[j], e[j].x, a.x); a.y = fmaf(wj[j], e[j].y, a.y);
                    a.z = fmaf(wj[j], e[j].z, a.z); a.w = fmaf(wj[j], e[j].w, a.w);
                }
        } else if (is_miss) {
            a = ld4(mrow + i);
        }
        embed_store4(dst + i, a);
    }
}

// Gradient of the miss row: g_miss[col] = sum over the positions p with index[p] == num_codes and pad[p] == 0 of g_out[p, col], fp32,
// in a FIXED order and without float atomics: a block owns MEDTOK_EMBED_GRAD_CHUNK consecutive positions and adds its miss rows in
// position order into partial[chunk, col] (embed_miss_grad_partial_kernel; a chunk without a miss writes zeros); the partials are then
// added in chunk order (embed_miss_grad_sum_kernel).  Two runs give the same bits.
//
// A block first compacts its chunk: thread t tests position chunk * 256 + t, a ballot per wavefront and the counts of the wavefronts
// before it place the miss positions into LDS in position order -- 1 % of the positions are misses at the consumer's shapes, and the
// column loop then touches those rows only.  grid = (chunks, ceil(width / 256)); a thread owns one column (coalesced over the block).
#define MEDTOK_EMBED_GRAD_CHUNK 256

__global__ __launch_bounds__(256) void embed_miss_grad_partial_kernel(const float *__restrict__ g_out, long g_stride, const int64_t *__restrict__ index,
                                                                      const uint8_t *__restrict__ pad, long n, long num_codes, int width,
                                                                      float *__restrict__ partial)
{
    __shared__ int list[MEDTOK_EMBED_GRAD_CHUNK];
    __shared__ int wave_count[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long first = (long)blockIdx.x * MEDTOK_EMBED_GRAD_CHUNK, p = first + t;
    const bool hit = p < n && !(pad && pad[p] != 0) && index[p] == num_codes;
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) wave_count[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        before += w < wave ? wave_count[w] : 0;
        total += wave_count[w];
    }
    if (hit) list[before + __popcll(votes & ((1ull << lane) - 1ull))] = t;
    __syncthreads();
    const int col = blockIdx.y * 256 + t;
    if (col >= width) return;
    float acc = 0.f;
    for (int r = 0; r < total; ++r) acc = acc + g_out[(first + list[r]) * g_stride + col];
    partial[(long)blockIdx.x * width + col] = acc;
}

__global__ __launch_bounds__(256) void embed_miss_grad_sum_kernel(const float *__restrict__ partial, long chunks, int width, float *__restrict__ g_miss)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= width) return;
    float acc = 0.f;
    for (long ch = 0; ch < chunks; ++ch) acc = acc + partial[ch * width + col];
    g_miss[col] = acc;
}

// The lookup with the consumer's projector folded in: out[p] = b + W . emb[p] without emb.  The lookup is linear in the codebook
// rows, so the projector is applied to the codebook once per weight version (ops.fold_projector: P_s = what[region_s] . W_s^T, one
// [K_s, hp] table per slot, stacked in one buffer `table` with the slots' row offsets in reg.lo) and a position is
//   out[p, h] = bias[h] + sum_s sum_j weights[c, s, j] * P_s[tokens[c, s, j], h]
// One item = one position; all slots land in one output row.  LANES = 16, 32 or 64 lanes own it: lane i < slots * topk <= LANES loads
// entry i of the code's ids and weights once (they are consecutive in memory), a shuffle hands them round, and the lanes cover the hp
// columns as float4 (hp % 4 == 0; the host pads).  Per column ONE fp32 chain in a fixed order: acc = bias[h], then slots ascending,
// then list order, acc = fmaf(w, P_s[id][h], acc); the k gathers of a slot are issued before its first fmaf.  Per position p with
// c = index[p] -- what projector(embed_codes(...)) gives:
//   pad[p] != 0               the bias row; index[p] is not read, nor are the tables, and status is not touched
//   0 <= c < num_codes        the chain above (a slot with an id outside its region contributes nothing, bit `slot` of *status)
//   c == num_codes, miss_row  a copy of miss_row [hp] (W . miss + b, made with the tables)
//   anything else             the bias row, bit 4 of *status
// No index and no id forms an address before it has been checked; every product with c is 64-bit.  The shuffles run with every lane
// of the wavefront active (the column loop's trip count is uniform; only loads, fmafs and stores are predicated).
template <int LANES, int MAXK, typename OUT>
__global__ __launch_bounds__(256) void embed_project_kernel(const int64_t *__restrict__ index, const uint8_t *__restrict__ pad, long n,
                                                            const int64_t *__restrict__ tokens, const float *__restrict__ weights, long num_codes,
                                                            int slots, int topk, const float *__restrict__ table, int hp, DecodeRegions reg,
                                                            const float *__restrict__ bias, const float *__restrict__ miss_row,
                                                            OUT *__restrict__ out, long out_stride, int *status)
{
    static_assert(LANES == 16 || LANES == 32 || LANES == 64, "a group is a power-of-two part of a wavefront");
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (LANES - 1), base = lane & ~(LANES - 1);
    long pos = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES;
    const bool live = pos < n;
    if (!live) pos = 0;
    // what this position is: the lanes of a group agree (one address each)
    const bool padded = !live || (pad && pad[pos] != 0);
    const long c = padded ? 0 : index[pos];
    const bool is_code = !padded && c >= 0 && c < num_codes;
    const bool is_miss = !padded && miss_row && c == num_codes;
    if (!padded && !is_code && !is_miss && sub == 0 && status) atomicOr(status, 1 << MEDTOK_EMBED_BAD_INDEX_BIT);
    const int entries = slots * topk;                             // <= LANES (checked on the host)
    const int eslot = sub / topk;                                 // the slot of this lane's entry
    long lo = reg.lo[0], size = reg.size[0];
#pragma unroll
    for (int s = 1; s < MEDTOK_DECODE_MAX_SLOTS; ++s)
        if (eslot == s) { lo = reg.lo[s]; size = reg.size[s]; }
    long id = 0;
    float wv = 0.f;
    if (is_code && sub < entries) {
        const long at = c * entries + sub;                        // 64-bit: c < num_codes was checked above
        id = tokens[at];
        wv = weights[at];
    }
    const bool bad_lane = id < 0 || id >= size;                   // (a lane without an entry holds 0: in range, size >= 1)
    const unsigned long long votes = __ballot(bad_lane);
    const unsigned long long mine = LANES == 64 ? votes : (votes >> base) & ((1ull << (LANES & 63)) - 1ull);
    const int row = bad_lane ? 0 : (int)(lo + id);                // lo + size <= rows of the table < 2^31 (checked on the host)
    int bad_slots = 0;
#pragma unroll
    for (int s = 0; s < MEDTOK_DECODE_MAX_SLOTS; ++s)
        if (s < slots && ((mine >> (s * topk)) & ((1ull << topk) - 1ull)) != 0ull) bad_slots |= 1 << s;
    if (bad_slots && sub == 0 && status) atomicOr(status, bad_slots);      // (bad implies is_code: only such groups loaded an id)
    const float *first = is_miss ? miss_row : bias;
    OUT *dst = out + pos * out_stride;
    for (int i0 = 0; i0 < hp; i0 += LANES * 4) {                  // uniform over the wavefront: the shuffles below see every lane
        const int i = i0 + sub * 4;
        const bool on = live && i < hp;
        float4 a = on ? ld4(first + i) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < MEDTOK_DECODE_MAX_SLOTS; ++s) {
            if (s >= slots) break;
            int rj[MAXK];
            float wj[MAXK];
#pragma unroll
            for (int j = 0; j < MAXK; ++j) {
                const int from = base + (j < topk ? s * topk + j : 0);
                rj[j] = __shfl(row, from, 64);
                wj[j] = __shfl(wv, from, 64);
            }
            if (on && is_code && !(bad_slots >> s & 1)) {
                float4 e[MAXK];
#pragma unroll
                for (int j = 0; j < MAXK; ++j)                    // the k gathers of this slot: in flight together
                    if (j < topk) e[j] = ld4(table + (long)rj[j] * hp + i);
#pragma unroll
                for (int j = 0; j < MAXK; ++j)
                    if (j < topk) {
                        a.x = fmaf(wj[j], e[j].x, a.x); a.y = fmaf(wj[j], e[j].y, a.y);
                        a.z = fmaf(wj[j], e[j].z, a.z); a.w = fmaf(wj[j], e[j].w, a.w);
                    }
            }
        }
        if (on) embed_store4(dst + i, a);
    }
}
