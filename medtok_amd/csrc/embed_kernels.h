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
        st4(dst + i, a);
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
// One item = one output row; all slots land in it.  LANES = 16, 32 or 64 lanes own it: lane i < slots * topk <= LANES loads entry i of
// the code's ids and weights once (they are consecutive in memory), a shuffle hands them round, and the lanes cover the hp columns as
// float4 (hp % 4 == 0; the host pads).  Per column ONE fp32 chain in a fixed order: acc = bias[h], then slots ascending, then list
// order, acc = fmaf(w, P_s[id][h], acc); the k gathers of a slot are issued before its first fmaf.  Per position p with
// c = index[p] -- what projector(embed_codes(...)) gives:
//   pad[p] != 0               the bias row; index[p] is not read, nor are the tables, and status is not touched
//   0 <= c < num_codes        the chain above (a slot with an id outside its region contributes nothing, bit `slot` of *status)
//   c == num_codes, miss_row  a copy of miss_row [hp] (W . miss + b, made with the tables)
//   anything else             the bias row, bit 4 of *status
// No index and no id forms an address before it has been checked; every product with c is 64-bit.  The shuffles run with every lane
// of the wavefront active (the column loop's trip count is uniform; only loads, fmafs and stores are predicated).  OUT = float, _Float16 or __bf16: the finished fp32 value is rounded once, to nearest even.
//
// PARTS: the consumer's input sequence behind the lookup, in the same launch.  What the EHR model does between
// `projector(med_code_emb[index])` and its first transformer layer (MedTok_EHR_Tutorial/EHRModel_token.py:220-232,
// PositionalEncoding.forward :65-78): x + pe[:L], + two time embeddings gathered per code through the code's visit, torch.concat of
// (cls, gender, ethnicity) rows in front.  Each of those steps reads and writes a [B, L, H] tensor; here the row is finished in
// registers and stored once.  out is [B, P + L, width], one item per row (b, r):
//   r < P                      a copy of prefix[b, r, :]
//   p = r - P, pad[b, p] != 0  the lookup's row r0 (the bias row); nothing is added, and neither index[b, p] nor segment_id[b, p] is read
//   otherwise                  ((r0 + position_rows[p]) + segment_rows0[b, g]) + segment_rows1[b, g],   g = segment_id[b, p]
// plain fp32 additions in that order on the fp32 value of the lookup's chain (the library is built with -ffp-contract=off: the bits are
// those of torch adding the tensors one after the other to the fp32 rows).  A miss position and a bad code index take the adds like
// any unpadded position.  g outside [0, V): no segment term, bit MEDTOK_EMBED_BAD_SEGMENT_BIT of *status; no address is formed from
// an unchecked id, and every address product is 64-bit.  Each absent part (position_rows, segment_id with its rows, the second segment
// term, prefix) is a null pointer.  A prefix row runs through the same code as a padded position whose first row is prefix[b, r] (so
// the shuffles see every lane under a uniform trip count).  The position row, the segment rows and the segment id are loaded before
// the chain's first gather: they are in flight with the gathers.  PARTS is a compile-time switch because the epilogue costs registers
// (20 VGPRs and a step of occupancy at <16, 8>): without it, nothing of it exists in the instantiation, and `len` (the positions per
// batch row) and `parts` are not looked at (one argument list serves both).
//
// (MEDTOK_EMBED_BAD_SEGMENT_BIT, MEDTOK_EMBED_SEQ_MAX_TERMS, MEDTOK_EMBED_SEQ_GRAD_CHUNK and MEDTOK_EMBED_SEQ_MAX_SEGMENTS come from
// include/medtok_vq.h: no second definition that could drift)
struct EmbedSeqParts {
    const float *position_rows;      // [>= len, width] or null
    const int64_t *segment_id;       // [batch, len] or null
    const float *segment_rows0;      // [batch, n_segments, width] or null
    const float *segment_rows1;      // [batch, n_segments, width] or null (only with segment_rows0)
    const float *prefix;             // [batch, n_prefix, width] or null
    long n_segments;
    long n_prefix;
};

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <int LANES, int MAXK, typename OUT, bool PARTS>
__global__ __launch_bounds__(256) void embed_folded_kernel(const int64_t *__restrict__ index, const uint8_t *__restrict__ pad, long items, long len,
                                                           const int64_t *__restrict__ tokens, const float *__restrict__ weights, long num_codes,
                                                           int slots, int topk, const float *__restrict__ table, int hp, DecodeRegions reg,
                                                           const float *__restrict__ bias, const float *__restrict__ miss_row, EmbedSeqParts parts,
                                                           OUT *__restrict__ out, long out_stride, int *status)
{
    static_assert(LANES == 16 || LANES == 32 || LANES == 64, "a group is a power-of-two part of a wavefront");
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (LANES - 1), base = lane & ~(LANES - 1);
    long item = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES;
    const bool live = item < items;
    if (!live) item = 0;
    long pos = item;                                              // the flat position whose index is looked up
    [[maybe_unused]] long b = 0, r = 0, p = 0;                    // PARTS: batch row, row inside it, position inside it
    [[maybe_unused]] bool is_prefix = false;
    if constexpr (PARTS) {
        const long per = parts.n_prefix + len;                    // rows per batch row (>= 1: items > 0)
        b = item / per;
        r = item - b * per;
        is_prefix = r < parts.n_prefix;
        p = is_prefix ? 0 : r - parts.n_prefix;                   // the position inside the batch row
        pos = b * len + p;                                        // (only used where !is_prefix)
    }
    // what this row is: the lanes of a group agree (one address each)
    const bool padded = !live || is_prefix || (pad && pad[pos] != 0);
    const long c = padded ? 0 : index[pos];
    [[maybe_unused]] long g = 0;
    if constexpr (PARTS) g = (padded || !parts.segment_id) ? 0 : parts.segment_id[pos];
    const bool is_code = !padded && c >= 0 && c < num_codes;
    const bool is_miss = !padded && miss_row && c == num_codes;
    [[maybe_unused]] bool seg_on = false;
    if constexpr (PARTS) {
        seg_on = !padded && parts.segment_id && g >= 0 && g < parts.n_segments;
        if (sub == 0 && status && !padded) {
            if (!is_code && !is_miss) atomicOr(status, 1 << MEDTOK_EMBED_BAD_INDEX_BIT);
            if (parts.segment_id && !seg_on) atomicOr(status, 1 << MEDTOK_EMBED_BAD_SEGMENT_BIT);
        }
    } else {
        if (!padded && !is_code && !is_miss && sub == 0 && status) atomicOr(status, 1 << MEDTOK_EMBED_BAD_INDEX_BIT);
    }
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
    [[maybe_unused]] const float *prow = nullptr, *s0 = nullptr, *s1 = nullptr;
    if constexpr (PARTS) {
        first = is_prefix ? parts.prefix + (b * parts.n_prefix + r) * hp : first;
        prow = (!padded && parts.position_rows) ? parts.position_rows + p * hp : nullptr;
        const long srow = (b * parts.n_segments + (seg_on ? g : 0)) * hp;     // 64-bit; g was checked above
        s0 = (seg_on && parts.segment_rows0) ? parts.segment_rows0 + srow : nullptr;
        s1 = (seg_on && parts.segment_rows1) ? parts.segment_rows1 + srow : nullptr;
    }
    OUT *dst = out + item * out_stride;
    for (int i0 = 0; i0 < hp; i0 += LANES * 4) {                  // uniform over the wavefront: the shuffles below see every lane
        const int i = i0 + sub * 4;
        const bool on = live && i < hp;
        float4 a = on ? ld4(first + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        [[maybe_unused]] float4 pe = make_float4(0.f, 0.f, 0.f, 0.f), t0 = pe, t1 = pe;
        if constexpr (PARTS) {
            if (on && prow) pe = ld4(prow + i);                   // issued before the gathers: in flight with them
            if (on && s0) t0 = ld4(s0 + i);
            if (on && s1) t1 = ld4(s1 + i);
        }
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
        if constexpr (PARTS) {
            if (prow) a = add4(a, pe);                            // (an absent part adds nothing at all: x + 0 would turn -0 into +0)
            if (s0) a = add4(a, t0);
            if (s1) a = add4(a, t1);
        }
        if (on) st4(dst + i, a);
    }
}

// Bag pooling: pooled[b] = (sum over the unpadded positions p of bag b of n(row(p))) / live_b, where row(p) is what embed_codes_kernel
// writes for position p (the same fp32 chain, the same four kinds of position, the same status bits), n(v) = v / max(|v|_2, 1e-12)
// over the WHOLE row of slots * d elements (normalize != 0) or v itself, and live_b counts the unpadded positions (a bad index counts,
// as a row of zeros).  What the reference's QA adapter does per sample in a Python loop over the materialised table
// (MedTok_QA_Tutorial/review.py:50-64); neither the table nor the [positions, width] rows ever exist.
//
// embed_pool_partial_kernel: a block of 4 wavefronts owns MEDTOK_EMBED_POOL_CHUNK consecutive positions of one bag (block =
// bag * chunks + chunk: the grid (chunks of a bag, bags) flattened, so that neither axis meets the 65,535 limit); the chunk is a
// compile-time constant, so the bits of the result never depend on the device or on a launch heuristic.  Position j of the chunk belongs
// to wavefront j % 4, and a wavefront takes its positions one at a time, all slots:
//   * up front, for each of its CHUNK / 4 positions: the mask byte and the index (not read under the mask), then the code's
//     slots * topk <= 64 ids and weights, entry i in lane i as in embed_folded_kernel -- every load of a level is in flight before the
//     first is used; ids are validated there (ballot), so no index and no id forms an address before it has been checked, and every
//     product with a code index is 64-bit;
//   * per position: lane l owns the float4 columns (r * 64 + l) * 4, r < R (R = 1, 4, 12 or 16 covers widths up to 256, 1024, 3072, 4096); a
//     column's slot varies by lane, so each lane fetches its slot's ids and weights with a per-lane source (every lane of the wavefront
//     is active at every shuffle: all branches around them are wavefront-uniform), issues the k gathers of the column together and
//     runs the chain acc = +0; acc = fmaf(w_j, e_j, acc) in list order.  The finished row stays in registers (4 R floats per lane);
//   * the squared norm: per lane over r ascending, x y z w (fmaf), then an xor butterfly over the wavefront, distances 32, 16 .. 1 (every
//     lane ends with the same bits); the row is scaled by 1 / max(sqrt(ss), 1e-12) (one correctly rounded division per row, then one
//     multiply per element; exactly 1 without normalisation) and added to the wavefront's accumulator, positions in ascending order.
// The four accumulators are then added in wavefront order through ONE LDS row (((w0 + w1) + w2) + w3; width * 4 <= 16 KiB of dynamic
// LDS) and written as partial[block, width]; the chunk's counts of live and of live-miss positions go to chunk_counts[block, 2].  A
// chunk without an unpadded position writes zeros and reads neither an index nor a table.  No float atomics anywhere.
//
// Row in registers, not in LDS: a per-wavefront LDS row of 4096 floats would be 64 KiB per block (two blocks per CU, no better than the
// registers allow) and every element would cross LDS twice.  A lane holds the row and the accumulator (8 R registers), eight gathered
// float4 and their ids and weights (48); lists of more than 8 entries are gathered eight at a time.  gfx950 build, <R, MAXK>: VGPRs /
// waves per SIMD -- <1, 8> 70 / 7, <1, 16> 73 / 6, <4, 8> 96 / 5, <4, 16> 99 / 4, <12, 8> 161 / 3, <12, 16> 163 / 3, <16, 8> 193 / 2,
// <16, 16> 195 / 2; no AGPRs, no scratch, no spills; LDS 32 bytes static + 4 bytes per column (at most 16 KiB; never the limit).
//
// embed_pool_finish_kernel adds a bag's partial rows in chunk order from +0, divides by (float)live_b (a true division; live_b == 0:
// zeros) and writes out[bag, :] and counts[bag] = (live_b, miss_b).
// (MEDTOK_EMBED_POOL_CHUNK = 16 and MEDTOK_EMBED_POOL_MAX_WIDTH = 4096 come from include/medtok_vq.h: the chunk is part of the result's bits)
#define MEDTOK_EMBED_POOL_TURNS (MEDTOK_EMBED_POOL_CHUNK / 4)

//
// LISTED: a bag is a LIST of positions instead of a row of index (MedTokEmbedding.pooled_segments: "the unpadded positions of row b whose
// segment is v"; embed_pool_segments_kernels.h makes the lists).  Bag g's list is sorted[offsets[g] .. offsets[g + 1]), flat positions in
// ascending order, cut into chunks of MEDTOK_EMBED_POOL_CHUNK entries; entry j of a chunk stands where position chunk * 16 + j of the bag
// stands above, and everything behind the position -- index and id validation, gathers, the chain, the norm, the wavefront sum, the order
// -- is the code above.  No mask is read (a listed position is unpadded).  The grid is the plan of embed_grad_chunk_kernel: blocks
// [0, bags) are the bags, and a bag of at most one chunk is FINISHED by its block (0 + the chunk's sum, divided by (float)count -- the
// arithmetic of embed_pool_finish_kernel over one chunk; an empty bag: zeros; counts[bag] = (count, miss positions)), so the many short
// or empty bags have no partial row; blocks [bags, bags + extra) are the chunks of the longer bags: block bags + q finds its bag by
// bisection in first_chunk[] and writes partial[q] and chunk_counts[q].  A block with nothing to do returns before its first barrier.
// Without LISTED nothing of this exists in the instantiation and `list` is not looked at (one argument list serves both): the figures
// above are unchanged.  With LISTED, VGPRs / waves per SIMD -- <1, 8> 70 / 7, <1, 16> 74 / 6, <4, 8> 98 / 4, <4, 16> 100 / 4, <12, 8>
// 162 / 3, <12, 16> 164 / 3, <16, 8> 194 / 2, <16, 16> 196 / 2; no AGPRs, no scratch, no spills.
struct EmbedPoolList {
    const uint32_t *sorted;          // [positions] flat positions b * L + p, sorted by bag, ascending inside a bag
    const int *offsets;              // [bags + 1]
    const int *first_chunk;          // [bags + 1]: the first partial row of a bag with several chunks
    long bags, extra;                // B * V, and the bound on the chunks of the longer bags
    float *out;                      // [bags, out_stride]
    long out_stride;
    int *counts;                     // [bags, 2]
};

template <int R, int MAXK, bool LISTED>
__global__ __launch_bounds__(256) void embed_pool_partial_kernel(const int64_t *__restrict__ index, const uint8_t *__restrict__ pad, long bag_len,
                                                                 int chunks, const int64_t *__restrict__ tokens, const float *__restrict__ weights,
                                                                 long num_codes, int slots, int topk, const float *__restrict__ what, int d,
                                                                 DecodeRegions reg, const float *__restrict__ miss, int normalize,
                                                                 float *__restrict__ partial, int *__restrict__ chunk_counts, int *status,
                                                                 EmbedPoolList list)
{
    extern __shared__ float4 pool_row[];                          // width / 4 float4: the running sum over the wavefronts
    __shared__ int wave_live[4], wave_miss[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long bag, row = (long)blockIdx.x;                             // row: where this block's sum and counts go in partial / chunk_counts
    int chunk;
    [[maybe_unused]] int first = 0, cnt = 0;                      // LISTED: this chunk is sorted[first .. first + cnt)
    [[maybe_unused]] bool whole = false;                          // LISTED: the chunk is the whole bag, finished here
    if constexpr (LISTED) {
        chunk = 0;
        if (row < list.bags) {
            bag = row;
            first = list.offsets[bag];
            cnt = list.offsets[bag + 1] - first;
            if (cnt > MEDTOK_EMBED_POOL_CHUNK) return;            // its chunks are further blocks (uniform over the block)
            whole = true;
        } else {
            row -= list.bags;
            if (row >= list.first_chunk[list.bags]) return;       // (uniform over the block)
            long a = 0, b = list.bags - 1;                        // the bag g with first_chunk[g] <= row < first_chunk[g + 1]
            while (a < b) {
                const long mid = (a + b) >> 1;
                if (list.first_chunk[mid + 1] > row) b = mid; else a = mid + 1;
            }
            bag = a;
            first = list.offsets[a] + ((int)row - list.first_chunk[a]) * MEDTOK_EMBED_POOL_CHUNK;
            const int left = list.offsets[a + 1] - first;
            cnt = left < MEDTOK_EMBED_POOL_CHUNK ? left : MEDTOK_EMBED_POOL_CHUNK;
        }
    } else {
        bag = row / chunks;
        chunk = (int)(row - bag * chunks);
    }
    const int width = slots * d, entries = slots * topk;         // entries <= 64, width <= 256 R (checked on the host)
    const int eslot = lane / topk;                                // the slot of this lane's entry
    long lo = reg.lo[0], size = reg.size[0];
#pragma unroll
    for (int s = 1; s < MEDTOK_DECODE_MAX_SLOTS; ++s)
        if (eslot == s) { lo = reg.lo[s]; size = reg.size[s]; }
    unsigned slot_of = 0;                                         // two bits per r: the slot of this lane's column (r * 64 + lane) * 4
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = (r * 64 + lane) * 4;
        slot_of |= (unsigned)(i < width ? i / d : 0) << (2 * r);
    }
    // level 1 and 2 of every position of this wavefront: mask and index, then the code's entries
    int kind[MEDTOK_EMBED_POOL_TURNS], rowv[MEDTOK_EMBED_POOL_TURNS], badv[MEDTOK_EMBED_POOL_TURNS];   // kind: 0 padded, 1 code, 2 miss, 3 bad index
    float wgt[MEDTOK_EMBED_POOL_TURNS];
    long cv[MEDTOK_EMBED_POOL_TURNS];
#pragma unroll
    for (int t = 0; t < MEDTOK_EMBED_POOL_TURNS; ++t) {
        const long p = (long)chunk * MEDTOK_EMBED_POOL_CHUNK + t * 4 + wave;
        bool in;
        long gp;
        if constexpr (LISTED) {
            in = p < cnt;
            gp = in ? (long)list.sorted[first + p] : 0;           // < B * L: the keys kernel wrote its own position
        } else {
            in = p < bag_len;
            gp = bag * bag_len + (in ? p : 0);
        }
        const bool padded = !in || (!LISTED && pad && pad[gp] != 0);
        const long c = padded ? 0 : index[gp];
        const bool is_code = !padded && c >= 0 && c < num_codes;
        const bool is_miss = !padded && miss && c == num_codes;
        kind[t] = __builtin_amdgcn_readfirstlane(padded ? 0 : is_code ? 1 : is_miss ? 2 : 3);   // (the lanes agree: one address each)
        cv[t] = c;
    }
    int live = 0, missed = 0;
#pragma unroll
    for (int t = 0; t < MEDTOK_EMBED_POOL_TURNS; ++t) {
        long id = 0;
        float wv = 0.f;
        if (kind[t] == 1 && lane < entries) {
            const long at = cv[t] * entries + lane;               // 64-bit: 0 <= c < num_codes was checked above
            id = tokens[at];
            wv = weights[at];
        }
        const bool bad_lane = id < 0 || id >= size;               // (a lane without an entry holds 0: in range, size >= 1)
        const unsigned long long votes = __ballot(bad_lane);
        int bad_slots = 0;
#pragma unroll
        for (int s = 0; s < MEDTOK_DECODE_MAX_SLOTS; ++s)
            if (s < slots && ((votes >> (s * topk)) & ((1ull << topk) - 1ull)) != 0ull) bad_slots |= 1 << s;
        rowv[t] = bad_lane ? 0 : (int)(lo + id);                  // lo + size <= n_codes < 2^31 (checked on the host)
        wgt[t] = wv;
        badv[t] = bad_slots;
        if (lane == 0 && status) {
            if (kind[t] == 3) atomicOr(status, 1 << MEDTOK_EMBED_BAD_INDEX_BIT);
            if (bad_slots) atomicOr(status, bad_slots);           // (bad implies a code: only such positions loaded an id)
        }
        live += kind[t] != 0;
        missed += kind[t] == 2;
    }
    float4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int t = 0; t < MEDTOK_EMBED_POOL_TURNS; ++t) {
        int what_kind = 0, row = 0, bad_slots = 0;
        float wv = 0.f;
#pragma unroll
        for (int u = 0; u < MEDTOK_EMBED_POOL_TURNS; ++u)          // (selects on constant indices: the arrays stay in registers)
            if (u == t) { what_kind = kind[u]; row = rowv[u]; bad_slots = badv[u]; wv = wgt[u]; }
        if (what_kind != 1 && what_kind != 2) continue;           // padded, or a bad index: a row of zeros adds nothing
        unsigned slots_now = slot_of;                             // opaque per position: the shuffle sources, masks and column addresses derived
        int lane_now = lane;                                      // from them are recomputed here, not kept in 12 R registers across the loop
        int topk_now = topk;
        asm volatile("" : "+v"(slots_now), "+v"(lane_now), "+s"(topk_now));
        float4 v[R];
        float ss = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            v[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r * 256 >= width) continue;                       // uniform over the wavefront
            const int i = (r * 64 + lane_now) * 4, slot = (int)(slots_now >> (2 * r)) & 3;
            const bool on = i < width;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (what_kind == 1) {
                const bool mix = on && !(bad_slots >> slot & 1);
                const float *src = what + (i - slot * d);
#pragma unroll
                for (int j0 = 0; j0 < MAXK; j0 += 8) {            // lists of more than 8: eight gathers at a time, the chain goes on
                    if (j0 >= topk_now) break;                        // uniform
                    int cj[8];
                    float wj[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {                 // every lane active; lane-dependent source: the column's slot
                        const int from = slot * topk_now + (j0 + j < topk_now ? j0 + j : 0);     // (a scalar select: entry 0 stands in)
                        cj[j] = __shfl(row, from, 64);
                        wj[j] = __shfl(wv, from, 64);
                    }
                    if (mix) {
                        float4 e[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j)               // the gathers of this column: in flight together
                            if (j0 + j < topk_now) e[j] = ld4(src + (long)cj[j] * d);
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (j0 + j < topk_now) {
                                a.x = fmaf(wj[j], e[j].x, a.x); a.y = fmaf(wj[j], e[j].y, a.y);
                                a.z = fmaf(wj[j], e[j].z, a.z); a.w = fmaf(wj[j], e[j].w, a.w);
                            }
                    }
                    __builtin_amdgcn_sched_barrier(0);            // (keeps the next group's gathers behind this group's fmafs: registers)
                }
            } else if (on) {
                a = ld4(miss + i);
            }
            v[r] = a;
            ss = fmaf(a.x, a.x, ss); ss = fmaf(a.y, a.y, ss); ss = fmaf(a.z, a.z, ss); ss = fmaf(a.w, a.w, ss);
        }
        float inv = 1.f;
        if (normalize) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ss = ss + __shfl_xor(ss, off, 64);
            inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            acc[r].x = fmaf(v[r].x, inv, acc[r].x); acc[r].y = fmaf(v[r].y, inv, acc[r].y);
            acc[r].z = fmaf(v[r].z, inv, acc[r].z); acc[r].w = fmaf(v[r].w, inv, acc[r].w);
        }
    }
    if (lane == 0) { wave_live[wave] = live; wave_miss[wave] = missed; }
    float *dst = partial + row * width;
    if constexpr (LISTED) {
        if (whole) dst = list.out + bag * list.out_stride;
    }
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {                                 // ((w0 + w1) + w2) + w3: a lane meets its own columns only
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int q = r * 64 + lane;
                if (q * 4 >= width) continue;
                float4 a = acc[r];
                if (w > 0) {
                    const float4 b = pool_row[q];
                    a.x = b.x + a.x; a.y = b.y + a.y; a.z = b.z + a.z; a.w = b.w + a.w;
                }
                if constexpr (LISTED) {
                    if (w == 3 && whole) {                        // embed_pool_finish_kernel over this one chunk: from +0, then the division
                        if (cnt > 0) {
                            const float n = (float)cnt;
                            a.x = (0.f + a.x) / n; a.y = (0.f + a.y) / n; a.z = (0.f + a.z) / n; a.w = (0.f + a.w) / n;
                        } else {
                            a = make_float4(0.f, 0.f, 0.f, 0.f);
                        }
                    }
                }
                if (w < 3) pool_row[q] = a;
                else st4(dst + q * 4, a);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int *to = chunk_counts + 2 * row;
        if constexpr (LISTED) {
            if (whole) to = list.counts + 2 * bag;
        }
        to[0] = wave_live[0] + wave_live[1] + wave_live[2] + wave_live[3];
        to[1] = wave_miss[0] + wave_miss[1] + wave_miss[2] + wave_miss[3];
    }
}

// grid = (bags, ceil(width / 1024)); a thread owns one float4 column of one bag.  first_chunk (the LISTED form of the partial kernel):
// a bag's partial rows are [first_chunk[bag], first_chunk[bag + 1]); a bag without any was finished by the partial kernel and is left alone.
__global__ __launch_bounds__(256) void embed_pool_finish_kernel(const float *__restrict__ partial, const int *__restrict__ chunk_counts, int chunks,
                                                                int width, float *__restrict__ out, long out_stride, int *__restrict__ counts,
                                                                const int *__restrict__ first_chunk)
{
    __shared__ int bag_live;
    long first = (long)blockIdx.x * chunks;                       // the bag's first chunk
    if (first_chunk) {
        first = first_chunk[blockIdx.x];
        chunks = first_chunk[blockIdx.x + 1] - (int)first;
        if (chunks == 0) return;                                  // (uniform over the block)
    }
    if (threadIdx.x == 0) {                                       // one thread adds the chunks' counts (integers: any order), the block reads the sum
        int live_sum = 0, missed = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            live_sum += chunk_counts[2 * (first + ch)];
            missed += chunk_counts[2 * (first + ch) + 1];
        }
        bag_live = live_sum;
        if (counts && blockIdx.y == 0) {
            counts[2 * (long)blockIdx.x] = live_sum;
            counts[2 * (long)blockIdx.x + 1] = missed;
        }
    }
    __syncthreads();
    const int live = bag_live;
    const int i = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (i >= width) return;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ch = 0; ch < chunks; ++ch) {
        const float4 p = ld4(partial + (first + ch) * width + i);
        a.x = a.x + p.x; a.y = a.y + p.y; a.z = a.z + p.z; a.w = a.w + p.w;
    }
    if (live > 0) {
        const float n = (float)live;
        a.x = a.x / n; a.y = a.y / n; a.z = a.z / n; a.w = a.w / n;
    } else {
        a = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    st4(out + (long)blockIdx.x * out_stride + i, a);
}

// Gradient of the miss row through the pool: every unpadded miss position of bag b carries the same vector, so with the upstream g_out
// [bags, width] the gradient w.r.t. that vector is G[col] = sum over the bags of (miss_b / live_b) * g_out[b, col] -- the whole gradient
// of the miss row without normalisation, and what the caller takes through the normalisation's backward with it.  Fixed order, no float
// atomics, the two stages of embed_miss_grad_*: a block owns MEDTOK_EMBED_GRAD_CHUNK consecutive bags and runs acc = fmaf(coef_b, g, acc)
// over them in bag order (bags with live_b == 0 or miss_b == 0 are skipped) into partial[chunk, col]; embed_miss_grad_sum_kernel then adds
// the partials in chunk order.  grid = (chunks of bags, ceil(width / 256)); a thread owns one column.
__global__ __launch_bounds__(256) void embed_pool_miss_grad_partial_kernel(const float *__restrict__ g_out, long g_stride, const int *__restrict__ counts,
                                                                           long bags, int width, float *__restrict__ partial)
{
    __shared__ float coef[MEDTOK_EMBED_GRAD_CHUNK];
    const int t = threadIdx.x;
    const long first = (long)blockIdx.x * MEDTOK_EMBED_GRAD_CHUNK, b = first + t;
    float cf = 0.f;
    if (b < bags) {
        const int live = counts[2 * b], missed = counts[2 * b + 1];
        if (live > 0 && missed > 0) cf = (float)missed / (float)live;
    }
    coef[t] = cf;
    __syncthreads();
    const int col = blockIdx.y * 256 + t;
    if (col >= width) return;
    const int rows = (int)(bags - first < MEDTOK_EMBED_GRAD_CHUNK ? bags - first : MEDTOK_EMBED_GRAD_CHUNK);
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) {
        const float cf_r = coef[r];
        if (cf_r != 0.f) acc = fmaf(cf_r, g_out[(first + r) * g_stride + col], acc);
    }
    partial[(long)blockIdx.x * width + col] = acc;
}
