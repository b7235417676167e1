// The consumer's input sequence behind the lookup, in one launch: the rows of embed_project_kernel (or dense fp32 rows), plus a row per
// position, plus one or two rows per (batch row, segment), behind P copied rows per batch row.  Included by medtok_vq.hip behind
// embed_kernels.h (uses ld4 / st4, embed_store4, DecodeRegions, MEDTOK_EMBED_BAD_INDEX_BIT).
//
// What the EHR model does between `projector(med_code_emb[index])` and its first transformer layer (MedTok_EHR_Tutorial/
// EHRModel_token.py:220-232, PositionalEncoding.forward :65-78): x + pe[:L], + two time embeddings gathered per code through the
// code's visit, torch.concat of (cls, gender, ethnicity) rows in front.  Each of those steps reads and writes a [B, L, H] tensor;
// here the row is finished in registers and stored once.
//
// out is [B, P + L, width].  Row (b, r):
//   r < P                      a copy of prefix[b, r, :]
//   p = r - P, pad[b, p] != 0  the lookup's row r0 (the bias row / zeros / whatever `rows` holds); nothing is added, and neither
//                              index[b, p] nor segment_id[b, p] is read
//   otherwise                  ((r0 + position_rows[p]) + segment_rows0[b, g]) + segment_rows1[b, g],   g = segment_id[b, p]
// plain fp32 additions in that order on the fp32 value of the lookup's chain (the library is built with -ffp-contract=off: the bits are
// those of torch adding the tensors one after the other to the fp32 rows).  A miss position and a bad code index take the adds like
// any unpadded position.  g outside [0, V): no segment term, bit MEDTOK_EMBED_BAD_SEGMENT_BIT of *status; no address is formed from
// an unchecked id, and every address product is 64-bit.  Each absent part (position_rows, segment_id with its rows, the second segment
// term, prefix) is a null pointer.  OUT = float, _Float16 or __bf16: the finished fp32 value is rounded once, to nearest even.
#pragma once

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

// embed_project_kernel with the epilogue above.  One item = one output row of [batch * (P + len)]; LANES = 16, 32 or 64 lanes own it,
// exactly as there: lane i < slots * topk loads entry i of the code's ids and weights, a shuffle hands them round, the lanes cover the
// hp columns as float4, per column ONE fp32 chain acc = bias[h], slots ascending, list order, acc = fmaf(w, P_s[id][h], acc) -- the
// same gathers and the same order, so the same bits.  A prefix row runs through the same code as a padded position whose first row is
// prefix[b, r] (so the shuffles below see every lane under a uniform trip count).  The position row, the segment rows and the segment id
// are loaded before the chain's first gather: they are in flight with the gathers.  One store per row.
template <int LANES, int MAXK, typename OUT>
__global__ __launch_bounds__(256) void embed_sequence_kernel(const int64_t *__restrict__ index, const uint8_t *__restrict__ pad, long items, long len,
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
    const long per = parts.n_prefix + len;                        // rows per batch row (>= 1: items > 0)
    const long b = item / per, r = item - b * per;
    const bool is_prefix = r < parts.n_prefix;
    const long p = is_prefix ? 0 : r - parts.n_prefix;            // the position inside the batch row
    const long pos = b * len + p;                                 // the flat position (only used where !is_prefix)
    // what this row is: the lanes of a group agree (one address each)
    const bool padded = !live || is_prefix || (pad && pad[pos] != 0);
    const long c = padded ? 0 : index[pos];
    const long g = (padded || !parts.segment_id) ? 0 : parts.segment_id[pos];
    const bool is_code = !padded && c >= 0 && c < num_codes;
    const bool is_miss = !padded && miss_row && c == num_codes;
    const bool seg_on = !padded && parts.segment_id && g >= 0 && g < parts.n_segments;
    if (sub == 0 && status && !padded) {
        if (!is_code && !is_miss) atomicOr(status, 1 << MEDTOK_EMBED_BAD_INDEX_BIT);
        if (parts.segment_id && !seg_on) atomicOr(status, 1 << MEDTOK_EMBED_BAD_SEGMENT_BIT);
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
    const float *first = is_prefix ? parts.prefix + (b * parts.n_prefix + r) * hp : is_miss ? miss_row : bias;
    const float *prow = (!padded && parts.position_rows) ? parts.position_rows + p * hp : nullptr;
    const long srow = (b * parts.n_segments + (seg_on ? g : 0)) * hp;     // 64-bit; g was checked above
    const float *s0 = (seg_on && parts.segment_rows0) ? parts.segment_rows0 + srow : nullptr;
    const float *s1 = (seg_on && parts.segment_rows1) ? parts.segment_rows1 + srow : nullptr;
    OUT *dst = out + item * out_stride;
    for (int i0 = 0; i0 < hp; i0 += LANES * 4) {                  // uniform over the wavefront: the shuffles below see every lane
        const int i = i0 + sub * 4;
        const bool on = live && i < hp;
        float4 a = on ? ld4(first + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 pe = make_float4(0.f, 0.f, 0.f, 0.f), t0 = pe, t1 = pe;
        if (on && prow) pe = ld4(prow + i);                       // issued before the gathers: in flight with them
        if (on && s0) t0 = ld4(s0 + i);
        if (on && s1) t1 = ld4(s1 + i);
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
        if (prow) a = add4(a, pe);                                // (an absent part adds nothing at all: x + 0 would turn -0 into +0)
        if (s0) a = add4(a, t0);
        if (s1) a = add4(a, t1);
        if (on) embed_store4(dst + i, a);
    }
}

__device__ __forceinline__ void embed_store1(float *p, float v) { *p = v; }
__device__ __forceinline__ void embed_store1(_Float16 *p, float v) { *p = (_Float16)v; }
__device__ __forceinline__ void embed_store1(__bf16 *p, float v) { *p = (__bf16)v; }

// The same epilogue over dense fp32 rows [batch * len, width] (unit column stride, row stride = width) instead of the tables: place, add,
// cast.  Serves every form of the module that does not run over folded tables (no projector, an unfolded projector, a codebook that
// trains, e_dim % 4 != 0).  VEC = 4: width % 4 == 0, a thread owns one float4 of one output row; VEC = 1: any width >= 1, a thread owns
// one element.  Elementwise: thread t owns element group t of the [batch * (P + len), width / VEC] grid (64-bit).
template <int VEC, typename OUT>
__global__ __launch_bounds__(256) void embed_sequence_rows_kernel(const float *__restrict__ rows, const uint8_t *__restrict__ pad, long items, long len,
                                                                  int width, EmbedSeqParts parts, OUT *__restrict__ out, int *status)
{
    static_assert(VEC == 1 || VEC == 4, "a float4 or one element per thread");
    const long groups = width / VEC;                              // per row
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= items * groups) return;
    const long item = t / groups;
    const int i = (int)(t - item * groups) * VEC;
    const long per = parts.n_prefix + len;
    const long b = item / per, r = item - b * per;
    OUT *dst = out + item * (long)width + i;
    const bool is_prefix = r < parts.n_prefix;
    const long p = is_prefix ? 0 : r - parts.n_prefix;
    const long pos = b * len + p;
    const bool padded = is_prefix || (pad && pad[pos] != 0);
    const long g = (padded || !parts.segment_id) ? 0 : parts.segment_id[pos];
    const bool seg_on = !padded && parts.segment_id && g >= 0 && g < parts.n_segments;
    if (i == 0 && status && !padded && parts.segment_id && !seg_on) atomicOr(status, 1 << MEDTOK_EMBED_BAD_SEGMENT_BIT);
    const float *first = is_prefix ? parts.prefix + (b * parts.n_prefix + r) * (long)width : rows + pos * (long)width;
    const float *prow = (!padded && parts.position_rows) ? parts.position_rows + p * (long)width : nullptr;
    const long srow = (b * parts.n_segments + (seg_on ? g : 0)) * (long)width;
    const float *s0 = (seg_on && parts.segment_rows0) ? parts.segment_rows0 + srow : nullptr;
    const float *s1 = (seg_on && parts.segment_rows1) ? parts.segment_rows1 + srow : nullptr;
    if (VEC == 4) {
        float4 a = ld4(first + i);
        float4 pe = make_float4(0.f, 0.f, 0.f, 0.f), t0 = pe, t1 = pe;
        if (prow) pe = ld4(prow + i);
        if (s0) t0 = ld4(s0 + i);
        if (s1) t1 = ld4(s1 + i);
        if (prow) a = add4(a, pe);
        if (s0) a = add4(a, t0);
        if (s1) a = add4(a, t1);
        embed_store4(dst, a);
    } else {
        float a = first[i];
        float pe = 0.f, t0 = 0.f, t1 = 0.f;
        if (prow) pe = prow[i];
        if (s0) t0 = s0[i];
        if (s1) t1 = s1[i];
        if (prow) a = a + pe;
        if (s0) a = a + t0;
        if (s1) a = a + t1;
        embed_store1(dst, a);
    }
}

// Gradient of the segment rows: G[b, v, col] = sum of g[b, P + p, col] over the unpadded p with segment_id[b, p] == v (both segment terms
// receive this tensor), fp32, in a FIXED order and without float atomics: per MEDTOK_EMBED_SEQ_GRAD_CHUNK consecutive positions of a
// batch row in ascending position order (embed_sequence_segment_grad_partial_kernel), then the chunk sums in chunk order from +0
// (embed_sequence_segment_grad_sum_kernel).  Two runs give the same bits.  Ids outside [0, V) and padded positions contribute nothing
// (under the mask the id is not read).
//
// Partial: block = (b * chunks + chunk) along x, a tile of `tile` columns along y (tile a power of two, 4 .. 256, V * tile * 4 bytes <= 64
// KiB of dynamic LDS: the host picks it).  acc[V][tile] lives in LDS; thread t < tile owns column y * tile + t and walks the chunk's
// positions in order, eight at a time: the eight mask bytes and ids (block-uniform addresses), then the eight upstream values, then the
// eight read-modify-writes of its own LDS column -- a thread meets its own column only, so no barrier is needed between them.  The block
// writes its V x tile sums to partial[b, chunk, v, col].
__global__ __launch_bounds__(256) void embed_sequence_segment_grad_partial_kernel(const float *__restrict__ g, const uint8_t *__restrict__ pad,
                                                                                  const int64_t *__restrict__ segment_id, long len, int chunks,
                                                                                  long n_prefix, int n_segments, int width, int tile,
                                                                                  float *__restrict__ partial)
{
    extern __shared__ float seg_acc[];                            // [n_segments][tile]
    const int t = threadIdx.x;
    const long b = (long)blockIdx.x / chunks;
    const int chunk = (int)((long)blockIdx.x - b * chunks);
    const int col = blockIdx.y * tile + t;
    const bool mine = t < tile && col < width;
    if (t < tile)
        for (int v = 0; v < n_segments; ++v) seg_acc[v * tile + t] = 0.f;
    const long first = (long)chunk * MEDTOK_EMBED_SEQ_GRAD_CHUNK;
    const int count = (int)(len - first < MEDTOK_EMBED_SEQ_GRAD_CHUNK ? len - first : MEDTOK_EMBED_SEQ_GRAD_CHUNK);
    const float *grow = g + (b * (n_prefix + len) + n_prefix + first) * (long)width + col;       // row of the chunk's first position
    const long at = b * len + first;
    for (int q0 = 0; q0 < count; q0 += 8) {
        int seg[8];
        float gv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + u;
            seg[u] = -1;
            if (q < count && !(pad && pad[at + q] != 0)) {
                const long id = segment_id[at + q];
                if (id >= 0 && id < n_segments) seg[u] = (int)id;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) gv[u] = (mine && seg[u] >= 0) ? grow[(long)(q0 + u) * width] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (mine && seg[u] >= 0) seg_acc[seg[u] * tile + t] = seg_acc[seg[u] * tile + t] + gv[u];
    }
    if (!mine) return;
    float *dst = partial + ((long)blockIdx.x * n_segments) * (long)width + col;
    for (int v = 0; v < n_segments; ++v) dst[(long)v * width] = seg_acc[v * tile + t];
}

// G[b, v, col] = the chunk sums of (b, v, col) added in chunk order from +0.  One thread per element of [batch * V, width].
__global__ __launch_bounds__(256) void embed_sequence_segment_grad_sum_kernel(const float *__restrict__ partial, long total, int chunks, int n_segments,
                                                                              int width, float *__restrict__ G)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long per = (long)n_segments * width;                    // elements per batch row
    const long b = t / per, rest = t - b * per;
    const float *src = partial + b * chunks * per + rest;
    float acc = 0.f;
    for (int ch = 0; ch < chunks; ++ch) acc = acc + src[(long)ch * per];
    G[t] = acc;
}

// Gradient of the position rows: dpos[p, col] = sum over b ascending of g[b, P + p, col] at the unpadded (b, p), from +0; the rows
// p >= len of position_rows get zeros.  One thread per (p, col) of [rows, width] loops over b (eight loads in flight).
__global__ __launch_bounds__(256) void embed_sequence_position_grad_kernel(const float *__restrict__ g, const uint8_t *__restrict__ pad, long batch,
                                                                           long len, long n_prefix, int width, long total, float *__restrict__ dpos)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long p = t / width;
    const int col = (int)(t - p * width);
    float acc = 0.f;
    if (p < len) {
        const long per = (n_prefix + len) * (long)width;          // elements of g per batch row
        const float *src = g + (n_prefix + p) * (long)width + col;
        for (long b0 = 0; b0 < batch; b0 += 8) {
            float gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long b = b0 + u;
                const bool on = b < batch && !(pad && pad[b * len + p] != 0);
                gv[u] = on ? src[b * per] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long b = b0 + u;
                if (b < batch && !(pad && pad[b * len + p] != 0)) acc = acc + gv[u];
            }
        }
    }
    dpos[t] = acc;
}
