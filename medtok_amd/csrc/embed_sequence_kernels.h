// The consumer's input sequence over dense rows, and the gradients of the rows a sequence adds.  Included by medtok_vq.hip behind
// embed_kernels.h (uses ld4 / st4 / st1, add4, EmbedSeqParts, MEDTOK_EMBED_BAD_SEGMENT_BIT).  The sequence over the folded tables is
// embed_folded_kernel<.., PARTS = true> there; what a row of the sequence is, and the order of its additions, is documented with it.
#pragma once

// The epilogue of embed_folded_kernel<.., true> over dense fp32 rows [batch * len, width] (unit column stride, row stride = width) instead of the tables: place, add,
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
        st4(dst, a);
    } else {
        float a = first[i];
        float pe = 0.f, t0 = 0.f, t1 = 0.f;
        if (prow) pe = prow[i];
        if (s0) t0 = s0[i];
        if (s1) t1 = s1[i];
        if (prow) a = a + pe;
        if (s0) a = a + t0;
        if (s1) a = a + t1;
        st1(dst, a);
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
