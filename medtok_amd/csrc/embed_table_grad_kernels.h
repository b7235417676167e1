// Per-table-row sums of the upstream gradient of the FOLDED lookup (embed_project_kernel / embed_sequence_kernel): what the projector's
// weight gradient and the codebook's gradient through the folded tables are both made of.  Included by medtok_vq.hip behind
// embed_grad_kernels.h (uses its key, zero, plan and combine kernels, ld4 / st4, and the scan and stable radix sort of the EMA statistics).
//
// The folded lookup writes out[p, :] = bias + sum_s sum_j weights[c, s, j] * table[offset_s + tokens[c, s, j], :], c = index[p]: every
// slot adds into the SAME hp columns.  Contribution ct = (p * S + s) * k + j is live by embed_code_grad_keys_kernel's rule (the rule of the
// forward), belongs to table row r = offset_s + tokens[c, s, j] and carries weights[c, s, j] * float(g[p, 0 : hp]) -- the whole row of g,
// the same for every slot.  G[r] is the sum of the row's contributions, bins[r] their number.  Keys, sort, plan and combine are the
// codebook gradient's (embed_grad_kernels.h) over the table's rows; the order is therefore its order: a row's contributions by
// increasing ct, one fp32 chain acc = +0; acc = fmaf(w, g, acc) per MEDTOK_EMBED_CODE_GRAD_CHUNK of them, the chunk sums added in chunk
// order.  On g tiled S times ([n, S * hp], block s a copy of g) medtok_embed_code_grad_f32 gives the same bits.
//
//   embed_table_grad_chunk_kernel<LANES, G_T>   embed_code_grad_chunk_kernel with two differences: the gather address of a contribution is
//                                  p * g_stride (no slot offset), and g is read in its own type G_T = float, _Float16 or __bf16: a 16-bit
//                                  row is loaded as 16-bit (8 bytes per lane and load for four columns) and widened in registers, which
//                                  is exact; no fp32 copy of the [n, hp] gradient is made.  Structure as there: LANES = 16 for hp <= 64
//                                  (four items per wavefront), else 64; the metadata of a chunk in flight together; four row gathers in
//                                  flight before the first fmaf; items [K, K + Q) spread the rows with several chunks, so no group adds
//                                  more than CHUNK rows whatever the code frequencies.  Every loop around a shuffle has a trip count
//                                  uniform over the wavefront.  No float atomics; every address product is 64-bit; an index is checked
//                                  again before it forms the address of a weight.
#pragma once

__device__ __forceinline__ float4 table_grad_ld4(const float *p) { return ld4(p); }
__device__ __forceinline__ float4 table_grad_ld4(const _Float16 *p)
{
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const h4 h = *reinterpret_cast<const h4 *>(p);
    return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
__device__ __forceinline__ float4 table_grad_ld4(const __bf16 *p)
{
    const uint2 u = *reinterpret_cast<const uint2 *>(p);          // bf16 is the upper half of the fp32 with the same value
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}

template <int LANES, typename G_T>
__global__ __launch_bounds__(256) void embed_table_grad_chunk_kernel(const G_T *__restrict__ g, long g_stride, const int64_t *__restrict__ index,
                                                                     const float *__restrict__ weights, long num_codes, int slots, int topk, int hp,
                                                                     const uint32_t *__restrict__ sorted, const int *__restrict__ offsets,
                                                                     const int *__restrict__ first_chunk, long n_rows, long extra,
                                                                     float *__restrict__ bins, float *__restrict__ G,
                                                                     float *__restrict__ chunk_sums)
{
    constexpr int CHUNK = MEDTOK_EMBED_CODE_GRAD_CHUNK;
    constexpr int R = LANES == 64 ? CHUNK / 64 : 4;               // rounds of LANES entries whose metadata a lane holds at once
    static_assert(CHUNK % (R * LANES) == 0, "a chunk is a whole number of batches");
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (LANES - 1), base = lane & ~(LANES - 1);
    const long item = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES;
    // what this group sums: entries sorted[first .. first + cnt) into dst (nullptr: nothing; the group still runs the uniform loops)
    int first = 0, cnt = 0;
    float *dst = nullptr;
    if (item < n_rows) {
        const int lo = offsets[item], len = offsets[item + 1] - lo;
        if (sub == 0) bins[item] = (float)len;
        if (len <= CHUNK) { first = lo; cnt = len; dst = G + item * hp; }
    } else if (item < n_rows + extra) {
        const int q = (int)(item - n_rows);
        if (q < first_chunk[n_rows]) {
            long a = 0, b = n_rows - 1;                           // the row r with first_chunk[r] <= q < first_chunk[r + 1]
            while (a < b) {
                const long mid = (a + b) >> 1;
                if (first_chunk[mid + 1] > q) b = mid; else a = mid + 1;
            }
            const int lo = offsets[a] + (q - first_chunk[a]) * CHUNK, left = offsets[a + 1] - lo;
            first = lo;
            cnt = left < CHUNK ? left : CHUNK;
            dst = chunk_sums + (long)q * hp;
        }
    }
    int most = cnt;                                               // uniform over the wavefront: the loops below hold shuffles
    if (LANES < 64) {
#pragma unroll
        for (int off = LANES; off < 64; off <<= 1) most = max(most, __shfl_xor(most, off, 64));
    }
    const long entries_per_pos = (long)slots * topk;
    float wm[R];
    long long gm[R];
    auto load_meta = [&](int b0) {                                // rounds b0 / LANES .. + R: entry b0 + r * LANES + sub in this lane
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = b0 + r * LANES + sub;
            wm[r] = 0.f;
            gm[r] = 0;
            if (e < cnt) {
                const long ct = sorted[first + e];
                const long pos = ct / entries_per_pos;
                const int rest = (int)(ct - pos * entries_per_pos);
                const long c = index[pos];
                if (c >= 0 && c < num_codes) {                    // (it was when the key was made: no address from an unchecked index)
                    wm[r] = weights[c * entries_per_pos + rest];  // 64-bit product
                    gm[r] = pos * g_stride;                       // the whole row: every slot of a position reads the same hp columns
                }
            }
        }
    };
    if (LANES == 64) load_meta(0);                                // CHUNK == R * 64: one batch, loaded once for every column pass
    const int passes = LANES == 64 ? (hp + 255) / 256 : 1;        // hp <= 64 with 16 lanes: one float4 column per lane
    for (int pass = 0; pass < passes; ++pass) {
        const int i = (pass * LANES + sub) * 4;
        const bool on = i < hp;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b0 = 0; b0 < most; b0 += R * LANES) {
            if (LANES < 64) load_meta(b0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int r0 = b0 + r * LANES;
                if (r0 >= most) break;                            // uniform
                for (int t = 0; t < LANES; t += 4) {
                    if (r0 + t >= most) break;                    // uniform
                    float w[4];
                    float4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {                 // four gathers in flight, the fmafs stay in list order
                        w[u] = __shfl(wm[r], base + t + u, 64);
                        const long long at = __shfl(gm[r], base + t + u, 64);
                        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (on && r0 + t + u < cnt) v[u] = table_grad_ld4(g + at + i);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (r0 + t + u < cnt) {
                            a.x = fmaf(w[u], v[u].x, a.x); a.y = fmaf(w[u], v[u].y, a.y);
                            a.z = fmaf(w[u], v[u].z, a.z); a.w = fmaf(w[u], v[u].w, a.w);
                        }
                }
            }
        }
        if (on && dst) st4(dst + i, a);
    }
}
