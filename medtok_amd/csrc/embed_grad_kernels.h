// Gradient of the normalised codebook through the embedding lookup, straight from the upstream gradient of embed_codes_kernel's rows.
// Included by medtok_vq.hip behind embed_kernels.h and ema_kernels.h (uses ld4 / st4, DecodeRegions, and the scan and stable radix sort
// of the EMA statistics).
//
// The lookup writes out[p, s * d : (s + 1) * d] = sum_j weights[c, s, j] * what[lo_s + tokens[c, s, j]], c = index[p].  Contribution
// number ct = (p * S + s) * k + j is LIVE exactly when embed_codes_kernel mixes that (position, slot): pad[p] == 0, 0 <= c < num_codes
// and EVERY one of the k ids of slot s of code c inside [0, size_s) (one bad id: the forward wrote the block as zeros, so all k
// contributions of the slot are dead).  A live contribution belongs to codebook row r = lo_s + tokens[c, s, j] and carries
// weights[c, s, j] * g_out[p, s * d : (s + 1) * d];  g_what[r] is the sum of the row's contributions, bins[r] their number.  No
// [n * S * k, d] buffer of contribution rows exists: the sort moves 8 bytes per contribution and the sums gather g_out directly.
//
//   embed_code_grad_keys_kernel    one sort key per contribution (the row; K = "one bin past the codebook" for a dead one), the payload
//                                  ct, and the integer histogram of the live keys.  Mapping and validation are embed_codes_kernel's: one
//                                  item = one (position, slot), LANES lanes per item, lane j < k loads id j, a ballot over the group's
//                                  lanes finds a bad id.  No index and no id forms an address before it has been checked; every product
//                                  with a code index is 64-bit.
//   scan_kernel, radix_*_kernel    (ema_kernels.h) offsets[r] and the stable sort by key: row r's contributions are
//                                  sorted[offsets[r] .. offsets[r + 1]) in increasing ct; the dead ones lie behind offsets[K].
//   embed_code_grad_plan_kernel    chunks[r] = number of chunks of a row with MORE than one chunk, else 0 (scanned into first_chunk[]).
//   embed_grad_chunk_kernel        the sums.  A row's list is cut into chunks of MEDTOK_EMBED_CODE_GRAD_CHUNK consecutive entries; a chunk
//                                  is, per element, ONE fp32 chain acc = +0; acc = fmaf(w, g, acc) in list order.  Items [0, K) are the
//                                  rows: a row of at most one chunk is finished here (an empty one: zeros), and every row's bin is
//                                  written.  Items [K, K + Q) are the chunks of the longer rows (Q = ceil(2 * n * S * k / CHUNK) bounds
//                                  them: a row of len > CHUNK has ceil(len / CHUNK) < 2 * len / CHUNK chunks): item K + q finds its row by
//                                  bisection in first_chunk[] and writes chunk_sums[q].  So no group of lanes adds more than CHUNK rows,
//                                  whatever the code frequencies: a hot code's rows are spread over n / CHUNK wavefronts each.
//   embed_code_grad_combine_kernel g_what[r] = the chunk sums of a row with several, added in chunk order from +0.
// No float atomics anywhere; the order is fixed by the data alone (not by the device or a launch heuristic): two runs give the same bits.
//
// The FOLDED lookup (embed_folded_kernel) writes out[p, :] = bias + sum_s sum_j weights[c, s, j] * table[offset_s + tokens[c, s, j], :]:
// every slot adds into the SAME hp columns.  Its per-table-row sums G[r] -- what the projector's weight gradient and the codebook's
// gradient through the folded tables are both made of -- are the same pipeline over the table's rows with two differences, both template
// arguments of the chunk kernel: a contribution carries the WHOLE row g[p, 0 : hp] (SLOT_BLOCKS = false: no slot offset in the gather
// address; true: the slot's block g_out[p, s * d : (s + 1) * d] of embed_codes_kernel's rows), and g is read in its own type G_T =
// float, _Float16 or __bf16: a 16-bit row is loaded as 16-bit (8 bytes per lane and load for four columns) and widened in registers,
// which is exact; no fp32 copy of the [n, hp] gradient is made.  Keys, sort, plan, combine and the order are shared, so on g tiled S
// times ([n, S * hp], block s a copy of g) the codebook gradient gives the same bits.
//
// The chunk kernel: LANES = 64 lanes per item (16 for d <= 64, four items per wavefront, as the other embed kernels).  Lane l of a group
// loads the metadata of entry l of a round of LANES entries -- sorted ct, then index[p], then the weight: three dependent loads, all
// rounds of a chunk in flight together (LANES == 64) -- and keeps (w, offset of the g_out block); a shuffle hands them round, four row
// gathers are in flight before the first fmaf.  Every loop around a shuffle has a trip count uniform over the wavefront.
#pragma once

// MEDTOK_EMBED_CODE_GRAD_CHUNK (256) is part of the result's bits and therefore of the ABI: include/medtok_vq.h defines it.

template <int LANES>
__global__ __launch_bounds__(256) void embed_code_grad_keys_kernel(const int64_t *__restrict__ index, const uint8_t *__restrict__ pad, long items,
                                                                   const int64_t *__restrict__ tokens, long num_codes, int slots, int topk,
                                                                   DecodeRegions reg, int n_codes, uint32_t *__restrict__ keys,
                                                                   uint32_t *__restrict__ vals, int *__restrict__ counts)
{
    static_assert(MEDTOK_MAX_TOPK <= LANES, "lane j of a group loads id j");
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (LANES - 1), base = lane & ~(LANES - 1);
    long item = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES;
    const bool live = item < items;
    if (!live) item = 0;
    const long pos = item / slots;
    const int slot = (int)(item - pos * slots);
    long lo = reg.lo[0], size = reg.size[0];
#pragma unroll
    for (int s = 1; s < MEDTOK_DECODE_MAX_SLOTS; ++s)
        if (slot == s) { lo = reg.lo[s]; size = reg.size[s]; }
    const bool padded = !live || (pad && pad[pos] != 0);
    const long c = padded ? 0 : index[pos];
    const bool is_code = !padded && c >= 0 && c < num_codes;
    long id = 0;
    if (is_code && sub < topk) id = tokens[(c * slots + slot) * topk + sub];     // 64-bit: c < num_codes was checked above
    const bool bad_lane = id < 0 || id >= size;                   // (a lane without an id holds 0: in range, size >= 1)
    const unsigned long long votes = __ballot(bad_lane);
    bool bad;
    if (LANES == 64) bad = votes != 0ull;
    else bad = ((votes >> base) & ((1ull << (LANES & 63)) - 1ull)) != 0ull;
    if (!live || sub >= topk) return;
    const uint32_t key = is_code && !bad ? (uint32_t)(lo + id) : (uint32_t)n_codes;      // lo + size <= n_codes < 2^31 (checked on the host)
    const long ct = item * topk + sub;                            // < 2^31 (checked on the host)
    keys[ct] = key;
    vals[ct] = (uint32_t)ct;
    if (key < (uint32_t)n_codes) atomicAdd(&counts[key], 1);      // (integer: exact in any order)
}

// the histogram's zeros, written by a kernel (not a memset node: the whole call is kernel launches, also when a graph records it)
__global__ __launch_bounds__(256) void embed_code_grad_zero_kernel(int *__restrict__ counts, long k_codes)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r < k_codes) counts[r] = 0;
}

// in place: counts[r] -> the number of chunks of row r where it has more than one, else 0 (CHUNK: MEDTOK_EMBED_CODE_GRAD_CHUNK here,
// MEDTOK_EMBED_POOL_CHUNK for the bags of embed_pool_segments_kernels.h)
template <int CHUNK>
__global__ __launch_bounds__(256) void embed_code_grad_plan_kernel(int *__restrict__ counts, long k_codes)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= k_codes) return;
    const int len = counts[r];
    counts[r] = len > CHUNK ? (len + CHUNK - 1) / CHUNK : 0;
}

template <int LANES, typename G_T, bool SLOT_BLOCKS>
__global__ __launch_bounds__(256) void embed_grad_chunk_kernel(const G_T *__restrict__ g_out, long g_stride, const int64_t *__restrict__ index,
                                                               const float *__restrict__ weights, long num_codes, int slots, int topk, int d,
                                                               const uint32_t *__restrict__ sorted, const int *__restrict__ offsets,
                                                               const int *__restrict__ first_chunk, long k_codes, long extra,
                                                               float *__restrict__ bins, float *__restrict__ g_what,
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
    if (item < k_codes) {
        const int lo = offsets[item], len = offsets[item + 1] - lo;
        if (sub == 0) bins[item] = (float)len;
        if (len <= CHUNK) { first = lo; cnt = len; dst = g_what + item * d; }
    } else if (item < k_codes + extra) {
        const int q = (int)(item - k_codes);
        if (q < first_chunk[k_codes]) {
            long a = 0, b = k_codes - 1;                          // the row r with first_chunk[r] <= q < first_chunk[r + 1]
            while (a < b) {
                const long mid = (a + b) >> 1;
                if (first_chunk[mid + 1] > q) b = mid; else a = mid + 1;
            }
            const int lo = offsets[a] + (q - first_chunk[a]) * CHUNK, left = offsets[a + 1] - lo;
            first = lo;
            cnt = left < CHUNK ? left : CHUNK;
            dst = chunk_sums + (long)q * d;
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
                const int rest = (int)(ct - pos * entries_per_pos), slot = SLOT_BLOCKS ? rest / topk : 0;
                const long c = index[pos];
                if (c >= 0 && c < num_codes) {                    // (it was when the key was made: no address from an unchecked index)
                    wm[r] = weights[c * entries_per_pos + rest];  // 64-bit product
                    gm[r] = pos * g_stride + (long)slot * d;      // the slot's block of the row; slot 0 without SLOT_BLOCKS: the whole row
                }
            }
        }
    };
    if (LANES == 64) load_meta(0);                                // CHUNK == R * 64: one batch, loaded once for every column pass
    const int passes = LANES == 64 ? (d + 255) / 256 : 1;         // d <= 64 with 16 lanes: one float4 column per lane
    for (int pass = 0; pass < passes; ++pass) {
        const int i = (pass * LANES + sub) * 4;
        const bool on = i < d;
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
                        if (on && r0 + t + u < cnt) v[u] = ld4(g_out + at + i);
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

// One wavefront per row with several chunks: their sums in chunk order.
__global__ __launch_bounds__(256) void embed_code_grad_combine_kernel(const float *__restrict__ chunk_sums, const int *__restrict__ first_chunk,
                                                                      long k_codes, int d, float *__restrict__ g_what)
{
    const int lane = threadIdx.x & 63;
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < k_codes; row += (long)gridDim.x * 4) {
        const int lo = first_chunk[row], hi = first_chunk[row + 1];
        if (hi == lo) continue;                                   // at most one chunk: the chunk kernel wrote the row
        for (int i = lane * 4; i < d; i += 256) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int ch = lo; ch < hi; ++ch) {
                const float4 v = ld4(chunk_sums + (long)ch * d + i);
                a.x = a.x + v.x; a.y = a.y + v.y; a.z = a.z + v.z; a.w = a.w + v.w;
            }
            st4(g_what + row * d + i, a);
        }
    }
}
