// ema_kernels.h -- codebook statistics of NormEMAVectorQuantizer: histogram, stable radix sort by code and segmented row sum, the EMA
// update, and the sliding usage window.  Included by medtok_vq.hip.
#pragma once

// ================================================================= EMA statistics
// bins: integer histogram.  embed_sum: rows are ordered by (code, row) with a stable LSD radix
// sort (8-bit digits), then one wavefront per code adds its rows in increasing row order.
constexpr int SORT_BLOCKS = 64;        // x 4 waves = 256 sorting waves (the digit x wave count table is scanned by ONE block)
constexpr int SORT_WAVES = SORT_BLOCKS * 4;

// ids outside [0, K) are clamped (same clamp in the sort) so the layout stays consistent
__device__ __forceinline__ uint32_t clamp_code(int64_t c, int k_codes)
{
    return (uint32_t)(c < 0 ? 0 : (c >= k_codes ? k_codes - 1 : c));
}

__global__ __launch_bounds__(256) void hist_kernel(const int64_t *__restrict__ idx, long n, int k_codes, int *__restrict__ counts)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        atomicAdd(&counts[clamp_code(idx[i], k_codes)], 1);
}

// exclusive scan of counts[0..k) -> offsets[0..k] (single block, fixed order).  A thread owns 16 consecutive entries of each of
// up to four 16384-entry slabs per pass (a wave's loads cover 4 KB of consecutive memory): per-thread sums, a shuffle scan inside
// the wave, one scan of the 64 (slab, wave) totals by wave 0, then the entries are written with their running offsets.  (The first
// form gave every thread one long contiguous chunk -- 64 lanes 256 bytes apart -- and took 30-40 us for the 65536-entry digit
// table of a radix pass.)
__global__ __launch_bounds__(1024) void scan_kernel(const int *__restrict__ counts, int k, int *__restrict__ offsets)
{
    constexpr int PER = 16, SLABS = 4;
    __shared__ int wave_tot[SLABS * 16], wave_pre[SLABS * 16], carry_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool vec = ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(offsets)) & 15) == 0;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < k; base += SLABS * 1024 * PER) {
        int v[SLABS][PER], incl[SLABS], sum[SLABS];
#pragma unroll
        for (int j = 0; j < SLABS; ++j) {
            const int start = base + (j * 1024 + t) * PER;
            if (vec && start + PER <= k) {
#pragma unroll
                for (int c = 0; c < PER / 4; ++c) {
                    const int4 q = *reinterpret_cast<const int4 *>(counts + start + 4 * c);
                    v[j][4 * c] = q.x; v[j][4 * c + 1] = q.y; v[j][4 * c + 2] = q.z; v[j][4 * c + 3] = q.w;
                }
            } else {
#pragma unroll
                for (int c = 0; c < PER; ++c) v[j][c] = start + c < k ? counts[start + c] : 0;
            }
            int sm = 0;
#pragma unroll
            for (int c = 0; c < PER; ++c) sm += v[j][c];
            sum[j] = sm;
            int in = sm;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(in, off, 64);
                if (lane >= off) in += o;
            }
            incl[j] = in;
            if (lane == 63) wave_tot[j * 16 + wave] = in;
        }
        __syncthreads();
        if (t < 64) {                                   // the 64 (slab, wave) totals in order
            const int carry = carry_s;                  // (only this wave touches carry_s inside the loop: read, then written below, in program order)
            const int x = wave_tot[t];
            int in = x;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(in, off, 64);
                if (lane >= off) in += o;
            }
            wave_pre[t] = carry + in - x;
            if (t == 63) carry_s = carry + in;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SLABS; ++j) {
            const int start = base + (j * 1024 + t) * PER;
            int run = wave_pre[j * 16 + wave] + incl[j] - sum[j];
            if (vec && start + PER <= k) {
#pragma unroll
                for (int c = 0; c < PER / 4; ++c) {
                    int4 o;
                    o.x = run; o.y = o.x + v[j][4 * c]; o.z = o.y + v[j][4 * c + 1]; o.w = o.z + v[j][4 * c + 2];
                    run = o.w + v[j][4 * c + 3];
                    *reinterpret_cast<int4 *>(offsets + start + 4 * c) = o;
                }
            } else {
#pragma unroll
                for (int c = 0; c < PER; ++c)
                    if (start + c < k) { offsets[start + c] = run; run += v[j][c]; }
            }
        }
        __syncthreads();                                // wave_tot / wave_pre are reused by the next pass
    }
    if (t == 0) offsets[k] = carry_s;
}

__device__ __forceinline__ void wave_chunk(long n, int gw, long &lo, long &hi)
{
    const long per = ((n + SORT_WAVES - 1) / SORT_WAVES + 63) / 64 * 64;
    lo = min(n, (long)gw * per);
    hi = min(n, lo + per);
}

// pass 0 reads keys from idx (payload = position); later passes read (key,payload) pairs
template <bool FIRST>
__global__ __launch_bounds__(256) void radix_count_kernel(const int64_t *__restrict__ idx, const uint32_t *__restrict__ keys_in,
                                                          long n, int k_codes, int shift, int *__restrict__ wave_counts)
{
    __shared__ int cnt[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gw = blockIdx.x * 4 + w;
    for (int i = lane; i < 256; i += 64) cnt[w][i] = 0;
    __syncthreads();
    long lo, hi;
    wave_chunk(n, gw, lo, hi);
    for (long i = lo + lane; i < hi; i += 64) {
        const uint32_t key = FIRST ? clamp_code(idx[i], k_codes) : keys_in[i];
        atomicAdd(&cnt[w][(key >> shift) & 255], 1);
    }
    __syncthreads();
    // digit-major so the scan below yields stable destinations
    for (int i = lane; i < 256; i += 64) wave_counts[(long)i * SORT_WAVES + gw] = cnt[w][i];
}

template <bool FIRST>
__global__ __launch_bounds__(256) void radix_scatter_kernel(const int64_t *__restrict__ idx, const uint32_t *__restrict__ keys_in,
                                                            const uint32_t *__restrict__ vals_in, long n, int k_codes, int shift,
                                                            const int *__restrict__ wave_offsets, uint32_t *__restrict__ keys_out,
                                                            uint32_t *__restrict__ vals_out)
{
    __shared__ int base[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gw = blockIdx.x * 4 + w;
    for (int i = lane; i < 256; i += 64) base[w][i] = wave_offsets[(long)i * SORT_WAVES + gw];
    __syncthreads();
    long lo, hi;
    wave_chunk(n, gw, lo, hi);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    for (long i0 = lo; i0 < hi; i0 += 64) {
        const long i = i0 + lane;
        const bool live = i < hi;
        uint32_t key = 0, val = 0;
        if (live) { key = FIRST ? clamp_code(idx[i], k_codes) : keys_in[i]; val = FIRST ? (uint32_t)i : vals_in[i]; }
        const uint32_t dg = (key >> shift) & 255;
        unsigned long long eq = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bal = __ballot((dg >> b) & 1);
            eq &= ((dg >> b) & 1) ? bal : ~bal;
        }
        const int rank = __popcll(eq & lt_mask);
        const int total = __popcll(eq);
        int dst = 0;
        if (live) dst = base[w][dg] + rank;
        __builtin_amdgcn_wave_barrier();
        if (live && rank == total - 1) base[w][dg] += total;   // one lane per digit group
        __builtin_amdgcn_wave_barrier();
        if (live) { keys_out[dst] = key; vals_out[dst] = val; }
    }
}

// One wavefront per code: add that code's rows in increasing row order.
__global__ __launch_bounds__(256) void segsum_kernel(const float *__restrict__ zhat, const uint32_t *__restrict__ sorted_rows,
                                                     const int *__restrict__ offsets, int k_codes, int d,
                                                     float *__restrict__ bins, float *__restrict__ embed_sum)
{
    const int lane = threadIdx.x & 63;
    for (long code = (long)blockIdx.x * 4 + (threadIdx.x >> 6); code < k_codes; code += (long)gridDim.x * 4) {
        const int lo = offsets[code], hi = offsets[code + 1];
        if (lane == 0) bins[code] = (float)(hi - lo);
        for (int i = lane * 4; i < d; i += 256) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            int r = lo;
            for (; r + 4 <= hi; r += 4) {      // 4 loads in flight, adds stay in row order
                const float4 v0 = ld4(zhat + (long)sorted_rows[r] * d + i);
                const float4 v1 = ld4(zhat + (long)sorted_rows[r + 1] * d + i);
                const float4 v2 = ld4(zhat + (long)sorted_rows[r + 2] * d + i);
                const float4 v3 = ld4(zhat + (long)sorted_rows[r + 3] * d + i);
                a.x += v0.x; a.y += v0.y; a.z += v0.z; a.w += v0.w;
                a.x += v1.x; a.y += v1.y; a.z += v1.z; a.w += v1.w;
                a.x += v2.x; a.y += v2.y; a.z += v2.z; a.w += v2.w;
                a.x += v3.x; a.y += v3.y; a.z += v3.z; a.w += v3.w;
            }
            for (; r < hi; ++r) {
                const float4 v = ld4(zhat + (long)sorted_rows[r] * d + i);
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
            st4(embed_sum + code * d + i, a);
        }
    }
}

// bins only (eval branch of the reference, norm_ema_quantizer.py:185-188)
__global__ __launch_bounds__(256) void counts_to_float_kernel(const int *__restrict__ counts, long k, float *__restrict__ bins)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < k) bins[i] = (float)counts[i];
}

// ================================================================= EMA apply
__global__ __launch_bounds__(256) void ema_apply_kernel(float *E, float *cluster_size, const float *__restrict__ bins,
                                                        const float *__restrict__ embed_sum, int k_codes, int d, float decay, float omd)
{
    const int lane = threadIdx.x & 63;
    const long code = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (code >= k_codes) return;
    const float b = bins[code];
    if (lane == 0) {
        const float a0 = cluster_size[code] * decay;
        const float a1 = b * omd;
        cluster_size[code] = a0 + a1;
    }
    float *e = E + code * d;
    const float *sm = embed_sum + code * d;
    const bool keep = (b == 0.0f);
    float den1 = 1.f;
    if (!keep) {
        float p = 0.f;
        for (int i = lane * 4; i < d; i += 256) {
            float4 v = ld4(sm + i);
            v.x = v.x / b; v.y = v.y / b; v.z = v.z / b; v.w = v.w / b;
            p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
        }
        den1 = fmaxf(sqrtf(wave_butterfly_sum(p)), 1e-12f);
    }
    auto mixed = [&](int i) {
        float4 nw;
        const float4 ev = ld4(e + i);
        if (keep) nw = ev;
        else {
            nw = ld4(sm + i);
            nw.x = (nw.x / b) / den1; nw.y = (nw.y / b) / den1; nw.z = (nw.z / b) / den1; nw.w = (nw.w / b) / den1;
        }
        float4 m;
        float t0, t1;
        t0 = ev.x * decay; t1 = nw.x * omd; m.x = t0 + t1;
        t0 = ev.y * decay; t1 = nw.y * omd; m.y = t0 + t1;
        t0 = ev.z * decay; t1 = nw.z * omd; m.z = t0 + t1;
        t0 = ev.w * decay; t1 = nw.w * omd; m.w = t0 + t1;
        return m;
    };
    float p = 0.f;
    for (int i = lane * 4; i < d; i += 256) {
        const float4 m = mixed(i);
        p = fmaf(m.x, m.x, p); p = fmaf(m.y, m.y, p); p = fmaf(m.z, m.z, p); p = fmaf(m.w, m.w, p);
    }
    const float den2 = fmaxf(sqrtf(wave_butterfly_sum(p)), 1e-12f);
    for (int i = lane * 4; i < d; i += 256) {
        float4 m = mixed(i);
        m.x = m.x / den2; m.y = m.y / den2; m.z = m.z / den2; m.w = m.w / den2;
        st4(e + i, m);
    }
}

__global__ __launch_bounds__(256) void ema_cluster_size_kernel(float *cs, const float *__restrict__ bins, long k, float decay, float omd)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const float a0 = cs[i] * decay;
    const float a1 = bins[i] * omd;
    cs[i] = a0 + a1;
}

// ================================================================= codebook usage window
__global__ __launch_bounds__(256) void usage_shift_kernel(const float *__restrict__ win, long wlen, const int64_t *__restrict__ ids,
                                                          long m, float *__restrict__ tmp)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < wlen; i += (long)gridDim.x * 256) {
        float v;
        if (m >= wlen) v = (float)ids[m - wlen + i];
        else v = (i < wlen - m) ? win[i + m] : (float)ids[i - (wlen - m)];
        tmp[i] = v;
    }
}

// Distinct count without atomics on the hot words: every window entry stores 1 into its code's flag byte (all
// writers write the same value, so the race is benign), then one block sums the n_codes + 1 flags.  (300 000 atomicOr
// operations on a 21 000-bit map serialise on ~650 words: 1.6 ms; this form takes microseconds.)
__global__ __launch_bounds__(256) void usage_mark_kernel(const float *__restrict__ tmp, long wlen, long n_codes, float *__restrict__ win,
                                                         unsigned char *__restrict__ flags)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < wlen; i += (long)gridDim.x * 256) {
        const float v = tmp[i];
        win[i] = v;
        long c = (long)v;
        if (c < 0 || c >= n_codes) c = n_codes;
        flags[c] = 1;
    }
}

__global__ __launch_bounds__(1024) void usage_sum_kernel(const unsigned char *__restrict__ flags, long n, int *__restrict__ count)
{
    __shared__ int sh[1024];
    int a = 0;
    for (long i = threadIdx.x; i < n; i += 1024) a += flags[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = sh[0];
}

// ---- the forward's three to five window updates (:241-250: shared, text, graph, and the aug views') in ONE call of two launches
// (twelve to twenty before: each update a memset and three launches over the 300 000-entry window).  Conceptually the updates slide
// one window over U = [old window | ids_1 | ids_2 | ...]: after update u the window is U[off_u, off_u + W), off_u = m_1 + ... + m_u.
// One pass over U marks every entry in the flag map of each update whose window holds it and writes the final window
// U[M, M + W) to scratch; a second pass copies it back and sums the maps.  Same values as the updates one by one.
constexpr int USAGE_MULTI_MAX = 6;
struct UsageMultiArgs { const int64_t *ids[USAGE_MULTI_MAX]; long m[USAGE_MULTI_MAX]; int count; };

__global__ __launch_bounds__(256) void usage_multi_mark_kernel(const float *__restrict__ win, long wlen, UsageMultiArgs a, long n_codes,
                                                               float *__restrict__ tmp, unsigned char *__restrict__ flags)
{
    long total = 0;
    for (int u = 0; u < a.count; ++u) total += a.m[u];
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < wlen + total; p += (long)gridDim.x * 256) {
        float v;
        if (p < wlen) v = win[p];
        else {
            long q = p - wlen;
            int u = 0;
            while (q >= a.m[u]) { q -= a.m[u]; ++u; }
            v = (float)a.ids[u][q];
        }
        long c = (long)v;
        if (c < 0 || c >= n_codes) c = n_codes;
        long off = 0;
        for (int u = 0; u < a.count; ++u) {
            off += a.m[u];
            if (p >= off && p < off + wlen) flags[(long)u * (n_codes + 1) + c] = 1;
        }
        if (p >= total) tmp[p - total] = v;
    }
}

__global__ __launch_bounds__(256) void usage_multi_finish_kernel(const float *__restrict__ tmp, long wlen, float *__restrict__ win,
                                                                 const unsigned char *__restrict__ flags, long n_codes, int count, int *__restrict__ counts,
                                                                 const int *__restrict__ extra_word = nullptr)
{
    // (extra_word: a device word the caller wants behind the counts -- its one host read then fetches both.  A NON-ZERO word vetoes
    // the window write: the caller's device-side input checks failed, the ids are not to be trusted, and the caller -- who sees the
    // word with the counts -- repeats the forward on repaired inputs against the window as it was)
    const bool veto = extra_word && extra_word[0] != 0;
    if (extra_word && blockIdx.x == 0 && threadIdx.x == 0) counts[count] = extra_word[0];
    if (!veto)
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < wlen; i += (long)gridDim.x * 256) win[i] = tmp[i];
    const int lane = threadIdx.x & 63;
    for (int u = 0; u < count; ++u) {
        int part = 0;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_codes + 1; i += (long)gridDim.x * 256) part += flags[(long)u * (n_codes + 1) + i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
        if (lane == 0 && part) atomicAdd(&counts[u], part);                // (integer: exact in any order)
    }
}
