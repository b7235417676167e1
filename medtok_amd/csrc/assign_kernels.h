// assign_kernels.h -- the soft assignment (softmax(-d), code mix, straight-through output, squared error) and the fixed-order fp64
// sum the losses are reduced with.  Included by medtok_vq.hip.
#pragma once

// ================================================================= soft assign
// One wavefront per row; lanes stride the D axis in float4.
template <int MAXK>
__global__ __launch_bounds__(256) void soft_assign_kernel(const float *__restrict__ xref, const float *__restrict__ what,
                                                          const int64_t *__restrict__ idx, const float *__restrict__ dist,
                                                          long n, int d, int topk, int flags, float *__restrict__ w_out,
                                                          float *zq_ste, long zq_stride, float *__restrict__ row_sqerr,
                                                          const int *__restrict__ row_list, const int *__restrict__ row_count)
{
    const bool hard = flags & MEDTOK_ASSIGN_HARD, raw = flags & MEDTOK_ASSIGN_RAW;
    const int lane = threadIdx.x & 63;
    long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    if (row_list) {                    // only the listed rows (the filter's exact-path leftovers after a fused assignment)
        if (row >= *row_count) return;
        row = row_list[row];
    }
    float wj[MAXK];
    long cj[MAXK];
    if (hard) {
        wj[0] = 1.f;
        cj[0] = idx[row];
    } else {
        const float m = -dist[row * topk];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < MAXK; ++j)
            if (j < topk) { wj[j] = expf(-dist[row * topk + j] - m); sum += wj[j]; cj[j] = idx[row * topk + j]; }
#pragma unroll
        for (int j = 0; j < MAXK; ++j)
            if (j < topk) wj[j] = wj[j] / sum;
    }
    if (w_out && lane < topk) {
        float v = wj[0];
#pragma unroll
        for (int j = 1; j < MAXK; ++j) v = (lane == j) ? wj[j] : v;
        w_out[row * topk + lane] = v;
    }
    const float *xr = xref + row * d;
    float *out = zq_ste + row * zq_stride;
    float se = 0.f;
    for (int i = lane * 4; i < d; i += 256) {
        float4 a;
        if (hard) {
            a = ld4(what + cj[0] * d + i);
        } else {
            a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < MAXK; ++j)
                if (j < topk) {
                    const float4 e = ld4(what + cj[j] * d + i);
                    a.x = fmaf(wj[j], e.x, a.x); a.y = fmaf(wj[j], e.y, a.y);
                    a.z = fmaf(wj[j], e.z, a.z); a.w = fmaf(wj[j], e.w, a.w);
                }
        }
        const float4 x = ld4(xr + i);
        float4 df;
        df.x = a.x - x.x; df.y = a.y - x.y; df.z = a.z - x.z; df.w = a.w - x.w;
        st4(out + i, raw ? a : make_float4(x.x + df.x, x.y + df.y, x.z + df.z, x.w + df.w));
        se = fmaf(df.x, df.x, se); se = fmaf(df.y, df.y, se); se = fmaf(df.z, df.z, se); se = fmaf(df.w, df.w, se);
    }
    se = wave_butterfly_sum(se);
    if (row_sqerr && lane == 0) row_sqerr[row] = se;
}

// ================================================================= fixed-order fp64 sum
__global__ __launch_bounds__(1024) void sum_scale_kernel(const float *__restrict__ v, long n, double scale, float *out)
{
    __shared__ double sh[1024];
    double a = 0.0;
    long i = threadIdx.x;
    // same order of additions as the plain loop; eight loads in flight per thread instead of one (one block: latency-bound)
    for (; i + 7 * 1024 < n; i += 8 * 1024) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = v[i + u * 1024];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += (double)x[u];
    }
    for (; i < n; i += 1024) a += (double)v[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(sh[0] * scale);
}
