// search_f32.h -- row norms and the exact fp32 nearest-code search: rownorm kernels, the top-k list helpers, the fp32-MFMA search
// kernel (plain, exclusion-pass and batched forms), the merges of partial lists and the k > 8 join.  Included by medtok_vq.hip
// (one translation unit); the launches and plans live there.
#pragma once

// ================================================================= rownorm
// One wavefront per row.  Lane l owns float4 #(l + 64 t): element i lands in chain
// (i/4)%64 and each chain accumulates in increasing i -- the oracle's canon_sumsq.
typedef _Float16 rn_half4 __attribute__((ext_vector_type(4)));
// xh (optional, NORMALIZE only): the fp16 filter's operand image of the normalised rows, [*, dp] prescaled by 2^8 exactly as
// to_half_kernel writes it -- the one-call forward saves that kernel's pass over xhat.
// n_img (with xh): the image has that many rows; those from n on are written as zeros (the filter reads whole row tiles).
// zero_word: an int the launch clears (the filter's count of rows handed to the exact kernel, when nothing else of the search's
// preparation runs: a prepared codebook).
template <bool NORMALIZE>
__global__ __launch_bounds__(256) void rownorm_kernel(const float *__restrict__ x, long n, int d,
                                                      float *xhat, float *__restrict__ sqn, _Float16 *__restrict__ xh = nullptr, int dp = 0,
                                                      long n_img = 0, int *__restrict__ zero_word = nullptr)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
    if (row >= n) {
        if (NORMALIZE && xh && row < n_img) {
            rn_half4 z;
            z[0] = z[1] = z[2] = z[3] = (_Float16)0.f;
            for (int i = lane * 4; i < dp; i += 256) *reinterpret_cast<rn_half4 *>(xh + row * dp + i) = z;
        }
        return;
    }
    const float *src = x + row * d;
    float *dst = xhat ? xhat + row * d : nullptr;
    float p = 0.f;
    if (NORMALIZE) {
        for (int i = lane * 4; i < d; i += 256) {
            float4 v = ld4(src + i);
            p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
        }
        const float nrm = sqrtf(wave_butterfly_sum(p));
        const float den = fmaxf(nrm, 1e-12f);
        p = 0.f;
        for (int i = lane * 4; i < d; i += 256) {
            float4 v = ld4(src + i);
            v.x = v.x / den; v.y = v.y / den; v.z = v.z / den; v.w = v.w / den;
            st4(dst + i, v);
            if (xh) {
                rn_half4 h;
                h[0] = (_Float16)(v.x * 256.0f); h[1] = (_Float16)(v.y * 256.0f); h[2] = (_Float16)(v.z * 256.0f); h[3] = (_Float16)(v.w * 256.0f);
                *reinterpret_cast<rn_half4 *>(xh + row * dp + i) = h;
            }
            p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
        }
        if (xh) {
            rn_half4 z;
            z[0] = z[1] = z[2] = z[3] = (_Float16)0.f;
            for (int i = d + lane * 4; i < dp; i += 256) *reinterpret_cast<rn_half4 *>(xh + row * dp + i) = z;
        }
    } else {
        for (int i = lane * 4; i < d; i += 256) {
            float4 v = ld4(src + i);
            if (dst && dst != src) st4(dst + i, v);
            p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
        }
    }
    p = wave_butterfly_sum(p);
    if (sqn && lane == 0) sqn[row] = p;
}

// Rows of at most 64 floats (the reference's e_dim): rownorm_kernel leaves 48 of a wavefront's 64 lanes without an element.  Here a
// row has 16 lanes (lane l of its group owns float4 #l, as there), four rows share a wavefront, and the butterfly runs over the
// offsets 8..1 only -- the offsets 32 and 16 of the one-row kernel add the zeros of idle lanes, so the bits are the same.
template <bool NORMALIZE>
__global__ __launch_bounds__(256) void rownorm16_kernel(const float *__restrict__ x, long n, int d,
                                                        float *xhat, float *__restrict__ sqn, _Float16 *__restrict__ xh = nullptr, int dp = 0,
                                                        long n_img = 0, int *__restrict__ zero_word = nullptr)
{
    const int sub = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
    if (NORMALIZE && xh && row >= n && row < n_img && sub * 4 < dp) {      // image rows past the last input row: zeros
        rn_half4 z;
        z[0] = z[1] = z[2] = z[3] = (_Float16)0.f;
        *reinterpret_cast<rn_half4 *>(xh + row * dp + sub * 4) = z;
    }
    const bool live = row < n, mine = live && sub * 4 < d;
    const long r = live ? row : 0;
    const float *src = x + r * d + sub * 4;
    float4 v = mine ? ld4(src) : make_float4(0.f, 0.f, 0.f, 0.f);
    float p = 0.f;
    p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    if (NORMALIZE) {
        const float den = fmaxf(sqrtf(p), 1e-12f);
        v.x = v.x / den; v.y = v.y / den; v.z = v.z / den; v.w = v.w / den;
        if (mine) {
            st4(xhat + r * d + sub * 4, v);
            if (xh) {
                rn_half4 h;
                h[0] = (_Float16)(v.x * 256.0f); h[1] = (_Float16)(v.y * 256.0f); h[2] = (_Float16)(v.z * 256.0f); h[3] = (_Float16)(v.w * 256.0f);
                *reinterpret_cast<rn_half4 *>(xh + r * dp + sub * 4) = h;
            }
        } else if (live && xh && sub * 4 < dp) {
            rn_half4 z;
            z[0] = z[1] = z[2] = z[3] = (_Float16)0.f;
            *reinterpret_cast<rn_half4 *>(xh + r * dp + sub * 4) = z;
        }
        p = 0.f;
        p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    } else if (mine && xhat && xhat != x) {
        st4(xhat + r * d + sub * 4, v);
    }
    if (sqn && live && sub == 0) sqn[row] = p;
}

// single VALU instructions (fminf on MFMA results makes hipcc put a canonicalising v_max in front of each operand)
__device__ __forceinline__ float vs_min(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vs_min3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// ================================================================= top-k list helpers
// Sorted ascending by (value, index).  A lane meets its codes in increasing index order,
// so a strict '<' on the value alone implements "ties -> lowest index" during the scan.
template <int T>
__device__ __forceinline__ void topk_insert(float (&bv)[T], int (&bi)[T], float v, int c)
{
    if (v < bv[T - 1]) {
#pragma unroll
        for (int j = T - 1; j >= 1; --j) {
            const bool lt_prev = v < bv[j - 1];
            const bool lt = v < bv[j];
            bv[j] = lt_prev ? bv[j - 1] : (lt ? v : bv[j]);
            bi[j] = lt_prev ? bi[j - 1] : (lt ? c : bi[j]);
        }
        const bool lt0 = v < bv[0];
        bv[0] = lt0 ? v : bv[0];
        bi[0] = lt0 ? c : bi[0];
    }
}

__device__ __forceinline__ bool lex_lt(float v, int c, float bv, int bc)
{
    return v < bv || (v == bv && c < bc);
}

// A row whose distances are NaN never inserts anything and its list keeps the sentinel index.  Token ids leave the library
// in range regardless -- slot j falls back to code j (torch.topk / argmin also return valid indices for such rows, so the
// reference's AMP loop survives an overflowed step; the gathers downstream index the codebook with these ids).
__device__ __forceinline__ int valid_code(int c, int j, int k_codes) { return (unsigned)c < (unsigned)k_codes ? c : j % k_codes; }

// Same, but for merging lists whose codes are not met in order: compare (value, index).
template <int T>
__device__ __forceinline__ void topk_insert_lex(float (&bv)[T], int (&bi)[T], float v, int c)
{
    if (lex_lt(v, c, bv[T - 1], bi[T - 1])) {
#pragma unroll
        for (int j = T - 1; j >= 1; --j) {
            const bool lt_prev = lex_lt(v, c, bv[j - 1], bi[j - 1]);
            const bool lt = lex_lt(v, c, bv[j], bi[j]);
            const float nv = lt_prev ? bv[j - 1] : (lt ? v : bv[j]);
            const int ni = lt_prev ? bi[j - 1] : (lt ? c : bi[j]);
            bv[j] = nv; bi[j] = ni;
        }
        const bool lt0 = lex_lt(v, c, bv[0], bi[0]);
        bv[0] = lt0 ? v : bv[0];
        bi[0] = lt0 ? c : bi[0];
    }
}

// ================================================================= fp32 MFMA search
// Block = 4 waves, tile = 128 codes x 128 rows, BK = 32.  Codes are the MFMA "A" rows and
// input rows the "B" columns, so after v_mfma_f32_32x32x2_f32 every lane holds 16 codes of
// ONE input row: the running top-k is lane-local (no cross-lane traffic until the end).
// Wave w owns input rows [32w, 32w+32) against all 128 codes (4 accumulator tiles).
//
// LDS keeps rows as they are in memory.  Lane (i, h) reads one float4 of each 8-wide k-group at
// +4h; register c then carries element 8g + 4h + c, and MFMA #c consumes (half 0 -> 8g+c,
// half 1 -> 8g+4+c).  The accumulation therefore visits each group as 0,4,1,5,2,6,3,7 -- the
// canonical chain order of the arithmetic contract (oracle/medtok_oracle.c) -- with no data
// permutation anywhere.  Rows are padded to 36 floats: conflict-free ds_read_b128 (16 lanes x
// stride 36 dwords hit 16 distinct 4-bank slots) and ds_write_b128.
constexpr int S_BM = 128, S_BN = 128;
constexpr int S_BK = 32;                                  // 2 blocks/CU (74 KB LDS); 16 with 3 blocks/CU measured the same
constexpr int S_LD = S_BK + 4;                            // row stride in floats (36 and 20 are both conflict-free)
constexpr int S_TILE = S_BM * S_LD;                       // floats per staged operand tile
constexpr size_t S_LDS_BYTES = (size_t)4 * S_TILE * sizeof(float);   // A[2] + B[2]
constexpr int S_TPR = S_BK / 8;                           // staging threads per tile row (8 floats each)
constexpr int S_RPP = 256 / S_TPR;                        // tile rows staged per pass
constexpr int S_PASSES = S_BM / S_RPP;
constexpr int S_WPS = S_BK == 32 ? 2 : 3;                 // waves per SIMD the register budget is sized for

// INDIRECT: the block's rows are row_list[row0 .. row0+128) (count read from *row_count on the
// device) -- the exact fallback for rows the fp16 filter could not shortlist.
// (the body is a force-inlined function of the block's coordinates: search_f32_kernel takes them from blockIdx, the batched kernel
// of the small-batch forward -- several searches in one launch -- from its descriptor table)
// EXCL (the second pass of a search for more than 8 codes per row): codes at or below the row's (distance, index) pair
// (excl_d[row], excl_i[row]) -- the last entry of the first pass's list -- are skipped, so the pass returns the NEXT best codes in the
// same total order (distance, then index).
template <int TOPK, bool FINAL, bool KTAIL, bool INDIRECT, bool EXCL = false>
__device__ __forceinline__ void search_f32_body(
    const float *__restrict__ xhat, const float *__restrict__ xsq, const float *__restrict__ what,
    const float *__restrict__ wsq, long n, int k_codes, int d, int codes_per_split, int topk_out,
    float *__restrict__ pval, int *__restrict__ pidx, int64_t *__restrict__ out_idx,
    float *__restrict__ out_dist, const int *__restrict__ row_list, const int *__restrict__ row_count,
    int list_begin, int list_end, const unsigned block_x, const unsigned block_y,
    const float *__restrict__ excl_d = nullptr, const int64_t *__restrict__ excl_i = nullptr, int excl_stride = 0)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    // direct form: this launch covers rows from list_begin on; its partial-result buffers span list_end rows (0 = all n)
    long row0 = (long)block_x * S_BN + (INDIRECT ? 0 : list_begin);
    const long part_rows = INDIRECT ? (long)(list_end - list_begin) : (list_end > 0 ? (long)list_end : n);     // row extent of the partial-result buffers
    if (INDIRECT) {
        // this launch covers list positions [list_begin, min(*row_count, list_end)); uniform for the whole grid
        n = min((long)*row_count, (long)list_end);
        row0 += list_begin;
        if (row0 >= n) return;
    }
    auto actual_row = [&](long pos) -> long {
        const long c = min(pos, n - 1);
        return INDIRECT ? (long)row_list[c] : c;
    };
    const int split = (int)block_y;
    const int code_lo = split * codes_per_split;
    const int code_hi = min(k_codes, code_lo + codes_per_split);
    const int nct = (code_hi - code_lo + S_BM - 1) / S_BM;
    const int nkb = (d + S_BK - 1) / S_BK;
    const int nstage = nct * nkb;

    const int srow = tid / S_TPR, sg = tid % S_TPR;
    float4 ra[S_PASSES][2], rb[S_PASSES][2];
    int kvalid = 0;                 // bit0/bit1: which float4 of the staged k-group lies inside D
    int pct = 0, pkb = 0;           // (code tile, k block) of the next stage to prefetch

    // Loads are unconditional: branching around them makes hipcc drain vmcnt(0) per load.  KTAIL
    // (D % 32 != 0) clamps the addresses into the row and zeroes the out-of-range float4 when it
    // is written to LDS (zeros leave the fmaf chain untouched).
    auto gload = [&]() {
        const int kofs = pkb * S_BK + sg * 8;
        int k0 = kofs, k1 = kofs + 4;
        if (KTAIL) {
            kvalid = (kofs < d ? 1 : 0) | (kofs + 4 < d ? 2 : 0);
            k0 = min(k0, d - 4);
            k1 = min(k1, d - 4);
        }
#pragma unroll
        for (int j = 0; j < S_PASSES; ++j) {
            const int crow = min(code_lo + pct * S_BM + srow + S_RPP * j, k_codes - 1);
            const float *p = what + (long)crow * d;
            const long xr = actual_row(row0 + srow + S_RPP * j);
            const float *q = xhat + xr * d;
            ra[j][0] = ld4(p + k0);
            ra[j][1] = ld4(p + k1);
            rb[j][0] = ld4(q + k0);
            rb[j][1] = ld4(q + k1);
        }
        if (++pkb == nkb) { pkb = 0; ++pct; }
    };
    auto lstore = [&](int buf) {
        float *A = smem + buf * S_TILE;
        float *B = smem + 2 * S_TILE + buf * S_TILE;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < S_PASSES; ++j) {
            float *pa = A + (srow + S_RPP * j) * S_LD + sg * 8;
            float *pb = B + (srow + S_RPP * j) * S_LD + sg * 8;
            if (KTAIL) {
                st4(pa, (kvalid & 1) ? ra[j][0] : z);
                st4(pa + 4, (kvalid & 2) ? ra[j][1] : z);
                st4(pb, (kvalid & 1) ? rb[j][0] : z);
                st4(pb + 4, (kvalid & 2) ? rb[j][1] : z);
            } else {
                st4(pa, ra[j][0]);
                st4(pa + 4, ra[j][1]);
                st4(pb, rb[j][0]);
                st4(pb + 4, rb[j][1]);
            }
        }
    };

    float bv[TOPK];
    int bi[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) { bv[j] = INFINITY; bi[j] = 0; }

    const long mypos = row0 + wave * 32 + li;
    const long myrow = actual_row(mypos);
    const float xn = xsq[myrow];
    float ex_d = -INFINITY;
    int ex_i = -1;
    if (EXCL) { ex_d = excl_d[myrow * excl_stride]; ex_i = (int)excl_i[myrow * excl_stride]; }

    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    // ---- epilogue of one code tile: d = (|x|^2 + |e|^2) - 2 x.e for this lane's 64 codes, fold into the list
    auto tile_epilogue = [&](int ct) __attribute__((always_inline)) {
        // ---- epilogue: d = (|x|^2 + |e|^2) - 2 x.e for this lane's 64 codes, fold into the list
        const int cbase = code_lo + ct * S_BM;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            // |e|^2 of this lane's 16 codes of the tile: four consecutive codes per register group, so four 16-byte loads
            // (+2.3 % at K = 16384, k = 5); a group that straddles K or sits on an unaligned slice takes the scalar form
            // codes at or beyond the split's end get |e|^2 = +inf, i.e. d = +inf: never inserted, and no range test per value
            float en[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = cbase + 32 * m + 8 * g + 4 * lh;
                // (argmin, TOPK = 1: the 16 scalar loads measured 4 % faster than the vector form -- its epilogue is nothing else)
                if (TOPK > 1 && c0 + 3 < code_hi && ((reinterpret_cast<uintptr_t>(wsq + c0) & 15) == 0)) {
                    const float4 e4 = ld4(wsq + c0);
                    en[4 * g] = e4.x; en[4 * g + 1] = e4.y; en[4 * g + 2] = e4.z; en[4 * g + 3] = e4.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float e = wsq[min(c0 + j, k_codes - 1)];        // (unconditional load: a branch around it drains vmcnt)
                        en[4 * g + j] = c0 + j < code_hi ? e : INFINITY;
                    }
                }
            }
            // four codes per test: the smallest of their distances against the list's last entry, ONE wave-uniform branch; a
            // quad in which some lane has a better code is then folded in value by value, in code order as before
            // (ties -> lowest index).  (+0.6 % at k = 5; the argmin kernel keeps the per-value form: -0.5 % there.)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float dv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sum = xn + en[4 * g + j];
                    const float two = 2.0f * acc[m][4 * g + j];
                    dv[j] = sum - two;
                    acc[m][4 * g + j] = 0.f;
                    if (EXCL) {
                        const int c = cbase + 32 * m + j + 8 * g + 4 * lh;
                        if (dv[j] < ex_d || (dv[j] == ex_d && c <= ex_i)) dv[j] = INFINITY;
                    }
                }
                bool any = true;
                if (TOPK > 1) {
                    const float mn = vs_min(vs_min3(dv[0], dv[1], dv[2]), dv[3]);      // (NaN never wins a v_min: a NaN distance is never inserted)
                    any = __builtin_amdgcn_ballot_w64(mn < bv[TOPK - 1]) != 0;
                }
                if (any) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) topk_insert<TOPK>(bv, bi, dv[j], cbase + 32 * m + j + 8 * g + 4 * lh);
                }
            }
        }
    };

    if constexpr (!KTAIL && !INDIRECT) {
        // ---- operand staging by LDS-DMA (D % 32 == 0, rows addressed directly).  A stage = 32 floats of 128 code rows and 128 input rows, each row 128 B =
        // eight 16-byte chunks; wave w copies rows [32w, 32w+32) of both tiles, eight rows per global_load_lds_dwordx4 (lane l:
        // row l >> 3, chunk slot l & 7), straight from L2 into one of TWO 32 KB buffers -- no staging registers, no ds_write pass,
        // nothing to wait for before the MFMAs of a stage but the barrier.  The rows are unpadded (the DMA's LDS image is
        // lane-linear), so chunk c of row r is stored in slot c ^ ((r >> 1) & 7): the 16 lanes a ds_read_b128 services together
        // then hit 16 distinct 16-byte bank groups (rows of equal parity in such a group differ in bits 1..3 of r).  The swizzle is
        // applied to the per-lane SOURCE address.  Staging through registers + ds_write (the KTAIL form below, which needs it to
        // zero the columns past D) measured 130.8 TFLOP/s in the main loop against 152 with the staging removed; this form 143.7
        // (N = 600k, K = 16 384, D = 768; whole kernel 123.2 -> 137.4 TFLOP/s at k = 5, 126.8 -> 134.9 for the argmin at 100k x 8192).
        constexpr int ROWB = S_BK * 4, TILEB = S_BM * ROWB;            // 128 B per staged row, 16 KB per tile
        char *lds = reinterpret_cast<char *>(smem);                      // [2 buffers][A tile | B tile]
        const int d_r = lane >> 3, d_p = lane & 7;                       // row within the instruction, chunk slot
        // buffer-addressed DMA (SGPR descriptor + loop-invariant 32-bit lane offset + SGPR stage offset; hipcc drains
        // vmcnt(0) before every ds_read that follows a global_load_lds, but not after the raw-buffer form).  The descriptors
        // carry the valid byte range: rows past K or past n read as zeros instead of touching memory (such codes get
        // |e|^2 = +inf in the epilogue, such rows are never written back).
        // The code-side descriptor is rebuilt per stage for the stage's code tile (base = the tile's first row, range = its rows
        // inside K: a handful of SALU operations), so every offset stays far below 2^31 whatever K * D is.
        const float *abase_p = what + (long)code_lo * d, *bbase_p = xhat + row0 * d;
        const long rows_left = n - row0;
        const int b_bytes = (int)(rows_left < S_BN ? rows_left : S_BN) * d * 4;
        const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void *)bbase_p, 0, b_bytes, 0x00020000);
        unsigned lane_off[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = wave * 32 + 8 * i + d_r;
            lane_off[i] = (unsigned)(r * d + 4 * (d_p ^ ((r >> 1) & 7))) * 4u;
        }
        const int wave_s = __builtin_amdgcn_readfirstlane(wave);
        int pct = 0, pkb = 0;
        // One stage = eight DMA instructions per wave.  Issued as a burst they hold the wave (and, through the CU's one address
        // path, its neighbours) at the head of the stage; instead the descriptor is prepared once per stage and the eight pieces
        // go out one per group of four MFMAs of the stage's first two k steps.  Past the last stage the same stage is issued
        // again into the buffer nobody reads (same bytes, harmless): no branch around a DMA.
        __amdgpu_buffer_rsrc_t ars = brs;
        int ub = 0;
        char *abase = lds, *bbase = lds;
        auto dma_prepare = [&](int buf) __attribute__((always_inline)) {
            abase = lds + buf * 2 * TILEB + (wave_s * 32) * ROWB; bbase = abase + TILEB;
            ub = __builtin_amdgcn_readfirstlane(pkb * S_BK * 4);
            const int tile_codes = __builtin_amdgcn_readfirstlane(min(S_BM, k_codes - code_lo - pct * S_BM));
            ars = __builtin_amdgcn_make_buffer_rsrc((void *)(abase_p + (long)__builtin_amdgcn_readfirstlane(pct) * S_BM * d), 0, tile_codes * d * 4, 0x00020000);
            const bool wrap = pkb + 1 == nkb, more = !(wrap && pct + 1 == nct);
            pkb = more ? (wrap ? 0 : pkb + 1) : pkb;
            pct += (more && wrap) ? 1 : 0;
        };
        auto dma_piece = [&](int i) __attribute__((always_inline)) {          // i = 0..7: A rows 8 (i/2) .. of the wave's 32, then B rows
            if (i & 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(brs, (__attribute__((address_space(3))) void *)(bbase + 8 * (i >> 1) * ROWB), 16, (int)lane_off[i >> 1], ub, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(ars, (__attribute__((address_space(3))) void *)(abase + 8 * (i >> 1) * ROWB), 16, (int)lane_off[i >> 1], ub, 0, 0);
        };
        // fragment addresses: lane (li, lh) reads chunk 2 kk + lh of row li (+ 32 m) -- slot (2 kk + lh) ^ ((li >> 1) & 7).
        // The fragment reads are asm: hipcc orders a C++ ds_read behind ALL pending LDS-DMA ("s_waitcnt vmcnt(0)": a DMA is a pending
        // LDS write that might alias), i.e. it drained the stage just issued -- a round trip to the L2 per stage in front of the
        // MFMAs.  The reads of step kk + 1 are issued before the MFMAs of step kk (two register sets); lgkmcnt is waited by hand.
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const unsigned lds0 = (unsigned)(size_t)lds;
        unsigned fragA[S_BK / 8], fragB[S_BK / 8];
#pragma unroll
        for (int kk = 0; kk < S_BK / 8; ++kk) {
            fragA[kk] = lds0 + li * ROWB + ((2 * kk + lh) ^ ((li >> 1) & 7)) * 16;
            fragB[kk] = fragA[kk] + TILEB + wave * 32 * ROWB;
        }
        f32x4 af[2][4], bf[2];
        auto frag_read = [&](int set, int kk, unsigned bufofs) __attribute__((always_inline)) {
            asm volatile("ds_read_b128 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %6 offset:4096\n\t"
                         "ds_read_b128 %3, %6 offset:8192\n\tds_read_b128 %4, %6 offset:12288"
                         : "=&v"(bf[set]), "=&v"(af[set][0]), "=&v"(af[set][1]), "=&v"(af[set][2]), "=&v"(af[set][3])
                         : "v"(fragB[kk] + bufofs), "v"(fragA[kk] + bufofs));
        };
        auto frag_wait = [&](int set) __attribute__((always_inline)) {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bf[set]), "+v"(af[set][0]), "+v"(af[set][1]), "+v"(af[set][2]), "+v"(af[set][3]));
        };
        static_assert(32 * ROWB == 4096, "fragment offsets above are written for 128-byte staged rows");
        dma_prepare(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) dma_piece(i);
        int ct = 0, kb = 0;
        for (int s = 0; s < nstage; ++s) {
            const unsigned bufofs = (unsigned)(s & 1) * (2 * TILEB);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // own part of stage s has landed
            __builtin_amdgcn_s_barrier();                               // everyone's has; everyone is done with the other buffer
            asm volatile("" ::: "memory");
            frag_read(0, 0, bufofs);
            dma_prepare((s & 1) ^ 1);
            frag_wait(0);
#pragma unroll
            for (int kk = 0; kk < S_BK / 8; ++kk) {
                const int cur = kk & 1;
                if (kk + 1 < S_BK / 8) frag_read(cur ^ 1, kk + 1, bufofs);
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][m].x, bf[cur].x, acc[m], 0, 0, 0);
                if (kk < 2) { dma_piece(4 * kk); asm volatile("" ::: "memory"); }
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][m].y, bf[cur].y, acc[m], 0, 0, 0);
                if (kk < 2) { dma_piece(4 * kk + 1); asm volatile("" ::: "memory"); }
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][m].z, bf[cur].z, acc[m], 0, 0, 0);
                if (kk < 2) { dma_piece(4 * kk + 2); asm volatile("" ::: "memory"); }
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][m].w, bf[cur].w, acc[m], 0, 0, 0);
                if (kk < 2) { dma_piece(4 * kk + 3); asm volatile("" ::: "memory"); }
                if (kk < 2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
                }
                if (kk + 1 < S_BK / 8) frag_wait(cur ^ 1);
            }
            if (++kb == nkb) {
                tile_epilogue(ct);
                kb = 0;
                ++ct;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
    gload();
    int ct = 0, kb = 0;
    for (int s = 0; s < nstage; ++s) {
        const int buf = s & 1;
        lstore(buf);
        __syncthreads();
        if (s + 1 < nstage) gload();
        const float *A = smem + buf * S_TILE + li * S_LD + lh * 4;
        const float *B = smem + 2 * S_TILE + buf * S_TILE + (wave * 32 + li) * S_LD + lh * 4;
#pragma unroll
        for (int kk = 0; kk < S_BK / 8; ++kk) {
            const float4 bf = ld4(B + kk * 8);
            float4 af[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) af[m] = ld4(A + m * 32 * S_LD + kk * 8);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].x, bf.x, acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].y, bf.y, acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].z, bf.z, acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].w, bf.w, acc[m], 0, 0, 0);
        }
        if (++kb == nkb) {
            tile_epilogue(ct);
            kb = 0;
            ++ct;
        }
    }
    }

    // ---- join the two half-waves that share an input row (disjoint code sets)
    float pv[TOPK];
    int pi[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) { pv[j] = __shfl_xor(bv[j], 32, 64); pi[j] = __shfl_xor(bi[j], 32, 64); }
#pragma unroll
    for (int j = 0; j < TOPK; ++j) topk_insert_lex<TOPK>(bv, bi, pv[j], pi[j]);

    if (lh == 0 && mypos < n) {
        if (FINAL) {
#pragma unroll
            for (int j = 0; j < TOPK; ++j)
                if (j < topk_out) { out_idx[myrow * topk_out + j] = bi[j]; out_dist[myrow * topk_out + j] = bv[j]; }
        } else {
            const long base = ((long)split * part_rows + (INDIRECT ? mypos - list_begin : myrow - list_begin)) * TOPK;
#pragma unroll
            for (int j = 0; j < TOPK; ++j) { pval[base + j] = bv[j]; pidx[base + j] = bi[j]; }
        }
    }
}

template <int TOPK, bool FINAL, bool KTAIL, bool INDIRECT>
__global__ __launch_bounds__(256, S_WPS) void search_f32_kernel(
    const float *__restrict__ xhat, const float *__restrict__ xsq, const float *__restrict__ what,
    const float *__restrict__ wsq, long n, int k_codes, int d, int codes_per_split, int topk_out,
    float *__restrict__ pval, int *__restrict__ pidx, int64_t *__restrict__ out_idx,
    float *__restrict__ out_dist, const int *__restrict__ row_list, const int *__restrict__ row_count,
    int list_begin, int list_end)
{
    search_f32_body<TOPK, FINAL, KTAIL, INDIRECT>(xhat, xsq, what, wsq, n, k_codes, d, codes_per_split, topk_out, pval, pidx, out_idx, out_dist,
                                                  row_list, row_count, list_begin, list_end, blockIdx.x, blockIdx.y);
}

template <int TOPK, bool FINAL, bool KTAIL>
__global__ __launch_bounds__(256, S_WPS) void search_f32_excl_kernel(
    const float *__restrict__ xhat, const float *__restrict__ xsq, const float *__restrict__ what,
    const float *__restrict__ wsq, long n, int k_codes, int d, int codes_per_split, int topk_out,
    float *__restrict__ pval, int *__restrict__ pidx, int64_t *__restrict__ out_idx,
    float *__restrict__ out_dist, int list_begin, int list_end,
    const float *__restrict__ excl_d, const int64_t *__restrict__ excl_i, int excl_stride)
{
    search_f32_body<TOPK, FINAL, KTAIL, false, true>(xhat, xsq, what, wsq, n, k_codes, d, codes_per_split, topk_out, pval, pidx, out_idx, out_dist,
                                                     (const int *)nullptr, (const int *)nullptr, list_begin, list_end, blockIdx.x, blockIdx.y,
                                                     excl_d, excl_i, excl_stride);
}

// ---- several small searches in ONE launch each of three kernels (the B = 256 forward of the reference's default configuration runs
// its specific and shared searches as four calls of four launches each: 16 launches of 4-30 us for 2 GFLOP; batched: 3 launches).
// Same kernels' bodies, same arithmetic, same bits; a descriptor per search, selected by blockIdx.z.
constexpr int MS_MAX = MEDTOK_MULTI_SEARCH_MAX;   // shared (merged) + text + graph + the two aug views
struct MultiSearchOne {
    const float *x;                             // [n, d] rows to quantise
    const float *what, *wsq;                    // the normalised codebook region [k_codes, d] and its squared norms
    float *xhat, *xsq;                          // out: F.normalize(x) [n, d], its squared norms [n] (scratch)
    float *pval; int *pidx;                     // scratch: per-split lists [splits][n][TOPK]
    int64_t *idx; float *dist, *w, *zq;         // out: [n, topk] ids / distances / weights; [n, d] rows with a row stride
    float *row_sqerr;                           // out (may be NULL): [n] squared error of the soft assignment per row (training losses)
    long n, zq_stride, x_stride;                // (x rows may be a column block of a wider matrix)
    int k_codes, codes_per_split, splits, row_tiles;
};
// block_base: the searches' (row tile, code split) blocks in ONE dimension, search after search (block_base[i] = first block of
// search i, block_base[count] = all).  The search kernel's grid holds exactly the blocks that have work: a 3-D grid of
// max_tiles x max_splits x count launched 996 blocks for the 444 of a B = 256 forward, and -- blocks going to the 8 XCDs by id --
// the active ones of the two short searches all landed on XCDs 0, 1, 4, 5: 70 blocks for 64 slots there, a second generation of a few
// blocks, twice the kernel time (round 6: rocprofv3 counters, profiles/r06_pmc_small_search_*.txt).
struct MultiSearchArgs { MultiSearchOne s[MS_MAX]; int block_base[MS_MAX + 1]; int count, d, topk; };

__global__ __launch_bounds__(256) void rownorm_multi_kernel(MultiSearchArgs a)
{
    const MultiSearchOne &m = a.s[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m.n) return;
    const int d = a.d;
    const float *src = m.x + row * m.x_stride;
    float *dst = m.xhat + row * d;
    // (rownorm_kernel<true>, statement for statement: the same bits)
    float p = 0.f;
    for (int i = lane * 4; i < d; i += 256) {
        float4 v = ld4(src + i);
        p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
    }
    const float nrm = sqrtf(wave_butterfly_sum(p));
    const float den = fmaxf(nrm, 1e-12f);
    p = 0.f;
    for (int i = lane * 4; i < d; i += 256) {
        float4 v = ld4(src + i);
        v.x = v.x / den; v.y = v.y / den; v.z = v.z / den; v.w = v.w / den;
        st4(dst + i, v);
        p = fmaf(v.x, v.x, p); p = fmaf(v.y, v.y, p); p = fmaf(v.z, v.z, p); p = fmaf(v.w, v.w, p);
    }
    p = wave_butterfly_sum(p);
    if (lane == 0) m.xsq[row] = p;
}

template <int TOPK, bool KTAIL>
__global__ __launch_bounds__(256, S_WPS) void search_f32_multi_kernel(MultiSearchArgs a)
{
    int z = 0;
#pragma unroll
    for (int i = 1; i < MS_MAX; ++i) z += (i < a.count && (int)blockIdx.x >= a.block_base[i]) ? 1 : 0;
    const MultiSearchOne &m = a.s[z];
    const unsigned local = blockIdx.x - (unsigned)a.block_base[z];
    const unsigned bx = local % (unsigned)m.row_tiles, by = local / (unsigned)m.row_tiles;
    search_f32_body<TOPK, false, KTAIL, false>(m.xhat, m.xsq, m.what, m.wsq, m.n, m.k_codes, a.d, m.codes_per_split, a.topk, m.pval, m.pidx,
                                               (int64_t *)nullptr, (float *)nullptr, (const int *)nullptr, (const int *)nullptr, 0, 0,
                                               bx, by);
}

// Joins the per-split candidate lists of one row: 8 lanes per row, each folds every 8th split, then three shuffle rounds.
// (d, index) is a total order, so the result does not depend on who inserts what when.  (A thread per row walked
// up to 64 splits x k entries serially: 90 us for a 256-row batch.)
// LPR lanes per row: 8, or a whole wave (64) for small batches with many splits (256 rows x 128 splits: 28 -> ~12 us).
template <int TOPK, int LPR = 8>
__global__ __launch_bounds__(256) void merge_topk_kernel(const float *__restrict__ pval, const int *__restrict__ pidx,
                                                         long n, int splits, int topk_out,
                                                         int64_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                         const int *__restrict__ row_list, const int *__restrict__ row_count, int k_codes)
{
    // with a row list: partial lists are indexed by list position (extent n), results go to row_list[position]
    constexpr int RPB = 256 / LPR;                       // rows per block
    const int l8 = threadIdx.x & (LPR - 1);
    const long pos = (long)blockIdx.x * RPB + (threadIdx.x / LPR);
    const long limit = row_list ? min(n, (long)*row_count) : n;
    if ((long)blockIdx.x * RPB >= limit) return;         // (block-uniform: the redo of the rows the filter gave up on normally has none)
    const long row = min(pos, n - 1);                    // lanes past the end keep shuffling with their group, write nothing
    float bv[TOPK];
    int bi[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) { bv[j] = INFINITY; bi[j] = 0x7fffffff; }
    for (int s = l8; s < splits; s += LPR) {
        const long base = ((long)s * n + row) * TOPK;
#pragma unroll
        for (int j = 0; j < TOPK; ++j) topk_insert_lex<TOPK>(bv, bi, pval[base + j], pidx[base + j]);
    }
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) {
        float pv[TOPK];
        int pi[TOPK];
#pragma unroll
        for (int j = 0; j < TOPK; ++j) { pv[j] = __shfl_xor(bv[j], off, LPR); pi[j] = __shfl_xor(bi[j], off, LPR); }
#pragma unroll
        for (int j = 0; j < TOPK; ++j) topk_insert_lex<TOPK>(bv, bi, pv[j], pi[j]);
    }
    if (l8 != 0 || pos >= limit) return;
    const long orow = row_list ? (long)row_list[pos] : row;
#pragma unroll
    for (int j = 0; j < TOPK; ++j)
        if (j < topk_out) { out_idx[orow * topk_out + j] = valid_code(bi[j], j, k_codes); out_dist[orow * topk_out + j] = bv[j]; }
}

// ================================================================= more than 8 codes per row: the join of the two passes' lists
// (medtok_vq.hip: search_wide)
constexpr int WIDE_T = 8;
__global__ __launch_bounds__(256) void join_lists_kernel(const int64_t *__restrict__ ia, const float *__restrict__ da, const int64_t *__restrict__ ib,
                                                         const float *__restrict__ db, long n, int kb, int64_t *__restrict__ idx, float *__restrict__ dist)
{
    const int k = WIDE_T + kb;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n * k; i += (long)gridDim.x * 256) {
        const long r = i / k;
        const int j = (int)(i - r * k);
        idx[i] = j < WIDE_T ? ia[r * WIDE_T + j] : ib[r * kb + (j - WIDE_T)];
        dist[i] = j < WIDE_T ? da[r * WIDE_T + j] : db[r * kb + (j - WIDE_T)];
    }
}

// ================================================================= merge of per-shard top-k lists
// Code-sharded search (SURVEY 8e variant): every shard returns, for the same rows, its own top-k over its slice of
// the codebook (global code ids); the exact top-k over the union is the (d, index)-lexicographic merge.
__global__ __launch_bounds__(256) void merge_lists_kernel(const float *__restrict__ dist_parts, const int64_t *__restrict__ idx_parts,
                                                          long n, int parts, int topk, int64_t *__restrict__ out_idx,
                                                          float *__restrict__ out_dist)
{
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    float bv[MEDTOK_MAX_TOPK];
    long bi[MEDTOK_MAX_TOPK];
#pragma unroll
    for (int j = 0; j < MEDTOK_MAX_TOPK; ++j) { bv[j] = INFINITY; bi[j] = 0x7fffffffffffffffl; }
    for (int p = 0; p < parts; ++p)
        for (int j = 0; j < topk; ++j) {
            const float v = dist_parts[((long)p * n + row) * topk + j];
            const long c = idx_parts[((long)p * n + row) * topk + j];
            // insertion by (value, index); the lists are short (parts * topk entries)
#pragma unroll
            for (int q = MEDTOK_MAX_TOPK - 1; q >= 0; --q) {
                const bool before = v < bv[q] || (v == bv[q] && c < bi[q]);
                if (before) {
                    if (q + 1 < MEDTOK_MAX_TOPK) { bv[q + 1] = bv[q]; bi[q + 1] = bi[q]; }
                    bv[q] = v; bi[q] = c;
                }
            }
        }
#pragma unroll
    for (int j = 0; j < MEDTOK_MAX_TOPK; ++j)
        if (j < topk) { out_idx[row * topk + j] = bi[j] == 0x7fffffffffffffffl ? (long)j : bi[j]; out_dist[row * topk + j] = bv[j]; }   // NaN rows: in range
}

// ================================================================= several small searches, batched (kernels next to search_f32_kernel)
// Joins the per-split lists of a row (merge_topk_kernel<T, 64>: a wavefront per row, (d, index) total order) and does the row's soft
// assignment at once (soft_assign_kernel's arithmetic on the values it would have read back: the same bits).
template <int TOPK>
__global__ __launch_bounds__(256) void merge_assign_multi_kernel(MultiSearchArgs a)
{
    const MultiSearchOne &m = a.s[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m.n) return;
    const int d = a.d, topk = a.topk;
    float bv[TOPK];
    int bi[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) { bv[j] = INFINITY; bi[j] = 0x7fffffff; }
    for (int sp = lane; sp < m.splits; sp += 64) {
        const long base = ((long)sp * m.n + row) * TOPK;
#pragma unroll
        for (int j = 0; j < TOPK; ++j) topk_insert_lex<TOPK>(bv, bi, m.pval[base + j], m.pidx[base + j]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        float pv[TOPK];
        int pi[TOPK];
#pragma unroll
        for (int j = 0; j < TOPK; ++j) { pv[j] = __shfl_xor(bv[j], off, 64); pi[j] = __shfl_xor(bi[j], off, 64); }
#pragma unroll
        for (int j = 0; j < TOPK; ++j) topk_insert_lex<TOPK>(bv, bi, pv[j], pi[j]);
    }
    long cj[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) cj[j] = valid_code(bi[j], j, m.k_codes);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < TOPK; ++j)
            if (j < topk) { m.idx[row * topk + j] = cj[j]; m.dist[row * topk + j] = bv[j]; }
    }
    float wj[TOPK];
    const float mx = -bv[0];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < TOPK; ++j)
        if (j < topk) { wj[j] = expf(-bv[j] - mx); sum += wj[j]; }
#pragma unroll
    for (int j = 0; j < TOPK; ++j)
        if (j < topk) wj[j] = wj[j] / sum;
    if (m.w && lane < topk) {
        float v = wj[0];
#pragma unroll
        for (int j = 1; j < TOPK; ++j) v = (lane == j) ? wj[j] : v;
        m.w[row * topk + lane] = v;
    }
    const float *xr = m.x + row * m.x_stride;
    float *out = m.zq + row * m.zq_stride;
    float se = 0.f;
    for (int i = lane * 4; i < d; i += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < TOPK; ++j)
            if (j < topk) {
                const float4 e = ld4(m.what + cj[j] * d + i);
                acc.x = fmaf(wj[j], e.x, acc.x); acc.y = fmaf(wj[j], e.y, acc.y);
                acc.z = fmaf(wj[j], e.z, acc.z); acc.w = fmaf(wj[j], e.w, acc.w);
            }
        const float4 x = ld4(xr + i);
        float4 df;
        df.x = acc.x - x.x; df.y = acc.y - x.y; df.z = acc.z - x.z; df.w = acc.w - x.w;
        st4(out + i, make_float4(x.x + df.x, x.y + df.y, x.z + df.z, x.w + df.w));
        se = fmaf(df.x, df.x, se); se = fmaf(df.y, df.y, se); se = fmaf(df.z, df.z, se); se = fmaf(df.w, df.w, se);
    }
    if (m.row_sqerr) {                              // (soft_assign_kernel's sum: 64 strided fmaf chains joined by the xor butterfly)
        se = wave_butterfly_sum(se);
        if (lane == 0) m.row_sqerr[row] = se;
    }
}
