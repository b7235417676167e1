// medtok_vq.hip -- gfx950 (MI355X / CDNA4): the C ABI of the MedTok VQ hot path and the host side of its kernels.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared
// (see medtok_amd/csrc/build.py).  Wave size is 64 everywhere; no other target.
//
// This file: error and profiler plumbing, launch plans and workspace layouts, launches, and the extern "C" entry points
// (reference call sites in include/medtok_vq.h).  The kernels live in the headers next to it, one per family:
//   search_f32.h          row norms, top-k list helpers, exact fp32-MFMA search, merges of partial lists, k > 8 join
//   filter_f16.h          fp16-MFMA shortlist filter (three kernels), operand images, exact re-score
//   assign_kernels.h      soft assignment, fixed-order fp64 sum
//   decode_kernels.h      (token ids, weights) -> embedding, and its backward
//   embed_kernels.h       code indices -> stored tokens -> embedding; the folded lookup, also as the consumer's input sequence; the pool
//   embed_sequence_kernels.h  the input sequence over dense rows, and the additive rows' gradients
//   embed_grad_kernels.h  the codebook's and the folded tables' gradient through the lookup: sort keys, chunked per-row sums
//   embed_pool_segments_kernels.h  the pool with a bag per (batch row, segment): the keys of the positions' lists
//   train_kernels.h       sparse backward, normalize backward, InfoNCE
//   loss_kernels.h        alignment / orthogonality losses
//   attention_*.h         ragged cross-attention cores (fp32, fp16 x 3, LDS-DMA, two-tile, e_dim = 64) and their backward
//   pack_kernels.h        the prologue of CrossAttention.pooled
//   split_gemm.h          split-fp16 and one-pass half-precision dense products, operand images
//   ema_kernels.h         EMA statistics (histogram, radix sort, segmented sum), EMA apply, usage window
//
// Arithmetic order is the one oracle/medtok_oracle.c documents; tests compare bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/medtok_vq.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- error plumbing
static thread_local char g_err[512] = "";

static int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}

static int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: %s", what, hipGetErrorString(e));
    return 0;
}

extern "C" int medtok_abi_version(void) { return MEDTOK_VQ_ABI_VERSION; }
extern "C" const char *medtok_last_error(void) { return g_err; }

// ---------------------------------------------------------------- optional self-profiling (bench.py)
// Between medtok_profile_begin() and medtok_profile_end() every launch of a search kernel is
// bracketed by HIP events recorded on its own launch stream; nothing synchronises until _end().
struct ProfRec { hipEvent_t a, b; double flops; int kind; };   // kind 0 = filter_f16_kernel, 1 = search_f32_kernel, 2 = attention forward (any kernel), 3 = attention backward (dQ + dKV), 4 = split_gemm_kernel
// Process-wide (the backward kernels are launched from autograd's own thread): a flag read on every launch, the records and the
// event pool behind one mutex that is only ever taken while profiling is on.
static std::atomic<bool> g_prof_on{false};
static std::atomic<unsigned> g_prof_kinds{~0u};      // bit k: launches of kind k are bracketed (medtok_profile_begin_kinds)
static inline bool prof_wanted(int kind) { return g_prof_on && ((g_prof_kinds >> kind) & 1u); }
static std::mutex g_prof_mu;
static std::vector<ProfRec> g_prof;

// Events come from a pool that medtok_profile_begin() fills BEFORE the timed region: recording is all a launch pays.
static std::vector<hipEvent_t> g_event_pool;
constexpr size_t PROF_POOL = 4096;

static hipEvent_t prof_mark(hipStream_t s)
{
    hipEvent_t e = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (!g_event_pool.empty()) { e = g_event_pool.back(); g_event_pool.pop_back(); }
    }
    if (!e && hipEventCreate(&e) != hipSuccess) return nullptr;
    (void)hipEventRecord(e, s);
    return e;
}
static void prof_push(hipEvent_t a, hipEvent_t b, double flops, int kind)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back({a, b, flops, kind});
}

static int profile_begin_impl(unsigned kinds)
{
    g_prof_kinds = kinds;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &r : g_prof) { if (r.a) g_event_pool.push_back(r.a); if (r.b) g_event_pool.push_back(r.b); }
    g_prof.clear();
    while (g_event_pool.size() < PROF_POOL) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return fail("profile_begin: hipEventCreate failed");
        g_event_pool.push_back(e);
    }
    g_prof_on = true;
    return 0;
}
extern "C" int medtok_profile_begin(void) { return profile_begin_impl(~0u); }
// ... bracketing only the launches of the kinds in `kinds` (bit k = kind k of medtok_profile_end's arrays): a training step is ~180
// library launches, and two event records per launch are 0.5 ms of an 11 ms step -- the timed region then carries the events of
// its dominant kernel only (bench.py), the other kinds come from a pass behind it
extern "C" int medtok_profile_begin_kinds(unsigned kinds) { return profile_begin_impl(kinds); }

extern "C" int medtok_profile_end(double *ms, double *flops, int *launches)
{
    g_prof_on = false;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int k = 0; k < MEDTOK_PROFILE_KINDS; ++k) { ms[k] = 0.0; flops[k] = 0.0; launches[k] = 0; }
    for (auto &r : g_prof) {
        float t = 0.f;
        if (r.a && r.b && hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            ms[r.kind] += t; flops[r.kind] += r.flops; launches[r.kind] += 1;
        }
        if (r.a) g_event_pool.push_back(r.a);
        if (r.b) g_event_pool.push_back(r.b);
    }
    g_prof.clear();
    return 0;
}

// ---------------------------------------------------------------- shader-clock probe (bench.py)
// The chip clocks to its power budget: a fp16-MFMA-bound kernel sags to ~1.7 of 2.4 GHz, and how far differs from box to box by a few
// per cent -- as much as a round's kernel work moves the headline.  One idle wavefront per XCD (blocks 0..7 go round-robin to the 8
// XCDs) reads the shader-cycle counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) when it starts and when the host
// raises `stop` (a word of pinned host memory, polled every ~20 us between s_sleeps; `max_ticks` of the 100 MHz counter bound the
// wait whatever happens to the flag), so that a bench line can state the clock its timed region ran at.  Launch it on a stream of its
// own, NOT one the measured work uses (streams that share a hardware queue serialise).  out: uint64 [8][4] = shader cycles, 100 MHz
// ticks, XCC id, polls.
__global__ __launch_bounds__(64) void clock_probe_kernel(const int *stop, unsigned long long max_ticks, unsigned long long *__restrict__ out)
{
    if (threadIdx.x != 0) return;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long polls = 0, c1 = c0, r1 = r0;
    for (;;) {
        for (int i = 0; i < 16; ++i) __builtin_amdgcn_s_sleep(127);
        c1 = __builtin_amdgcn_s_memtime();
        r1 = __builtin_amdgcn_s_memrealtime();
        ++polls;
        if (__hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0 || r1 - r0 >= max_ticks) break;
    }
    unsigned long long *o = out + (size_t)blockIdx.x * 4;
    o[0] = c1 - c0; o[1] = r1 - r0;
    o[2] = (unsigned long long)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 0xf);       // HW_REG_XCC_ID[3:0]
    o[3] = polls;
}

extern "C" int medtok_debug_clock_probe(const int *stop_flag, uint64_t max_ticks_100mhz, uint64_t *out, void *stream)
{
    if (!stop_flag || !out) return fail("clock_probe: NULL argument");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(8), dim3(64), 0, (hipStream_t)stream, stop_flag, (unsigned long long)max_ticks_100mhz,
                       (unsigned long long *)out);
    return check_launch("clock_probe");
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the kernel, not of the launch: set it once per instantiation
// (and device), not before every launch.
template <auto Kernel>
static bool set_lds_once(size_t bytes)
{
    static thread_local int done_dev = -1;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (done_dev == dev) return true;
    if (hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    done_dev = dev;
    return true;
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline long lmin(long a, long b) { return a < b ? a : b; }
static inline long lmax(long a, long b) { return a > b ? a : b; }

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ float wave_butterfly_sum(float p)
{
    // xor butterfly, offsets 32..1: every lane ends with the same bits (a+b == b+a).
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    return p;
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void st1(float *p, float v) { *p = v; }

// The same four columns in a 16-bit type.  A load widens in registers, which is exact; a store rounds each fp32 element once, to nearest even.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const _Float16 *p)
{
    const f16x4 h = *reinterpret_cast<const f16x4 *>(p);
    return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
__device__ __forceinline__ float4 ld4(const __bf16 *p)
{
    const uint2 u = *reinterpret_cast<const uint2 *>(p);          // bf16 is the upper half of the fp32 with the same value
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ void st4(_Float16 *p, float4 v)
{
    f16x4 h;
    h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
    *reinterpret_cast<f16x4 *>(p) = h;
}
__device__ __forceinline__ void st4(__bf16 *p, float4 v)
{
    bf16x4 h;
    h[0] = (__bf16)v.x; h[1] = (__bf16)v.y; h[2] = (__bf16)v.z; h[3] = (__bf16)v.w;
    *reinterpret_cast<bf16x4 *>(p) = h;
}
__device__ __forceinline__ void st1(_Float16 *p, float v) { *p = (_Float16)v; }
__device__ __forceinline__ void st1(__bf16 *p, float v) { *p = (__bf16)v; }

// ================================================================= row norms and the exact fp32 search (kernels: search_f32.h)
#include "search_f32.h"

// the launch every caller of the row-norm kernels goes through: the 16-lanes-per-row form where a row fits it
template <bool NORMALIZE>
static inline void launch_rownorm(hipStream_t s, const float *x, long n, int d, float *xhat, float *sqn, _Float16 *xh = nullptr, int dp = 0,
                                  long n_img = 0, int *zero_word = nullptr)
{
    const long rows = xh && n_img > n ? n_img : n;
    if (d <= 64 && (!xh || dp <= 64))
        hipLaunchKernelGGL(rownorm16_kernel<NORMALIZE>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, s, x, n, d, xhat, sqn, xh, dp, n_img, zero_word);
    else
        hipLaunchKernelGGL(rownorm_kernel<NORMALIZE>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, n, d, xhat, sqn, xh, dp, n_img, zero_word);
}

extern "C" int medtok_rownorm_f32(const float *x, int64_t n, int d, int normalize, float *xhat,
                                  float *sqn, void *stream)
{
    if (n < 0 || d <= 0 || (d & 3)) return fail("rownorm: need n >= 0, d > 0, d %% 4 == 0 (n=%ld d=%d)", (long)n, d);
    if (n == 0) return 0;                      // (an empty torch tensor has a null data pointer: sizes first, pointers after)
    if (normalize && !xhat) return fail("rownorm: xhat required when normalize != 0");
    hipStream_t s = (hipStream_t)stream;
    if (normalize) launch_rownorm<true>(s, x, (long)n, d, xhat, sqn);
    else launch_rownorm<false>(s, x, (long)n, d, xhat, sqn);
    return check_launch("rownorm");
}

#include "filter_f16.h"

// Test hook: plan branches that the default heuristics only take at very large shapes can be forced PER CALL through the upper
// bits of the `path` argument (MEDTOK_PLAN_* in medtok_vq.h), so small parity tests cover them.  No process state: the
// workspace query and the launch decode the same argument.  The product path never reads the environment.
struct PlanOverride { long filter_splits = -1, filter_xcd = -1, filter_tail_min_blocks = -1, search_max_splits = -1, filter_rows64 = -1; };
static PlanOverride decode_plan(int path)
{
    PlanOverride o;
    const int fs = (path >> 8) & 0xFF, xcd = (path >> 16) & 3, tail = (path >> 18) & 3, ss = (path >> 20) & 0xFF;
    if (fs) o.filter_splits = fs;
    if (xcd) o.filter_xcd = xcd - 1;
    if (tail) o.filter_tail_min_blocks = tail == 1 ? 0 : 256;
    if (ss) o.search_max_splits = ss;
    const int r64 = (path >> 28) & 3;          // 1 = off, 2 = on (the default at D <= 64), 3 = on, the earlier 128 x 64 wave-tile kernel
    if (r64) o.filter_rows64 = r64 - 1;
    return o;
}
static inline int path_id(int path) { return path & MEDTOK_PATH_MASK; }

// Device geometry the launch plans are sized for, queried once per device (hipDeviceGetAttribute); without a device (a
// workspace query on a CPU-only box) the full MI355X is assumed.  `full` = the unpartitioned chip (256 CUs in 8 XCDs of 32):
// the XCD-aware block order is only used there; on a partitioned device (CPX / a CU mask) the round arithmetic follows the
// CU count that is actually visible.
struct DevInfo { int cus; bool full; };
static DevInfo dev_info()
{
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return {256, true}; }
    int cus = cached[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
        cached[dev].store(cus, std::memory_order_relaxed);
    }
    return {cus, cus == 256};
}

// list length the search kernels are instantiated with for a request of topk <= 8 codes per row
static inline int list_slots(int topk) { return topk == 1 ? 1 : (topk <= 5 ? 5 : 8); }

// (list length, ragged depth) -> compile-time constants: fn(std::integral_constant<int, T>, std::bool_constant<KTAIL>), T = 1, 5
// or 8, KTAIL = D % 32 != 0.  Every launch of a kernel that is instantiated per list length goes through here.
template <typename F>
static int dispatch_lists(int tslots, bool ragged, F &&fn)
{
    auto by_depth = [&](auto t) { return ragged ? fn(t, std::true_type{}) : fn(t, std::false_type{}); };
    switch (tslots) {
    case 1: return by_depth(std::integral_constant<int, 1>{});
    case 5: return by_depth(std::integral_constant<int, 5>{});
    default: return by_depth(std::integral_constant<int, 8>{});
    }
}

struct SearchPlan {
    int tslots;          // list length the kernels are instantiated with (1, 5 or 8)
    int splits;          // code-range splits (grid.y)
    int codes_per_split; // multiple of 128
    long row_tiles;
    // large searches: the first main_tiles row tiles (whole rounds of 512 resident blocks) walk ALL codes in one block; the
    // row tiles of the last, partly filled round form a second launch with tail_splits code splits (0 = no tail launch)
    long main_tiles;
    int tail_splits, tail_codes_per_split;
};

static SearchPlan plan_search(int64_t n, int64_t k_codes, int topk, const PlanOverride &ov)
{
    SearchPlan p;
    const DevInfo di = dev_info();
    p.tslots = list_slots(topk);
    p.row_tiles = (n + S_BN - 1) / S_BN;
    const long code_tiles = (k_codes + S_BM - 1) / S_BM;
    // Blocks all cost the same and run 2-3 per CU, so a launch of B blocks wastes up to one "round" of ~2.3 blocks per CU
    // (600 on the full chip); ask for >= 64 blocks per CU (16384: tail <= ~4%) by splitting the code range.
    long want = (64L * di.cus + p.row_tiles - 1) / p.row_tiles;
    if (want < 1) want = 1;
    if (want > code_tiles) want = code_tiles;
    // at most 64 splits -- except for one or two row tiles (batches of <= 256 rows), where 64 splits would leave half
    // the CUs without a block: n = 256, K = 49152: 463 -> 276 us with 128 splits; n = 64: 459 -> 202 us with 256
    // (three to seven row tiles -- 257 .. 896 rows: 128 splits, i.e. 384 .. 896 blocks of short code ranges, keep two blocks on every CU;
    // with 64 a 512-row search left half the CUs one block: 0.376 -> 0.322 ms at K = 49152, D = 768, 0.063 -> 0.055 at the reference's
    // shape -- tools/r06/exact_splits_small.py, profiles/r06_exact_splits_small.txt)
    long cap = p.row_tiles <= 2 ? lmin(256, di.cus) / p.row_tiles : (p.row_tiles <= 7 ? 128 : 64);
    if (ov.search_max_splits > 0) cap = ov.search_max_splits;
    if (want > cap) want = cap;
    const long tiles_per_split = (code_tiles + want - 1) / want;
    p.codes_per_split = (int)(tiles_per_split * S_BM);
    p.splits = (int)((code_tiles + tiles_per_split - 1) / tiles_per_split);
    p.main_tiles = p.row_tiles; p.tail_splits = 0; p.tail_codes_per_split = 0;
    // From two full rounds of blocks up (2 blocks per CU resident: 512 per round) the code range is NOT split: every split
    // restarts the lane-local top-k lists, and a young list sends the whole wave through the insertion code for most values
    // (measured at N = 600k, K = 16384: the epilogue is 10 % of the kernel with 4 splits).  What splitting bought -- a short
    // last round -- comes from a second launch instead: the row tiles of the partly filled last round, with enough splits to be
    // one round of short blocks.
    if (p.row_tiles >= 4L * di.cus && n < (1ll << 31) && ov.search_max_splits <= 0) {
        const long round = 2L * di.cus;      // two blocks per CU resident
        const long main_tiles = p.row_tiles / round * round, tail_tiles = p.row_tiles - main_tiles;
        p.splits = 1;
        p.codes_per_split = (int)(code_tiles * S_BM);
        long ts = tail_tiles > 0 ? lmin(lmin(64, code_tiles), round / tail_tiles) : 0;
        if (ts >= 2) {
            const long tps = (code_tiles + ts - 1) / ts;
            p.main_tiles = main_tiles;
            p.tail_codes_per_split = (int)(tps * S_BM);
            p.tail_splits = (int)((code_tiles + tps - 1) / tps);
        }
    }
    return p;
}

// The exact path's workspace: the partial lists [splits][rows][tslots] of the launch that splits the code range -- the whole search
// (rows = n), or the tail launch behind whole rounds of unsplit blocks (rows = those of the last round's row tiles).  A search whose
// blocks all walk every code writes its final lists and needs none: 256 bytes, so that a caller can always allocate what the query
// returns.  ws == nullptr: sizes only.
struct ExactWs { float *pval; int *pidx; long rows; size_t total; };
static ExactWs exact_ws_layout(void *ws, int64_t n, const SearchPlan &p)
{
    ExactWs w = {nullptr, nullptr, 0, 256};
    if (p.tail_splits == 0 && p.splits == 1) return w;
    const int splits = p.tail_splits > 0 ? p.tail_splits : p.splits;
    w.rows = p.tail_splits > 0 ? (long)(n - p.main_tiles * S_BN) : (long)n;
    const size_t vbytes = align_up((size_t)splits * w.rows * p.tslots * sizeof(float), 256);
    const size_t ibytes = align_up((size_t)splits * w.rows * p.tslots * sizeof(int), 256);
    if (ws) { w.pval = (float *)ws; w.pidx = (int *)((char *)ws + vbytes); }
    w.total = vbytes + ibytes;
    return w;
}

// ---- more than 8 codes per row (k = 9 .. MEDTOK_MAX_TOPK; the reference takes any k, vector_quantization_soft_one_new.py:91,157,203):
// the lane-local lists of the kernels hold 8 entries, so the search runs as TWO passes of the exact kernel -- the 8 best codes, then
// the best k - 8 among the codes behind the row's 8th (distance, index) pair -- and a join.  Same total order (distance, then
// lowest index) as one list of k: bit-identical to the oracle's top-k.  Always the exact fp32 path (the shortlist kernels keep lists
// of at most 8).  Workspace: the two passes' lists (ids, then distances), then the workspace both passes use in turn.
struct WideWs { int64_t *ia, *ib; float *da, *db; void *inner; size_t total; };
static WideWs wide_ws_layout(void *ws, int64_t n, size_t inner_bytes)
{
    WideWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = ws ? (char *)ws + off : nullptr; off += align_up(bytes, 256); return (void *)p; };
    w.ia = (int64_t *)take((size_t)n * WIDE_T * sizeof(int64_t));
    w.ib = (int64_t *)take((size_t)n * WIDE_T * sizeof(int64_t));
    w.da = (float *)take((size_t)n * WIDE_T * sizeof(float));
    w.db = (float *)take((size_t)n * WIDE_T * sizeof(float));
    w.inner = ws ? (char *)ws + off : nullptr;
    w.total = off + inner_bytes;
    return w;
}

// ---- fp16 filter path: plan + workspace layout
struct FilterPlan {
    long n_pad, k_pad, row_tiles;
    int dp, splits, codes_per_split, own_total, tslots;
    int xcd_rows;      // > 0: XCD-aware block order with this many row tiles per XCD at a time (32 / splits)
    bool rows64;       // dp == 64: the narrow-row kernels (row tiles of 128, 4-wave blocks, no tail launch)
    bool rows64_wide;  // ... of which filter_rows64_kernel (128 x 64 wave tiles, two blocks per CU) instead of filter_rows64n_kernel (plan bit)
    int row_bn;        // rows per row tile of the kernel that runs
    // tail launch: the last main_tiles..row_tiles row tiles with more, shorter splits (0 tiles = none)
    long main_tiles;
    int tail_splits, tail_codes_per_split, own_tail;
};

// width of the filter's fp16 operand images at depth d.
// At least TWO 32-deep stages per code tile: the start values of code tile t + 2 are copied (LDS-DMA, wave 0) at the end of tile
// t's scan and read at the end of tile t + 1's, and what guarantees that they have landed is the counted vmcnt wait of a LATER
// stage -- with one stage per tile there is none in between (found by tools/fuzz_search.py at D = 4 / 32: one wave's 64 rows
// wrong in ~1 % of the searches).  D <= 32 is zero-padded to 64 and takes the narrow-row kernel like every D <= 64.
static inline int filter_image_dp(int d) { return (int)lmax(2 * F_BK, (d + F_BK - 1) / F_BK * F_BK); }

static FilterPlan plan_filter(int64_t n, int64_t k_codes, int d, int topk, const PlanOverride &ov)
{
    FilterPlan f;
    const DevInfo di = dev_info();
    f.tslots = list_slots(topk);
    f.n_pad = (n + F_BN - 1) / F_BN * F_BN;
    f.k_pad = (k_codes + F_BM - 1) / F_BM * F_BM;
    f.dp = filter_image_dp(d);
    f.row_tiles = f.n_pad / F_BN;
    const long code_tiles = f.k_pad / F_BM;
    f.rows64 = f.dp == 64 && ov.filter_rows64 != 0;
    f.rows64_wide = f.rows64 && ov.filter_rows64 == 2;
    f.row_bn = f.rows64 ? R64_BN : F_BN;
    if (f.rows64) {
        // two or three blocks per CU, every one walking its whole code range with the x rows in registers: nothing is shared between
        // blocks but the codebook (K x 128 B, L2-resident), so one split as soon as the chip is full four times over --
        // every split adds candidate lists per row (four; two with 32-row wave tiles) and restarts the thresholds
        f.row_tiles = f.n_pad / R64_BN;
        const long slots = (f.rows64_wide ? 2L : 3L) * di.cus;
        long want = f.row_tiles >= 4 * slots ? 1 : (4 * slots + f.row_tiles - 1) / f.row_tiles;
        if (ov.filter_splits > 0) want = ov.filter_splits;
        if (want > code_tiles) want = code_tiles;
        if (want > 16) want = 16;
        if (want < 1) want = 1;
        const long tiles_per_split = (code_tiles + want - 1) / want;
        f.codes_per_split = (int)(tiles_per_split * R64_BM);
        f.splits = (int)((code_tiles + tiles_per_split - 1) / tiles_per_split);
        f.own_total = f.splits * (f.rows64_wide ? F_OWN_PER_SPLIT : R64N_OWN_PER_SPLIT);
        f.xcd_rows = 0;
        f.main_tiles = f.row_tiles; f.tail_splits = 0; f.tail_codes_per_split = 0; f.own_tail = 0;
        return f;
    }
    // every split adds 4 candidate lists per row, so split only as far as filling the chip needs
    // one 8-wave block per CU: a launch of B equal blocks wastes up to one round of 256
    long want = f.row_tiles >= 4L * di.cus ? 2 : (4L * di.cus + f.row_tiles - 1) / f.row_tiles;
    // With >= 1024 row tiles the blocks are ordered XCD-aware (see filter_f16_kernel): the 32 CUs of an XCD share
    // 32/splits x tiles, which then stay in its 4 MB L2 (393 KB each at D = 768) instead of being re-streamed from
    // the Infinity Cache once per code tile (measured at N = 600k, K = 49152: 6-8 % on the kernel).  Two splits: more
    // would keep more of the x tiles resident but loosen the per-split thresholds (4: +3.6 %, 8: +7.7 % kernel time).
    bool xcd = di.full && f.row_tiles >= 1024;      // (the block order below is written for 8 XCDs of 32 CUs)
    if (ov.filter_splits > 0) want = ov.filter_splits;
    if (ov.filter_xcd >= 0) xcd = di.full && ov.filter_xcd != 0;
    if (want > code_tiles) want = code_tiles;
    if (want > 16) want = 16;      // (more splits for small batches were measured: slower from 32 up)
    if (want < 1) want = 1;
    const long tiles_per_split = (code_tiles + want - 1) / want;
    f.codes_per_split = (int)(tiles_per_split * F_BM);
    f.splits = (int)((code_tiles + tiles_per_split - 1) / tiles_per_split);
    f.own_total = f.splits * F_OWN_PER_SPLIT;
    f.xcd_rows = (xcd && f.splits >= 2 && 32 % f.splits == 0) ? 32 / f.splits : 0;
    // One 8-wave block per CU and equal-cost blocks: B blocks take ceil(B / 256) rounds, the last one however few blocks it
    // holds (N = 600k: 4688 blocks = 18.3 rounds -> 19).  The row tiles of that last round go into a second launch
    // with enough splits to be ONE round of short blocks (N = 600k: 40 row tiles x 6 splits, a third of a round).
    f.main_tiles = f.row_tiles; f.tail_splits = 0; f.tail_codes_per_split = 0; f.own_tail = 0;
    const long blocks = f.row_tiles * f.splits;
    long tail_min_blocks = 8L * di.cus;
    if (ov.filter_tail_min_blocks >= 0)
        tail_min_blocks = ov.filter_tail_min_blocks > 0 ? ov.filter_tail_min_blocks : (1L << 60);   // 0 = off
    const bool tail = blocks >= tail_min_blocks && f.splits <= 4 && code_tiles >= 4L * f.splits;
    if (tail) {
        const long round = (long)di.cus / f.splits * f.splits;     // one block per CU, whole row tiles (splits <= 4)
        const long main_blocks = blocks / round * round;
        const long main_tiles = main_blocks / f.splits;
        // as many splits as make the tail ONE round of short blocks (at most 16: every split costs candidates)
        const long tail_tiles = f.row_tiles - main_tiles;
        const long ts = tail_tiles > 0 ? lmin(lmin(16, code_tiles), round / tail_tiles) : 0;
        if (ts >= 2L * f.splits) {
            const long tps = (code_tiles + ts - 1) / ts;
            f.main_tiles = main_tiles;
            f.tail_codes_per_split = (int)(tps * F_BM);
            f.tail_splits = (int)((code_tiles + tps - 1) / tps);
            f.own_tail = f.tail_splits * F_OWN_PER_SPLIT;
        }
    }
    return f;
}

struct FilterWs {
    _Float16 *xh, *wh;
    float *en_max, *wsqp, *dump;
    uint2 *cand, *cand_tail;
    int *cnt_tail;
    int *cand_cnt, *fb_count, *fb_rows, *fb_pidx;
    float *fb_pval;
    long n_main, n_tail;     // rows whose candidate lists the main / the tail launch writes
    size_t total;
};

// Exact redo of the few rows the filter gives up on: the first FB_ROWS list entries are searched with the
// code range split FB_SPLITS ways (a handful of rows would otherwise crawl through all K codes in one
// block); anything beyond that many rows is plentiful enough for the plain one-block-per-128-rows form.
constexpr int FB_ROWS = 8192, FB_SPLITS = 32;

static FilterWs filter_ws_layout(void *ws, int64_t n, const FilterPlan &f)
{
    FilterWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = ws ? (char *)ws + off : nullptr; off += align_up(bytes, 256); return (void *)p; };
    w.xh = (_Float16 *)take((size_t)f.n_pad * f.dp * 2);
    w.wh = (_Float16 *)take((size_t)f.k_pad * f.dp * 2);
    w.en_max = (float *)take(4);
    w.wsqp = (float *)take((size_t)f.k_pad * 4);
    w.fb_count = (int *)take(4);
    w.fb_rows = (int *)take((size_t)n * 4);
    w.fb_pval = (float *)take((size_t)FB_SPLITS * FB_ROWS * MEDTOK_MAX_TOPK * 4);
    w.fb_pidx = (int *)take((size_t)FB_SPLITS * FB_ROWS * MEDTOK_MAX_TOPK * 4);
    w.n_main = lmin(n, f.main_tiles * f.row_bn); w.n_tail = (long)n - w.n_main;
    w.cand_cnt = (int *)take((size_t)w.n_main * f.own_total * 4);
    w.cand = (uint2 *)take((size_t)w.n_main * f.own_total * F_CAP * 8);
    w.cnt_tail = (int *)take((size_t)w.n_tail * f.own_tail * 4);
    w.cand_tail = (uint2 *)take((size_t)w.n_tail * f.own_tail * F_CAP * 8);
    w.dump = nullptr;
    w.total = off;
    return w;
}

static bool filter_eligible(int64_t n, int64_t k_codes, int d, int topk)
{
    // the filter path has ~0.1-0.2 ms of fixed cost (operand conversion, three extra launches); measured
    // crossover against the exact kernel on MI355X is around 1e10 flop (tools/path_crossover.py)
    // (k_codes * d < 2^29: the kernel addresses a code split's fp16 image with a 32-bit buffer offset)
    const double flops = 2.0 * (double)n * (double)k_codes * (double)d;
    if (!(n >= 512 && k_codes >= 1024 && flops >= 1.0e10 && topk <= 8 && n < (1ll << 31) &&
          (double)k_codes * (double)(d + 64) < 536870912.0))
        return false;
    // Few rows: the filter has a floor -- converting the codebook, one block walking its share of the codes, the re-score and the
    // (empty) redo launches -- while the exact kernel runs at about 100 TFLOP/s from 512 rows up once D is a few hundred.  Floor
    // fitted in round 6 on MI355X (tools/r06/crossover_small.py, profiles/r06_path_crossover_small.txt: D = 768 / 256, K = 8192 ..
    // 49152, N = 128 .. 4096): 61.5 us + 0.70 us per 256-code tile and k block of a 16th of the codebook + 1.04 ns per code; the
    // round-2 floor (170 us + 1.1 us per unit) sent 512 x 49152 and 1024 x 16384 searches at D = 768 to the exact kernel, which
    // takes 0.38 / 0.24 ms there against 0.32 / 0.15 ms.  5 % in favour of the exact kernel (fewer launches).
    if (d >= 256) {
        const double filter_floor = 61.5e-6 + ((double)k_codes / 4096.0) * ((double)d / 32.0) * 0.703e-6 + (double)k_codes * 1.04e-9;
        if (flops / 1.0e14 + 20.0e-6 < 1.05 * filter_floor) return false;
    }
    return true;
}

static int resolve_path(int path, int64_t n, int64_t k_codes, int d, int topk)
{
    path = path_id(path);
    if (topk > 8) return MEDTOK_PATH_F32_MFMA;          // (the shortlist kernels keep lists of at most 8: search_wide)
    if (path == MEDTOK_PATH_AUTO) return filter_eligible(n, k_codes, d, topk) ? MEDTOK_PATH_F16_FILTER : MEDTOK_PATH_F32_MFMA;
    if (path == MEDTOK_PATH_F16_FILTER && (double)k_codes * (double)(d + 64) >= 536870912.0) return MEDTOK_PATH_F32_MFMA;
    return path;
}

// Everything a search call derives from its shape and its `path` argument, derived ONCE: the size queries, the launches and the
// test hooks all read this struct, so a plan and the workspace laid out for it cannot disagree.  Built for any arguments (the
// entry points check theirs later, after what they launch first): a shape no search runs on gives the exact path with no workspace.
struct SearchCall {
    PlanOverride ov;
    int requested = MEDTOK_PATH_AUTO;        // the `path` argument's path id, as the caller gave it
    int path = MEDTOK_PATH_F32_MFMA;         // the path that runs: MEDTOK_PATH_F32_MFMA or MEDTOK_PATH_F16_FILTER
    int tslots = 0;                          // list length of the kernels' instantiation; 8 for both passes of a search for k > 8
    bool ragged = false;                     // d % S_BK != 0: the KTAIL instantiations of the exact kernel
    bool wide = false;                       // k > 8: two exact passes and a join (search_wide)
    SearchPlan exact = {};                   // path == MEDTOK_PATH_F32_MFMA
    FilterPlan filter = {};                  // path == MEDTOK_PATH_F16_FILTER
    size_t ws_bytes = 0;
};

static SearchCall plan_search_call(int64_t n, int64_t k_codes, int d, int topk, int path)
{
    SearchCall c;
    c.ov = decode_plan(path);
    c.requested = path_id(path);
    c.ragged = d % S_BK != 0;
    if (n <= 0 || k_codes <= 0 || topk < 1 || topk > MEDTOK_MAX_TOPK) return c;
    c.path = resolve_path(path, n, k_codes, d, topk);
    c.wide = topk > 8;
    if (c.path == MEDTOK_PATH_F16_FILTER) {
        c.filter = plan_filter(n, k_codes, d, topk, c.ov);
        c.tslots = c.filter.tslots;
        c.ws_bytes = filter_ws_layout(nullptr, n, c.filter).total;
    } else {
        c.exact = plan_search(n, k_codes, c.wide ? WIDE_T : topk, c.ov);
        c.tslots = c.exact.tslots;
        c.ws_bytes = exact_ws_layout(nullptr, n, c.exact).total;
        if (c.wide) c.ws_bytes = wide_ws_layout(nullptr, n, c.ws_bytes).total;
    }
    return c;
}

extern "C" size_t medtok_search_workspace_bytes(int64_t n, int64_t k_codes, int d, int topk, int path)
{
    return plan_search_call(n, k_codes, d, topk, path).ws_bytes;
}

extern "C" int medtok_search_resolved_path(int64_t n, int64_t k_codes, int d, int topk, int path)
{
    if (d <= 0) return MEDTOK_PATH_F32_MFMA;
    return plan_search_call(n, k_codes, d, topk, path).path;
}

// the second pass of a search for k > 8: skip, per row, the codes at or below the (distance, index) pair at excl_d / excl_i [row * stride]
struct Exclude { const float *d; const int64_t *i; int stride; };

// The exact search of one plan (lists of T entries): one launch whose blocks walk all codes and write the final lists, or partial
// lists per code split and their merge, or -- large searches -- whole rounds of the first form and a tail launch of the second.
// EXCL: the exclusion pass (lists of 8 only).
template <int T, bool KTAIL, bool EXCL = false>
static int launch_search(const float *xhat, const float *xsq, int64_t n, const float *what, const float *wsq,
                         int64_t k_codes, int d, int topk, int64_t *idx, float *dist, void *ws, size_t ws_bytes,
                         const SearchPlan &p, hipStream_t s, Exclude ex = {nullptr, nullptr, 0})
{
    static_assert(!EXCL || T == WIDE_T, "the exclusion pass runs with lists of 8");
    dim3 grid((unsigned)p.row_tiles, (unsigned)p.splits), block(256);
    hipEvent_t pa = prof_wanted(1) ? prof_mark(s) : nullptr;
    const double pflops = 2.0 * (double)n * (double)k_codes * (double)d;
    // one launch of the exact kernel: FINAL (a block walks all codes and writes the row's list) or partial lists per code split
    auto go = [&](auto final_, dim3 g, int cps, float *pv, int *pi, int64_t *oi, float *od, int lb, int le) {
        constexpr bool FINAL = decltype(final_)::value;
        if constexpr (EXCL) {
            (void)set_lds_once<search_f32_excl_kernel<T, FINAL, KTAIL>>(S_LDS_BYTES);
            hipLaunchKernelGGL((search_f32_excl_kernel<T, FINAL, KTAIL>), g, block, S_LDS_BYTES, s, xhat, xsq, what, wsq, (long)n, (int)k_codes, d, cps, topk,
                               pv, pi, oi, od, lb, le, ex.d, ex.i, ex.stride);
        } else {
            (void)set_lds_once<search_f32_kernel<T, FINAL, KTAIL, false>>(S_LDS_BYTES);
            hipLaunchKernelGGL((search_f32_kernel<T, FINAL, KTAIL, false>), g, block, S_LDS_BYTES, s, xhat, xsq, what, wsq, (long)n, (int)k_codes, d, cps, topk,
                               pv, pi, oi, od, (const int *)nullptr, (const int *)nullptr, lb, le);
        }
    };
    const ExactWs w = exact_ws_layout(ws, n, p);
    if (p.tail_splits == 0 && p.splits == 1) {
        go(std::true_type{}, grid, p.codes_per_split, (float *)nullptr, (int *)nullptr, idx, dist, 0, 0);
        if (pa) prof_push(pa, prof_mark(s), pflops, 1);
        return check_launch("search_f32");
    }
    if (!ws || ws_bytes < w.total) return fail("search: workspace too small (%zu < %zu)", ws_bytes, w.total);
    if (p.tail_splits > 0) {
        // whole rounds of unsplit blocks, then the last round's row tiles with their own code splits + merge
        const long tail_start = p.main_tiles * S_BN;
        go(std::true_type{}, dim3((unsigned)p.main_tiles, 1), p.codes_per_split, (float *)nullptr, (int *)nullptr, idx, dist, 0, 0);
        go(std::false_type{}, dim3((unsigned)(p.row_tiles - p.main_tiles), (unsigned)p.tail_splits), p.tail_codes_per_split, w.pval, w.pidx, (int64_t *)nullptr,
           (float *)nullptr, (int)tail_start, (int)w.rows);
        if (pa) prof_push(pa, prof_mark(s), pflops, 1);
        if (check_launch("search_f32(main + tail)")) return 1;
        hipLaunchKernelGGL((merge_topk_kernel<T>), dim3((unsigned)((w.rows + 31) / 32)), dim3(256), 0, s, w.pval, w.pidx, w.rows,
                           p.tail_splits, topk, idx + tail_start * topk, dist + tail_start * topk, (const int *)nullptr, (const int *)nullptr,
                           (int)k_codes);
        return check_launch("merge_topk(tail)");
    }
    go(std::false_type{}, grid, p.codes_per_split, w.pval, w.pidx, (int64_t *)nullptr, (float *)nullptr, 0, 0);
    if (pa) prof_push(pa, prof_mark(s), pflops, 1);
    if (check_launch("search_f32(split)")) return 1;
    if (p.splits >= 64 && n <= 8192)     // few rows, many lists each: a wave per row
        hipLaunchKernelGGL((merge_topk_kernel<T, 64>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, w.pval, w.pidx, (long)n,
                           p.splits, topk, idx, dist, (const int *)nullptr, (const int *)nullptr, (int)k_codes);
    else
        hipLaunchKernelGGL((merge_topk_kernel<T>), dim3((unsigned)((n + 31) / 32)), dim3(256), 0, s, w.pval, w.pidx, (long)n,
                           p.splits, topk, idx, dist, (const int *)nullptr, (const int *)nullptr, (int)k_codes);
    return check_launch("merge_topk");
}

// the two passes and the join of a search for more than 8 codes per row (wide_ws_layout)
static int search_wide(const SearchCall &c, const float *xhat, const float *xsq, int64_t n, const float *what, const float *wsq, int64_t k_codes, int d,
                       int topk, int64_t *idx, float *dist, void *ws, size_t ws_bytes, hipStream_t s)
{
    const size_t inner_bytes = exact_ws_layout(nullptr, n, c.exact).total;
    const WideWs w = wide_ws_layout(ws, n, inner_bytes);
    if (!ws || ws_bytes < w.total) return fail("search(k > 8): workspace too small (%zu < %zu)", ws_bytes, w.total);
    const int kb = topk - WIDE_T;
    const int rc = dispatch_lists(c.tslots, c.ragged, [&](auto t, auto ktail) {
        constexpr int T = decltype(t)::value;
        constexpr bool KTAIL = decltype(ktail)::value;
        if constexpr (T == WIDE_T) {
            if (launch_search<T, KTAIL>(xhat, xsq, n, what, wsq, k_codes, d, WIDE_T, w.ia, w.da, w.inner, inner_bytes, c.exact, s)) return 1;
            return launch_search<T, KTAIL, true>(xhat, xsq, n, what, wsq, k_codes, d, kb, w.ib, w.db, w.inner, inner_bytes, c.exact, s,
                                                 Exclude{w.da + (WIDE_T - 1), w.ia + (WIDE_T - 1), WIDE_T});
        } else {
            return fail("search: the exclusion pass runs with lists of 8");
        }
    });
    if (rc) return rc;
    hipLaunchKernelGGL(join_lists_kernel, dim3((unsigned)lmin(4096, (n * topk + 255) / 256)), dim3(256), 0, s, w.ia, w.da, w.ib, w.db, (long)n, kb, idx, dist);
    return check_launch("join_lists");
}

// Handed by medtok_soft_vq_forward_f32 to its search call: when the filter path runs, its re-score kernel also does the
// soft assignment (and the exact-path leftovers get it from soft_assign_kernel through the row list).
struct FuseAssign { const float *xref; float *w; float *zq; long zq_stride; bool done; const int *fb_rows, *fb_count; bool xh_done;
                    // a codebook region prepared once per weight version (medtok_codebook_prepare_f32): its fp16 image, its padded start
                    // values and its largest squared norm -- the search then skips its own passes over the codebook
                    const _Float16 *p_wh = nullptr; const float *p_wsqp = nullptr; const float *p_en_max = nullptr; bool fb_zeroed = false; };

template <int T, bool KTAIL>
static int launch_filter(const float *xhat, const float *xsq, int64_t n, const float *what, const float *wsq,
                         int64_t k_codes, int d, int topk, int64_t *idx, float *dist, void *ws, size_t ws_bytes,
                         hipStream_t s, FuseAssign *fuse, const FilterPlan &f)
{
    const FilterWs w = filter_ws_layout(ws, n, f);
    if (!ws || ws_bytes < w.total) return fail("search(filter): workspace too small (%zu < %zu)", ws_bytes, w.total);
    const bool prep = fuse && fuse->p_wh && fuse->p_wsqp && fuse->p_en_max;
    const _Float16 *const c_wh = prep ? fuse->p_wh : w.wh;
    const float *const c_wsqp = prep ? fuse->p_wsqp : w.wsqp, *const c_en_max = prep ? fuse->p_en_max : w.en_max;
    if (!(fuse && fuse->xh_done))      // (the one-call forward's rownorm has already written the fp16 image of x)
        hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)lmin(4096, (f.n_pad * (f.dp / 8) + 255) / 256)), dim3(256), 0, s, xhat, (long)n, d, f.n_pad, f.dp, w.xh,
                           prep ? w.fb_count : (int *)nullptr);
    else if (prep && !fuse->fb_zeroed && hipMemsetAsync(w.fb_count, 0, 4, s) != hipSuccess)
        return fail("search(filter): memset failed");
    if (!prep) {
        hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)lmin(4096, (f.k_pad * (f.dp / 8) + 255) / 256)), dim3(256), 0, s, what, (long)k_codes, d, f.k_pad, f.dp, w.wh);
        hipLaunchKernelGGL(wsq_max_kernel, dim3(1), dim3(1024), 0, s, wsq, (int)k_codes, w.en_max, w.wsqp, (int)f.k_pad, w.fb_count);
    }
    hipEvent_t pa = prof_wanted(0) ? prof_mark(s) : nullptr;
    if (f.rows64 && !f.rows64_wide) {
        hipLaunchKernelGGL((filter_rows64n_kernel<T>), dim3((unsigned)f.row_tiles, (unsigned)f.splits), dim3(R64N_THREADS), R64N_SMEM_BYTES, s,
                           w.xh, c_wh, xsq, c_wsqp, c_en_max, (long)n, (int)k_codes, d, f.codes_per_split, f.own_total, w.cand, w.cand_cnt);
    } else if (f.rows64) {
        (void)set_lds_once<filter_rows64_kernel<T>>(R64_SMEM_BYTES);
        hipLaunchKernelGGL((filter_rows64_kernel<T>), dim3((unsigned)f.row_tiles, (unsigned)f.splits), dim3(R64_THREADS), R64_SMEM_BYTES, s,
                           w.xh, c_wh, xsq, c_wsqp, c_en_max, (long)n, (int)k_codes, d, f.codes_per_split, f.own_total, w.cand, w.cand_cnt);
    } else {
        (void)set_lds_once<filter_f16_kernel<T, false>>(F_SMEM_BYTES);
        dim3 fgrid((unsigned)f.main_tiles, (unsigned)f.splits);
        if (f.xcd_rows) fgrid = dim3((unsigned)(((f.main_tiles + 8 * f.xcd_rows - 1) / (8 * f.xcd_rows)) * 256), 1);
        hipLaunchKernelGGL((filter_f16_kernel<T, false>), fgrid, dim3(F_THREADS), F_SMEM_BYTES, s,
                           w.xh, c_wh, xsq, c_wsqp, c_en_max, (long)n, (int)k_codes, f.dp, d, f.codes_per_split, f.own_total,
                           w.cand, w.cand_cnt, (float *)nullptr, f.xcd_rows, f.splits, 0, (int)f.main_tiles);
    }
    const long tail_start = f.main_tiles * f.row_bn;
    if (f.main_tiles < f.row_tiles) {
        // the kernel indexes its lists by absolute row: bias the tail region's base pointers accordingly
        hipLaunchKernelGGL((filter_f16_kernel<T, false>), dim3((unsigned)(f.row_tiles - f.main_tiles), (unsigned)f.tail_splits), dim3(F_THREADS),
                           F_SMEM_BYTES, s, w.xh, c_wh, xsq, c_wsqp, c_en_max, (long)n, (int)k_codes, f.dp, d, f.tail_codes_per_split, f.own_tail,
                           w.cand_tail - tail_start * f.own_tail * F_CAP, w.cnt_tail - tail_start * f.own_tail, (float *)nullptr, 0, f.tail_splits,
                           (int)f.main_tiles, (int)f.row_tiles);
    }
    if (pa) prof_push(pa, prof_mark(s), 2.0 * (double)n * (double)k_codes * (double)d, 0);
    if (check_launch("filter_f16")) return 1;
    // few rows: one wavefront per row (latency-bound: rescore_wave_kernel); many rows: 32-row blocks
#define MEDTOK_RESCORE_ARGS                                                                                                      \
    w.cand, w.cand_cnt, f.own_total, w.cand_tail, w.cnt_tail, f.own_tail, f.main_tiles < f.row_tiles ? tail_start : (long)n,     \
    xhat, xsq, what, wsq, c_en_max, (long)n, (int)k_codes, d, topk, idx, dist, w.fb_count, w.fb_rows,                             \
    fuse ? fuse->xref : (const float *)nullptr, fuse ? fuse->w : (float *)nullptr,                                                \
    fuse ? fuse->zq : (float *)nullptr, fuse ? fuse->zq_stride : 0L
    if (n < 32L * 4 * dev_info().cus && f.own_total <= 64 && f.own_tail <= 64)
        hipLaunchKernelGGL((rescore_wave_kernel<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, MEDTOK_RESCORE_ARGS);
    else
        hipLaunchKernelGGL((rescore_kernel<T, 32>), dim3((unsigned)((n + 31) / 32)), dim3(256), 0, s, MEDTOK_RESCORE_ARGS);
#undef MEDTOK_RESCORE_ARGS
    if (check_launch("rescore")) return 1;
    // exact redo of the rows the filter gave up on (normally none: every block exits on *fb_count)
    const long code_tiles = (k_codes + S_BM - 1) / S_BM;
    const int fb_splits = (int)lmin(FB_SPLITS, code_tiles);
    const int fb_cps = (int)((code_tiles + fb_splits - 1) / fb_splits * S_BM);
    const int fb_nsplit = (int)((code_tiles * S_BM + fb_cps - 1) / fb_cps);
    const int head = (int)lmin(n, FB_ROWS);
    (void)set_lds_once<search_f32_kernel<T, false, KTAIL, true>>(S_LDS_BYTES);
    hipLaunchKernelGGL((search_f32_kernel<T, false, KTAIL, true>), dim3((unsigned)((head + S_BN - 1) / S_BN), (unsigned)fb_nsplit), dim3(256), S_LDS_BYTES, s,
                       xhat, xsq, what, wsq, (long)n, (int)k_codes, d, fb_cps, topk, w.fb_pval, w.fb_pidx, (int64_t *)nullptr, (float *)nullptr,
                       (const int *)w.fb_rows, (const int *)w.fb_count, 0, head);
    hipLaunchKernelGGL((merge_topk_kernel<T>), dim3((unsigned)((head + 31) / 32)), dim3(256), 0, s, w.fb_pval, w.fb_pidx, (long)head,
                       fb_nsplit, topk, idx, dist, (const int *)w.fb_rows, (const int *)w.fb_count, (int)k_codes);
    if (n > head) {
        (void)set_lds_once<search_f32_kernel<T, true, KTAIL, true>>(S_LDS_BYTES);
        hipLaunchKernelGGL((search_f32_kernel<T, true, KTAIL, true>), dim3((unsigned)((n - head + S_BN - 1) / S_BN), 1), dim3(256), S_LDS_BYTES, s,
                           xhat, xsq, what, wsq, (long)n, (int)k_codes, d, (int)(code_tiles * S_BM), topk,
                           (float *)nullptr, (int *)nullptr, idx, dist, (const int *)w.fb_rows, (const int *)w.fb_count, head, (int)n);
    }
    if (fuse) { fuse->done = true; fuse->fb_rows = w.fb_rows; fuse->fb_count = w.fb_count; }
    return check_launch("search_f32(fallback)");
}

// The search of a planned call (c = plan_search_call of the same shape and `path`).
// `fuse` (internal callers only): when the filter path runs, its re-score kernel also does the soft assignment described there
static int search_impl(const SearchCall &c, const float *xhat, const float *xsq, int64_t n, const float *what,
                       const float *wsq, int64_t k_codes, int d, int topk, int64_t *idx, float *dist,
                       void *ws, size_t ws_bytes, void *stream, FuseAssign *fuse)
{
    if (n < 0 || k_codes <= 0 || d <= 0 || (d & 3)) return fail("search: bad shape n=%ld K=%ld d=%d (d %% 4 == 0)", (long)n, (long)k_codes, d);
    if (topk < 1 || topk > MEDTOK_MAX_TOPK || topk > k_codes) return fail("search: topk=%d unsupported (1..%d, <= K)", topk, MEDTOK_MAX_TOPK);
    if (k_codes >= (1ll << 31)) return fail("search: K too large");
    if (c.requested != MEDTOK_PATH_AUTO && c.requested != MEDTOK_PATH_F32_MFMA && c.requested != MEDTOK_PATH_F16_FILTER) return fail("search: unknown path %d", c.requested);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (c.wide) return search_wide(c, xhat, xsq, n, what, wsq, k_codes, d, topk, idx, dist, ws, ws_bytes, s);
    if (c.path == MEDTOK_PATH_F16_FILTER && n >= (1ll << 31)) return fail("search(filter): n too large");
    return dispatch_lists(c.tslots, c.ragged, [&](auto t, auto ktail) {
        constexpr int T = decltype(t)::value;
        constexpr bool KTAIL = decltype(ktail)::value;
        if (c.path == MEDTOK_PATH_F16_FILTER)
            return launch_filter<T, KTAIL>(xhat, xsq, n, what, wsq, k_codes, d, topk, idx, dist, ws, ws_bytes, s, fuse, c.filter);
        return launch_search<T, KTAIL>(xhat, xsq, n, what, wsq, k_codes, d, topk, idx, dist, ws, ws_bytes, c.exact, s);
    });
}

extern "C" int medtok_topk_search_f32(const float *xhat, const float *xsq, int64_t n, const float *what,
                                      const float *wsq, int64_t k_codes, int d, int topk, int64_t *idx, float *dist,
                                      void *ws, size_t ws_bytes, int path, void *stream)
{
    return search_impl(plan_search_call(n, k_codes, d, topk, path), xhat, xsq, n, what, wsq, k_codes, d, topk, idx, dist, ws, ws_bytes, stream, nullptr);
}

// Test hook: byte offset, inside a filter-path search workspace, of the int32 count of rows the filter handed to the exact kernel
// (candidate list overflow, norms outside the bound's range, NaN) -- tests and tools read it after a search; (size_t)-1 if the shape
// does not take the filter path.
extern "C" size_t medtok_debug_filter_fallback_count_offset(int64_t n, int64_t k_codes, int d, int topk, int path)
{
    const SearchCall c = plan_search_call(n, k_codes, d, topk, path);
    if (c.path != MEDTOK_PATH_F16_FILTER) return (size_t)-1;
    const FilterWs w = filter_ws_layout((void *)256, n, c.filter);
    return (size_t)((char *)w.fb_count - (char *)256);
}

// Measurement hook (bench.py --data ..., tests): what the filter pass of a finished search left in its workspace -- how many candidates
// it shortlisted, how many of a row's lists are full, how many rows it handed to the exact kernel (filter_stats_kernel).  `ws` is the
// workspace of the search call (soft_vq_ws != 0: of a medtok_soft_vq_forward*_f32 call, whose search workspace starts behind |x|^2),
// read after the call on the same stream.  out[0] = candidates over all rows and lists, out[1] = lists at or over capacity, out[2] =
// rows handed to the exact kernel, out[3] = lists in total (rows x owners).
extern "C" int medtok_debug_filter_stats(const void *ws, size_t ws_bytes, int soft_vq_ws, int64_t n, int64_t k_codes, int d, int topk, int path,
                                         uint64_t *out, void *stream)
{
    if (!ws || !out || n <= 0 || k_codes <= 0) return fail("filter_stats: bad arguments");
    const SearchCall c = plan_search_call(n, k_codes, d, topk, path);
    if (c.path != MEDTOK_PATH_F16_FILTER) return fail("filter_stats: this shape does not take the filter path");
    const size_t head = soft_vq_ws ? align_up((size_t)n * 4, 256) : 0;
    const FilterPlan &f = c.filter;
    const FilterWs w = filter_ws_layout((char *)const_cast<void *>(ws) + head, n, f);
    if (ws_bytes < head + w.total) return fail("filter_stats: workspace too small (%zu < %zu)", ws_bytes, head + w.total);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, 32, s) != hipSuccess) return fail("filter_stats: memset failed");
    const long lists = w.n_main * f.own_total, lists_tail = w.n_tail * f.own_tail;
    hipLaunchKernelGGL(filter_stats_kernel, dim3((unsigned)lmin(1024, (lists + lists_tail + 255) / 256)), dim3(256), 0, s, w.cand_cnt, lists, w.cnt_tail, lists_tail,
                       w.fb_count, (unsigned long long *)out);
    return check_launch("filter_stats");
}

// Test hook: the filter's approximate scores s~ [n, k_codes] (same MFMA sequence as the search uses),
// so tests can measure |s~ - s| against the bound filter_f16.h assumes.  The score dump is an instantiation of the general
// kernel (same MFMA order at any D), so both entry points force that kernel's plan whatever the depth.
struct ScoreDumpWs { _Float16 *xh, *wh; float *en_max, *wsqp; size_t total; };
static ScoreDumpWs score_dump_layout(void *ws, const FilterPlan &f)
{
    const size_t xb = align_up((size_t)f.n_pad * f.dp * 2, 256), wb = align_up((size_t)f.k_pad * f.dp * 2, 256);
    char *b = (char *)ws;
    return {(_Float16 *)b, (_Float16 *)(b + xb), (float *)(b + xb + wb), (float *)(b + xb + wb + 512), xb + wb + 512 + align_up((size_t)f.k_pad * 4, 256)};
}
static FilterPlan score_dump_plan(int64_t n, int64_t k_codes, int d)
{
    PlanOverride gen; gen.filter_rows64 = 0;
    return plan_filter(n, k_codes, d, 5, gen);
}

extern "C" size_t medtok_debug_filter_scores_workspace_bytes(int64_t n, int64_t k_codes, int d)
{
    if (n <= 0 || k_codes <= 0 || d <= 0) return 0;
    return score_dump_layout(nullptr, score_dump_plan(n, k_codes, d)).total;
}

extern "C" int medtok_debug_filter_scores_f32(const float *xhat, const float *xsq, int64_t n, const float *what, const float *wsq,
                                              int64_t k_codes, int d, float *scores, void *ws, size_t ws_bytes, void *stream)
{
    if (n <= 0 || k_codes <= 0 || d <= 0 || (d & 3)) return fail("debug_filter_scores: bad shape");
    const FilterPlan f = score_dump_plan(n, k_codes, d);
    const ScoreDumpWs w = score_dump_layout(ws, f);
    if (!ws || ws_bytes < w.total) return fail("debug_filter_scores: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pad_wsq_kernel, dim3((unsigned)((f.k_pad + 255) / 256)), dim3(256), 0, s, wsq, (int)k_codes, (int)f.k_pad, w.wsqp);
    hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)lmin(4096, (f.n_pad * (f.dp / 8) + 255) / 256)), dim3(256), 0, s, xhat, (long)n, d, f.n_pad, f.dp, w.xh);
    hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)lmin(4096, (f.k_pad * (f.dp / 8) + 255) / 256)), dim3(256), 0, s, what, (long)k_codes, d, f.k_pad, f.dp, w.wh);
    hipLaunchKernelGGL(wsq_max_kernel, dim3(1), dim3(1024), 0, s, wsq, (int)k_codes, w.en_max, (float *)nullptr, 0, (int *)nullptr);
    (void)set_lds_once<filter_f16_kernel<5, true>>(F_SMEM_BYTES);
    hipLaunchKernelGGL((filter_f16_kernel<5, true>), dim3((unsigned)f.row_tiles, 1), dim3(F_THREADS), F_SMEM_BYTES, s, w.xh, w.wh, xsq, w.wsqp, w.en_max,
                       (long)n, (int)k_codes, f.dp, d, (int)f.k_pad, F_OWN_PER_SPLIT, (uint2 *)nullptr, (int *)nullptr, scores, 0, 1,
                       0, (int)f.row_tiles);
    return check_launch("filter_f16(dump)");
}

// ================================================================= merge of per-shard top-k lists (merge_lists_kernel)
extern "C" int medtok_merge_topk_lists_f32(const float *dist_parts, const int64_t *idx_parts, int64_t n, int parts, int topk,
                                           int64_t *idx, float *dist, void *stream)
{
    if (n < 0 || parts < 1 || topk < 1 || topk > MEDTOK_MAX_TOPK) return fail("merge_topk_lists: bad args");
    if (n == 0) return 0;
    hipLaunchKernelGGL(merge_lists_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dist_parts, idx_parts,
                       (long)n, parts, topk, idx, dist);
    return check_launch("merge_topk_lists");
}

// ================================================================= soft assign, fixed-order fp64 sum (assign_kernels.h)
#include "assign_kernels.h"

extern "C" int medtok_soft_assign_f32(const float *xref, const float *what, const int64_t *idx, const float *dist,
                                      int64_t n, int d, int topk, int flags, float *w, float *zq_ste, int64_t zq_stride,
                                      float *row_sqerr, void *stream)
{
    if (zq_stride == 0) zq_stride = d;
    if (zq_stride < d || (zq_stride & 3)) return fail("soft_assign: zq_stride must be >= d and a multiple of 4");
    const int hard = flags & MEDTOK_ASSIGN_HARD;
    if (n < 0 || d <= 0 || (d & 3)) return fail("soft_assign: bad shape n=%ld d=%d", (long)n, d);
    if (topk < 1 || topk > MEDTOK_MAX_TOPK) return fail("soft_assign: topk=%d unsupported", topk);
    if (hard && topk != 1) return fail("soft_assign: hard assignment needs topk == 1");
    if (!hard && !dist) return fail("soft_assign: dist required");
    if (n == 0) return 0;
    if (!zq_ste) return fail("soft_assign: zq_ste required");
    // (lists of up to 8 codes -- every shipped configuration -- keep the 8-slot instantiation; 9 .. 16 take the 16-slot one)
    if (topk <= 8)
        hipLaunchKernelGGL((soft_assign_kernel<8>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                           xref, what, idx, dist, (long)n, d, topk, flags, w, zq_ste, (long)zq_stride, row_sqerr,
                           (const int *)nullptr, (const int *)nullptr);
    else
        hipLaunchKernelGGL((soft_assign_kernel<MEDTOK_MAX_TOPK>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                           xref, what, idx, dist, (long)n, d, topk, flags, w, zq_ste, (long)zq_stride, row_sqerr,
                           (const int *)nullptr, (const int *)nullptr);
    return check_launch("soft_assign");
}

extern "C" int medtok_sum_scale_f32(const float *vals, int64_t n, double scale, float *out, void *stream)
{
    if (n < 0 || !out) return fail("sum_scale: bad args");
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, vals, (long)n, scale, out);
    return check_launch("sum_scale");
}

// ================================================================= several small searches, batched (kernels in search_f32.h)
constexpr int64_t MS_MAX_ROWS = 4096;

extern "C" int medtok_soft_vq_multi_eligible(int64_t n, int64_t k_codes, int d, int topk)
{
    return n >= 1 && n <= MS_MAX_ROWS && k_codes >= 1 && k_codes < (1ll << 31) && d > 0 && !(d & 3) && topk >= 1 && topk <= 8 &&
           topk <= k_codes && plan_search_call(n, k_codes, d, topk, MEDTOK_PATH_AUTO).path == MEDTOK_PATH_F32_MFMA;
}

// code splits of every search of a batched call: about two rounds' worth of blocks over the whole call (two 256-thread blocks are
// resident per CU), every search's code tiles cut into splits of equal length
static void multi_plan(const medtok_search_desc *descs, int count, int *splits, int *cps)
{
    const DevInfo di = dev_info();
    long tiles_total = 0;
    for (int i = 0; i < count; ++i) tiles_total += ((descs[i].n + S_BN - 1) / S_BN) * ((descs[i].k_codes + S_BM - 1) / S_BM);
    const long per_block = lmax(1, (tiles_total + 2L * di.cus - 1) / (2L * di.cus));
    for (int i = 0; i < count; ++i) {
        const long code_tiles = (descs[i].k_codes + S_BM - 1) / S_BM;
        const long tps = lmin(per_block, code_tiles);
        cps[i] = (int)(tps * S_BM);
        splits[i] = (int)((code_tiles + tps - 1) / tps);
    }
}

extern "C" size_t medtok_soft_vq_forward_multi_workspace_bytes(const medtok_search_desc *descs, int count, int d, int topk)
{
    if (!descs || count < 1 || count > MS_MAX) return 0;
    int splits[MS_MAX], cps[MS_MAX];
    multi_plan(descs, count, splits, cps);
    const int tslots = list_slots(topk);
    size_t total = 0;
    for (int i = 0; i < count; ++i) {
        const size_t n = (size_t)(descs[i].n > 0 ? descs[i].n : 1);
        total += align_up(n * 4, 256) + 2 * align_up((size_t)splits[i] * n * tslots * 4, 256);
    }
    return total + 256;
}

extern "C" int medtok_soft_vq_forward_multi_f32(const medtok_search_desc *descs, int count, int d, int topk, void *ws, size_t ws_bytes, void *stream)
{
    if (!descs || count < 1 || count > MS_MAX) return fail("soft_vq_forward_multi: 1..%d searches per call", MS_MAX);
    for (int i = 0; i < count; ++i) {
        const medtok_search_desc &q = descs[i];
        if (!medtok_soft_vq_multi_eligible(q.n, q.k_codes, d, topk))
            return fail("soft_vq_forward_multi: search %d (n=%ld K=%ld d=%d topk=%d) does not take the batched exact path", i, (long)q.n, (long)q.k_codes, d, topk);
        if (!q.x || !q.what || !q.wsq || !q.xhat || !q.idx || !q.dist || !q.zq) return fail("soft_vq_forward_multi: NULL argument in search %d", i);
        const int64_t zs = q.zq_stride ? q.zq_stride : d, xs = q.x_stride ? q.x_stride : d;
        if (zs < d || (zs & 3) || xs < d || (xs & 3)) return fail("soft_vq_forward_multi: zq_stride / x_stride must be >= d and multiples of 4");
        if (((uintptr_t)q.x | (uintptr_t)q.what | (uintptr_t)q.xhat | (uintptr_t)q.zq) & 15) return fail("soft_vq_forward_multi: pointers must be 16-byte aligned");
    }
    const size_t need = medtok_soft_vq_forward_multi_workspace_bytes(descs, count, d, topk);
    if (!ws || ws_bytes < need) return fail("soft_vq_forward_multi: workspace too small (%zu < %zu)", ws_bytes, need);
    int splits[MS_MAX], cps[MS_MAX];
    multi_plan(descs, count, splits, cps);
    const int tslots = list_slots(topk);
    MultiSearchArgs a;
    memset(&a, 0, sizeof a);
    a.count = count; a.d = d; a.topk = topk;
    char *p = (char *)ws;
    auto take = [&](size_t bytes) { char *q = p; p += align_up(bytes, 256); return (void *)q; };
    long max_rows = 0;
    int max_tiles = 0, max_splits = 0;
    for (int i = 0; i < count; ++i) {
        const medtok_search_desc &q = descs[i];
        MultiSearchOne &m = a.s[i];
        m.x = q.x; m.what = q.what; m.wsq = q.wsq; m.xhat = q.xhat; m.idx = q.idx; m.dist = q.dist; m.w = q.w; m.zq = q.zq; m.row_sqerr = q.row_sqerr;
        m.n = (long)q.n; m.zq_stride = (long)(q.zq_stride ? q.zq_stride : d); m.x_stride = (long)(q.x_stride ? q.x_stride : d);
        m.k_codes = (int)q.k_codes; m.codes_per_split = cps[i]; m.splits = splits[i]; m.row_tiles = (int)((q.n + S_BN - 1) / S_BN);
        m.xsq = (float *)take((size_t)q.n * 4);
        m.pval = (float *)take((size_t)splits[i] * q.n * tslots * 4);
        m.pidx = (int *)take((size_t)splits[i] * q.n * tslots * 4);
        max_rows = lmax(max_rows, m.n); max_tiles = max_tiles > m.row_tiles ? max_tiles : m.row_tiles; max_splits = max_splits > m.splits ? max_splits : m.splits;
        a.block_base[i + 1] = a.block_base[i] + m.row_tiles * m.splits;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rownorm_multi_kernel, dim3((unsigned)((max_rows + 3) / 4), (unsigned)count), dim3(256), 0, s, a);
    hipEvent_t pa = prof_wanted(1) ? prof_mark(s) : nullptr;
    double pflops = 0.0;
    for (int i = 0; i < count; ++i) pflops += 2.0 * (double)descs[i].n * (double)descs[i].k_codes * (double)d;
    (void)max_tiles; (void)max_splits;
    const dim3 grid((unsigned)a.block_base[count]);          // exactly the blocks that have work, search after search
    dispatch_lists(tslots, d % S_BK != 0, [&](auto t, auto ktail) {
        constexpr int T = decltype(t)::value;
        constexpr bool KTAIL = decltype(ktail)::value;
        (void)set_lds_once<search_f32_multi_kernel<T, KTAIL>>(S_LDS_BYTES);
        hipLaunchKernelGGL((search_f32_multi_kernel<T, KTAIL>), grid, dim3(256), S_LDS_BYTES, s, a);
        if (pa) prof_push(pa, prof_mark(s), pflops, 1);
        hipLaunchKernelGGL((merge_assign_multi_kernel<T>), dim3((unsigned)((max_rows + 3) / 4), (unsigned)count), dim3(256), 0, s, a);
        return 0;
    });
    return check_launch("soft_vq_forward_multi");
}

// ================================================================= decode: (token ids, weights) -> embedding, and its backward
#include "decode_kernels.h"

// the argument checks both decode entries share; fills the per-slot regions the kernels take by value
static int decode_args(const char *fn, int64_t n, int slots, int topk, int64_t n_codes, int d, const int64_t *region_lo,
                       const int64_t *region_size, DecodeRegions &reg)
{
    if (n < 0 || d <= 0 || (d & 3)) return fail("%s: bad shape n=%ld d=%d (need n >= 0, d > 0, d %% 4 == 0)", fn, (long)n, d);
    if (slots < 1 || slots > MEDTOK_DECODE_MAX_SLOTS) return fail("%s: slots=%d unsupported (1 .. %d)", fn, slots, MEDTOK_DECODE_MAX_SLOTS);
    if (topk < 1 || topk > MEDTOK_MAX_TOPK) return fail("%s: topk=%d unsupported", fn, topk);
    if (n_codes < 1 || n_codes >= (1ll << 31)) return fail("%s: n_codes=%ld unsupported", fn, (long)n_codes);
    if (!region_lo || !region_size) return fail("%s: region_lo and region_size are required", fn);
    for (int s = 0; s < MEDTOK_DECODE_MAX_SLOTS; ++s) {
        const int t = s < slots ? s : 0;
        if (region_lo[t] < 0 || region_size[t] < 1 || region_lo[t] > n_codes - region_size[t])
            return fail("%s: region %d = [%ld, +%ld) is not inside the %ld codes", fn, t, (long)region_lo[t], (long)region_size[t], (long)n_codes);
        reg.lo[s] = (long)region_lo[t];
        reg.size[s] = (long)region_size[t];
    }
    if (n > ((1ll << 31) - 1) * 4 / slots) return fail("%s: n=%ld rows x %d slots exceed one launch", fn, (long)n, slots);
    return 0;
}

// a row stride of the caller's: 0 means dense; otherwise it covers the row and keeps float4 alignment
static int row_stride(const char *fn, const char *name, int64_t &stride, int64_t least, const char *least_name)
{
    if (stride == 0) stride = least;
    if (stride < least || (stride & 3)) return fail("%s: %s must be >= %s and a multiple of 4", fn, name, least_name);
    return 0;
}

// (first template constant, list length) -> compile-time constants: fn(std::integral_constant<int, V>, std::integral_constant<int, MAXK>)
// with V = the one of VALUES... that equals `value` (the lanes per group, or the pool's float4 per lane) and MAXK = 8 for lists of up to
// 8 codes (they keep the 8-slot instantiation, as soft_assign), else MEDTOK_MAX_TOPK.  Every launch of a decode or lookup kernel that is
// instantiated per list length goes through here, so only the listed instantiations exist.
template <int... VALUES, typename F>
static void dispatch_group(int value, int topk, F &&fn)
{
    auto by_k = [&](auto v) {
        if (topk <= 8) fn(v, std::integral_constant<int, 8>{});
        else fn(v, std::integral_constant<int, MEDTOK_MAX_TOPK>{});
        return true;
    };
    (void)((value == VALUES && by_k(std::integral_constant<int, VALUES>{})) || ...);
}

// lanes per (row, slot) item of the decode-layout kernels: sixteen for rows of at most 64 floats, else a wavefront
static inline int item_lanes(int d) { return d <= 64 ? 16 : 64; }

// a launch holds at most 2^32 threads along x: 2^24 - 1 blocks of 256
static const int64_t kMaxBlocks = 0xffffffffll / 256;

extern "C" int medtok_decode_tokens_f32(const int64_t *tokens, const float *weights, int64_t n, int slots, int topk, const float *what,
                                        int64_t n_codes, int d, const int64_t *region_lo, const int64_t *region_size, float *out,
                                        int64_t out_stride, int *status, void *stream)
{
    DecodeRegions reg;
    if (int rc = decode_args("decode_tokens", n, slots, topk, n_codes, d, region_lo, region_size, reg)) return rc;
    if (int rc = row_stride("decode_tokens", "out_stride", out_stride, (int64_t)slots * d, "slots * d")) return rc;
    if (n == 0) return 0;
    if (!tokens || !weights || !what || !out) return fail("decode_tokens: tokens, weights, what and out are required");
    const long items = (long)n * slots;
    hipStream_t s = (hipStream_t)stream;
    dispatch_group<16, 64>(item_lanes(d), topk, [&](auto lanes, auto maxk) {
        constexpr int LANES = decltype(lanes)::value, MAXK = decltype(maxk)::value;
        hipLaunchKernelGGL((decode_tokens_kernel<LANES, MAXK>), dim3((unsigned)((items + 256 / LANES - 1) / (256 / LANES))), dim3(256), 0, s,
                           tokens, weights, items, slots, topk, what, d, reg, out, (long)out_stride, status);
    });
    return check_launch("decode_tokens");
}

extern "C" int medtok_decode_tokens_backward_f32(const float *g_out, int64_t g_stride, const int64_t *tokens, const float *weights, int64_t n,
                                                 int slots, int topk, const float *what, int64_t n_codes, int d, const int64_t *region_lo,
                                                 const int64_t *region_size, float *g_w, float *g_code, int64_t *g_ids, int *status,
                                                 void *stream)
{
    DecodeRegions reg;
    if (int rc = decode_args("decode_tokens_backward", n, slots, topk, n_codes, d, region_lo, region_size, reg)) return rc;
    if (int rc = row_stride("decode_tokens_backward", "g_stride", g_stride, (int64_t)slots * d, "slots * d")) return rc;
    if (!g_w && !g_code) return fail("decode_tokens_backward: nothing to compute (g_w and g_code are both NULL)");
    if ((g_code != nullptr) != (g_ids != nullptr)) return fail("decode_tokens_backward: g_code and g_ids go together");
    if (n == 0) return 0;
    if (!g_out || !tokens || !weights || !what) return fail("decode_tokens_backward: g_out, tokens, weights and what are required");
    const long items = (long)n * slots;
    hipStream_t s = (hipStream_t)stream;
    dispatch_group<16, 64>(item_lanes(d), topk, [&](auto lanes, auto maxk) {
        constexpr int LANES = decltype(lanes)::value, MAXK = decltype(maxk)::value;
        hipLaunchKernelGGL((decode_tokens_backward_kernel<LANES, MAXK>), dim3((unsigned)((items + 256 / LANES - 1) / (256 / LANES))), dim3(256), 0, s,
                           g_out, (long)g_stride, tokens, weights, items, slots, topk, what, d, reg, g_w, g_code, g_ids, status);
    });
    return check_launch("decode_tokens_backward");
}

// ================================================================= embedding lookup: code indices -> stored tokens -> embedding
#include "embed_kernels.h"

// What every medtok_embed_* lookup entry is given: the positions' code indices and mask, the stored lists [num_codes, slots, topk], and
// the table they point into -- the normalised codebook [rows, width = d] or the folded tables [rows, width = hp] -- with a region of its
// rows per slot.  The extern "C" entries fill it and hand it on.
struct EmbedLookup {
    const int64_t *index;
    const uint8_t *pad;
    const int64_t *tokens;
    const float *weights;
    int64_t num_codes;
    int slots, topk;
    const float *table;
    int64_t rows;
    int width;
    const int64_t *region_lo, *region_size;
};

// the shape checks of a lookup over n positions: decode's, the range of num_codes, and, for a kernel that gives a code's entries one lane
// each (the folded lookup, the pool), that they fit a wavefront; fills the regions
static int embed_args(const char *fn, const EmbedLookup &a, int64_t n, bool entry_per_lane, DecodeRegions &reg)
{
    if (int rc = decode_args(fn, n, a.slots, a.topk, a.rows, a.width, a.region_lo, a.region_size, reg)) return rc;
    if (a.num_codes < 1 || a.num_codes > (1ll << 40)) return fail("%s: num_codes=%ld unsupported", fn, (long)a.num_codes);
    if (entry_per_lane && a.slots * a.topk > 64)
        return fail("%s: slots * topk = %d entries per code exceed one wavefront", fn, a.slots * a.topk);
    return 0;
}

// all output widths of medtok_embed_codes_*: the checks, then one launch
template <typename OUT>
static int embed_codes_launch(const char *fn, const EmbedLookup &a, int64_t n, const float *miss, OUT *out, int64_t out_stride, int *status,
                              void *stream)
{
    DecodeRegions reg;
    if (int rc = embed_args(fn, a, n, false, reg)) return rc;
    if (int rc = row_stride(fn, "out_stride", out_stride, (int64_t)a.slots * a.width, "slots * d")) return rc;
    if (n == 0) return 0;
    if (!a.index || !a.tokens || !a.weights || !a.table || !out) return fail("%s: index, tokens, weights, what and out are required", fn);
    const long items = (long)n * a.slots;
    hipStream_t s = (hipStream_t)stream;
    dispatch_group<16, 64>(item_lanes(a.width), a.topk, [&](auto lanes, auto maxk) {
        constexpr int LANES = decltype(lanes)::value, MAXK = decltype(maxk)::value;
        hipLaunchKernelGGL((embed_codes_kernel<LANES, MAXK, OUT>), dim3((unsigned)((items + 256 / LANES - 1) / (256 / LANES))), dim3(256), 0, s,
                           a.index, a.pad, items, a.tokens, a.weights, (long)a.num_codes, a.slots, a.topk, a.table, a.width, reg, miss, out,
                           (long)out_stride, status);
    });
    return check_launch(fn);
}

extern "C" int medtok_embed_codes_f32(const int64_t *index, const uint8_t *pad, int64_t n, const int64_t *tokens, const float *weights,
                                      int64_t num_codes, int slots, int topk, const float *what, int64_t n_codes, int d,
                                      const int64_t *region_lo, const int64_t *region_size, const float *miss, float *out, int64_t out_stride,
                                      int *status, void *stream)
{
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, what, n_codes, d, region_lo, region_size};
    return embed_codes_launch<float>("embed_codes", a, n, miss, out, out_stride, status, stream);
}

extern "C" int medtok_embed_codes_f16(const int64_t *index, const uint8_t *pad, int64_t n, const int64_t *tokens, const float *weights,
                                      int64_t num_codes, int slots, int topk, const float *what, int64_t n_codes, int d,
                                      const int64_t *region_lo, const int64_t *region_size, const float *miss, void *out, int64_t out_stride,
                                      int bf16, int *status, void *stream)
{
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, what, n_codes, d, region_lo, region_size};
    if (bf16) return embed_codes_launch<__bf16>("embed_codes_f16(bf16)", a, n, miss, (__bf16 *)out, out_stride, status, stream);
    return embed_codes_launch<_Float16>("embed_codes_f16", a, n, miss, (_Float16 *)out, out_stride, status, stream);
}

// Every entry of the folded lookup (embed_folded_kernel): medtok_embed_project_* (parts == nullptr: one output row per position) and
// medtok_embed_sequence_* (items = batch * (n_prefix + len) output rows over batch * len positions).
template <typename OUT>
static int embed_folded_launch(const char *fn, const EmbedLookup &a, int64_t positions, int64_t items, int64_t len, const EmbedSeqParts *parts,
                               const float *bias, const float *miss_row, OUT *out, int64_t out_stride, int *status, void *stream)
{
    DecodeRegions reg;
    if (int rc = embed_args(fn, a, positions, true, reg)) return rc;
    if (int rc = row_stride(fn, "out_stride", out_stride, a.width, "hp")) return rc;
    if (items == 0) return 0;
    if (!a.tokens || !a.weights || !a.table || !bias || !out || (positions > 0 && !a.index))
        return fail("%s: index, tokens, weights, table, bias and out are required", fn);
    hipStream_t s = (hipStream_t)stream;
    // the smallest group that holds the code's slots * topk entries and, up to a wavefront, covers the row in one float4 pass
    int group = 16;
    while (group < 64 && (group < a.slots * a.topk || group * 4 < a.width)) group *= 2;
    const int64_t blocks = (items + 256 / group - 1) / (256 / group);
    if (parts && blocks > kMaxBlocks) return fail("%s: %ld rows exceed one launch (%ld blocks of 256 threads)", fn, (long)items, (long)kMaxBlocks);
    dispatch_group<16, 32, 64>(group, a.topk, [&](auto lanes, auto maxk) {
        auto launch = [&](auto with_parts) {
            hipLaunchKernelGGL((embed_folded_kernel<decltype(lanes)::value, decltype(maxk)::value, OUT, decltype(with_parts)::value>),
                               dim3((unsigned)blocks), dim3(256), 0, s, a.index, a.pad, (long)items, (long)len, a.tokens, a.weights,
                               (long)a.num_codes, a.slots, a.topk, a.table, a.width, reg, bias, miss_row, parts ? *parts : EmbedSeqParts{}, out,
                               (long)out_stride, status);
        };
        if (parts) launch(std::true_type{}); else launch(std::false_type{});
    });
    return check_launch(fn);
}

extern "C" int medtok_embed_project_f32(const int64_t *index, const uint8_t *pad, int64_t n, const int64_t *tokens, const float *weights,
                                        int64_t num_codes, int slots, int topk, const float *table, int64_t n_rows, int hp,
                                        const int64_t *row_lo, const int64_t *row_size, const float *bias, const float *miss_row, float *out,
                                        int64_t out_stride, int *status, void *stream)
{
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, table, n_rows, hp, row_lo, row_size};
    return embed_folded_launch<float>("embed_project", a, n, n, 0, nullptr, bias, miss_row, out, out_stride, status, stream);
}

extern "C" int medtok_embed_project_f16(const int64_t *index, const uint8_t *pad, int64_t n, const int64_t *tokens, const float *weights,
                                        int64_t num_codes, int slots, int topk, const float *table, int64_t n_rows, int hp,
                                        const int64_t *row_lo, const int64_t *row_size, const float *bias, const float *miss_row, void *out,
                                        int64_t out_stride, int bf16, int *status, void *stream)
{
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, table, n_rows, hp, row_lo, row_size};
    if (bf16)
        return embed_folded_launch<__bf16>("embed_project_f16(bf16)", a, n, n, 0, nullptr, bias, miss_row, (__bf16 *)out, out_stride, status, stream);
    return embed_folded_launch<_Float16>("embed_project_f16", a, n, n, 0, nullptr, bias, miss_row, (_Float16 *)out, out_stride, status, stream);
}

extern "C" size_t medtok_embed_codes_miss_grad_workspace_bytes(int64_t n, int width)
{
    if (n < 0 || width < 1) return 0;
    const size_t chunks = (size_t)((n + MEDTOK_EMBED_GRAD_CHUNK - 1) / MEDTOK_EMBED_GRAD_CHUNK);
    return (chunks * (size_t)width * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int medtok_embed_codes_miss_grad_f32(const float *g_out, int64_t g_stride, const int64_t *index, const uint8_t *pad, int64_t n,
                                                int64_t num_codes, int width, float *g_miss, void *ws, size_t ws_bytes, void *stream)
{
    if (n < 0 || width < 1) return fail("embed_codes_miss_grad: bad shape n=%ld width=%d", (long)n, width);
    if (g_stride == 0) g_stride = width;
    if (g_stride < width) return fail("embed_codes_miss_grad: g_stride must be >= width");
    if (!g_miss) return fail("embed_codes_miss_grad: g_miss is required");
    if (n > 0 && (!g_out || !index)) return fail("embed_codes_miss_grad: g_out and index are required");
    const long chunks = (long)((n + MEDTOK_EMBED_GRAD_CHUNK - 1) / MEDTOK_EMBED_GRAD_CHUNK);
    if (chunks > 0x7fffffffl) return fail("embed_codes_miss_grad: n=%ld positions exceed one launch", (long)n);
    if (chunks && (!ws || ws_bytes < medtok_embed_codes_miss_grad_workspace_bytes(n, width)))
        return fail("embed_codes_miss_grad: workspace too small (%zu bytes given)", ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    const unsigned col_blocks = (unsigned)((width + 255) / 256);
    if (chunks)
        hipLaunchKernelGGL(embed_miss_grad_partial_kernel, dim3((unsigned)chunks, col_blocks), dim3(256), 0, s, g_out, (long)g_stride, index, pad,
                           (long)n, (long)num_codes, width, (float *)ws);
    hipLaunchKernelGGL(embed_miss_grad_sum_kernel, dim3(col_blocks), dim3(256), 0, s, (const float *)ws, chunks, width, g_miss);
    return check_launch("embed_codes_miss_grad");
}

// ---- bag pooling: the normalised mean of the unpadded positions of each bag (embed_pool_*_kernel)
static size_t pool_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

extern "C" size_t medtok_embed_pool_workspace_bytes(int64_t bags, int64_t bag_len, int width)
{
    if (bags < 0 || bag_len < 0 || width < 1) return 0;
    const size_t blocks = (size_t)bags * (size_t)((bag_len + MEDTOK_EMBED_POOL_CHUNK - 1) / MEDTOK_EMBED_POOL_CHUNK);
    // partial sums [bags, chunks, width] fp32, then the chunks' (live, miss) counts [bags, chunks, 2] int32
    return pool_round(blocks * (size_t)width * sizeof(float)) + pool_round(blocks * 2 * sizeof(int));
}

extern "C" int medtok_embed_pool_f32(const int64_t *index, const uint8_t *pad, int64_t bags, int64_t bag_len, const int64_t *tokens,
                                     const float *weights, int64_t num_codes, int slots, int topk, const float *what, int64_t n_codes, int d,
                                     const int64_t *region_lo, const int64_t *region_size, const float *miss, int normalize, float *out,
                                     int64_t out_stride, int *counts, int *status, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "embed_pool";
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, what, n_codes, d, region_lo, region_size};
    DecodeRegions reg;
    if (bag_len < 0 || bag_len >= (1ll << 31)) return fail("%s: bag_len=%ld unsupported", fn, (long)bag_len);
    if (int rc = embed_args(fn, a, bags, true, reg)) return rc;
    const int64_t wide = (int64_t)slots * d;
    if (wide > MEDTOK_EMBED_POOL_MAX_WIDTH) return fail("%s: rows of slots * d = %ld floats exceed %d", fn, (long)wide, MEDTOK_EMBED_POOL_MAX_WIDTH);
    const int width = (int)wide;
    if (int rc = row_stride(fn, "out_stride", out_stride, width, "slots * d")) return rc;
    if (bags == 0) return 0;
    const int64_t chunks = (bag_len + MEDTOK_EMBED_POOL_CHUNK - 1) / MEDTOK_EMBED_POOL_CHUNK;
    // (one block per chunk in the first kernel, one per bag in the second)
    if (bags > kMaxBlocks || (chunks && bags > kMaxBlocks / chunks))
        return fail("%s: %ld bags x %ld chunks exceed one launch (%ld blocks of 256 threads)", fn, (long)bags, (long)chunks, (long)kMaxBlocks);
    if (!tokens || !weights || !what || !out || (bag_len > 0 && !index)) return fail("%s: index, tokens, weights, what and out are required", fn);
    const size_t need = medtok_embed_pool_workspace_bytes(bags, bag_len, width);
    if (need && (!ws || ws_bytes < need)) return fail("%s: workspace too small (%zu bytes given, %zu needed)", fn, ws_bytes, need);
    const size_t blocks = (size_t)(bags * chunks);
    float *partial = (float *)ws;
    int *chunk_counts = (int *)((char *)ws + pool_round(blocks * (size_t)width * sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    // (float4 per lane by the row's width: 4, 16, 48 or 64 floats)
    const int per_lane = width <= 256 ? 1 : width <= 1024 ? 4 : width <= 3072 ? 12 : 16;
    if (blocks)
        dispatch_group<1, 4, 12, 16>(per_lane, topk, [&](auto r, auto maxk) {
            hipLaunchKernelGGL((embed_pool_partial_kernel<decltype(r)::value, decltype(maxk)::value, false>), dim3((unsigned)blocks), dim3(256),
                               (size_t)width * sizeof(float), s, index, pad, (long)bag_len, (int)chunks, tokens, weights, (long)num_codes, slots,
                               topk, what, d, reg, miss, normalize, partial, chunk_counts, status, EmbedPoolList{});
        });
    hipLaunchKernelGGL(embed_pool_finish_kernel, dim3((unsigned)bags, (unsigned)((width + 1023) / 1024)), dim3(256), 0, s, (const float *)partial,
                       (const int *)chunk_counts, (int)chunks, width, out, (long)out_stride, counts, (const int *)nullptr);
    return check_launch(fn);
}

extern "C" int medtok_embed_pool_miss_grad_f32(const float *g_out, int64_t g_stride, const int *counts, int64_t bags, int width, float *g_acc,
                                               void *ws, size_t ws_bytes, void *stream)
{
    if (bags < 0 || width < 1) return fail("embed_pool_miss_grad: bad shape bags=%ld width=%d", (long)bags, width);
    if (g_stride == 0) g_stride = width;
    if (g_stride < width) return fail("embed_pool_miss_grad: g_stride must be >= width");
    if (!g_acc) return fail("embed_pool_miss_grad: g_acc is required");
    if (bags > 0 && (!g_out || !counts)) return fail("embed_pool_miss_grad: g_out and counts are required");
    const long chunks = (long)((bags + MEDTOK_EMBED_GRAD_CHUNK - 1) / MEDTOK_EMBED_GRAD_CHUNK);
    if (chunks > 0x7fffffffl) return fail("embed_pool_miss_grad: %ld bags exceed one launch", (long)bags);
    if (chunks && (!ws || ws_bytes < pool_round((size_t)chunks * (size_t)width * sizeof(float))))
        return fail("embed_pool_miss_grad: workspace too small (%zu bytes given)", ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    const unsigned col_blocks = (unsigned)((width + 255) / 256);
    if (chunks)
        hipLaunchKernelGGL(embed_pool_miss_grad_partial_kernel, dim3((unsigned)chunks, col_blocks), dim3(256), 0, s, g_out, (long)g_stride, counts,
                           (long)bags, width, (float *)ws);
    hipLaunchKernelGGL(embed_miss_grad_sum_kernel, dim3(col_blocks), dim3(256), 0, s, (const float *)ws, chunks, width, g_acc);
    return check_launch("embed_pool_miss_grad");
}

// ---- the consumer's input sequence behind the lookup: position rows, segment rows and prefix rows in the lookup's launch
#include "embed_sequence_kernels.h"

// the checks every medtok_embed_sequence_* entry shares: shapes and which parts are present, before any pointer of a tensor is looked at
static int sequence_parts(const char *fn, int64_t batch, int64_t len, int width, const float *position_rows, int64_t n_position_rows,
                          const int64_t *segment_id, const float *segment_rows0, const float *segment_rows1, int64_t n_segments,
                          const float *prefix, int64_t n_prefix, EmbedSeqParts &parts)
{
    if (batch < 0 || len < 0 || n_prefix < 0 || width < 1)
        return fail("%s: bad shape batch=%ld len=%ld n_prefix=%ld width=%d", fn, (long)batch, (long)len, (long)n_prefix, width);
    if (batch >= (1ll << 31) || len >= (1ll << 31) || n_prefix >= (1ll << 31) || batch * (n_prefix + len) >= (1ll << 31))
        return fail("%s: batch * (n_prefix + len) = %ld x (%ld + %ld) rows reach 2^31", fn, (long)batch, (long)n_prefix, (long)len);
    if (segment_rows1 && !segment_rows0) return fail("%s: segment_rows1 without segment_rows0", fn);
    if ((segment_id != nullptr) != (segment_rows0 != nullptr)) return fail("%s: segment_id and segment_rows0 come together", fn);
    if (segment_id && (n_segments < 1 || n_segments > MEDTOK_EMBED_SEQ_MAX_SEGMENTS))
        return fail("%s: n_segments=%ld unsupported (1 .. %d)", fn, (long)n_segments, MEDTOK_EMBED_SEQ_MAX_SEGMENTS);
    if (position_rows && n_position_rows < len)
        return fail("%s: position_rows holds %ld rows, fewer than len=%ld", fn, (long)n_position_rows, (long)len);
    if (batch > 0 && n_prefix > 0 && !prefix) return fail("%s: prefix is required for n_prefix=%ld", fn, (long)n_prefix);
    parts.position_rows = position_rows;
    parts.segment_id = segment_id;
    parts.segment_rows0 = segment_rows0;
    parts.segment_rows1 = segment_rows1;
    parts.prefix = n_prefix > 0 ? prefix : nullptr;
    parts.n_segments = segment_id ? (long)n_segments : 1;
    parts.n_prefix = (long)n_prefix;
    return 0;
}

// all output widths of medtok_embed_sequence_*: the parts, then the folded lookup's checks and launch
template <typename OUT>
static int embed_sequence_launch(const char *fn, const EmbedLookup &a, int64_t batch, int64_t len, const float *bias, const float *miss_row,
                                 const float *position_rows, int64_t n_position_rows, const int64_t *segment_id, const float *segment_rows0,
                                 const float *segment_rows1, int64_t n_segments, const float *prefix, int64_t n_prefix, OUT *out,
                                 int64_t out_stride, int *status, void *stream)
{
    EmbedSeqParts parts;
    if (int rc = sequence_parts(fn, batch, len, a.width, position_rows, n_position_rows, segment_id, segment_rows0, segment_rows1, n_segments,
                                prefix, n_prefix, parts))
        return rc;
    return embed_folded_launch<OUT>(fn, a, batch * len, batch * (n_prefix + len), len, &parts, bias, miss_row, out, out_stride, status, stream);
}

extern "C" int medtok_embed_sequence_f32(const int64_t *index, const uint8_t *pad, int64_t batch, int64_t len, const int64_t *tokens,
                                         const float *weights, int64_t num_codes, int slots, int topk, const float *table, int64_t n_rows,
                                         int hp, const int64_t *row_lo, const int64_t *row_size, const float *bias, const float *miss_row,
                                         const float *position_rows, int64_t n_position_rows, const int64_t *segment_id,
                                         const float *segment_rows0, const float *segment_rows1, int64_t n_segments, const float *prefix,
                                         int64_t n_prefix, float *out, int64_t out_stride, int *status, void *stream)
{
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, table, n_rows, hp, row_lo, row_size};
    return embed_sequence_launch<float>("embed_sequence", a, batch, len, bias, miss_row, position_rows, n_position_rows, segment_id, segment_rows0,
                                        segment_rows1, n_segments, prefix, n_prefix, out, out_stride, status, stream);
}

extern "C" int medtok_embed_sequence_f16(const int64_t *index, const uint8_t *pad, int64_t batch, int64_t len, const int64_t *tokens,
                                         const float *weights, int64_t num_codes, int slots, int topk, const float *table, int64_t n_rows,
                                         int hp, const int64_t *row_lo, const int64_t *row_size, const float *bias, const float *miss_row,
                                         const float *position_rows, int64_t n_position_rows, const int64_t *segment_id,
                                         const float *segment_rows0, const float *segment_rows1, int64_t n_segments, const float *prefix,
                                         int64_t n_prefix, void *out, int64_t out_stride, int bf16, int *status, void *stream)
{
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, table, n_rows, hp, row_lo, row_size};
    if (bf16)
        return embed_sequence_launch<__bf16>("embed_sequence_f16(bf16)", a, batch, len, bias, miss_row, position_rows, n_position_rows, segment_id,
                                             segment_rows0, segment_rows1, n_segments, prefix, n_prefix, (__bf16 *)out, out_stride, status, stream);
    return embed_sequence_launch<_Float16>("embed_sequence_f16", a, batch, len, bias, miss_row, position_rows, n_position_rows, segment_id,
                                           segment_rows0, segment_rows1, n_segments, prefix, n_prefix, (_Float16 *)out, out_stride, status, stream);
}

// both output widths of medtok_embed_sequence_rows_*: the epilogue over dense fp32 rows
template <typename OUT>
static int embed_sequence_rows_launch(const char *fn, const float *rows, const uint8_t *pad, int64_t batch, int64_t len, int width,
                                      const float *position_rows, int64_t n_position_rows, const int64_t *segment_id, const float *segment_rows0,
                                      const float *segment_rows1, int64_t n_segments, const float *prefix, int64_t n_prefix, OUT *out, int *status,
                                      void *stream)
{
    EmbedSeqParts parts;
    if (int rc = sequence_parts(fn, batch, len, width, position_rows, n_position_rows, segment_id, segment_rows0, segment_rows1, n_segments, prefix,
                                n_prefix, parts))
        return rc;
    const int64_t items = batch * (n_prefix + len);
    if (items == 0) return 0;
    if (!out || (len > 0 && !rows)) return fail("%s: rows and out are required", fn);
    const int vec = (width & 3) ? 1 : 4;
    const int64_t blocks = (items * (width / vec) + 255) / 256;   // items < 2^31, width < 2^31: no overflow
    if (blocks > kMaxBlocks) return fail("%s: %ld rows of %d exceed one launch (%ld blocks of 256 threads)", fn, (long)items, width, (long)kMaxBlocks);
    hipStream_t s = (hipStream_t)stream;
    if (vec == 4)
        hipLaunchKernelGGL((embed_sequence_rows_kernel<4, OUT>), dim3((unsigned)blocks), dim3(256), 0, s, rows, pad, (long)items, (long)len, width, parts,
                           out, status);
    else
        hipLaunchKernelGGL((embed_sequence_rows_kernel<1, OUT>), dim3((unsigned)blocks), dim3(256), 0, s, rows, pad, (long)items, (long)len, width, parts,
                           out, status);
    return check_launch(fn);
}

extern "C" int medtok_embed_sequence_rows_f32(const float *rows, const uint8_t *pad, int64_t batch, int64_t len, int width,
                                              const float *position_rows, int64_t n_position_rows, const int64_t *segment_id,
                                              const float *segment_rows0, const float *segment_rows1, int64_t n_segments, const float *prefix,
                                              int64_t n_prefix, float *out, int *status, void *stream)
{
    return embed_sequence_rows_launch<float>("embed_sequence_rows", rows, pad, batch, len, width, position_rows, n_position_rows, segment_id,
                                             segment_rows0, segment_rows1, n_segments, prefix, n_prefix, out, status, stream);
}

extern "C" int medtok_embed_sequence_rows_f16(const float *rows, const uint8_t *pad, int64_t batch, int64_t len, int width,
                                              const float *position_rows, int64_t n_position_rows, const int64_t *segment_id,
                                              const float *segment_rows0, const float *segment_rows1, int64_t n_segments, const float *prefix,
                                              int64_t n_prefix, void *out, int bf16, int *status, void *stream)
{
    if (bf16)
        return embed_sequence_rows_launch<__bf16>("embed_sequence_rows_f16(bf16)", rows, pad, batch, len, width, position_rows, n_position_rows,
                                                  segment_id, segment_rows0, segment_rows1, n_segments, prefix, n_prefix, (__bf16 *)out, status, stream);
    return embed_sequence_rows_launch<_Float16>("embed_sequence_rows_f16", rows, pad, batch, len, width, position_rows, n_position_rows, segment_id,
                                                segment_rows0, segment_rows1, n_segments, prefix, n_prefix, (_Float16 *)out, status, stream);
}

// the partial sums [batch, chunks, n_segments, width] fp32 of medtok_embed_sequence_segment_grad_f32; 0 for a shape the entry refuses
extern "C" size_t medtok_embed_sequence_grad_workspace_bytes(int64_t batch, int64_t len, int64_t n_segments, int width)
{
    if (batch < 0 || len < 0 || width < 1 || n_segments < 1 || n_segments > MEDTOK_EMBED_SEQ_MAX_SEGMENTS) return 0;
    if (batch >= (1ll << 31) || len >= (1ll << 31)) return 0;
    const size_t chunks = (size_t)((len + MEDTOK_EMBED_SEQ_GRAD_CHUNK - 1) / MEDTOK_EMBED_SEQ_GRAD_CHUNK);
    return ((size_t)batch * chunks * (size_t)n_segments * (size_t)width * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int medtok_embed_sequence_segment_grad_f32(const float *g, const uint8_t *pad, const int64_t *segment_id, int64_t batch, int64_t len,
                                                      int64_t n_prefix, int64_t n_segments, int width, float *g_segment, void *ws, size_t ws_bytes,
                                                      void *stream)
{
    const char *fn = "embed_sequence_segment_grad";
    if (n_segments < 1 || n_segments > MEDTOK_EMBED_SEQ_MAX_SEGMENTS)
        return fail("%s: n_segments=%ld unsupported (1 .. %d)", fn, (long)n_segments, MEDTOK_EMBED_SEQ_MAX_SEGMENTS);
    if (batch < 0 || len < 0 || n_prefix < 0 || width < 1)
        return fail("%s: bad shape batch=%ld len=%ld n_prefix=%ld width=%d", fn, (long)batch, (long)len, (long)n_prefix, width);
    if (batch >= (1ll << 31) || len >= (1ll << 31) || n_prefix >= (1ll << 31) || batch * (n_prefix + len) >= (1ll << 31))
        return fail("%s: batch * (n_prefix + len) = %ld x (%ld + %ld) rows reach 2^31", fn, (long)batch, (long)n_prefix, (long)len);
    if (batch == 0) return 0;
    if (!g_segment) return fail("%s: g_segment is required", fn);
    const int64_t chunks = (len + MEDTOK_EMBED_SEQ_GRAD_CHUNK - 1) / MEDTOK_EMBED_SEQ_GRAD_CHUNK;
    if (chunks && (!g || !segment_id)) return fail("%s: g and segment_id are required", fn);
    // the widest power-of-two column tile (4 .. 256) whose [n_segments][tile] accumulators fit 64 KiB of LDS, no wider than the rows need
    int tile = 256;
    while (tile > 4 && ((int64_t)n_segments * tile * 4 > 65536 || tile / 2 >= width)) tile /= 2;
    const int64_t col_blocks = (width + tile - 1) / tile;
    const int64_t total = batch * n_segments * (int64_t)width;
    if (batch * chunks > kMaxBlocks || col_blocks > 65535 || (total + 255) / 256 > kMaxBlocks)
        return fail("%s: batch=%ld x len=%ld x n_segments=%ld x width=%d exceed one launch", fn, (long)batch, (long)len, (long)n_segments, width);
    if (chunks && (!ws || ws_bytes < medtok_embed_sequence_grad_workspace_bytes(batch, len, n_segments, width)))
        return fail("%s: workspace too small (%zu bytes given)", fn, ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (chunks)
        hipLaunchKernelGGL(embed_sequence_segment_grad_partial_kernel, dim3((unsigned)(batch * chunks), (unsigned)col_blocks),
                           dim3(tile < 64 ? 64 : tile), (size_t)n_segments * tile * sizeof(float), s, g, pad, segment_id, (long)len, (int)chunks,
                           (long)n_prefix, (int)n_segments, width, tile, (float *)ws);
    hipLaunchKernelGGL(embed_sequence_segment_grad_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float *)ws, (long)total,
                       (int)chunks, (int)n_segments, width, g_segment);
    return check_launch(fn);
}

extern "C" int medtok_embed_sequence_position_grad_f32(const float *g, const uint8_t *pad, int64_t batch, int64_t len, int64_t n_prefix, int width,
                                                       int64_t n_position_rows, float *g_position, void *stream)
{
    const char *fn = "embed_sequence_position_grad";
    if (batch < 0 || len < 0 || n_prefix < 0 || width < 1 || n_position_rows < len)
        return fail("%s: bad shape batch=%ld len=%ld n_prefix=%ld width=%d n_position_rows=%ld", fn, (long)batch, (long)len, (long)n_prefix, width,
                    (long)n_position_rows);
    if (batch >= (1ll << 31) || len >= (1ll << 31) || n_prefix >= (1ll << 31) || batch * (n_prefix + len) >= (1ll << 31))
        return fail("%s: batch * (n_prefix + len) = %ld x (%ld + %ld) rows reach 2^31", fn, (long)batch, (long)n_prefix, (long)len);
    if (n_position_rows == 0) return 0;
    if (n_position_rows >= (1ll << 31)) return fail("%s: n_position_rows=%ld unsupported", fn, (long)n_position_rows);
    const int64_t total = n_position_rows * (int64_t)width;
    if ((total + 255) / 256 > kMaxBlocks) return fail("%s: %ld rows of %d exceed one launch", fn, (long)n_position_rows, width);
    if (!g_position || (batch > 0 && len > 0 && !g)) return fail("%s: g and g_position are required", fn);
    hipLaunchKernelGGL(embed_sequence_position_grad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, pad,
                       (long)batch, (long)len, (long)n_prefix, width, (long)total, g_position);
    return check_launch(fn);
}

// ================================================================= training half: sparse backward, normalize backward, InfoNCE
#include "train_kernels.h"

extern "C" int medtok_soft_vq_backward_f32(const float *x, const float *xhat, const float *what, const int64_t *idx, const float *w,
                                           int64_t n, int d, int topk, const float *g_zq, const float *g_xhat, const float *g_out,
                                           const float *g_vq, const float *g_commit, float vq_scale, float commit_scale,
                                           float *gx, float *g_code, void *stream)
{
    if (n < 0 || d <= 0 || (d & 3)) return fail("soft_vq_backward: bad shape n=%ld d=%d", (long)n, d);
    if (topk < 1 || topk > MEDTOK_MAX_TOPK) return fail("soft_vq_backward: topk=%d unsupported", topk);
    if (n == 0) return 0;
    if (!x || !xhat || !what || !idx || !w) return fail("soft_vq_backward: x, xhat, what, idx and w are required");
    if (!gx && !g_code) return fail("soft_vq_backward: nothing to compute (gx and g_code are both NULL)");
    if (topk <= 8)
        hipLaunchKernelGGL((soft_vq_backward_kernel<8>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       x, xhat, what, idx, w, (long)n, d, topk, g_zq, g_xhat, g_out, g_vq, g_commit, vq_scale, commit_scale, gx, g_code);
    else
        hipLaunchKernelGGL((soft_vq_backward_kernel<MEDTOK_MAX_TOPK>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       x, xhat, what, idx, w, (long)n, d, topk, g_zq, g_xhat, g_out, g_vq, g_commit, vq_scale, commit_scale, gx, g_code);
    return check_launch("soft_vq_backward");
}

extern "C" int medtok_normalize_backward_f32(const float *g, const float *vhat, const float *v, int64_t n, int d, float *out, void *stream)
{
    if (n < 0 || d <= 0 || (d & 3)) return fail("normalize_backward: bad shape n=%ld d=%d", (long)n, d);
    if (n == 0) return 0;
    if (!g || !vhat || !v || !out) return fail("normalize_backward: NULL argument");
    hipLaunchKernelGGL(normalize_backward_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, vhat, v, (long)n, d, out);
    return check_launch("normalize_backward");
}
// ... with `live` [n]: rows whose live entry is 0 hold an all-zero g (e.g. the bins of medtok_ema_stats_f32 for a code gradient): their
// output rows are written as zeros without reading g / vhat / v -- the same bits, a third of the traffic for a sparse g
extern "C" int medtok_normalize_backward_sparse_f32(const float *g, const float *vhat, const float *v, const float *live, int64_t n, int d, float *out,
                                                    void *stream)
{
    if (n < 0 || d <= 0 || (d & 3)) return fail("normalize_backward_sparse: bad shape n=%ld d=%d", (long)n, d);
    if (n == 0) return 0;
    if (!g || !vhat || !v || !live || !out) return fail("normalize_backward_sparse: NULL argument");
    hipLaunchKernelGGL(normalize_backward_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, vhat, v, (long)n, d, out, live);
    return check_launch("normalize_backward_sparse");
}

// rows per block of the InfoNCE kernels: sharing a fetched key row among 8 / 4 / 2 rows cuts the L2 traffic, but only once
// there are enough rows to keep >= 256 blocks (at the training batch of 256, one row per block: parallelism wins)
static int info_nce_rows(int64_t b, int d)
{
    for (int rt = 8; rt > 1; rt >>= 1)
        if (b / rt >= 256 && ((size_t)rt * ((size_t)b + (size_t)d) + 4) * sizeof(float) <= 64 * 1024) return rt;
    return 1;
}
static size_t info_nce_lds_bytes(int64_t b, int d, int rt) { return ((size_t)rt * ((size_t)b + (size_t)d) + 4) * sizeof(float); }

extern "C" size_t medtok_info_nce_workspace_bytes(int64_t b, int d)
{
    return (2 * (size_t)b * (size_t)d + (size_t)b) * sizeof(float);     // qhat | khat | row_loss
}

extern "C" int medtok_info_nce_forward_f32(const float *q, const float *k, int64_t b, int d, float temperature, float *loss, float *prob,
                                           void *ws, size_t ws_bytes, void *stream)
{
    if (b <= 0 || d <= 0 || (d & 3)) return fail("info_nce: bad shape b=%ld d=%d", (long)b, d);
    if (!(temperature > 0.f)) return fail("info_nce: temperature must be positive");
    if (!q || !k || !loss || !prob || !ws) return fail("info_nce: NULL argument");
    if (ws_bytes < medtok_info_nce_workspace_bytes(b, d)) return fail("info_nce: workspace too small");
    const int rt = info_nce_rows(b, d);
    if (info_nce_lds_bytes(b, d, rt) > 64 * 1024) return fail("info_nce: b + d = %ld exceeds the 64 KB LDS row budget", (long)(b + d));
    hipStream_t s = (hipStream_t)stream;
    float *qhat = (float *)ws, *khat = qhat + b * d, *row_loss = khat + b * d;
    hipLaunchKernelGGL(info_nce_prepare_kernel, dim3((unsigned)((2 * b + 3) / 4)), dim3(256), 0, s, q, k, (long)b, d, qhat, khat);
    const dim3 fgrid((unsigned)((b + rt - 1) / rt));
    const size_t lds = info_nce_lds_bytes(b, d, rt);
    switch (rt) {
    case 8: hipLaunchKernelGGL(info_nce_forward_kernel<8>, fgrid, dim3(NCE_THREADS), lds, s, qhat, khat, (int)b, d, 1.f / temperature, prob, row_loss); break;
    case 4: hipLaunchKernelGGL(info_nce_forward_kernel<4>, fgrid, dim3(NCE_THREADS), lds, s, qhat, khat, (int)b, d, 1.f / temperature, prob, row_loss); break;
    case 2: hipLaunchKernelGGL(info_nce_forward_kernel<2>, fgrid, dim3(NCE_THREADS), lds, s, qhat, khat, (int)b, d, 1.f / temperature, prob, row_loss); break;
    default: hipLaunchKernelGGL(info_nce_forward_kernel<1>, fgrid, dim3(NCE_THREADS), lds, s, qhat, khat, (int)b, d, 1.f / temperature, prob, row_loss); break;
    }
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(1024), 0, s, row_loss, (long)b, 1.0 / (double)b, loss);
    return check_launch("info_nce_forward");
}

extern "C" int medtok_info_nce_backward_f32(const float *q, const float *k, const float *prob, const float *g_loss, int64_t b, int d,
                                            float temperature, float *gq, float *gk, const void *ws, size_t ws_bytes, void *stream)
{
    if (b <= 0 || d <= 0 || (d & 3)) return fail("info_nce_backward: bad shape b=%ld d=%d", (long)b, d);
    if (!q || !k || !prob || !g_loss || !gq || !gk || !ws) return fail("info_nce_backward: NULL argument");
    if (ws_bytes < medtok_info_nce_workspace_bytes(b, d)) return fail("info_nce_backward: workspace too small");
    const int rt = info_nce_rows(b, d);
    if (info_nce_lds_bytes(b, d, rt) > 64 * 1024) return fail("info_nce_backward: b + d = %ld exceeds the 64 KB LDS row budget", (long)(b + d));
    const float *qhat = (const float *)ws, *khat = qhat + b * d;
    const dim3 bgrid((unsigned)(2 * ((b + rt - 1) / rt)));
    const size_t lds = info_nce_lds_bytes(b, d, rt);
    hipStream_t s = (hipStream_t)stream;
    switch (rt) {
    case 8: hipLaunchKernelGGL(info_nce_backward_kernel<8>, bgrid, dim3(NCE_THREADS), lds, s, q, k, qhat, khat, prob, g_loss, (int)b, d, 1.f / temperature, gq, gk); break;
    case 4: hipLaunchKernelGGL(info_nce_backward_kernel<4>, bgrid, dim3(NCE_THREADS), lds, s, q, k, qhat, khat, prob, g_loss, (int)b, d, 1.f / temperature, gq, gk); break;
    case 2: hipLaunchKernelGGL(info_nce_backward_kernel<2>, bgrid, dim3(NCE_THREADS), lds, s, q, k, qhat, khat, prob, g_loss, (int)b, d, 1.f / temperature, gq, gk); break;
    default: hipLaunchKernelGGL(info_nce_backward_kernel<1>, bgrid, dim3(NCE_THREADS), lds, s, q, k, qhat, khat, prob, g_loss, (int)b, d, 1.f / temperature, gq, gk); break;
    }
    return check_launch("info_nce_backward");
}

// ================================================================= alignment / orthogonality losses
#include "loss_kernels.h"

extern "C" int medtok_row_dot_f32(const float *a, const float *b, int64_t n, int d, float *out, void *stream)
{
    if (n < 0 || d <= 0 || (d & 3)) return fail("row_dot: bad shape n=%ld d=%d (d %% 4 == 0)", (long)n, d);
    if (n == 0) return 0;
    if (!a || !b || !out) return fail("row_dot: NULL argument");
    hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, b, (long)n, d, out);
    return check_launch("row_dot");
}

extern "C" int medtok_small_gemm_f32(const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbk, int64_t sbn, int m, int n, int k,
                                     float *C, void *stream)
{
    if (m <= 0 || n <= 0 || k <= 0) return fail("small_gemm: bad shape m=%d n=%d k=%d", m, n, k);
    if (!A || !B || !C) return fail("small_gemm: NULL argument");
    const long tiles = (long)((m + 31) / 32) * ((n + 31) / 32);
    // an operand that is contiguous along k, 16-byte aligned in every row: four consecutive k per load
    const bool av = sak == 1 && (sam & 3) == 0 && ((uintptr_t)A & 15) == 0, bv = sbk == 1 && (sbn & 3) == 0 && ((uintptr_t)B & 15) == 0;
#define MEDTOK_SMALL_GEMM(AV, BV)                                                                                                 \
    hipLaunchKernelGGL((small_gemm_f32_kernel<AV, BV>), dim3((unsigned)tiles), dim3(64), 0, (hipStream_t)stream, A, (long)sam,              \
                       (long)sak, B, (long)sbk, (long)sbn, m, n, k, C)
    if (av && bv) MEDTOK_SMALL_GEMM(true, true); else if (av) MEDTOK_SMALL_GEMM(true, false);
    else if (bv) MEDTOK_SMALL_GEMM(false, true); else MEDTOK_SMALL_GEMM(false, false);
#undef MEDTOK_SMALL_GEMM
    return check_launch("small_gemm");
}

extern "C" size_t medtok_frobenius_workspace_bytes(int64_t rows) { return rows > 0 ? align_up((size_t)rows * 4, 256) : 256; }

extern "C" int medtok_frobenius_f32(const float *x, int64_t rows, int d, float *out, void *ws, size_t ws_bytes, void *stream)
{
    if (rows <= 0 || d <= 0 || (d & 3)) return fail("frobenius: bad shape rows=%ld d=%d (d %% 4 == 0)", (long)rows, d);
    if (!x || !out || !ws || ws_bytes < (size_t)rows * 4) return fail("frobenius: NULL argument or workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *sq = (float *)ws;
    launch_rownorm<false>(s, x, (long)rows, d, (float *)nullptr, sq);
    hipLaunchKernelGGL(frobenius_kernel, dim3(1), dim3(1024), 0, s, sq, (long)rows, out);
    return check_launch("frobenius");
}

extern "C" int medtok_scale_by_device_scalar_f32(const float *x, int64_t count, const float *num, const float *den, float c, float *out,
                                                 void *stream)
{
    if (count < 0 || !x || !num || !out) return fail("scale_by_device_scalar: bad arguments");
    if (count == 0) return 0;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) return fail("scale_by_device_scalar: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(scale_by_device_scalar_kernel, dim3((unsigned)lmin(2048, (count + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream,
                       x, (long)count, num, den, c, out);
    return check_launch("scale_by_device_scalar");
}

// ================================================================= cross-attention core (ragged, shared key/value rows)
#include "attention_kernels.h"

#include "attention_backward.h"
#include "attention_dma.h"
#include "attention_pp.h"
#include "attention_small.h"
#include "pack_kernels.h"

static int attention_shape_ok(int d) { return d == 64 || (d > 0 && d % 128 == 0 && d <= 768); }

// forward, shared by the inference and the training entry point
static int attention_forward(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv, const int64_t *kv_start,
                             const int64_t *kv_len, int64_t n_codes, int64_t max_q_len, int d, float scale, float *out, float *lse,
                             float dropout_p, unsigned seed, hipStream_t s)
{
    const int64_t q_tiles = (max_q_len + 31) / 32;
    if (q_tiles * n_codes >= (1ll << 31)) return fail("shared_kv_attention: n_codes * ceil(max_q_len / 32) = %ld exceeds the grid limit", (long)(q_tiles * n_codes));
    const dim3 grid((unsigned)(q_tiles * n_codes));
    hipEvent_t pa = prof_wanted(2) ? prof_mark(s) : nullptr;
    const int waves = d == 64 ? 2 : (d % 256 == 0 ? 8 : 4);
    const size_t lds = ((size_t)32 * (d + 4 * waves) + (waves + 1) * 32 * 33 + 64) * sizeof(float);   // key chunk (one padded column slice per wave) + per-wave partial scores + probabilities + row state
    const unsigned thresh = dropout_p > 0.f ? (unsigned)fmin(4294967295.0, (double)dropout_p * 4294967296.0) : 0u;
    const float keep_scale = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
#define MEDTOK_ATT(W, NT)                                                                                                        \
    do {                                                                                                                         \
        if (lds > 64 * 1024 && !set_lds_once<shared_kv_attention_kernel<W, NT>>(lds))                                            \
            return fail("shared_kv_attention: cannot reserve %zu bytes of LDS", lds);                                            \
        hipLaunchKernelGGL((shared_kv_attention_kernel<W, NT>), grid, dim3(64 * W), lds, s, q, q_start, q_len, kv, kv_start, kv_len, scale, out, \
                           (int)q_tiles, lse, thresh, seed, keep_scale);                                                        \
    } while (0)
    switch (d / 128) {
    case 0: MEDTOK_ATT(2, 1); break;      // d = 64, the reference's default e_dim
    case 1: MEDTOK_ATT(4, 1); break;
    case 2: MEDTOK_ATT(8, 1); break;
    case 3: MEDTOK_ATT(4, 3); break;
    case 4: MEDTOK_ATT(8, 2); break;
    case 5: MEDTOK_ATT(4, 5); break;
    default: MEDTOK_ATT(8, 3); break;
    }
#undef MEDTOK_ATT
    if (pa) prof_push(pa, prof_mark(s), 0.0, 2);      // the row / key counts live on the device: the caller prices the launch
    return check_launch("shared_kv_attention");
}

static int attention_forward_f16s(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv, const int64_t *kv_start,
                                  const int64_t *kv_len, int64_t n_codes, int64_t max_q_len, int d, float scale, float *out, _Float16 *out_h,
                                  _Float16 *out_l, hipStream_t s)
{
    const int64_t q_tiles = (max_q_len + 31) / 32;
    if (q_tiles * n_codes >= (1ll << 31)) return fail("shared_kv_attention: n_codes * ceil(max_q_len / 32) = %ld exceeds the grid limit", (long)(q_tiles * n_codes));
    const dim3 grid((unsigned)(q_tiles * n_codes));
    hipEvent_t pa = prof_wanted(2) ? prof_mark(s) : nullptr;
    if (max_q_len <= 8) {
        // a few query rows per code (the text side: one row per head): one wavefront per code, plain fp32 (attention_kernels.h)
        const dim3 fgrid((unsigned)((n_codes + 3) / 4));
        if (d > 768) {          // (D = 1024, e.g. BERT-large text features: four column chunks per lane; at most 4 query rows fit the registers)
            if (max_q_len > 4) return fail("shared_kv_attention: d=%d takes at most 4 query rows per code on this path (heads <= 4)", d);
            hipLaunchKernelGGL((shared_kv_attention_fewq_kernel<4, 4>), fgrid, dim3(256), 0, s, q, q_start, q_len, kv, kv_start, kv_len, (long)n_codes, d, scale,
                               out, out_h, out_l);
        } else if (max_q_len <= 4)
            hipLaunchKernelGGL(shared_kv_attention_fewq_kernel<4>, fgrid, dim3(256), 0, s, q, q_start, q_len, kv, kv_start, kv_len, (long)n_codes, d, scale,
                               out, out_h, out_l);
        else
            hipLaunchKernelGGL(shared_kv_attention_fewq_kernel<8>, fgrid, dim3(256), 0, s, q, q_start, q_len, kv, kv_start, kv_len, (long)n_codes, d, scale,
                               out, out_h, out_l);
        if (pa) prof_push(pa, prof_mark(s), 0.0, 2);
        return check_launch("shared_kv_attention(few rows)");
    }
    if (d > 768) return fail("shared_kv_attention: d=%d with more than 8 query rows per code runs on the image form (medtok_shared_kv_attention_split_f32)", d);
    const int waves = d == 64 ? 2 : (d % 256 == 0 ? 8 : 4);
    // (hi, lo) key planes of W slices, 32 keys x (d / W + 8) halves each; per-wave partial scores; probabilities (hi, lo); row state
    const size_t lds = (size_t)waves * 2 * 32 * (d / waves + 8) * 2 + (size_t)waves * 32 * 33 * 4 + 2 * 32 * 40 * 2 + 64 * 4;
#define MEDTOK_ATT16(W, NT)                                                                                                      \
    do {                                                                                                                         \
        if (lds > 64 * 1024 && !set_lds_once<shared_kv_attention_f16s_kernel<W, NT>>(lds))                                       \
            return fail("shared_kv_attention: cannot reserve %zu bytes of LDS", lds);                                            \
        hipLaunchKernelGGL((shared_kv_attention_f16s_kernel<W, NT>), grid, dim3(64 * W), lds, s, q, q_start, q_len, kv, kv_start, kv_len, scale, \
                           out, out_h, out_l, (int)q_tiles);                                                                     \
    } while (0)
    switch (d / 128) {
    case 0: MEDTOK_ATT16(2, 1); break;
    case 1: MEDTOK_ATT16(4, 1); break;
    case 2: MEDTOK_ATT16(8, 1); break;
    case 3: MEDTOK_ATT16(4, 3); break;
    case 4: MEDTOK_ATT16(8, 2); break;
    case 5: MEDTOK_ATT16(4, 5); break;
    default: MEDTOK_ATT16(8, 3); break;
    }
#undef MEDTOK_ATT16
    if (pa) prof_push(pa, prof_mark(s), 0.0, 2);
    return check_launch("shared_kv_attention(f16 x 3)");
}

// 64-row blocks, keys from (hi, lo) fp16 images by LDS-DMA (attention_dma.h)
static bool attention_dma_shape_ok(int d) { return d == 128 || d == 256 || d == 384 || d == 512 || d == 768 || d == 1024; }

extern "C" int medtok_shared_kv_attention_split_f32(const float *q, const int64_t *q_start, const int64_t *q_len, const void *kv_hi, const void *kv_lo,
                                                    const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                                    int d, float scale, float *out, void *out_hi, void *out_lo, int variant, void *stream)
{
    if ((out_hi == nullptr) != (out_lo == nullptr)) return fail("shared_kv_attention_split: out_hi and out_lo go together");
    if (n_codes < 0 || max_q_len < 0) return fail("shared_kv_attention_split: bad sizes n_codes=%ld max_q_len=%ld", (long)n_codes, (long)max_q_len);
    if (!attention_dma_shape_ok(d)) return fail("shared_kv_attention_split: d=%d must be 128, 256, 384, 512, 768 or 1024", d);
    if (n_codes == 0 || max_q_len == 0) return 0;
    const int vform = variant & 15;
    const bool pp_shape = vform == 2 && (d == 256 || d == 512 || d == 768);
    // MEDTOK_ATTENTION_F32_KEYS: kv_hi points at the caller's fp32 key rows, which the kernel turns into their (hi, lo) images itself
    const bool f32_keys = (variant & MEDTOK_ATTENTION_F32_KEYS) != 0;
    if (f32_keys && !pp_shape) return fail("shared_kv_attention_split: fp32 keys converted in the kernel need variant 2 and d = 256, 512 or 768");
    if (!q || !q_start || !q_len || !kv_hi || !kv_start || !kv_len || (!out && !out_hi)) return fail("shared_kv_attention_split: NULL argument");
    if (!kv_lo && !f32_keys && !pp_shape) return fail("shared_kv_attention_split: keys without a lo image (fp16 keys as they stand) need variant 2 and d = 256, 512 or 768");
    if (((uintptr_t)q | (uintptr_t)kv_hi | (uintptr_t)kv_lo | (uintptr_t)out) & 15) return fail("shared_kv_attention_split: pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pa = prof_wanted(2) ? prof_mark(s) : nullptr;
#define MEDTOK_ATT_DMA(W, NT, MT, RING)                                                                                          \
    do {                                                                                                                         \
        const size_t lds = AttDma<W, NT, MT, RING>::LDS_BYTES;                                                                   \
        const int64_t q_tiles = (max_q_len + 32 * MT - 1) / (32 * MT);                                                           \
        if (q_tiles * (n_codes + 8) >= (1ll << 31)) return fail("shared_kv_attention_split: grid limit exceeded");                \
        if (lds > 64 * 1024 && !set_lds_once<shared_kv_attention_dma_kernel<W, NT, MT, RING>>(lds))                              \
            return fail("shared_kv_attention_split: cannot reserve %zu bytes of LDS", lds);                                      \
        hipLaunchKernelGGL((shared_kv_attention_dma_kernel<W, NT, MT, RING>), dim3((unsigned)(q_tiles * ((n_codes + 7) / 8 * 8))), dim3(64 * W), \
                           lds, s, q, q_start, q_len, (const _Float16 *)kv_hi, (const _Float16 *)kv_lo, kv_start, kv_len, scale, out, \
                           (_Float16 *)out_hi, (_Float16 *)out_lo, (int)q_tiles, (int)n_codes);                                  \
    } while (0)
    if (pp_shape) {
        // two 32-row tiles of a code per block, run one phase apart on one copy of the keys (attention_pp.h)
        const int64_t q_pairs = (max_q_len + 63) / 64;
        if (q_pairs * (n_codes + 8) >= (1ll << 31)) return fail("shared_kv_attention_split: grid limit exceeded");
#define MEDTOK_ATT_PP(NT, KLO, ...)                                                                                                \
    do {                                                                                                                          \
        const size_t lds = AttPP<NT>::LDS_BYTES;                                                                                  \
        if (!set_lds_once<shared_kv_attention_pp_kernel<NT, KLO __VA_ARGS__>>(lds)) return fail("shared_kv_attention_split: cannot reserve %zu bytes of LDS", lds); \
        hipLaunchKernelGGL((shared_kv_attention_pp_kernel<NT, KLO __VA_ARGS__>), dim3((unsigned)(q_pairs * ((n_codes + 7) / 8 * 8))), dim3(512), lds, s, q, q_start, \
                           q_len, (const _Float16 *)kv_hi, (const _Float16 *)kv_lo, kv_start, kv_len, scale, out, (_Float16 *)out_hi,             \
                           (_Float16 *)out_lo, (int)q_pairs, (int)n_codes);                                                        \
    } while (0)
        if (f32_keys) { if (d == 256) MEDTOK_ATT_PP(2, true, , true); else if (d == 512) MEDTOK_ATT_PP(4, true, , true); else MEDTOK_ATT_PP(6, true, , true); }
        else if (!kv_lo) { if (d == 256) MEDTOK_ATT_PP(2, false); else if (d == 512) MEDTOK_ATT_PP(4, false); else MEDTOK_ATT_PP(6, false); }
        else if (d == 256) MEDTOK_ATT_PP(2, true); else if (d == 512) MEDTOK_ATT_PP(4, true);
        else MEDTOK_ATT_PP(6, true);
#undef MEDTOK_ATT_PP
        if (pa) prof_push(pa, prof_mark(s), 0.0, 2);
        return check_launch("shared_kv_attention_split(pp)");
    }
    switch (d) {
    case 128: MEDTOK_ATT_DMA(4, 1, 2, 2); break;
    case 256: MEDTOK_ATT_DMA(8, 1, 2, 2); break;
    case 384: MEDTOK_ATT_DMA(4, 3, 2, 2); break;
    case 512: MEDTOK_ATT_DMA(8, 2, 2, 2); break;
    case 1024: MEDTOK_ATT_DMA(4, 8, 1, 2); break;      // (BERT-large width: 32 rows per block, one wave per SIMD with 512 registers, two-deep ring)
    default:                               // 768: variant 0 = 32 rows per block, two blocks per CU; 1 = 64 rows per block, one per CU
        if (variant == 1) MEDTOK_ATT_DMA(8, 3, 2, 2); else MEDTOK_ATT_DMA(4, 6, 1, 1);
        break;
    }
#undef MEDTOK_ATT_DMA
    if (pa) prof_push(pa, prof_mark(s), 0.0, 2);
    return check_launch("shared_kv_attention_split");
}

extern "C" int medtok_shared_kv_attention_f32(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv,
                                              const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                              int d, float scale, float *out, void *out_hi, void *out_lo, int exact_f32, void *stream)
{
    if ((out_hi == nullptr) != (out_lo == nullptr)) return fail("shared_kv_attention: out_hi and out_lo go together");
    if (exact_f32 && out_hi) return fail("shared_kv_attention: the (hi, lo) output images come from the inference kernels (exact_f32 = 0)");
    if (!out && !out_hi && n_codes > 0 && max_q_len > 0) return fail("shared_kv_attention: no output buffer");
    if (n_codes < 0 || max_q_len < 0) return fail("shared_kv_attention: bad sizes n_codes=%ld max_q_len=%ld", (long)n_codes, (long)max_q_len);
    // (d = 1024: the inference form only, with at most 4 query rows per code -- the text side's CLS row per head; wider query sets
    // run on medtok_shared_kv_attention_split_f32; the exact fp32 kernel's 32-key chunk of fp32 rows does not fit the LDS there)
    if (!attention_shape_ok(d) && !(d == 1024 && !exact_f32)) return fail("shared_kv_attention: d=%d must be 64 or a multiple of 128, at most 768 (1024: inference only)", d);
    if (n_codes == 0 || max_q_len == 0) return 0;
    if (!q || !q_start || !q_len || !kv || !kv_start || !kv_len) return fail("shared_kv_attention: NULL argument");
    if (!exact_f32) return attention_forward_f16s(q, q_start, q_len, kv, kv_start, kv_len, n_codes, max_q_len, d, scale, out, (_Float16 *)out_hi,
                                                  (_Float16 *)out_lo, (hipStream_t)stream);
    return attention_forward(q, q_start, q_len, kv, kv_start, kv_len, n_codes, max_q_len, d, scale, out, nullptr, 0.f, 0u, (hipStream_t)stream);
}

// CrossAttention.pooled at e_dim = 64, 4 heads (the reference's default shape) in two launches (attention_small.h)
static int cross_attention_small_impl(bool exact, const float *text, const void *mask, int mask_elem_bytes, int64_t n_codes, int64_t seq_len,
                                                const float *nodes, const int64_t *batch, int64_t n_nodes, int d, int heads, int layers,
                                                const float *weights, float scale, float ln_eps, float *y_nodes, float *pooled,
                                                int64_t pooled_stride, int64_t graph_off, int32_t *status, void *stream)
{
    if (d != XS_D || heads != XS_H) return fail("cross_attention_small: d=%d heads=%d (this path is e_dim = 64 with 4 heads)", d, heads);
    if (n_codes < 0 || seq_len <= 0 || n_nodes < 0 || layers <= 0) return fail("cross_attention_small: bad sizes n_codes=%ld seq_len=%ld n_nodes=%ld layers=%d", (long)n_codes, (long)seq_len, (long)n_nodes, layers);
    if (mask_elem_bytes != 1 && mask_elem_bytes != 4 && mask_elem_bytes != 8) return fail("cross_attention_small: mask elements of %d bytes (bool / int32 / int64 expected)", mask_elem_bytes);
    if (n_codes == 0) return 0;
    if (!text || !mask || !weights || !pooled || !status || (n_nodes && (!nodes || !batch || !y_nodes))) return fail("cross_attention_small: NULL argument");
    if (((uintptr_t)text | (uintptr_t)nodes | (uintptr_t)weights | (uintptr_t)y_nodes) & 15) return fail("cross_attention_small: pointers must be 16-byte aligned");
    if (pooled_stride < XS_D || graph_off < 0) return fail("cross_attention_small: bad output layout");
    const int64_t tiles = (n_nodes + XS_G - 1) / XS_G;
    if (tiles + n_codes >= (1ll << 31)) return fail("cross_attention_small: grid limit exceeded");
    XSmallArgs a;
    a.text = text; a.mask = mask; a.nodes = nodes; a.batch = batch; a.weights = weights; a.y_nodes = y_nodes; a.pooled = pooled; a.status = status;
    a.n_codes = (long)n_codes; a.seq_len = (long)seq_len; a.n_nodes = (long)n_nodes; a.pooled_stride = (long)pooled_stride; a.graph_off = (long)graph_off;
    a.mask_bytes = mask_elem_bytes; a.layers = layers; a.n_graph_tiles = (int)tiles; a.scale = scale; a.ln_eps = ln_eps;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pa = prof_wanted(2) ? prof_mark(s) : nullptr;
    if (exact) hipLaunchKernelGGL(cross_attention64_kernel<false>, dim3((unsigned)(tiles + n_codes)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(cross_attention64_kernel<true>, dim3((unsigned)(tiles + n_codes)), dim3(256), 0, s, a);
    if (pa) prof_push(pa, prof_mark(s), 0.0, 2);
    hipLaunchKernelGGL(cross_attention64_mean_kernel, dim3((unsigned)((n_codes + 3) / 4)), dim3(256), 0, s, y_nodes, batch, (long)n_nodes, (long)n_codes,
                       pooled, (long)pooled_stride, (long)graph_off);
    return check_launch("cross_attention_small");
}

extern "C" int medtok_cross_attention_small_f32(const float *text, const void *mask, int mask_elem_bytes, int64_t n_codes, int64_t seq_len,
                                                const float *nodes, const int64_t *batch, int64_t n_nodes, int d, int heads, int layers,
                                                const float *weights, float scale, float ln_eps, float *y_nodes, float *pooled,
                                                int64_t pooled_stride, int64_t graph_off, int32_t *status, void *stream)
{
    return cross_attention_small_impl(false, text, mask, mask_elem_bytes, n_codes, seq_len, nodes, batch, n_nodes, d, heads, layers, weights, scale, ln_eps,
                                      y_nodes, pooled, pooled_stride, graph_off, status, stream);
}

// Test hook: the same call with the attention core on the fp32 matrix pipe (exact fmaf chains; the round-5 form) -- a second opinion
// on the split-fp16 core that the product runs
extern "C" int medtok_debug_cross_attention_small_exact_f32(const float *text, const void *mask, int mask_elem_bytes, int64_t n_codes, int64_t seq_len,
                                                            const float *nodes, const int64_t *batch, int64_t n_nodes, int d, int heads, int layers,
                                                            const float *weights, float scale, float ln_eps, float *y_nodes, float *pooled,
                                                            int64_t pooled_stride, int64_t graph_off, int32_t *status, void *stream)
{
    return cross_attention_small_impl(true, text, mask, mask_elem_bytes, n_codes, seq_len, nodes, batch, n_nodes, d, heads, layers, weights, scale, ln_eps,
                                      y_nodes, pooled, pooled_stride, graph_off, status, stream);
}

// the prologue of CrossAttention.pooled (pack_kernels.h)
extern "C" size_t medtok_pack_codes_workspace_bytes(int64_t n_codes)
{
    return align_up((size_t)(n_codes > 0 ? n_codes : 1) * 4, 256) * 2 + 256;        // counts32 | order | stats32
}

extern "C" int medtok_pack_codes_checked(const void *mask, int mask_elem_bytes, int64_t n_codes, int64_t seq_len, const int64_t *batch, int64_t n_nodes,
                                         int heads, int lpt, int64_t *valid_len, int64_t *counts, int64_t *starts, int64_t *t_start, int64_t *t_len,
                                         int64_t *g_start, int64_t *g_len, int64_t *tok_start, int64_t *g_kv_len, int64_t *stats,
                                         int64_t count_bound, int *status, void *ws, size_t ws_bytes, void *stream)
{
    if (count_bound < 0) return fail("pack_codes: count_bound=%ld must be >= 0 (0 = none)", (long)count_bound);
    if (n_codes <= 0 || seq_len < 0 || n_nodes < 0 || heads <= 0) return fail("pack_codes: bad sizes n_codes=%ld seq_len=%ld n_nodes=%ld heads=%d", (long)n_codes, (long)seq_len, (long)n_nodes, heads);
    if (n_codes >= (1ll << 31) - 1 || n_nodes >= (1ll << 31) * 256ll) return fail("pack_codes: too many codes / nodes");
    if (mask_elem_bytes != 1 && mask_elem_bytes != 4 && mask_elem_bytes != 8) return fail("pack_codes: mask elements of %d bytes (bool / int32 / int64 expected)", mask_elem_bytes);
    if (!mask || (!batch && n_nodes) || !valid_len || !counts || !starts || !t_start || !t_len || !g_start || !g_len || !tok_start || !g_kv_len || !stats)
        return fail("pack_codes: NULL argument");
    const size_t need = medtok_pack_codes_workspace_bytes(n_codes);
    if (!ws || ws_bytes < need) return fail("pack_codes: workspace too small (%zu < %zu)", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const size_t seg = align_up((size_t)n_codes * 4, 256);
    int *counts32 = (int *)ws, *order = (int *)((char *)ws + seg), *stats32 = (int *)((char *)ws + 2 * seg);
    const unsigned mgrid = (unsigned)((n_codes + 3) / 4);
    if (mask_elem_bytes == 1) hipLaunchKernelGGL(pack_mask_len_kernel<uint8_t>, dim3(mgrid), dim3(256), 0, s, (const uint8_t *)mask, (long)n_codes, (long)seq_len, valid_len, counts32, stats32);
    else if (mask_elem_bytes == 4) hipLaunchKernelGGL(pack_mask_len_kernel<int32_t>, dim3(mgrid), dim3(256), 0, s, (const int32_t *)mask, (long)n_codes, (long)seq_len, valid_len, counts32, stats32);
    else hipLaunchKernelGGL(pack_mask_len_kernel<int64_t>, dim3(mgrid), dim3(256), 0, s, (const int64_t *)mask, (long)n_codes, (long)seq_len, valid_len, counts32, stats32);
    if (n_nodes > 0)
        hipLaunchKernelGGL(pack_count_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, batch, (long)n_nodes, (long)n_codes, counts32, stats32);
    const bool sort = lpt && seq_len < PACK_MAX_KEYS && n_codes <= PACK_SORT_MAX_CODES;
    size_t pw = 1;
    while ((int64_t)pw < n_codes) pw <<= 1;
    hipLaunchKernelGGL(pack_lists_kernel, dim3(1), dim3(PACK_THREADS), sort ? pw * 4 : 0, s, counts32, stats32, valid_len, (long)n_codes,
                       (long)seq_len, heads, lpt, order, counts, starts, t_start, t_len, g_start, g_len, tok_start, g_kv_len, stats, (long)count_bound, status);
    return check_launch("pack_codes");
}

extern "C" int medtok_pack_codes(const void *mask, int mask_elem_bytes, int64_t n_codes, int64_t seq_len, const int64_t *batch, int64_t n_nodes,
                                 int heads, int lpt, int64_t *valid_len, int64_t *counts, int64_t *starts, int64_t *t_start, int64_t *t_len,
                                 int64_t *g_start, int64_t *g_len, int64_t *tok_start, int64_t *g_kv_len, int64_t *stats, void *ws, size_t ws_bytes,
                                 void *stream)
{
    return medtok_pack_codes_checked(mask, mask_elem_bytes, n_codes, seq_len, batch, n_nodes, heads, lpt, valid_len, counts, starts, t_start, t_len,
                                     g_start, g_len, tok_start, g_kv_len, stats, 0, nullptr, ws, ws_bytes, stream);
}

// the layer tail and the node mean around the attention core (attention_kernels.h)
extern "C" int medtok_residual_layernorm_split_f32(const float *a, const float *b, const float *gamma, const float *beta, int64_t n, int d,
                                                   float eps, float *y, void *y_hi, void *y_lo, int dp, void *stream)
{
    if (n < 0 || d <= 0 || d % 4 != 0 || d > 4 * 64 * LN_MAXV) return fail("residual_layernorm: bad shape n=%ld d=%d (d %% 4 == 0, d <= %d)", (long)n, d, 4 * 64 * LN_MAXV);
    if (!(eps >= 0.f)) return fail("residual_layernorm: eps=%g must be >= 0", (double)eps);
    if ((y_hi == nullptr) != (y_lo == nullptr)) return fail("residual_layernorm: y_hi and y_lo go together");
    if (y_hi && (dp < d || dp % 8 != 0 || dp > 4 * 64 * LN_MAXV)) return fail("residual_layernorm: image width dp=%d (>= d, a multiple of 8)", dp);
    if (n == 0) return 0;
    if (!a || !b || !gamma || !beta || !y) return fail("residual_layernorm: NULL argument");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y | (uintptr_t)y_hi | (uintptr_t)y_lo) & 15) return fail("residual_layernorm: pointers must be 16-byte aligned");
    if ((n + 3) / 4 >= (1ll << 31)) return fail("residual_layernorm: too many rows");
    if (y_hi)
        hipLaunchKernelGGL(residual_layernorm_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, b, gamma, beta, (long)n, d, eps, y,
                           (_Float16 *)y_hi, (_Float16 *)y_lo, dp);
    else
        hipLaunchKernelGGL(residual_layernorm_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, b, gamma, beta, (long)n, d, eps, y,
                           (_Float16 *)nullptr, (_Float16 *)nullptr, 0);
    return check_launch("residual_layernorm");
}

extern "C" int medtok_residual_layernorm_f32(const float *a, const float *b, const float *gamma, const float *beta, int64_t n, int d,
                                             float eps, float *y, void *stream)
{
    return medtok_residual_layernorm_split_f32(a, b, gamma, beta, n, d, eps, y, nullptr, nullptr, 0, stream);
}

// One CrossAttentionLayer at inference in ONE call: the seven launches of CrossAttention._folded_rows_split (rows -> images ->
// in_proj -> per-head fold -> attention core -> per-head W_v -> out_proj -> residual + LayerNorm), composed from the entry points
// above with the intermediates in caller-provided scratch.  Same kernels, same arguments, same bits as the seven separate calls;
// what it saves is the host side of six of them (a B = 256 forward is host-bound: ~55 calls of ~15 us against 0.45 ms of kernels).
extern "C" size_t medtok_cross_attention_layer_workspace_bytes(int64_t n_rows, int d, int dw, int heads, int hp)
{
    const size_t r = (size_t)(n_rows > 0 ? n_rows : 1);
    return 2 * align_up(r * dw * 2, 256) + 2 * align_up(r * heads * hp * 2, 256) + align_up(r * heads * dw * 4, 256) +
           2 * align_up(r * heads * dw * 2, 256) + 2 * align_up(r * heads * hp * 2, 256) + align_up(r * d * 4, 256);
}

extern "C" int medtok_cross_attention_layer_f32(
    const float *rows, const void *rows_hi, const void *rows_lo, int64_t n_rows, int d, int dw, int heads, int hp,
    const void *wq_hi, const void *wq_lo, float wq_unscale, const float *bq, const void *wk_hi, const void *wk_lo, float wk_unscale,
    const void *wv_hi, const void *wv_lo, float wv_unscale, const float *bv, const void *wo_hi, const void *wo_lo, float wo_unscale, const float *bo,
    const int64_t *q_start, const int64_t *q_len, int64_t n_codes, int64_t max_q_len, const float *kv, const void *kv_hi, const void *kv_lo,
    const int64_t *kv_start, const int64_t *kv_len, float scale, int variant, const float *ln_gamma, const float *ln_beta, float ln_eps,
    float *y, void *y_hi, void *y_lo, void *ws, size_t ws_bytes, void *stream)
{
    if (n_rows < 0 || d <= 0 || dw < d || heads <= 0 || hp <= 0) return fail("cross_attention_layer: bad shape n_rows=%ld d=%d dw=%d heads=%d hp=%d", (long)n_rows, d, dw, heads, hp);
    if (n_rows == 0) return 0;
    const size_t need = medtok_cross_attention_layer_workspace_bytes(n_rows, d, dw, heads, hp);
    if (!ws || ws_bytes < need) return fail("cross_attention_layer: workspace too small (%zu < %zu)", ws_bytes, need);
    if (!rows || !y || (!kv && !kv_hi)) return fail("cross_attention_layer: NULL argument");
    char *p = (char *)ws;
    auto take = [&](size_t bytes) { char *q = p; p += align_up(bytes, 256); return (void *)q; };
    const size_t r = (size_t)n_rows;
    void *x_hi = take(r * dw * 2), *x_lo = take(r * dw * 2);
    void *q_hi = take(r * heads * hp * 2), *q_lo = take(r * heads * hp * 2);
    float *qf = (float *)take(r * heads * dw * 4);
    void *c_hi = take(r * heads * dw * 2), *c_lo = take(r * heads * dw * 2);
    void *a_hi = take(r * heads * hp * 2), *a_lo = take(r * heads * hp * 2);
    float *o = (float *)take(r * d * 4);
    if (rows_hi && rows_lo) { x_hi = (void *)rows_hi; x_lo = (void *)rows_lo; }
    else if (medtok_split_half_f32(rows, n_rows, d, d, dw, 1.0f, x_hi, x_lo, nullptr, 0, stream)) return 1;
    if (medtok_split_gemm_f16(x_hi, x_lo, n_rows, dw, 0, wq_hi, wq_lo, (int64_t)heads * hp, dw, 0, heads * hp, dw, 1, bq, wq_unscale, nullptr, 0, q_hi, q_lo,
                              heads * hp, stream)) return 1;
    if (medtok_split_gemm_f16(q_hi, q_lo, n_rows, heads * hp, hp, wk_hi, wk_lo, (int64_t)heads * dw, hp, dw, dw, hp, heads, nullptr, wk_unscale, qf, heads * dw,
                              nullptr, nullptr, 0, stream)) return 1;
    if (kv_hi) {
        if (medtok_shared_kv_attention_split_f32(qf, q_start, q_len, kv_hi, kv_lo, kv_start, kv_len, n_codes, max_q_len, dw, scale, nullptr, c_hi, c_lo, variant, stream))
            return 1;
    } else if (medtok_shared_kv_attention_f32(qf, q_start, q_len, kv, kv_start, kv_len, n_codes, max_q_len, dw, scale, nullptr, c_hi, c_lo, 0, stream)) {
        return 1;
    }
    if (medtok_split_gemm_f16(c_hi, c_lo, n_rows, heads * dw, dw, wv_hi, wv_lo, (int64_t)heads * hp, dw, hp, hp, dw, heads, bv, wv_unscale, nullptr, 0, a_hi, a_lo,
                              heads * hp, stream)) return 1;
    if (medtok_split_gemm_f16(a_hi, a_lo, n_rows, heads * hp, 0, wo_hi, wo_lo, d, heads * hp, 0, d, heads * hp, 1, bo, wo_unscale, o, d, nullptr, nullptr, 0, stream))
        return 1;
    return medtok_residual_layernorm_split_f32(rows, o, ln_gamma, ln_beta, n_rows, d, ln_eps, y, y_hi, y_lo, y_hi ? dw : 0, stream);
}

extern "C" int medtok_segment_mean_f32(const float *x, const int64_t *seg_start, const int64_t *seg_len, int64_t n_seg, int d, float *out,
                                       void *stream)
{
    if (n_seg < 0 || d <= 0 || d % 4 != 0 || n_seg >= (1ll << 31)) return fail("segment_mean: bad shape n_seg=%ld d=%d (d %% 4 == 0)", (long)n_seg, d);
    if (n_seg == 0) return 0;
    if (!x || !seg_start || !seg_len || !out) return fail("segment_mean: NULL argument");
    if (((uintptr_t)x | (uintptr_t)out) & 15) return fail("segment_mean: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)n_seg, (unsigned)((d / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, seg_start,
                       seg_len, d, out);
    return check_launch("segment_mean");
}

// ================================================================= split-fp16 dense products (split_gemm.h)
#include "split_gemm.h"

extern "C" int medtok_split_half_f32(const float *src, int64_t n, int d, int64_t src_stride, int dp, float scale, void *hi, void *lo,
                                     const int64_t *seg_len, int seg_rows, void *stream)
{
    if (seg_len && (seg_rows <= 0 || n % seg_rows)) return fail("split_half: n=%ld is not a whole number of segments of %d rows", (long)n, seg_rows);
    if (n < 0 || d <= 0 || (d & 3) || dp < d || (dp & 7) || src_stride < d || (src_stride & 3))
        return fail("split_half: bad shape n=%ld d=%d stride=%ld dp=%d (d %% 4 == 0, dp %% 8 == 0, dp >= d)", (long)n, d, (long)src_stride, dp);
    if (n == 0) return 0;
    if (!src || !hi || !lo) return fail("split_half: NULL argument");
    if (((uintptr_t)src | (uintptr_t)hi | (uintptr_t)lo) & 15) return fail("split_half: pointers must be 16-byte aligned");
    const long total = n * (dp / 8);
    // (the segmented form is the text-image pass of a forward, gigabytes of HBM-bound streaming: six blocks per CU keep the memory
    // system full and leave a quarter of the wave slots for the small launches that run beside it; in-box A/B of the forward: 2 per CU
    // 382 k, 4: 394 k, 6: 398 k, 32: 390-397 k codes/s)
    const long grid = seg_len ? lmin(6L * dev_info().cus, (total + 1023) / 1024) : lmin(8192, (total + 1023) / 1024);
    hipLaunchKernelGGL(split_half_kernel<4>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, (long)n, d,
                       (long)src_stride, dp, scale, (_Float16 *)hi, (_Float16 *)lo, seg_len, seg_rows > 0 ? seg_rows : 1);
    return check_launch("split_half");
}

extern "C" int medtok_absmax_f32(const float *x, int64_t count, float *amax, void *stream)
{
    if (count < 0 || !amax || (!x && count)) return fail("absmax: bad arguments");
    if (((uintptr_t)x) & 15) return fail("absmax: x must be 16-byte aligned");
    if (hipMemsetAsync(amax, 0, 4, (hipStream_t)stream) != hipSuccess) return fail("absmax: memset failed");
    if (count == 0) return 0;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)lmin(512, (count + 4095) / 4096)), dim3(256), 0, (hipStream_t)stream, x, (long)count, amax);
    return check_launch("absmax");
}

extern "C" int medtok_split_half_scaled_f32(const float *src, int64_t n, int d, int64_t src_stride, int64_t dp, const float *amax, int transpose,
                                            int64_t group_cols, void *hi, void *lo, void *stream)
{
    if (n < 0 || d <= 0 || (d & 3) || (dp & 7) || src_stride < d || (src_stride & 3) || dp < (transpose ? n : (int64_t)d))
        return fail("split_half_scaled: bad shape n=%ld d=%d stride=%ld dp=%ld transpose=%d", (long)n, d, (long)src_stride, (long)dp, transpose);
    if (group_cols == 0) group_cols = dp;
    if (transpose && (group_cols <= 0 || dp % group_cols || (group_cols != dp && group_cols % 64)))
        return fail("split_half_scaled: group_cols=%ld must divide dp=%ld and be a multiple of 64", (long)group_cols, (long)dp);
    if (n == 0 && !transpose) return 0;
    if ((!src && n) || !hi || !lo) return fail("split_half_scaled: NULL argument");
    if (((uintptr_t)src | (uintptr_t)hi | (uintptr_t)lo) & 15) return fail("split_half_scaled: pointers must be 16-byte aligned");
    if (!transpose) {
        if (dp >= (1ll << 31)) return fail("split_half_scaled: dp too large");
        const long total = n * (dp / 8);
        hipLaunchKernelGGL(split_half_kernel<4>, dim3((unsigned)lmin(8192, (total + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, src, (long)n, d,
                           (long)src_stride, (int)dp, 1.0f, (_Float16 *)hi, (_Float16 *)lo, (const int64_t *)nullptr, 1, amax);
        return check_launch("split_half_scaled");
    }
    // transposed: the images are [d, dp], dp >= n columns (the zero tail is written by the tiles that cover it)
    const long row_tiles = (dp + 63) / 64;
    if (row_tiles >= (1ll << 31) || (d + 63) / 64 > 65535) return fail("split_half_scaled: too large");
    hipLaunchKernelGGL(split_half_t_kernel, dim3((unsigned)row_tiles, (unsigned)((d + 63) / 64)), dim3(256), 0, (hipStream_t)stream, src, (long)n, d,
                       (long)src_stride, (long)dp, (long)group_cols, 1.0f, (_Float16 *)hi, (_Float16 *)lo, amax);
    return check_launch("split_half_scaled(transposed)");
}

// The 16-bit image (fp16, or bf16 with bf16 != 0) of an fp32 matrix [n, d]: row-major [n, dp] with zero columns past d, or (transpose) the
// image of the transpose [d, dp], dp >= n, grouped along the rows like medtok_split_half_scaled_f32 -- operands of medtok_half_gemm_f32.
static int half_image_impl(const float *src, int64_t n, int d, int64_t src_stride, int64_t dp, int transpose, int64_t group_cols, int bf16,
                           void *out, float *col_partials, void *stream)
{
    if (n < 0 || d <= 0 || (d & 3) || (dp & 7) || src_stride < d || (src_stride & 3) || dp < (transpose ? n : (int64_t)d))
        return fail("half_image: bad shape n=%ld d=%d stride=%ld dp=%ld transpose=%d", (long)n, d, (long)src_stride, (long)dp, transpose);
    if (group_cols == 0) group_cols = dp;
    if (transpose && (group_cols <= 0 || dp % group_cols || (group_cols != dp && group_cols % 64)))
        return fail("half_image: group_cols=%ld must divide dp=%ld and be a multiple of 64", (long)group_cols, (long)dp);
    if (n == 0 && !transpose) return 0;
    if ((!src && n) || !out) return fail("half_image: NULL argument");
    if (((uintptr_t)src | (uintptr_t)out) & 15) return fail("half_image: pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (!transpose) {
        if (dp >= (1ll << 31)) return fail("half_image: dp too large");
        const long total = n * (dp / 8);
        const dim3 grid((unsigned)lmin(8192, (total + 255) / 256));
        if (bf16) hipLaunchKernelGGL(half_image_kernel<true>, grid, dim3(256), 0, s, src, (long)n, d, (long)src_stride, (int)dp, (unsigned short *)out);
        else hipLaunchKernelGGL(half_image_kernel<false>, grid, dim3(256), 0, s, src, (long)n, d, (long)src_stride, (int)dp, (unsigned short *)out);
        return check_launch("half_image");
    }
    const long row_tiles = (dp + 63) / 64;
    if (row_tiles >= (1ll << 31) || (d + 63) / 64 > 65535) return fail("half_image: too large");
    const dim3 grid((unsigned)row_tiles, (unsigned)((d + 63) / 64));
    if (bf16) hipLaunchKernelGGL(half_image_t_kernel<true>, grid, dim3(256), 0, s, src, (long)n, d, (long)src_stride, (long)dp, (long)group_cols, (unsigned short *)out, (unsigned short *)nullptr, 0, col_partials);
    else hipLaunchKernelGGL(half_image_t_kernel<false>, grid, dim3(256), 0, s, src, (long)n, d, (long)src_stride, (long)dp, (long)group_cols, (unsigned short *)out, (unsigned short *)nullptr, 0, col_partials);
    return check_launch("half_image(transposed)");
}
extern "C" int medtok_half_image_f32(const float *src, int64_t n, int d, int64_t src_stride, int64_t dp, int transpose, int64_t group_cols, int bf16,
                                     void *out, void *stream)
{
    return half_image_impl(src, n, d, src_stride, dp, transpose, group_cols, bf16, out, nullptr, stream);
}
// the transposed image and, from the same pass, col_partials [(dp + 63) / 64, d]: the sums over every 64-row tile of each column of src
// (medtok_half_image_pair_sums_f32's, for a product that needs no row-major image of its upstream gradient)
extern "C" int medtok_half_image_t_sums_f32(const float *src, int64_t n, int d, int64_t src_stride, int64_t dp, int64_t group_cols, int bf16,
                                            void *out, float *col_partials, void *stream)
{
    if (!col_partials) return fail("half_image_t_sums: NULL argument");
    return half_image_impl(src, n, d, src_stride, dp, 1, group_cols, bf16, out, col_partials, stream);
}

// both images of one matrix in one pass over it: out_plain [n, dp_plain] (zero columns past d; dp_plain <= d rounded up to 64) and
// out_t = the transposed image of medtok_half_image_f32(transpose = 1, dp = np, group_cols)
static int half_image_pair_impl(const float *src, int64_t n, int d, int64_t src_stride, int64_t dp_plain, int64_t np, int64_t group_cols,
                                int bf16, void *out_plain, void *out_t, float *col_partials, void *stream)
{
    if (n <= 0 || d <= 0 || (d & 3) || (np & 7) || (dp_plain & 7) || src_stride < d || (src_stride & 3) || np < n || dp_plain < d || dp_plain > (d + 63) / 64 * 64)
        return fail("half_image_pair: bad shape n=%ld d=%d stride=%ld dp_plain=%ld np=%ld", (long)n, d, (long)src_stride, (long)dp_plain, (long)np);
    if (group_cols == 0) group_cols = np;
    if (group_cols <= 0 || np % group_cols || (group_cols != np && group_cols % 64)) return fail("half_image_pair: group_cols=%ld must divide np=%ld and be a multiple of 64", (long)group_cols, (long)np);
    if (!src || !out_plain || !out_t) return fail("half_image_pair: NULL argument");
    if (((uintptr_t)src | (uintptr_t)out_plain | (uintptr_t)out_t) & 15) return fail("half_image_pair: pointers must be 16-byte aligned");
    const long row_tiles = (np + 63) / 64;
    if (row_tiles >= (1ll << 31) || (d + 63) / 64 > 65535) return fail("half_image_pair: too large");
    const dim3 grid((unsigned)row_tiles, (unsigned)((d + 63) / 64));
    hipStream_t s = (hipStream_t)stream;
    if (bf16) hipLaunchKernelGGL(half_image_t_kernel<true>, grid, dim3(256), 0, s, src, (long)n, d, (long)src_stride, (long)np, (long)group_cols, (unsigned short *)out_t, (unsigned short *)out_plain, (int)dp_plain, col_partials);
    else hipLaunchKernelGGL(half_image_t_kernel<false>, grid, dim3(256), 0, s, src, (long)n, d, (long)src_stride, (long)np, (long)group_cols, (unsigned short *)out_t, (unsigned short *)out_plain, (int)dp_plain, col_partials);
    return check_launch("half_image_pair");
}
extern "C" int medtok_half_image_pair_f32(const float *src, int64_t n, int d, int64_t src_stride, int64_t dp_plain, int64_t np, int64_t group_cols,
                                          int bf16, void *out_plain, void *out_t, void *stream)
{
    return half_image_pair_impl(src, n, d, src_stride, dp_plain, np, group_cols, bf16, out_plain, out_t, nullptr, stream);
}
// ... and, from the same pass, col_partials [(np + 63) / 64, d] fp32: the sums over every 64-row tile of each column (fixed order): the
// column sums of src -- a Linear's bias gradient when src is its upstream gradient -- are the sum of these rows
extern "C" int medtok_half_image_pair_sums_f32(const float *src, int64_t n, int d, int64_t src_stride, int64_t dp_plain, int64_t np, int64_t group_cols,
                                               int bf16, void *out_plain, void *out_t, float *col_partials, void *stream)
{
    if (!col_partials) return fail("half_image_pair_sums: NULL argument");
    return half_image_pair_impl(src, n, d, src_stride, dp_plain, np, group_cols, bf16, out_plain, out_t, col_partials, stream);
}

static bool g_gemm_k32 = false;        // test hook: the one-pass products with 32-deep stages, as before round 6
extern "C" void medtok_debug_set_half_gemm_k32(int on) { g_gemm_k32 = (on & 1) != 0; }

static int split_gemm_impl(const void *a_hi, const void *a_lo, int64_t m, int lda, int a_group_cols,
                           const void *b_hi, const void *b_lo, int64_t b_rows, int ldb, int b_group_rows,
                           int n_g, int k_g, int groups, const float *bias, float unscale, const float *amax_a, const float *amax_b,
                           float *c, int ldc, void *c_hi, void *c_lo, int ldch, void *stream, int one_pass = 0)
{
    if (m < 0 || groups < 1 || n_g <= 0 || k_g <= 0 || (n_g & 3) || (k_g % G_BK) || (lda & 7) || (ldb & 7) || (a_group_cols & 7) || lda < k_g || ldb < k_g)
        return fail("split_gemm: bad shape m=%ld groups=%d n_g=%d k_g=%d lda=%d ldb=%d a_group_cols=%d (n_g %% 4 == 0, k_g %% 32 == 0, strides %% 8 == 0)",
                    (long)m, groups, n_g, k_g, lda, ldb, a_group_cols);
    if ((long)(groups - 1) * a_group_cols + k_g > lda || (long)(groups - 1) * b_group_rows + n_g > b_rows)
        return fail("split_gemm: the last group reads past its operand (A columns %ld > lda %d or B rows %ld > %ld)",
                    (long)(groups - 1) * a_group_cols + k_g, lda, (long)(groups - 1) * b_group_rows + n_g, (long)b_rows);
    if (m == 0) return 0;
    if (!a_hi || !a_lo || !b_hi || !b_lo || (!c && !c_hi)) return fail("split_gemm: NULL argument");
    if ((c_hi == nullptr) != (c_lo == nullptr)) return fail("split_gemm: c_hi and c_lo go together");
    if (c && ((ldc & 3) || ldc < groups * n_g)) return fail("split_gemm: ldc=%d must be a multiple of 4 and >= groups * n_g", ldc);
    if (c_hi && ((ldch & 3) || ldch < groups * n_g)) return fail("split_gemm: ldch=%d must be a multiple of 4 and >= groups * n_g", ldch);
    if (((uintptr_t)a_hi | (uintptr_t)a_lo | (uintptr_t)b_hi | (uintptr_t)b_lo | (uintptr_t)c | (uintptr_t)c_hi | (uintptr_t)c_lo | (uintptr_t)bias) & 15)
        return fail("split_gemm: pointers must be 16-byte aligned");
    if ((double)m * lda * 2 >= 2147483647.0 * 256 || (double)b_rows * ldb * 2 >= 2147483647.0) return fail("split_gemm: operand too large");
    SplitGemmArgs p;
    p.ah = (const _Float16 *)a_hi; p.al = (const _Float16 *)a_lo; p.bh = (const _Float16 *)b_hi; p.bl = (const _Float16 *)b_lo;
    p.bias = bias; p.c = c; p.ch = (_Float16 *)c_hi; p.cl = (_Float16 *)c_lo;
    p.M = (long)m; p.a_bytes = (long)m * lda * 2; p.b_bytes = (long)b_rows * ldb * 2;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ldch = ldch; p.n_g = n_g; p.k_g = k_g; p.groups = groups;
    p.a_group_cols = a_group_cols; p.b_group_rows = b_group_rows; p.unscale = unscale; p.amax_a = amax_a; p.amax_b = amax_b;
    // tile height: 256 features, or 192 where that pads the group's features by > 10 % less (n_g = 192: the per-head W_v product)
    const long pad4 = (long)((n_g + 255) / 256) * 256, pad3 = (long)((n_g + 191) / 192) * 192;
    const bool mt3 = pad3 * 10 < pad4 * 9;
    p.row_tiles = (int)((m + G_BN - 1) / G_BN);
    const long row_ids = (long)((p.row_tiles + 7) / 8) * 8;
    // ... or fewer where the 256-feature tiles would leave most of the chip without a block (a product of a few thousand rows: the
    // text side of a forward, the node side of a training batch): 128 or 64 features per tile double / quadruple the blocks at the
    // same bytes per block-stage of the activation tile -- a launch of that size is latency, not throughput
    int mt = mt3 ? 3 : 4;
    const long half_chip = dev_info().cus / 2;
    if (!mt3 && row_ids * ((n_g + 255) / 256) * groups < half_chip) mt = row_ids * ((n_g + 127) / 128) * groups < half_chip ? 1 : 2;
    const int bm = 64 * mt;
    p.ftiles = (n_g + bm - 1) / bm;
    // few row tiles (less than 0.8 of the 8-padded count: a weight-gradient product's 3 or 12, the 1 of a small batch): the dense order
    // (split_gemm.h) instead of "XCD = row tile mod 8", which would leave XCDs without a tile
    const long n_tiles = (long)p.row_tiles * p.ftiles * groups;
    p.per_xcd = p.row_tiles * 10 < row_ids * 8 ? (int)((n_tiles + 7) / 8) : 0;
    const long ids = p.per_xcd ? (long)p.per_xcd * 8 : row_ids * p.ftiles * groups;
    if (ids >= (1ll << 31)) return fail("split_gemm: grid too large");
    // persistent: one block per CU (a multiple of 8: the XCD round-robin; never fewer than 8 -- a CU-masked or partitioned device
    // with < 8 CUs still gets a valid launch, its blocks just share CUs)
    const long blocks = lmin(ids, lmax(8, (long)(dev_info().cus / 8) * 8));
    const size_t lds = mt == 3 ? GemmShape<3>::LDS_BYTES : mt == 4 ? GemmShape<4>::LDS_BYTES : mt == 2 ? GemmShape<2>::LDS_BYTES : GemmShape<1>::LDS_BYTES;
    hipEvent_t pa = nullptr;
#define MEDTOK_GEMM_LAUNCH(...)                                                                                                   \
    do {                                                                                                                          \
        if (!set_lds_once<split_gemm_kernel<__VA_ARGS__>>(lds)) return fail("split_gemm: cannot reserve %zu bytes of LDS", lds);  \
        pa = prof_wanted(4) ? prof_mark((hipStream_t)stream) : nullptr;                                                                \
        hipLaunchKernelGGL((split_gemm_kernel<__VA_ARGS__>), dim3((unsigned)blocks), dim3(G_THREADS), lds, (hipStream_t)stream, p); \
    } while (0)
#define MEDTOK_GEMM_BY_MT(...)                                                                                                    \
    do {                                                                                                                          \
        if (mt == 3) MEDTOK_GEMM_LAUNCH(3 __VA_ARGS__); else if (mt == 4) MEDTOK_GEMM_LAUNCH(4 __VA_ARGS__);                      \
        else if (mt == 2) MEDTOK_GEMM_LAUNCH(2 __VA_ARGS__); else MEDTOK_GEMM_LAUNCH(1 __VA_ARGS__);                              \
    } while (0)
    // (one pass: 64-deep stages wherever the depth allows -- a copy then has 32 MFMAs of time to arrive instead of 16)
    const bool k64 = one_pass != 0 && k_g % (2 * G_BK) == 0 && !g_gemm_k32;
    if (one_pass == 0) MEDTOK_GEMM_BY_MT();
    else if (one_pass == 1) { if (k64) MEDTOK_GEMM_BY_MT(, true, false, true); else MEDTOK_GEMM_BY_MT(, true, false); }
    else { if (k64) MEDTOK_GEMM_BY_MT(, true, true, true); else MEDTOK_GEMM_BY_MT(, true, true); }
#undef MEDTOK_GEMM_BY_MT
#undef MEDTOK_GEMM_LAUNCH
    if (pa) prof_push(pa, prof_mark((hipStream_t)stream), 2.0 * (double)m * (double)n_g * (double)k_g * (double)groups, 4);     // fp32-equivalent flops (x3 on the fp16 pipe)
    return check_launch("split_gemm");
}

// C = unscale * (A . B^T) + bias in ONE half-precision pass with fp32 accumulation: a [m, lda], b [b_rows, ldb] are fp16 (bf16 = 0) or
// bf16 (bf16 = 1) matrices -- the product torch.autocast makes of an nn.Linear (train_MedTok.py:212,394); grouped as medtok_split_gemm_f16.
extern "C" int medtok_half_gemm_f32(const void *a, int64_t m, int lda, int a_group_cols, const void *b, int64_t b_rows, int ldb, int b_group_rows,
                                    int n_g, int k_g, int groups, const float *bias, float unscale, float *c, int ldc, int bf16, void *stream)
{
    return split_gemm_impl(a, a, m, lda, a_group_cols, b, b, b_rows, ldb, b_group_rows, n_g, k_g, groups, bias, unscale, nullptr, nullptr, c, ldc,
                           nullptr, nullptr, 0, stream, bf16 ? 2 : 1);
}

extern "C" int medtok_split_gemm_scaled_f16(const void *a_hi, const void *a_lo, int64_t m, int lda, int a_group_cols, const void *b_hi, const void *b_lo,
                                            int64_t b_rows, int ldb, int b_group_rows, int n_g, int k_g, int groups, const float *bias, float unscale,
                                            const float *amax_a, const float *amax_b, float *c, int ldc, void *stream)
{
    return split_gemm_impl(a_hi, a_lo, m, lda, a_group_cols, b_hi, b_lo, b_rows, ldb, b_group_rows, n_g, k_g, groups, bias, unscale, amax_a, amax_b, c, ldc,
                           nullptr, nullptr, 0, stream);
}

extern "C" int medtok_split_gemm_f16(const void *a_hi, const void *a_lo, int64_t m, int lda, int a_group_cols,
                                     const void *b_hi, const void *b_lo, int64_t b_rows, int ldb, int b_group_rows,
                                     int n_g, int k_g, int groups, const float *bias, float unscale,
                                     float *c, int ldc, void *c_hi, void *c_lo, int ldch, void *stream)
{
    return split_gemm_impl(a_hi, a_lo, m, lda, a_group_cols, b_hi, b_lo, b_rows, ldb, b_group_rows, n_g, k_g, groups, bias, unscale, nullptr, nullptr,
                           c, ldc, c_hi, c_lo, ldch, stream);
}

extern "C" int medtok_shared_kv_attention_train_f32(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv,
                                                    const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                                    int d, float scale, float dropout_p, uint32_t seed, float *out, float *lse, void *stream)
{
    if (n_codes < 0 || max_q_len < 0) return fail("shared_kv_attention_train: bad sizes n_codes=%ld max_q_len=%ld", (long)n_codes, (long)max_q_len);
    if (!attention_shape_ok(d)) return fail("shared_kv_attention_train: d=%d must be 64 or a multiple of 128, at most 768", d);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail("shared_kv_attention_train: dropout_p=%g must be in [0, 1)", (double)dropout_p);
    if (n_codes == 0 || max_q_len == 0) return 0;
    if (!q || !q_start || !q_len || !kv || !kv_start || !kv_len || !out || !lse) return fail("shared_kv_attention_train: NULL argument");
    return attention_forward(q, q_start, q_len, kv, kv_start, kv_len, n_codes, max_q_len, d, scale, out, lse, dropout_p, seed, (hipStream_t)stream);
}

// The training forward on the three-pass fp16 products (attention_pp.h, TRAIN form): two 32-row query tiles of a code per block on one
// copy of its keys, which the kernel turns from the caller's fp32 rows into (hi, lo) images itself.  Same outputs as
// medtok_shared_kv_attention_train_f32 to ~1e-6 relative (same dropout mask bits), about a third of its time at d = 768; d = 256, 512, 768.
extern "C" int medtok_shared_kv_attention_train_split_f32(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv,
                                                          const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                                          int d, float scale, float dropout_p, uint32_t seed, float *out, float *lse, void *stream)
{
    if (n_codes < 0 || max_q_len < 0) return fail("shared_kv_attention_train_split: bad sizes n_codes=%ld max_q_len=%ld", (long)n_codes, (long)max_q_len);
    if (d != 256 && d != 512 && d != 768) return fail("shared_kv_attention_train_split: d=%d must be 256, 512 or 768", d);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail("shared_kv_attention_train_split: dropout_p=%g must be in [0, 1)", (double)dropout_p);
    if (n_codes == 0 || max_q_len == 0) return 0;
    if (!q || !q_start || !q_len || !kv || !kv_start || !kv_len || !out || !lse) return fail("shared_kv_attention_train_split: NULL argument");
    if (((uintptr_t)q | (uintptr_t)kv | (uintptr_t)out) & 15) return fail("shared_kv_attention_train_split: pointers must be 16-byte aligned");
    const int64_t q_pairs = (max_q_len + 63) / 64;
    if (q_pairs * (n_codes + 8) >= (1ll << 31)) return fail("shared_kv_attention_train_split: grid limit exceeded");
    hipStream_t s = (hipStream_t)stream;
    const unsigned thresh = dropout_p > 0.f ? (unsigned)fmin(4294967295.0, (double)dropout_p * 4294967296.0) : 0u;
    const float keep_scale = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
    hipEvent_t pa = prof_wanted(2) ? prof_mark(s) : nullptr;
#define MEDTOK_ATT_PP_TRAIN(NT)                                                                                                   \
    do {                                                                                                                          \
        const size_t lds = AttPP<NT>::LDS_BYTES;                                                                                  \
        if (!set_lds_once<shared_kv_attention_pp_kernel<NT, true, true, true>>(lds))                                        \
            return fail("shared_kv_attention_train_split: cannot reserve %zu bytes of LDS", lds);                                 \
        hipLaunchKernelGGL((shared_kv_attention_pp_kernel<NT, true, true, true>), dim3((unsigned)(q_pairs * ((n_codes + 7) / 8 * 8))), dim3(512), lds, s, \
                           q, q_start, q_len, (const _Float16 *)kv, (const _Float16 *)nullptr, kv_start, kv_len, scale, out, (_Float16 *)nullptr,  \
                           (_Float16 *)nullptr, (int)q_pairs, (int)n_codes, lse, thresh, seed, keep_scale);                            \
    } while (0)
    if (d == 256) MEDTOK_ATT_PP_TRAIN(2); else if (d == 512) MEDTOK_ATT_PP_TRAIN(4); else MEDTOK_ATT_PP_TRAIN(6);
#undef MEDTOK_ATT_PP_TRAIN
    if (pa) prof_push(pa, prof_mark(s), 0.0, 2);
    return check_launch("shared_kv_attention_train_split");
}

extern "C" size_t medtok_shared_kv_attention_backward_workspace_bytes(int64_t q_rows) { return q_rows > 0 ? align_up((size_t)q_rows * 4, 256) : 256; }

static int attention_backward_impl(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv,
                                   const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                   int64_t max_kv_len, int64_t q_rows, int64_t kv_rows, int d, float scale, float dropout_p,
                                   uint32_t seed, const float *out, const float *lse, const float *d_out, float *dq,
                                   float *dkv, void *ws, size_t ws_bytes, void *stream, int hm, int acc_dkv = 0)
{
    if (n_codes < 0 || max_q_len < 0 || max_kv_len < 0 || q_rows < 0 || kv_rows < 0) return fail("shared_kv_attention_backward: bad sizes");
    if (!attention_shape_ok(d)) return fail("shared_kv_attention_backward: d=%d must be 64 or a multiple of 128, at most 768", d);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail("shared_kv_attention_backward: dropout_p=%g must be in [0, 1)", (double)dropout_p);
    if (q_rows == 0 && kv_rows == 0) return 0;                 // nothing to write
    const bool dq_only = acc_dkv == 2;                         // (the caller takes the key gradient later: medtok_shared_kv_attention_dkv_multi_f32)
    if (!q_start || !q_len || !kv_start || !kv_len || (q_rows > 0 && (!q || !out || !lse || !d_out || !dq)) || (kv_rows > 0 && (!kv || (!dkv && !dq_only))))
        return fail("shared_kv_attention_backward: NULL argument");
    if (!ws || ws_bytes < (size_t)q_rows * 4) return fail("shared_kv_attention_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    // rows no block owns (key rows past a code's kv_len inside its slot, query rows of no code) get a zero gradient
    if (q_rows > 0 && hipMemsetAsync(dq, 0, (size_t)q_rows * d * 4, s) != hipSuccess) return fail("shared_kv_attention_backward: memset failed");
    if (kv_rows > 0 && !acc_dkv && hipMemsetAsync(dkv, 0, (size_t)kv_rows * d * 4, s) != hipSuccess) return fail("shared_kv_attention_backward: memset failed");
    DkvSources srcs;
    memset(&srcs, 0, sizeof srcs);
    if (n_codes == 0 || q_rows == 0) return 0;
    float *delta = (float *)ws;
    hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)((q_rows + 3) / 4)), dim3(256), 0, s, d_out, out, (long)q_rows, d, delta);
    const int64_t q_tiles = (max_q_len + 31) / 32, kv_tiles = (max_kv_len + 31) / 32;
    if (q_tiles * n_codes >= (1ll << 31) || kv_tiles * n_codes >= (1ll << 31)) return fail("shared_kv_attention_backward: grid limit exceeded");
    const unsigned thresh = dropout_p > 0.f ? (unsigned)fmin(4294967295.0, (double)dropout_p * 4294967296.0) : 0u;
    const float keep_scale = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
    srcs.count = 1;
    srcs.s[0] = DkvSource{q, d_out, lse, delta, q_start, q_len, scale, keep_scale, thresh, seed};
    hipEvent_t pa_bwd = prof_wanted(3) ? prof_mark(s) : nullptr;
#define MEDTOK_ATT_BWD_HM(W, NT, HM)                                                                                             \
    do {                                                                                                                         \
        const size_t lds = AttShape<W, NT>::LDS_FLOATS * sizeof(float);                                                          \
        if (lds > 64 * 1024 && (!set_lds_once<shared_kv_attention_dq_kernel<W, NT, HM>>(lds) || !set_lds_once<shared_kv_attention_dkv_kernel<W, NT, HM>>(lds))) \
            return fail("shared_kv_attention_backward: cannot reserve %zu bytes of LDS", lds);                                   \
        if (q_tiles > 0)                                                                                                         \
            hipLaunchKernelGGL((shared_kv_attention_dq_kernel<W, NT, HM>), dim3((unsigned)(q_tiles * n_codes)), dim3(64 * W), lds, s, q, q_start, q_len, \
                               kv, kv_start, kv_len, d_out, lse, delta, scale, dq, (int)q_tiles, thresh, seed, keep_scale);      \
        if (kv_tiles > 0 && !dq_only)                                                                                            \
            hipLaunchKernelGGL((shared_kv_attention_dkv_kernel<W, NT, HM>), dim3((unsigned)(kv_tiles * n_codes)), dim3(64 * W), lds, s, srcs, \
                               kv, kv_start, kv_len, dkv, (int)kv_tiles, acc_dkv);                                               \
    } while (0)
#define MEDTOK_ATT_BWD(W, NT)                                                                                                    \
    do {                                                                                                                         \
        if (hm == 0) MEDTOK_ATT_BWD_HM(W, NT, 0); else if (hm == 1) MEDTOK_ATT_BWD_HM(W, NT, 1); else MEDTOK_ATT_BWD_HM(W, NT, 2); \
    } while (0)
    switch (d / 128) {
    case 0: MEDTOK_ATT_BWD(2, 1); break;
    case 1: MEDTOK_ATT_BWD(4, 1); break;
    case 2: MEDTOK_ATT_BWD(8, 1); break;
    case 3: MEDTOK_ATT_BWD(4, 3); break;
    case 4: MEDTOK_ATT_BWD(8, 2); break;
    case 5: MEDTOK_ATT_BWD(4, 5); break;
    default: MEDTOK_ATT_BWD(8, 3); break;
    }
#undef MEDTOK_ATT_BWD_HM
#undef MEDTOK_ATT_BWD
    if (pa_bwd) prof_push(pa_bwd, prof_mark(s), 0.0, 3);     // dQ + dKV; the caller prices the pair (ragged counts live on the device)
    return check_launch("shared_kv_attention_backward");
}

extern "C" int medtok_shared_kv_attention_backward_f32(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv,
                                                       const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                                       int64_t max_kv_len, int64_t q_rows, int64_t kv_rows, int d, float scale, float dropout_p,
                                                       uint32_t seed, const float *out, const float *lse, const float *d_out, float *dq,
                                                       float *dkv, void *ws, size_t ws_bytes, void *stream)
{
    return attention_backward_impl(q, q_start, q_len, kv, kv_start, kv_len, n_codes, max_q_len, max_kv_len, q_rows, kv_rows, d, scale, dropout_p, seed, out,
                                   lse, d_out, dq, dkv, ws, ws_bytes, stream, 0);
}

// the same backward with its four matrix products in ONE half-precision pass (fp16; bf16 != 0: bf16) with fp32 accumulation -- the
// precision class of nn.MultiheadAttention under torch.autocast (train_MedTok.py:212,394); operands, softmax rebuild and outputs fp32
extern "C" int medtok_shared_kv_attention_backward_half_f32(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv,
                                                            const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                                            int64_t max_kv_len, int64_t q_rows, int64_t kv_rows, int d, float scale, float dropout_p,
                                                            uint32_t seed, const float *out, const float *lse, const float *d_out, float *dq,
                                                            float *dkv, void *ws, size_t ws_bytes, int bf16, void *stream)
{
    return attention_backward_impl(q, q_start, q_len, kv, kv_start, kv_len, n_codes, max_q_len, max_kv_len, q_rows, kv_rows, d, scale, dropout_p, seed, out,
                                   lse, d_out, dq, dkv, ws, ws_bytes, stream, bf16 ? 2 : 1);
}

// ... the same (mode 0: exact fp32, 1: fp16, 2: bf16 products) with dKV ADDED to what dkv already holds (accumulate_dkv != 0): the
// layers of CrossAttention all attend to the ORIGINAL other modality (:83,86), so their key gradients land in one buffer -- no second
// [kv_rows, d] tensor, no zero fill of it, no pass that adds the two.  Rows no block owns are then left as they are.
extern "C" int medtok_shared_kv_attention_backward_acc_f32(const float *q, const int64_t *q_start, const int64_t *q_len, const float *kv,
                                                           const int64_t *kv_start, const int64_t *kv_len, int64_t n_codes, int64_t max_q_len,
                                                           int64_t max_kv_len, int64_t q_rows, int64_t kv_rows, int d, float scale, float dropout_p,
                                                           uint32_t seed, const float *out, const float *lse, const float *d_out, float *dq,
                                                           float *dkv, void *ws, size_t ws_bytes, int mode, int accumulate_dkv, void *stream)
{
    if (mode < 0 || mode > 2) return fail("shared_kv_attention_backward_acc: mode=%d must be 0 (fp32), 1 (fp16) or 2 (bf16)", mode);
    return attention_backward_impl(q, q_start, q_len, kv, kv_start, kv_len, n_codes, max_q_len, max_kv_len, q_rows, kv_rows, d, scale, dropout_p, seed, out,
                                   lse, d_out, dq, dkv, ws, ws_bytes, stream, mode, accumulate_dkv == 2 ? 2 : (accumulate_dkv != 0));
}

// The key gradient of SEVERAL attention calls over the same keys in one launch (attention_backward.h: DkvSources): every source brings its
// queries, upstream gradient, log-sum-exp, delta (= <d_out, out> per query row: the workspace a dQ-only call of
// medtok_shared_kv_attention_backward_acc_f32 filled), dropout parameters and its own q_start / q_len; kv, kv_start, kv_len are common.
// dkv [kv_rows, d] is written once (rows no block owns zeroed).  mode: 0 exact fp32, 1 fp16, 2 bf16 products.
extern "C" int medtok_shared_kv_attention_dkv_multi_f32(const medtok_dkv_source *sources, int count, const float *kv, const int64_t *kv_start,
                                                        const int64_t *kv_len, int64_t n_codes, int64_t max_kv_len, int64_t kv_rows, int d,
                                                        float *dkv, int mode, void *stream)
{
    if (!sources || count < 1 || count > DKV_SRC_MAX) return fail("shared_kv_attention_dkv_multi: 1..%d sources per call", DKV_SRC_MAX);
    if (n_codes < 0 || max_kv_len < 0 || kv_rows < 0) return fail("shared_kv_attention_dkv_multi: bad sizes");
    if (!attention_shape_ok(d)) return fail("shared_kv_attention_dkv_multi: d=%d must be 64 or a multiple of 128, at most 768", d);
    if (mode < 0 || mode > 2) return fail("shared_kv_attention_dkv_multi: mode=%d must be 0 (fp32), 1 (fp16) or 2 (bf16)", mode);
    if (kv_rows == 0) return 0;
    if (!kv || !kv_start || !kv_len || !dkv) return fail("shared_kv_attention_dkv_multi: NULL argument");
    DkvSources srcs;
    memset(&srcs, 0, sizeof srcs);
    srcs.count = count;
    for (int i = 0; i < count; ++i) {
        const medtok_dkv_source &m = sources[i];
        if (!m.q || !m.d_out || !m.lse || !m.delta || !m.q_start || !m.q_len) return fail("shared_kv_attention_dkv_multi: NULL argument in source %d", i);
        if (!(m.dropout_p >= 0.f && m.dropout_p < 1.f)) return fail("shared_kv_attention_dkv_multi: dropout_p=%g must be in [0, 1)", (double)m.dropout_p);
        const unsigned thresh = m.dropout_p > 0.f ? (unsigned)fmin(4294967295.0, (double)m.dropout_p * 4294967296.0) : 0u;
        srcs.s[i] = DkvSource{m.q, m.d_out, m.lse, m.delta, m.q_start, m.q_len, m.scale, m.dropout_p > 0.f ? 1.f / (1.f - m.dropout_p) : 1.f, thresh, m.seed};
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dkv, 0, (size_t)kv_rows * d * 4, s) != hipSuccess) return fail("shared_kv_attention_dkv_multi: memset failed");
    const int64_t kv_tiles = (max_kv_len + 31) / 32;
    if (n_codes == 0 || kv_tiles == 0) return 0;
    if (kv_tiles * n_codes >= (1ll << 31)) return fail("shared_kv_attention_dkv_multi: grid limit exceeded");
    hipEvent_t pa = prof_wanted(3) ? prof_mark(s) : nullptr;
#define MEDTOK_DKV_HM(W, NT, HM)                                                                                                 \
    do {                                                                                                                         \
        const size_t lds = AttShape<W, NT>::LDS_FLOATS * sizeof(float);                                                          \
        if (lds > 64 * 1024 && !set_lds_once<shared_kv_attention_dkv_kernel<W, NT, HM>>(lds))                                    \
            return fail("shared_kv_attention_dkv_multi: cannot reserve %zu bytes of LDS", lds);                                  \
        hipLaunchKernelGGL((shared_kv_attention_dkv_kernel<W, NT, HM>), dim3((unsigned)(kv_tiles * n_codes)), dim3(64 * W), lds, s, srcs, \
                           kv, kv_start, kv_len, dkv, (int)kv_tiles, 0);                                                         \
    } while (0)
#define MEDTOK_DKV(W, NT)                                                                                                        \
    do {                                                                                                                         \
        if (mode == 0) MEDTOK_DKV_HM(W, NT, 0); else if (mode == 1) MEDTOK_DKV_HM(W, NT, 1); else MEDTOK_DKV_HM(W, NT, 2);        \
    } while (0)
    switch (d / 128) {
    case 0: MEDTOK_DKV(2, 1); break;
    case 1: MEDTOK_DKV(4, 1); break;
    case 2: MEDTOK_DKV(8, 1); break;
    case 3: MEDTOK_DKV(4, 3); break;
    case 4: MEDTOK_DKV(8, 2); break;
    case 5: MEDTOK_DKV(4, 5); break;
    default: MEDTOK_DKV(8, 3); break;
    }
#undef MEDTOK_DKV_HM
#undef MEDTOK_DKV
    if (pa) prof_push(pa, prof_mark(s), 0.0, 3);
    return check_launch("shared_kv_attention_dkv_multi");
}

// ================================================================= EMA statistics, EMA apply, codebook usage window (ema_kernels.h)
#include "ema_kernels.h"

struct EmaWs {
    int *counts, *offsets, *wave_counts, *wave_offsets;
    uint32_t *keys[2], *vals[2];
    size_t total;
};

static EmaWs ema_ws_layout(void *ws, int64_t n, int64_t k_codes)
{
    EmaWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = ws ? (char *)ws + off : nullptr; off += align_up(bytes, 256); return (void *)p; };
    w.counts = (int *)take((size_t)k_codes * 4);
    w.offsets = (int *)take((size_t)(k_codes + 1) * 4);
    w.wave_counts = (int *)take((size_t)256 * SORT_WAVES * 4);
    w.wave_offsets = (int *)take(((size_t)256 * SORT_WAVES + 1) * 4);
    for (int i = 0; i < 2; ++i) { w.keys[i] = (uint32_t *)take((size_t)n * 4); w.vals[i] = (uint32_t *)take((size_t)n * 4); }
    w.total = off;
    return w;
}

extern "C" size_t medtok_ema_stats_workspace_bytes(int64_t n, int64_t k_codes)
{
    if (n < 0 || k_codes <= 0) return 0;
    return ema_ws_layout(nullptr, n, k_codes).total;
}

extern "C" int medtok_ema_stats_f32(const float *zhat, const int64_t *idx, int64_t n, int d, int64_t k_codes, float *bins,
                                    float *embed_sum, void *ws, size_t ws_bytes, void *stream)
{
    if (n < 0 || d <= 0 || (d & 3) || k_codes <= 0 || k_codes >= (1ll << 31) || n >= (1ll << 31))
        return fail("ema_stats: bad shape n=%ld d=%d K=%ld", (long)n, d, (long)k_codes);
    EmaWs w = ema_ws_layout(ws, n, k_codes);
    if (!ws || ws_bytes < w.total) return fail("ema_stats: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w.counts, 0, (size_t)k_codes * 4, s) != hipSuccess) return fail("ema_stats: memset failed");
    if (n > 0) {
        hipLaunchKernelGGL(hist_kernel, dim3((unsigned)lmin(2048, (n + 255) / 256)), dim3(256), 0, s, idx, (long)n, (int)k_codes, w.counts);
    }
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.counts, (int)k_codes, w.offsets);
    int cur = 0;
    bool first = true;
    for (int shift = 0; n > 0 && (first || (k_codes - 1) >> shift); shift += 8) {
        if (first) hipLaunchKernelGGL((radix_count_kernel<true>), dim3(SORT_BLOCKS), dim3(256), 0, s, idx, (const uint32_t *)nullptr, (long)n, (int)k_codes, shift, w.wave_counts);
        else hipLaunchKernelGGL((radix_count_kernel<false>), dim3(SORT_BLOCKS), dim3(256), 0, s, idx, w.keys[cur], (long)n, (int)k_codes, shift, w.wave_counts);
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.wave_counts, 256 * SORT_WAVES, w.wave_offsets);
        if (first) hipLaunchKernelGGL((radix_scatter_kernel<true>), dim3(SORT_BLOCKS), dim3(256), 0, s, idx, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (long)n, (int)k_codes, shift, w.wave_offsets, w.keys[cur ^ 1], w.vals[cur ^ 1]);
        else hipLaunchKernelGGL((radix_scatter_kernel<false>), dim3(SORT_BLOCKS), dim3(256), 0, s, idx, w.keys[cur], w.vals[cur], (long)n, (int)k_codes, shift, w.wave_offsets, w.keys[cur ^ 1], w.vals[cur ^ 1]);
        cur ^= 1;
        first = false;
    }
    hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)lmin(4096, (k_codes + 3) / 4)), dim3(256), 0, s, zhat, w.vals[cur], w.offsets, (int)k_codes, d, bins, embed_sum);
    return check_launch("ema_stats");
}

// ---- the codebook's gradient through the embedding lookup (embed_grad_kernels.h): keys, the sort above, chunked sums
#include "embed_grad_kernels.h"

struct CodeGradWs {
    int *counts, *offsets, *first_chunk, *wave_counts, *wave_offsets;
    uint32_t *keys[2], *vals[2];
    float *chunk_sums;
    long extra;                 // Q: the bound on the chunks of rows with several
    size_t total;
};

// everything from (contributions, K, d): nothing here depends on the data
static CodeGradWs code_grad_ws_layout(void *ws, int64_t contributions, int64_t k_codes, int d)
{
    CodeGradWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = ws ? (char *)ws + off : nullptr; off += align_up(bytes, 256); return (void *)p; };
    w.counts = (int *)take((size_t)k_codes * 4);                  // the histogram, then (in place) the rows' chunk counts
    w.offsets = (int *)take((size_t)(k_codes + 1) * 4);
    w.first_chunk = (int *)take((size_t)(k_codes + 1) * 4);
    w.wave_counts = (int *)take((size_t)256 * SORT_WAVES * 4);
    w.wave_offsets = (int *)take(((size_t)256 * SORT_WAVES + 1) * 4);
    for (int i = 0; i < 2; ++i) { w.keys[i] = (uint32_t *)take((size_t)contributions * 4); w.vals[i] = (uint32_t *)take((size_t)contributions * 4); }
    w.extra = (long)((2 * contributions + MEDTOK_EMBED_CODE_GRAD_CHUNK - 1) / MEDTOK_EMBED_CODE_GRAD_CHUNK);
    w.chunk_sums = (float *)take((size_t)w.extra * (size_t)d * sizeof(float));
    w.total = off;
    return w;
}

static bool code_grad_shape_ok(int64_t n, int slots, int topk, int64_t n_codes, int d)
{
    return n >= 0 && slots >= 1 && slots <= MEDTOK_DECODE_MAX_SLOTS && topk >= 1 && topk <= MEDTOK_MAX_TOPK && n_codes >= 1 && n_codes < (1ll << 31) &&
           d > 0 && !(d & 3);
}

// What both gradients are after their checks: the keys and their histogram, offsets[], first_chunk[] and the stable sort by row, then the
// chunked sums of embed_grad_chunk_kernel<.., G_T, SLOT_BLOCKS> and the combine.  g is [n, slots * width] fp32 (SLOT_BLOCKS: the
// upstream gradient of embed_codes' rows) or [n, width] in g_dtype (the upstream gradient of the folded lookup).
template <bool SLOT_BLOCKS>
static int embed_grad_sums(const char *fn, const void *g, int g_dtype, int64_t g_stride, const EmbedLookup &a, int64_t n, const DecodeRegions &reg,
                           const CodeGradWs &w, float *G, float *bins, hipStream_t s)
{
    const long contributions = (long)n * a.slots * a.topk, items = (long)n * a.slots, rows = (long)a.rows, work = rows + w.extra;
    hipLaunchKernelGGL(embed_code_grad_zero_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, w.counts, rows);
    auto keys = [&](auto lanes) {
        constexpr int per = 256 / decltype(lanes)::value;         // items per block
        hipLaunchKernelGGL((embed_code_grad_keys_kernel<decltype(lanes)::value>), dim3((unsigned)((items + per - 1) / per)), dim3(256), 0, s, a.index,
                           a.pad, items, a.tokens, (long)a.num_codes, a.slots, a.topk, reg, (int)rows, w.keys[0], w.vals[0], w.counts);
    };
    const bool narrow = item_lanes(a.width) == 16;
    if (narrow) keys(std::integral_constant<int, 16>{}); else keys(std::integral_constant<int, 64>{});
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.counts, (int)rows, w.offsets);
    hipLaunchKernelGGL(embed_code_grad_plan_kernel<MEDTOK_EMBED_CODE_GRAD_CHUNK>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, w.counts, rows);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.counts, (int)rows, w.first_chunk);
    int cur = 0;
    for (int shift = 0; shift == 0 || (rows >> shift); shift += 8) {         // keys lie in [0, rows]: the dead ones sort to the end
        hipLaunchKernelGGL((radix_count_kernel<false>), dim3(SORT_BLOCKS), dim3(256), 0, s, (const int64_t *)nullptr, w.keys[cur], contributions,
                           (int)rows, shift, w.wave_counts);
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.wave_counts, 256 * SORT_WAVES, w.wave_offsets);
        hipLaunchKernelGGL((radix_scatter_kernel<false>), dim3(SORT_BLOCKS), dim3(256), 0, s, (const int64_t *)nullptr, w.keys[cur], w.vals[cur],
                           contributions, (int)rows, shift, w.wave_offsets, w.keys[cur ^ 1], w.vals[cur ^ 1]);
        cur ^= 1;
    }
    auto chunks = [&](auto lanes, auto *typed) {                  // typed: a null pointer that carries the type of g
        using G_T = std::remove_pointer_t<decltype(typed)>;
        constexpr int per = 256 / decltype(lanes)::value;
        hipLaunchKernelGGL((embed_grad_chunk_kernel<decltype(lanes)::value, G_T, SLOT_BLOCKS>), dim3((unsigned)((work + per - 1) / per)), dim3(256), 0,
                           s, (const G_T *)g, (long)g_stride, a.index, a.weights, (long)a.num_codes, a.slots, a.topk, a.width, w.vals[cur], w.offsets,
                           w.first_chunk, rows, w.extra, bins, G, w.chunk_sums);
    };
    auto by_type = [&](auto lanes) {
        if constexpr (SLOT_BLOCKS) chunks(lanes, (float *)nullptr);
        else if (g_dtype == MEDTOK_EMBED_G_F32) chunks(lanes, (float *)nullptr);
        else if (g_dtype == MEDTOK_EMBED_G_F16) chunks(lanes, (_Float16 *)nullptr);
        else chunks(lanes, (__bf16 *)nullptr);
    };
    if (narrow) by_type(std::integral_constant<int, 16>{}); else by_type(std::integral_constant<int, 64>{});
    hipLaunchKernelGGL(embed_code_grad_combine_kernel, dim3((unsigned)lmin(4096, (rows + 3) / 4)), dim3(256), 0, s, w.chunk_sums, w.first_chunk, rows,
                       a.width, G);
    return check_launch(fn);
}

extern "C" size_t medtok_embed_code_grad_workspace_bytes(int64_t n, int slots, int topk, int64_t n_codes, int d)
{
    if (!code_grad_shape_ok(n, slots, topk, n_codes, d) || n > ((1ll << 31) - 1) / (slots * topk)) return 0;
    return code_grad_ws_layout(nullptr, n * slots * topk, n_codes, d).total;
}

extern "C" int medtok_embed_code_grad_f32(const float *g_out, int64_t g_stride, const int64_t *index, const uint8_t *pad, int64_t n,
                                          const int64_t *tokens, const float *weights, int64_t num_codes, int slots, int topk, int64_t n_codes,
                                          int d, const int64_t *region_lo, const int64_t *region_size, float *g_what, float *bins, void *ws,
                                          size_t ws_bytes, void *stream)
{
    const char *fn = "embed_code_grad";
    if (!code_grad_shape_ok(n, slots, topk, n_codes, d))
        return fail("%s: bad shape n=%ld slots=%d topk=%d n_codes=%ld d=%d", fn, (long)n, slots, topk, (long)n_codes, d);
    if (n > ((1ll << 31) - 1) / (slots * topk))
        return fail("%s: n * slots * topk = %ld x %d x %d contributions reach 2^31 (the sort's payload is 32-bit): split the batch", fn, (long)n,
                    slots, topk);
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, nullptr, n_codes, d, region_lo, region_size};
    DecodeRegions reg;
    if (int rc = embed_args(fn, a, n, false, reg)) return rc;
    if (int rc = row_stride(fn, "g_stride", g_stride, (int64_t)slots * d, "slots * d")) return rc;
    if (!g_what || !bins) return fail("%s: g_what and bins are required", fn);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(g_what, 0, (size_t)n_codes * d * sizeof(float), s) != hipSuccess || hipMemsetAsync(bins, 0, (size_t)n_codes * sizeof(float), s) != hipSuccess)
            return fail("%s: memset failed", fn);
        return 0;
    }
    if (!g_out || !index || !tokens || !weights) return fail("%s: g_out, index, tokens and weights are required", fn);
    const CodeGradWs w = code_grad_ws_layout(ws, (int64_t)n * slots * topk, n_codes, d);
    if (!ws || ws_bytes < w.total) return fail("%s: workspace too small (%zu < %zu)", fn, ws_bytes, w.total);
    return embed_grad_sums<true>(fn, g_out, MEDTOK_EMBED_G_F32, g_stride, a, n, reg, w, g_what, bins, s);
}

// ---- per-table-row sums of the folded lookup's upstream gradient: the same keys, sort, plan and combine
extern "C" size_t medtok_embed_table_grad_workspace_bytes(int64_t n, int slots, int topk, int64_t table_rows, int hp)
{
    if (!code_grad_shape_ok(n, slots, topk, table_rows, hp) || n > ((1ll << 31) - 1) / (slots * topk)) return 0;
    return code_grad_ws_layout(nullptr, n * slots * topk, table_rows, hp).total;
}

extern "C" int medtok_embed_table_grad(const void *g, int g_dtype, int64_t g_stride, const int64_t *index, const uint8_t *pad, int64_t n,
                                       const int64_t *tokens, const float *weights, int64_t num_codes, int slots, int topk, int64_t table_rows,
                                       int hp, const int64_t *row_offset, const int64_t *row_size, float *G, float *bins, void *ws,
                                       size_t ws_bytes, void *stream)
{
    const char *fn = "embed_table_grad";
    if (hp > 0 && (hp & 3)) return fail("%s: hp=%d is not a multiple of 4", fn, hp);
    if (table_rows >= (1ll << 31)) return fail("%s: table_rows = %ld reach 2^31 (the sort's keys are 32-bit)", fn, (long)table_rows);
    if (!code_grad_shape_ok(n, slots, topk, table_rows, hp))
        return fail("%s: bad shape n=%ld slots=%d topk=%d table_rows=%ld hp=%d", fn, (long)n, slots, topk, (long)table_rows, hp);
    if (n > ((1ll << 31) - 1) / (slots * topk))
        return fail("%s: n * slots * topk = %ld x %d x %d contributions reach 2^31 (the sort's payload is 32-bit): split the batch", fn, (long)n,
                    slots, topk);
    if (g_dtype != MEDTOK_EMBED_G_F32 && g_dtype != MEDTOK_EMBED_G_F16 && g_dtype != MEDTOK_EMBED_G_BF16)
        return fail("%s: g_dtype=%d unsupported (MEDTOK_EMBED_G_F32, _F16 or _BF16)", fn, g_dtype);
    const CodeGradWs need = code_grad_ws_layout(nullptr, (int64_t)n * slots * topk, table_rows, hp);
    if (n > 0 && ws_bytes < need.total) return fail("%s: workspace too small (%zu < %zu)", fn, ws_bytes, need.total);
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, nullptr, table_rows, hp, row_offset, row_size};
    DecodeRegions reg;
    if (int rc = embed_args(fn, a, n, false, reg)) return rc;
    if (int rc = row_stride(fn, "g_stride", g_stride, hp, "hp")) return rc;
    if (!G || !bins) return fail("%s: G and bins are required", fn);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(G, 0, (size_t)table_rows * hp * sizeof(float), s) != hipSuccess || hipMemsetAsync(bins, 0, (size_t)table_rows * sizeof(float), s) != hipSuccess)
            return fail("%s: memset failed", fn);
        return 0;
    }
    if (!g || !index || !tokens || !weights || !ws) return fail("%s: g, index, tokens, weights and ws are required", fn);
    if (((uintptr_t)g & (g_dtype == MEDTOK_EMBED_G_F32 ? 15 : 7))) return fail("%s: g must be aligned to four of its elements", fn);
    const CodeGradWs w = code_grad_ws_layout(ws, (int64_t)n * slots * topk, table_rows, hp);
    return embed_grad_sums<false>(fn, g, g_dtype, g_stride, a, n, reg, w, G, bins, s);
}

// ---- segment pooling: a row per (batch row, segment) -- the keys, the sort above, then the pool's kernels over listed positions
#include "embed_pool_segments_kernels.h"

struct PoolSegmentsWs {
    int *counts, *offsets, *first_chunk, *wave_counts, *wave_offsets;
    uint32_t *keys[2], *vals[2];
    float *partial;
    int *chunk_counts;
    long extra;                 // Q: the bound on the chunks of bags with several
    size_t total;
};

// everything from (B, L, V, width): nothing here depends on the data
static PoolSegmentsWs pool_segments_ws_layout(void *ws, int64_t n, int64_t bags, int width)
{
    PoolSegmentsWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = ws ? (char *)ws + off : nullptr; off += align_up(bytes, 256); return (void *)p; };
    w.counts = (int *)take((size_t)bags * 4);                     // the histogram, then (in place) the bags' chunk counts
    w.offsets = (int *)take((size_t)(bags + 1) * 4);
    w.first_chunk = (int *)take((size_t)(bags + 1) * 4);
    w.wave_counts = (int *)take((size_t)256 * SORT_WAVES * 4);
    w.wave_offsets = (int *)take(((size_t)256 * SORT_WAVES + 1) * 4);
    for (int i = 0; i < 2; ++i) { w.keys[i] = (uint32_t *)take((size_t)n * 4); w.vals[i] = (uint32_t *)take((size_t)n * 4); }
    w.extra = (long)((2 * n + MEDTOK_EMBED_POOL_CHUNK - 1) / MEDTOK_EMBED_POOL_CHUNK);
    w.partial = (float *)take((size_t)w.extra * (size_t)width * sizeof(float));
    w.chunk_counts = (int *)take((size_t)w.extra * 2 * sizeof(int));
    w.total = off;
    return w;
}

// the limits of one call, in the order they are reported; nullptr: supported
static const char *pool_segments_limit(int64_t batch, int64_t len, int64_t n_segments, int64_t width)
{
    if (batch < 0 || len < 0) return "batch and len must be >= 0";
    if (n_segments < 1) return "n_segments must be >= 1";
    if (batch > 0 && len > ((1ll << 31) - 1) / batch) return "batch * len positions reach 2^31 (the sort's payload is 32-bit): split the batch";
    if (batch > 0 && n_segments > ((1ll << 31) - 2) / batch) return "batch * n_segments + 1 bags reach 2^31 (the sort's keys are 32-bit): split the batch";
    if (width < 1) return "width must be >= 1";
    if (width > MEDTOK_EMBED_POOL_MAX_WIDTH) return "rows of slots * d floats exceed MEDTOK_EMBED_POOL_MAX_WIDTH";
    return nullptr;
}

extern "C" size_t medtok_embed_pool_segments_workspace_bytes(int64_t batch, int64_t len, int64_t n_segments, int width)
{
    if (pool_segments_limit(batch, len, n_segments, width) || batch == 0) return 0;
    return pool_segments_ws_layout(nullptr, batch * len, batch * n_segments, width).total;
}

extern "C" int medtok_embed_pool_segments_f32(const int64_t *index, const uint8_t *pad, const int64_t *segment_id, int64_t batch, int64_t len,
                                              int64_t n_segments, const int64_t *tokens, const float *weights, int64_t num_codes, int slots,
                                              int topk, const float *what, int64_t n_codes, int d, const int64_t *region_lo,
                                              const int64_t *region_size, const float *miss, int normalize, float *out, int64_t out_stride,
                                              int *counts, int *status, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "embed_pool_segments";
    if (slots >= 1 && topk >= 1 && (int64_t)slots * topk > 64)
        return fail("%s: slots * topk = %ld entries per code exceed one wavefront", fn, (long)slots * topk);
    if (const char *why = pool_segments_limit(batch, len, n_segments, slots >= 1 && d >= 1 ? (int64_t)slots * d : 1))
        return fail("%s: %s (batch=%ld len=%ld n_segments=%ld slots=%d d=%d)", fn, why, (long)batch, (long)len, (long)n_segments, slots, d);
    const int64_t n = batch * len, bags = batch * n_segments;
    const EmbedLookup a = {index, pad, tokens, weights, num_codes, slots, topk, what, n_codes, d, region_lo, region_size};
    DecodeRegions reg;
    if (int rc = embed_args(fn, a, n, true, reg)) return rc;
    const int width = slots * d;
    if (int rc = row_stride(fn, "out_stride", out_stride, width, "slots * d")) return rc;
    if (batch == 0) return 0;
    const PoolSegmentsWs w = pool_segments_ws_layout(ws, n, bags, width);
    if (bags + w.extra > kMaxBlocks)
        return fail("%s: %ld bags + %ld chunks exceed one launch (%ld blocks of 256 threads)", fn, (long)bags, (long)w.extra, (long)kMaxBlocks);
    if (!ws || ws_bytes < w.total) return fail("%s: workspace too small (%zu bytes given, %zu needed)", fn, ws_bytes, w.total);
    if (!tokens || !weights || !what || !out || !counts || (n > 0 && (!index || !segment_id)))
        return fail("%s: index, segment_id, tokens, weights, what, out and counts are required", fn);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(embed_code_grad_zero_kernel, dim3((unsigned)((bags + 255) / 256)), dim3(256), 0, s, w.counts, (long)bags);
    if (n > 0)
        hipLaunchKernelGGL(embed_pool_segments_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pad, segment_id, (long)n, (long)len,
                           (long)n_segments, (uint32_t)bags, w.keys[0], w.vals[0], w.counts, status);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.counts, (int)bags, w.offsets);
    hipLaunchKernelGGL(embed_code_grad_plan_kernel<MEDTOK_EMBED_POOL_CHUNK>, dim3((unsigned)((bags + 255) / 256)), dim3(256), 0, s, w.counts, (long)bags);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.counts, (int)bags, w.first_chunk);
    int cur = 0;
    for (int shift = 0; n > 0 && (shift == 0 || (bags >> shift)); shift += 8) {          // keys lie in [0, bags]: the dead ones sort to the end
        hipLaunchKernelGGL((radix_count_kernel<false>), dim3(SORT_BLOCKS), dim3(256), 0, s, (const int64_t *)nullptr, w.keys[cur], (long)n, 0, shift,
                           w.wave_counts);
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.wave_counts, 256 * SORT_WAVES, w.wave_offsets);
        hipLaunchKernelGGL((radix_scatter_kernel<false>), dim3(SORT_BLOCKS), dim3(256), 0, s, (const int64_t *)nullptr, w.keys[cur], w.vals[cur],
                           (long)n, 0, shift, w.wave_offsets, w.keys[cur ^ 1], w.vals[cur ^ 1]);
        cur ^= 1;
    }
    const EmbedPoolList list = {w.vals[cur], w.offsets, w.first_chunk, (long)bags, w.extra, out, (long)out_stride, counts};
    const int per_lane = width <= 256 ? 1 : width <= 1024 ? 4 : width <= 3072 ? 12 : 16;
    dispatch_group<1, 4, 12, 16>(per_lane, topk, [&](auto r, auto maxk) {
        hipLaunchKernelGGL((embed_pool_partial_kernel<decltype(r)::value, decltype(maxk)::value, true>), dim3((unsigned)(bags + w.extra)), dim3(256),
                           (size_t)width * sizeof(float), s, index, (const uint8_t *)nullptr, 0l, 0, tokens, weights, (long)num_codes, slots, topk,
                           what, d, reg, miss, normalize, w.partial, w.chunk_counts, status, list);
    });
    hipLaunchKernelGGL(embed_pool_finish_kernel, dim3((unsigned)bags, (unsigned)((width + 1023) / 1024)), dim3(256), 0, s, (const float *)w.partial,
                       (const int *)w.chunk_counts, 0, width, out, (long)out_stride, counts, (const int *)w.first_chunk);
    return check_launch(fn);
}

extern "C" size_t medtok_code_histogram_workspace_bytes(int64_t k_codes)
{
    return k_codes > 0 ? align_up((size_t)k_codes * 4, 256) : 0;
}

extern "C" int medtok_code_histogram_f32(const int64_t *idx, int64_t n, int64_t k_codes, float *bins, void *ws, size_t ws_bytes,
                                         void *stream)
{
    if (n < 0 || k_codes <= 0 || k_codes >= (1ll << 31)) return fail("code_histogram: bad shape n=%ld K=%ld", (long)n, (long)k_codes);
    if (!ws || ws_bytes < (size_t)k_codes * 4) return fail("code_histogram: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int *counts = (int *)ws;
    if (hipMemsetAsync(counts, 0, (size_t)k_codes * 4, s) != hipSuccess) return fail("code_histogram: memset failed");
    if (n > 0) hipLaunchKernelGGL(hist_kernel, dim3((unsigned)lmin(2048, (n + 255) / 256)), dim3(256), 0, s, idx, (long)n, (int)k_codes, counts);
    hipLaunchKernelGGL(counts_to_float_kernel, dim3((unsigned)((k_codes + 255) / 256)), dim3(256), 0, s, counts, (long)k_codes, bins);
    return check_launch("code_histogram");
}

extern "C" int medtok_ema_apply_f32(float *E, float *cluster_size, const float *bins, const float *embed_sum, int64_t k_codes,
                                    int d, float decay, float one_minus_decay, void *stream)
{
    if (k_codes <= 0 || d <= 0 || (d & 3)) return fail("ema_apply: bad shape K=%ld d=%d", (long)k_codes, d);
    hipLaunchKernelGGL(ema_apply_kernel, dim3((unsigned)((k_codes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, E, cluster_size, bins,
                       embed_sum, (int)k_codes, d, decay, one_minus_decay);
    return check_launch("ema_apply");
}

extern "C" int medtok_ema_cluster_size_f32(float *cluster_size, const float *bins, int64_t k_codes, float decay,
                                           float one_minus_decay, void *stream)
{
    if (k_codes <= 0) return fail("ema_cluster_size: bad K");
    hipLaunchKernelGGL(ema_cluster_size_kernel, dim3((unsigned)((k_codes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       cluster_size, bins, (long)k_codes, decay, one_minus_decay);
    return check_launch("ema_cluster_size");
}

extern "C" size_t medtok_usage_workspace_bytes(int64_t window_len, int64_t n_codes)
{
    if (window_len <= 0 || n_codes <= 0) return 0;
    return align_up((size_t)window_len * 4, 256) + align_up((size_t)n_codes + 1, 256);
}

extern "C" int medtok_usage_update(float *window, int64_t window_len, const int64_t *ids, int64_t m, int64_t n_codes,
                                   int32_t *count_out, void *ws, size_t ws_bytes, void *stream)
{
    if (window_len <= 0 || n_codes <= 0 || m < 0 || !count_out) return fail("usage_update: bad args");
    const size_t need = medtok_usage_workspace_bytes(window_len, n_codes);
    if (!ws || ws_bytes < need) return fail("usage_update: workspace too small (%zu < %zu)", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    float *tmp = (float *)ws;
    unsigned char *flags = (unsigned char *)ws + align_up((size_t)window_len * 4, 256);
    if (hipMemsetAsync(flags, 0, (size_t)n_codes + 1, s) != hipSuccess) return fail("usage_update: memset failed");
    const unsigned blocks = (unsigned)lmin(1024, (window_len + 255) / 256);
    hipLaunchKernelGGL(usage_shift_kernel, dim3(blocks), dim3(256), 0, s, window, (long)window_len, ids, (long)m, tmp);
    hipLaunchKernelGGL(usage_mark_kernel, dim3(blocks), dim3(256), 0, s, tmp, (long)window_len, (long)n_codes, window, flags);
    hipLaunchKernelGGL(usage_sum_kernel, dim3(1), dim3(1024), 0, s, flags, (long)n_codes + 1, count_out);
    return check_launch("usage_update");
}

extern "C" size_t medtok_usage_multi_workspace_bytes(int64_t window_len, int64_t n_codes, int count)
{
    if (window_len <= 0 || n_codes <= 0 || count < 1 || count > USAGE_MULTI_MAX) return 0;
    return align_up((size_t)window_len * 4, 256) + align_up((size_t)count * ((size_t)n_codes + 1), 256);
}

// ... with a device word copied behind the counts (counts_out [count + 1]): the caller's one host read of the usage counts also brings
// e.g. the cross-attention's status word, without a concatenation launch
extern "C" int medtok_usage_update_multi_word(float *window, int64_t window_len, const int64_t *const *ids, const int64_t *m, int count, int64_t n_codes,
                                              int32_t *counts_out, const int32_t *extra_word, void *ws, size_t ws_bytes, void *stream)
{
    if (window_len <= 0 || n_codes <= 0 || count < 1 || count > USAGE_MULTI_MAX || !ids || !m || !counts_out || !window)
        return fail("usage_update_multi: bad args (1..%d updates)", USAGE_MULTI_MAX);
    const size_t need = medtok_usage_multi_workspace_bytes(window_len, n_codes, count);
    if (!ws || ws_bytes < need) return fail("usage_update_multi: workspace too small (%zu < %zu)", ws_bytes, need);
    UsageMultiArgs a;
    a.count = count;
    long total = 0;
    for (int u = 0; u < USAGE_MULTI_MAX; ++u) {
        a.ids[u] = u < count ? ids[u] : nullptr;
        a.m[u] = u < count ? (long)m[u] : 0;
        if (u < count && (m[u] < 0 || (m[u] > 0 && !ids[u]))) return fail("usage_update_multi: update %d has no ids", u);
        total += a.m[u];
    }
    hipStream_t s = (hipStream_t)stream;
    float *tmp = (float *)ws;
    unsigned char *flags = (unsigned char *)ws + align_up((size_t)window_len * 4, 256);
    if (hipMemsetAsync(flags, 0, (size_t)count * ((size_t)n_codes + 1), s) != hipSuccess) return fail("usage_update_multi: memset failed");
    if (hipMemsetAsync(counts_out, 0, (size_t)count * 4, s) != hipSuccess) return fail("usage_update_multi: memset failed");
    const unsigned blocks = (unsigned)lmin(1024, (window_len + total + 255) / 256);
    hipLaunchKernelGGL(usage_multi_mark_kernel, dim3(blocks), dim3(256), 0, s, window, (long)window_len, a, (long)n_codes, tmp, flags);
    hipLaunchKernelGGL(usage_multi_finish_kernel, dim3((unsigned)lmin(256, (window_len + 255) / 256)), dim3(256), 0, s, tmp, (long)window_len, window, flags,
                       (long)n_codes, count, counts_out, (const int *)extra_word);
    return check_launch("usage_update_multi");
}

extern "C" int medtok_usage_update_multi(float *window, int64_t window_len, const int64_t *const *ids, const int64_t *m, int count, int64_t n_codes,
                                         int32_t *counts_out, void *ws, size_t ws_bytes, void *stream)
{
    return medtok_usage_update_multi_word(window, window_len, ids, m, count, n_codes, counts_out, nullptr, ws, ws_bytes, stream);
}

// ================================================================= one-call soft VQ forward
// l2norm + nearest codes in one call (the head of NormEMAVectorQuantizer.forward): on the filter path the fp16 image of the
// normalised rows that the shortlist pass streams comes out of the pass that normalises them (one read of z less).
extern "C" size_t medtok_normalized_search_workspace_bytes(int64_t n, int64_t k_codes, int d, int topk, int path)
{
    return medtok_search_workspace_bytes(n, k_codes, d, topk, path);
}

extern "C" int medtok_normalized_search_f32(const float *z, int64_t n, int d, const float *what, const float *wsq, int64_t k_codes, int topk,
                                            int path, float *zhat, float *zsq, int64_t *idx, float *dist, void *ws, size_t ws_bytes,
                                            void *stream)
{
    if (n < 0 || k_codes <= 0 || d <= 0 || (d & 3)) return fail("normalized_search: bad shape n=%ld K=%ld d=%d (d %% 4 == 0)", (long)n, (long)k_codes, d);
    if (n == 0) return 0;
    if (!z || !zhat || !zsq || !what || !wsq || !idx || !dist) return fail("normalized_search: NULL argument");
    const SearchCall c = plan_search_call(n, k_codes, d, topk, path);
    FuseAssign fuse = {nullptr, nullptr, nullptr, 0L, false, nullptr, nullptr, false};
    const bool filter_path = c.path == MEDTOK_PATH_F16_FILTER && k_codes < (1ll << 31) && n < (1ll << 31);
    if (filter_path) {
        const FilterPlan &f = c.filter;
        const FilterWs fw = filter_ws_layout(ws, n, f);
        if (!ws || ws_bytes < fw.total) return fail("normalized_search: workspace too small (%zu < %zu)", ws_bytes, fw.total);
        hipStream_t s = (hipStream_t)stream;
        launch_rownorm<true>(s, z, (long)n, d, zhat, zsq, fw.xh, f.dp);
        if (f.n_pad > n && hipMemsetAsync(fw.xh + (size_t)n * f.dp, 0, (size_t)(f.n_pad - n) * f.dp * 2, s) != hipSuccess)
            return fail("normalized_search: memset failed");
        if (check_launch("rownorm(+fp16)")) return 1;
        fuse.xh_done = true;
    } else if (medtok_rownorm_f32(z, n, d, 1, zhat, zsq, stream)) {
        return 1;
    }
    return search_impl(c, zhat, zsq, n, what, wsq, k_codes, d, topk, idx, dist, ws, ws_bytes, stream, filter_path ? &fuse : nullptr);
}

// the one-call forward's workspace: |x|^2 per row, then the search's
static inline size_t soft_vq_head_bytes(int64_t n) { return align_up((size_t)n * 4, 256); }

extern "C" size_t medtok_soft_vq_workspace_bytes(int64_t n, int64_t k_codes, int d, int topk, int path)
{
    if (n <= 0) return 256;
    return soft_vq_head_bytes(n) + plan_search_call(n, k_codes, d, topk, path).ws_bytes;
}

static int soft_vq_forward_impl(const float *x, int64_t n, int d, const float *what, const float *wsq, int64_t k_codes,
                                int topk, int path, float *xhat, int64_t *idx, float *dist, float *w, float *zq_ste,
                                int64_t zq_stride, float *row_sqerr, void *ws, size_t ws_bytes, void *stream,
                                const _Float16 *p_wh, const float *p_wsqp, const float *p_en_max)
{
    if (n == 0) return 0;
    const SearchCall c = plan_search_call(n, k_codes, d, topk, path);
    const size_t head = n > 0 ? soft_vq_head_bytes(n) : 0, need = n > 0 ? head + c.ws_bytes : 256;      // (n < 0 is refused below)
    if (!ws || ws_bytes < need) return fail("soft_vq_forward: workspace too small (%zu < %zu)", ws_bytes, need);
    float *xsq = (float *)ws;
    void *sws = (char *)ws + head;
    // Without the squared-error output (its summation order is the stand-alone kernel's) the filter path's re-score kernel
    // does the soft assignment itself, bit for bit the same, while the top-k code rows are hot in the L2.
    if (zq_stride == 0) zq_stride = d;
    FuseAssign fuse = {x, w, zq_ste, (long)zq_stride, false, nullptr, nullptr, false};
    fuse.p_wh = p_wh; fuse.p_wsqp = p_wsqp; fuse.p_en_max = p_en_max;
    const bool try_fuse = !row_sqerr && zq_ste && zq_stride >= d && !(zq_stride & 3) && topk <= 8;
    if (try_fuse && c.path == MEDTOK_PATH_F16_FILTER && xhat && !(d & 3)) {
        // the filter's fp16 image of the normalised rows comes out of the same pass that normalises them
        const FilterPlan &f = c.filter;
        const FilterWs fw = filter_ws_layout(sws, n, f);
        hipStream_t s = (hipStream_t)stream;
        // (the image's padding rows are written by the same launch; with a prepared codebook it also clears the count of rows the
        // filter hands to the exact kernel -- nothing else of the search's preparation runs then)
        launch_rownorm<true>(s, x, (long)n, d, xhat, xsq, fw.xh, f.dp, (long)f.n_pad, p_wh ? fw.fb_count : (int *)nullptr);
        if (check_launch("rownorm(+fp16)")) return 1;
        fuse.xh_done = true;
        fuse.fb_zeroed = p_wh != nullptr;
    } else if (medtok_rownorm_f32(x, n, d, 1, xhat, xsq, stream)) {
        return 1;
    }
    const int rc = search_impl(c, xhat, xsq, n, what, wsq, k_codes, d, topk, idx, dist, sws, ws_bytes - head, stream, try_fuse ? &fuse : nullptr);
    if (rc) return 1;
    if (!fuse.done) return medtok_soft_assign_f32(x, what, idx, dist, n, d, topk, 0, w, zq_ste, zq_stride, row_sqerr, stream);
    // rows the filter handed to the exact kernel: assignment through the device-side row list (normally empty)
    hipLaunchKernelGGL((soft_assign_kernel<8>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,          // (the filter path: topk <= 8)
                       x, what, idx, dist, (long)n, d, topk, 0, w, zq_ste, (long)zq_stride, (float *)nullptr, fuse.fb_rows, fuse.fb_count);
    return check_launch("soft_assign(list)");
}

extern "C" int medtok_soft_vq_forward_f32(const float *x, int64_t n, int d, const float *what, const float *wsq, int64_t k_codes,
                                          int topk, int path, float *xhat, int64_t *idx, float *dist, float *w, float *zq_ste,
                                          int64_t zq_stride, float *row_sqerr, void *ws, size_t ws_bytes, void *stream)
{
    return soft_vq_forward_impl(x, n, d, what, wsq, k_codes, topk, path, xhat, idx, dist, w, zq_ste, zq_stride, row_sqerr, ws, ws_bytes, stream,
                                nullptr, nullptr, nullptr);
}

// ---- a codebook prepared once per weight version
extern "C" int medtok_filter_image_width(int d)
{
    return d > 0 ? filter_image_dp(d) : 0;
}

extern "C" int medtok_rownorm_image_f32(const float *x, int64_t n, int d, float *xhat, float *sqn, void *image, int64_t image_rows, int dp, void *stream)
{
    if (n <= 0 || d <= 0 || (d & 3)) return fail("rownorm_image: need n > 0, d > 0, d %% 4 == 0 (n=%ld d=%d)", (long)n, d);
    if (!x || !xhat || !sqn || !image) return fail("rownorm_image: NULL argument");
    if (dp != medtok_filter_image_width(d)) return fail("rownorm_image: dp=%d, the filter reads images of width %d at d=%d", dp, medtok_filter_image_width(d), d);
    if (image_rows < n) return fail("rownorm_image: image_rows=%ld < n=%ld", (long)image_rows, (long)n);
    if (((uintptr_t)x | (uintptr_t)xhat | (uintptr_t)image) & 15) return fail("rownorm_image: pointers must be 16-byte aligned");
    launch_rownorm<true>((hipStream_t)stream, x, (long)n, d, xhat, sqn, (_Float16 *)image, dp, (long)image_rows);
    return check_launch("rownorm_image");
}

extern "C" int medtok_codebook_image_f32(const float *what, int64_t n, int d, void *image, int64_t image_rows, int dp, void *stream)
{
    if (n <= 0 || d <= 0 || (d & 3) || !what || !image) return fail("codebook_image: bad arguments (n=%ld d=%d)", (long)n, d);
    if (dp != medtok_filter_image_width(d) || image_rows < n) return fail("codebook_image: dp=%d (expected %d), image_rows=%ld (>= %ld)", dp, medtok_filter_image_width(d), (long)image_rows, (long)n);
    if (((uintptr_t)what | (uintptr_t)image) & 15) return fail("codebook_image: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)lmin(4096, (image_rows * (dp / 8) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, what, (long)n, d,
                       (long)image_rows, dp, (_Float16 *)image, (int *)nullptr);
    return check_launch("codebook_image");
}

extern "C" int medtok_codebook_prepare_f32(const float *wsq, const medtok_region_desc *regions, int count, void *stream)
{
    if (!wsq || !regions || count < 1 || count > PREP_MAX_REGIONS) return fail("codebook_prepare: 1..%d regions", PREP_MAX_REGIONS);
    RegionPrepArgs a;
    for (int i = 0; i < count; ++i) {
        const medtok_region_desc &r = regions[i];
        if (r.lo < 0 || r.k <= 0 || r.lo + r.k >= (1ll << 31) || !r.wsqp || !r.en_max) return fail("codebook_prepare: bad region %d", i);
        a.r[i] = RegionPrep{wsq + r.lo, (int)r.k, r.en_max, r.wsqp, (int)((r.k + F_BM - 1) / F_BM * F_BM)};
    }
    hipLaunchKernelGGL(wsq_max_regions_kernel, dim3((unsigned)count), dim3(1024), 0, (hipStream_t)stream, a);
    return check_launch("codebook_prepare");
}

extern "C" int medtok_soft_vq_forward_prepared_f32(const float *x, int64_t n, int d, const float *what, const float *wsq, int64_t k_codes,
                                                   int topk, int path, const void *image, const float *wsqp, const float *en_max,
                                                   float *xhat, int64_t *idx, float *dist, float *w, float *zq_ste,
                                                   int64_t zq_stride, void *ws, size_t ws_bytes, void *stream)
{
    if (!image || !wsqp || !en_max) return fail("soft_vq_forward_prepared: NULL prepared argument");
    if ((uintptr_t)image & 15) return fail("soft_vq_forward_prepared: the image must be 16-byte aligned");
    return soft_vq_forward_impl(x, n, d, what, wsq, k_codes, topk, path, xhat, idx, dist, w, zq_ste, zq_stride, nullptr, ws, ws_bytes, stream,
                                (const _Float16 *)image, wsqp, en_max);
}
