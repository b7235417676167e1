"""Tensor-level wrappers over the C ABI (include/medtok_vq.h).

torch is used for device memory and the current HIP stream only; every
computation below runs in the hand-written gfx950 kernels.  CPU tensors are
rejected: there is no fallback path.
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib
from ._lib import PATH_AUTO, PATH_F16_FILTER, PATH_F32_MFMA, MAX_TOPK, plan_path  # noqa: F401


# Profiling hook (bench.py): when set to a list, every search CALL (all of its kernels) is bracketed
# by HIP events on its launch stream and (start, stop, algorithmic_flops) is appended.  None = no overhead.
SEARCH_TIMER = None


DKV_SOURCES_MAX = _lib.DKV_SOURCES_MAX
PROFILE_KINDS = ("filter_f16_kernel", "search_f32_kernel", "shared_kv_attention_kernel", "shared_kv_attention_backward_kernels", "split_gemm_kernel")


def profile_begin(kinds=None) -> None:
    """Start the library's own per-kernel timing (HIP events around each matrix-pipe launch).  kinds: names out of PROFILE_KINDS to
    bracket (None: all) -- a training step has ~180 library launches, and the event pairs of all of them cost it ~0.5 ms."""
    if kinds is None:
        _lib.check(_lib.load().medtok_profile_begin(), "medtok_profile_begin")
        return
    mask = 0
    for k in kinds:
        mask |= 1 << PROFILE_KINDS.index(k)
    _lib.check(_lib.load().medtok_profile_begin_kinds(mask), "medtok_profile_begin_kinds")


def profile_end() -> dict:
    """Stop it; returns {kernel: dict(ms, flops, launches)} (synchronises on the recorded events)."""
    import ctypes as C
    names = PROFILE_KINDS
    n = len(names)
    ms, fl, ln = (C.c_double * n)(), (C.c_double * n)(), (C.c_int * n)()
    _lib.check(_lib.load().medtok_profile_end(ms, fl, ln), "medtok_profile_end")
    return {names[i]: dict(ms=ms[i], flops=fl[i], launches=ln[i]) for i in range(n)}


MedTokLibraryError = _lib.MedTokLibraryError


class ClockProbe:
    """Shader clock of a timed region (bench.py): `with ClockProbe(device, max_seconds) as p: ...timed work on OTHER streams...`;
    afterwards p.result() = dict(ghz_mean, ghz_min, ghz_max, per_xcd).  One idle wavefront per XCD on a stream of its own; it ends
    when the context exits (a pinned host flag) or after max_seconds, whichever is first."""

    def __init__(self, device, max_seconds: float = 30.0):
        self.device = torch.device(device)
        self.max_ticks = int(max_seconds * 1e8)
        self.flag = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.out = torch.zeros((8, 4), dtype=torch.int64, device=self.device)
        self.stream = torch.cuda.Stream(device=self.device)

    def __enter__(self):
        with _on(self.device):
            _lib.check(_lib.load().medtok_debug_clock_probe(self.flag.data_ptr(), self.max_ticks, self.out.data_ptr(), self.stream.cuda_stream),
                       "medtok_debug_clock_probe")
        return self

    def __exit__(self, *exc):
        self.flag[0] = 1
        self.stream.synchronize()
        return False

    def result(self) -> dict:
        o = self.out.cpu().tolist()
        ghz = [c / (r * 10.0) for c, r, _, _ in o if r > 0]          # cycles per 10 ns tick -> GHz
        if not ghz:
            return {}
        return dict(ghz_mean=sum(ghz) / len(ghz), ghz_min=min(ghz), ghz_max=max(ghz), seconds=max(r for _, r, _, _ in o) / 1e8,
                    per_xcd={int(x): c / (r * 10.0) for c, r, x, _ in o if r > 0},
                    how="s_memtime cycles / s_memrealtime (100 MHz) ticks of one idle wavefront per XCD while the probe ran")


ATTENTION_MAX_WIDTH = 1024                 # widest cross-attention: inference only above ATTENTION_MAX_TRAIN_WIDTH
ATTENTION_MAX_TRAIN_WIDTH = 768


def attention_width(d: int) -> int:
    """Width the ragged attention kernels run a D-wide problem at: D itself for 64 and multiples of 128 up to 768, and 1024 (BERT-large
    features; inference only: the training kernels' 32-key chunk of fp32 rows does not fit the LDS there), else the next such width
    (the caller appends zero columns).  Wider than 1024 is refused."""
    if d <= 64:
        return 64
    w = (d + 127) // 128 * 128
    if w > 768:
        w = 1024
    if d > ATTENTION_MAX_WIDTH:
        raise _lib.MedTokLibraryError(f"cross-attention width D = {d} is not supported by the gfx950 attention kernels: they take D <= 1024 "
                                      f"(64, a multiple of 128 up to 768, or 1024 natively; anything else zero-padded to the next such width)")
    return w


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_SAME_DEVICE = contextlib.nullcontext()


def _stream(t: torch.Tensor) -> int:
    """the raw handle of torch's current stream on t's device (the C accessor where this torch has it: every wrapper below asks once per
    launch, and the Python-level Stream object costs more than some of the launches)"""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


def _stream_of(dev: torch.device) -> int:
    """raw handle of torch's current stream on `dev`"""
    if _raw_stream is not None:
        return _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


def _on(dev: torch.device):
    """`with torch.cuda.device(dev)` only where it changes something: a tensor on another device than the current one"""
    return _SAME_DEVICE if dev.index is None or dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MedTokLibraryError(
            f"{name}: expected a tensor on an MI355X (cuda/HIP) device, got "
            f"{getattr(t, 'device', type(t))}; medtok_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _ws(nbytes: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=like.device)


def pad_dim(d: int) -> int:
    """Kernels need D % 4 == 0; zero columns change neither norms nor dots."""
    return (d + 3) // 4 * 4


def rownorm(x: torch.Tensor, normalize: bool = True, want_xhat: bool = True):
    """(xhat, |xhat|^2) of F.normalize(x, dim=-1). x: [n, d] fp32."""
    x = _dev(x, "x")
    n, d = x.shape
    lib = _lib.load()
    sqn = torch.empty(n, dtype=torch.float32, device=x.device)
    if normalize:
        xhat = torch.empty_like(x)
    else:
        xhat = x if want_xhat else None
    with _on(x.device):
        _lib.check(lib.medtok_rownorm_f32(x.data_ptr(), n, d, int(normalize), _ptr(xhat), sqn.data_ptr(),
                                          _stream(x)), "medtok_rownorm_f32")
    return xhat, sqn


# Test hook: when set to a dict, topk_search records how many rows the fp16 filter handed to the exact kernel ("fallback_rows";
# one host sync per search -- never set in product code).
SEARCH_STATS = None


def topk_search(xhat, xsq, what, wsq, topk: int, path: int = PATH_AUTO):
    """idx [n, topk] int64, dist [n, topk] fp32: the topk nearest codes per row."""
    xhat, xsq = _dev(xhat, "xhat"), _dev(xsq, "xsq")
    what, wsq = _dev(what, "what"), _dev(wsq, "wsq")
    n, d = xhat.shape
    k = what.shape[0]
    if what.shape[1] != d or xsq.shape[0] != n or wsq.shape[0] != k:
        raise ValueError("topk_search: shape mismatch")
    lib = _lib.load()
    idx = torch.empty((n, topk), dtype=torch.int64, device=xhat.device)
    dist = torch.empty((n, topk), dtype=torch.float32, device=xhat.device)
    nb = lib.medtok_search_workspace_bytes(n, k, d, topk, path)
    ws = _ws(nb, xhat)
    timer = SEARCH_TIMER
    with _on(xhat.device):
        if timer is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        _lib.check(lib.medtok_topk_search_f32(xhat.data_ptr(), xsq.data_ptr(), n, what.data_ptr(), wsq.data_ptr(),
                                              k, d, topk, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(),
                                              ws.numel(), path, _stream(xhat)), "medtok_topk_search_f32")
        if timer is not None:
            e1.record()
            timer.append((e0, e1, 2.0 * n * k * d))
        if SEARCH_STATS is not None:
            off = lib.medtok_debug_filter_fallback_count_offset(n, k, d, topk, path)
            if off != 2 ** 64 - 1:
                SEARCH_STATS["fallback_rows"] = int(ws[off: off + 4].view(torch.int32).item())
                SEARCH_STATS["rows"] = n
    return idx, dist


def merge_topk_lists(dist_parts, idx_parts):
    """Exact top-k of the union of per-shard lists: dist_parts [P, n, k] fp32, idx_parts [P, n, k] int64 (global ids)."""
    dist_parts, idx_parts = _dev(dist_parts, "dist_parts"), _dev(idx_parts, "idx_parts", torch.int64)
    parts, n, k = dist_parts.shape
    lib = _lib.load()
    idx = torch.empty((n, k), dtype=torch.int64, device=dist_parts.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=dist_parts.device)
    with _on(dist_parts.device):
        _lib.check(lib.medtok_merge_topk_lists_f32(dist_parts.data_ptr(), idx_parts.data_ptr(), n, parts, k, idx.data_ptr(),
                                                   dist.data_ptr(), _stream(dist_parts)), "medtok_merge_topk_lists_f32")
    return idx, dist


def debug_filter_scores(xhat, xsq, what, wsq):
    """Test hook: approximate scores s~ [n, K] of the fp16 filter."""
    xhat, xsq, what, wsq = _dev(xhat, "xhat"), _dev(xsq, "xsq"), _dev(what, "what"), _dev(wsq, "wsq")
    n, d = xhat.shape
    k = what.shape[0]
    lib = _lib.load()
    out = torch.empty((n, k), dtype=torch.float32, device=xhat.device)
    ws = _ws(lib.medtok_debug_filter_scores_workspace_bytes(n, k, d), xhat)
    with _on(xhat.device):
        _lib.check(lib.medtok_debug_filter_scores_f32(xhat.data_ptr(), xsq.data_ptr(), n, what.data_ptr(), wsq.data_ptr(), k, d,
                                                      out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(xhat)),
                   "medtok_debug_filter_scores_f32")
    return out


def _zq_out(out, n, d, like):
    """Output buffer for zq: a fresh [n, d] tensor, or the caller's column block of a wider row-major tensor."""
    if out is None:
        return torch.empty((n, d), dtype=torch.float32, device=like.device), d
    if not (out.is_cuda and out.dtype == torch.float32 and out.shape == (n, d) and out.stride(1) == 1 and out.stride(0) % 4 == 0
            and out.data_ptr() % 16 == 0):
        raise ValueError("out must be an fp32 [n, d] device view with unit column stride and 16-byte aligned rows")
    return out, out.stride(0)


def soft_assign(xref, what, idx, dist, hard: bool = False, want_w: bool = True, want_sqerr: bool = True,
                raw: bool = False, out=None):
    """(w [n,k], zq [n,d], row_sqerr [n]); zq is the straight-through value unless raw.
    `out` may be a column block of a wider tensor (e.g. emb[:, d:2*d])."""
    xref, what = _dev(xref, "xref"), _dev(what, "what")
    idx = _dev(idx, "idx", torch.int64)
    n, d = xref.shape
    topk = 1 if idx.dim() == 1 else idx.shape[1]
    dist = None if hard and dist is None else _dev(dist, "dist")
    lib = _lib.load()
    w = torch.empty((n, topk), dtype=torch.float32, device=xref.device) if want_w else None
    zq, zstride = _zq_out(out, n, d, xref)
    se = torch.empty(n, dtype=torch.float32, device=xref.device) if want_sqerr else None
    with _on(xref.device):
        _lib.check(lib.medtok_soft_assign_f32(xref.data_ptr(), what.data_ptr(), idx.data_ptr(), _ptr(dist), n, d, topk,
                                              int(hard) | (2 if raw else 0), _ptr(w), zq.data_ptr(), zstride, _ptr(se), _stream(xref)),
                   "medtok_soft_assign_f32")
    return w, zq, se


DECODE_MAX_SLOTS = _lib.DECODE_MAX_SLOTS


def _decode_args(fn, tokens, weights, what, regions, g_out=None):
    """shared checks of decode_tokens / decode_tokens_backward: shapes and regions raise ValueError before any library call; tensors
    that are not on the device raise MedTokLibraryError (_dev).  Returns (tokens [n, s, k], weights, what, lo[], size[])."""
    tokens, weights, regions = _decode_shapes(fn, tokens, weights, what, regions, g_out)
    return _decode_on_device(tokens, weights, what, regions)


def _decode_shapes(fn, tokens, weights, what, regions, g_out=None):
    """the ValueError half of _decode_args: (tokens [n, s, k], weights [n, s, k], [(lo, size)] per slot); nothing is moved or loaded"""
    if not isinstance(tokens, torch.Tensor) or not isinstance(weights, torch.Tensor) or not isinstance(what, torch.Tensor):
        raise ValueError(f"{fn}: tokens, weights and what must be tensors")
    if tokens.dtype != torch.int64 or weights.dtype != torch.float32 or what.dtype != torch.float32:
        raise ValueError(f"{fn}: expected int64 tokens and fp32 weights / codebook, got {tokens.dtype}, {weights.dtype}, {what.dtype}")
    if tokens.dim() == 2:
        tokens, weights = tokens.unsqueeze(1), weights.unsqueeze(1) if weights.dim() == 2 else weights
    if tokens.dim() != 3 or weights.shape != tokens.shape:
        raise ValueError(f"{fn}: tokens and weights must both be [n, slots, k] (or [n, k]); got {tuple(tokens.shape)} and {tuple(weights.shape)}")
    n, s, k = tokens.shape
    if not 1 <= s <= DECODE_MAX_SLOTS or not 1 <= k <= MAX_TOPK:
        raise ValueError(f"{fn}: {s} slots of {k} ids per row unsupported (1 .. {DECODE_MAX_SLOTS} slots, 1 .. {MAX_TOPK} ids)")
    if what.dim() != 2 or what.shape[1] % 4 or what.shape[0] < 1:
        raise ValueError(f"{fn}: the normalised codebook must be [n_codes, d] with d % 4 == 0, got {tuple(what.shape)}")
    regions = [(0, what.shape[0])] * s if regions is None else [(int(lo), int(size)) for lo, size in regions]
    if len(regions) != s:
        raise ValueError(f"{fn}: {len(regions)} regions for {s} slots")
    for lo, size in regions:
        if lo < 0 or size < 1 or lo + size > what.shape[0]:
            raise ValueError(f"{fn}: region [{lo}, +{size}) is not inside the {what.shape[0]} codes")
    if g_out is not None and (not isinstance(g_out, torch.Tensor) or g_out.dtype != torch.float32 or g_out.shape != (n, s * what.shape[1])):
        raise ValueError(f"{fn}: g_out must be fp32 [{n}, {s * what.shape[1]}]")
    return tokens, weights, regions


def _decode_on_device(tokens, weights, what, regions):
    """the device half of _decode_args: contiguous device tensors (MedTokLibraryError for anything else) and the regions as C arrays"""
    tokens, weights, what = _dev(tokens, "tokens", torch.int64), _dev(weights, "weights"), _dev(what, "what")
    import ctypes as C
    arr = C.c_int64 * len(regions)
    return tokens, weights, what, arr(*[r[0] for r in regions]), arr(*[r[1] for r in regions])


def decode_tokens(tokens, weights, what, regions=None, out=None, status=None):
    """Embedding from stored tokens: out[r, s*d:(s+1)*d] = sum_j weights[r, s, j] * what[lo_s + tokens[r, s, j]] -> [n, slots * d].

    tokens int64 / weights fp32 [n, slots, k] (or [n, k]: one slot), region-local ids; what [n_codes, d]: the NORMALISED codebook;
    regions: per slot (lo, size) in rows of `what` (default: the whole table for every slot).  `out` may be a column block of a wider
    tensor.  status: an int32 device tensor of one ZEROED element, or None; bit s is set when slot s held an id outside its region
    (those blocks are written as zeros) -- nothing is read back here."""
    tokens, weights, what, los, sizes = _decode_args("decode_tokens", tokens, weights, what, regions)
    n, s, k = tokens.shape
    d = what.shape[1]
    zq, stride = _zq_out(out, n, s * d, what)
    if status is not None:
        status = _dev(status, "status", torch.int32)
    lib = _lib.load()
    with _on(what.device):
        _lib.check(lib.medtok_decode_tokens_f32(tokens.data_ptr(), weights.data_ptr(), n, s, k, what.data_ptr(), what.shape[0], d, los, sizes,
                                                zq.data_ptr(), stride, _ptr(status), _stream(what)), "medtok_decode_tokens_f32")
    return zq


def decode_tokens_backward(g_out, tokens, weights, what, regions=None, want_g_w: bool = True, want_g_code: bool = True, status=None):
    """Backward of decode_tokens from g_out [n, slots * d]: (g_w [n, slots, k] or None, g_code [n * slots * k, d] or None, g_ids
    [n * slots * k] int64 or None).  g_code[i] = w_i * g_out block is the gradient w.r.t. the normalised code what[g_ids[i]] (GLOBAL
    ids): `ema_stats(g_code, g_ids, n_codes)` sums it per code in row order, `normalize_backward(..., live=bins)` takes it to the weight."""
    if not want_g_w and not want_g_code:
        raise ValueError("decode_tokens_backward: nothing to compute")
    if g_out is None:
        raise ValueError("decode_tokens_backward: g_out is required")
    tokens, weights, what, los, sizes = _decode_args("decode_tokens_backward", tokens, weights, what, regions, g_out=g_out)
    n, s, k = tokens.shape
    d = what.shape[1]
    if not g_out.is_cuda:
        _dev(g_out, "g_out")
    if n and not (g_out.stride(1) == 1 and g_out.stride(0) >= s * d and g_out.stride(0) % 4 == 0 and g_out.data_ptr() % 16 == 0):
        g_out = g_out.contiguous()
    if status is not None:
        status = _dev(status, "status", torch.int32)
    dev = what.device
    g_w = torch.empty((n, s, k), dtype=torch.float32, device=dev) if want_g_w else None
    g_code = torch.empty((n * s * k, d), dtype=torch.float32, device=dev) if want_g_code else None
    g_ids = torch.empty(n * s * k, dtype=torch.int64, device=dev) if want_g_code else None
    lib = _lib.load()
    with _on(dev):
        _lib.check(lib.medtok_decode_tokens_backward_f32(g_out.data_ptr(), g_out.stride(0) if n else 0, tokens.data_ptr(), weights.data_ptr(), n, s, k,
                                                         what.data_ptr(), what.shape[0], d, los, sizes, _ptr(g_w), _ptr(g_code), _ptr(g_ids),
                                                         _ptr(status), _stream(what)), "medtok_decode_tokens_backward_f32")
    return g_w, g_code, g_ids


EMBED_BAD_INDEX_BIT = 4
EMBED_OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _embed_mask(fn, pad_mask, index):
    """pad_mask (bool or uint8, the shape of index, True / non-zero = padded) as a flat uint8 view, or None"""
    if pad_mask is None:
        return None
    if not isinstance(pad_mask, torch.Tensor) or pad_mask.dtype not in (torch.bool, torch.uint8) or pad_mask.shape != index.shape:
        raise ValueError(f"{fn}: pad_mask must be a bool or uint8 tensor of index's shape {tuple(index.shape)}, got "
                         f"{getattr(pad_mask, 'dtype', type(pad_mask))} {tuple(getattr(pad_mask, 'shape', ()))}")
    return pad_mask


def _embed_mask_on_device(pad_mask):
    if pad_mask is None:
        return None
    if not pad_mask.is_cuda:
        _dev(pad_mask, "pad_mask", pad_mask.dtype)
    pad_mask = pad_mask.contiguous()
    return pad_mask.view(torch.uint8) if pad_mask.dtype == torch.bool else pad_mask


def _embed_miss(fn, miss, width):
    """the miss row of embed_codes / embed_pool: None, or fp32 [width] or [1, width]"""
    if miss is not None and (not isinstance(miss, torch.Tensor) or miss.dtype != torch.float32 or miss.numel() != width or miss.dim() not in (1, 2)
                             or miss.shape[-1] != width):
        raise ValueError(f"{fn}: miss must be fp32 [{width}] or [1, {width}], got {getattr(miss, 'dtype', type(miss))} "
                         f"{tuple(getattr(miss, 'shape', ()))}")


def embed_codes(index, tokens, weights, what, regions=None, miss=None, pad_mask=None, out=None, out_dtype=torch.float32, status=None):
    """Embeddings of code indices straight from the stored token table: what `table[index]` gives over the table
    decode_tokens(tokens, weights, ...) would build (plus a miss row), in one launch and without the table -> [*index.shape, slots * d].

    index int64, any shape; tokens int64 / weights fp32 [num_codes, slots, k] (region-local ids); what, regions: as decode_tokens.
    miss: fp32 [slots * d] (or [1, slots * d]), the row of index == num_codes, or None; pad_mask: bool / uint8 of index's shape,
    True = padded.  Padded positions are zeros whatever their index holds; an index in [0, num_codes) gives the bits of decode_tokens
    on that code's rows; num_codes gives `miss`; any other index gives zeros and sets bit 4 of `status` (an int32 device tensor of one
    ZEROED element, or None; bit s: slot s of some code held an id outside its region) -- nothing is read back here.
    out_dtype: torch.float32, float16 or bfloat16 (the fp32 result rounded once to nearest even: equal to `.to(out_dtype)` of it).
    `out`: a [index.numel(), slots * d] device view of that dtype with unit column stride, e.g. a column block of a wider tensor."""
    fn = "embed_codes"
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"{fn}: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
    if out_dtype not in EMBED_OUT_DTYPES:
        raise ValueError(f"{fn}: out_dtype must be one of {EMBED_OUT_DTYPES}, got {out_dtype!r}")
    pad_mask = _embed_mask(fn, pad_mask, index)
    tokens, weights, regions = _decode_shapes(fn, tokens, weights, what, regions)
    num_codes, s, k = tokens.shape
    if num_codes < 1:
        raise ValueError(f"{fn}: the token table is empty")
    d = what.shape[1]
    n, width = index.numel(), s * d
    _embed_miss(fn, miss, width)
    if out is not None:
        align = 16 if out_dtype == torch.float32 else 8
        if not (isinstance(out, torch.Tensor) and out.dtype == out_dtype and tuple(out.shape) == (n, width) and out.stride(1) == 1
                and out.stride(0) % 4 == 0 and out.data_ptr() % align == 0):
            raise ValueError(f"{fn}: out must be a {out_dtype} [{n}, {width}] view with unit column stride and {align}-byte aligned rows")
    index = _dev(index, "index", torch.int64)
    tokens, weights, what, los, sizes = _decode_on_device(tokens, weights, what, regions)
    miss = None if miss is None else _dev(miss, "miss")
    pad_mask = _embed_mask_on_device(pad_mask)
    if out is not None and not out.is_cuda:
        _dev(out, "out", out_dtype)
    if status is not None:
        status = _dev(status, "status", torch.int32)
    res = torch.empty((n, width), dtype=out_dtype, device=what.device) if out is None else out
    stride = res.stride(0) if n else 0
    lib = _lib.load()
    with _on(what.device):
        head = (index.data_ptr(), _ptr(pad_mask), n, tokens.data_ptr(), weights.data_ptr(), num_codes, s, k, what.data_ptr(), what.shape[0], d,
                los, sizes, _ptr(miss), res.data_ptr(), stride)
        if out_dtype == torch.float32:
            _lib.check(lib.medtok_embed_codes_f32(*head, _ptr(status), _stream(what)), "medtok_embed_codes_f32")
        else:
            _lib.check(lib.medtok_embed_codes_f16(*head, int(out_dtype == torch.bfloat16), _ptr(status), _stream(what)), "medtok_embed_codes_f16")
    return res.view(*index.shape, width) if out is None else out


def embed_codes_miss_grad(g_out, index, num_codes, pad_mask=None):
    """Gradient of embed_codes' miss row: the fp32 sum [width] of g_out [*index.shape, width] over the positions with
    index == num_codes that are not padded, added in a fixed order (no float atomics: two runs give the same bits).  A half-precision
    g_out is converted to fp32 first."""
    fn = "embed_codes_miss_grad"
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"{fn}: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
    if (not isinstance(g_out, torch.Tensor) or g_out.dtype not in EMBED_OUT_DTYPES or g_out.dim() < 1
            or g_out.numel() != index.numel() * g_out.shape[-1] or g_out.shape[-1] < 1):
        raise ValueError(f"{fn}: g_out must be a floating [*{tuple(index.shape)}, width] tensor, got {tuple(getattr(g_out, 'shape', ()))}")
    pad_mask = _embed_mask(fn, pad_mask, index)
    index = _dev(index, "index", torch.int64)
    pad_mask = _embed_mask_on_device(pad_mask)
    width, n = g_out.shape[-1], index.numel()
    g_out = _dev(g_out.float().reshape(n, width), "g_out")
    g_miss = torch.empty(width, dtype=torch.float32, device=g_out.device)
    lib = _lib.load()
    ws = _ws(lib.medtok_embed_codes_miss_grad_workspace_bytes(n, width), g_out)
    with _on(g_out.device):
        _lib.check(lib.medtok_embed_codes_miss_grad_f32(g_out.data_ptr(), width, index.data_ptr(), _ptr(pad_mask), n, int(num_codes), width,
                                                        g_miss.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g_out)),
                   "medtok_embed_codes_miss_grad_f32")
    return g_miss


EMBED_CODE_GRAD_CHUNK = 256                 # contributions per fmaf chain of embed_codes_code_grad (MEDTOK_EMBED_CODE_GRAD_CHUNK: part of the bits)


def _embed_grad_prepare(fn, index, tokens, weights, regions, pad_mask, g, g_name):
    """What embed_codes_code_grad and embed_project_table_grad do between their shape checks and the call: the bound of the sort's 32-bit payload, then index, lists and mask
    as device tensors, g checked to be one, and the regions as C arrays -> (index, tokens, weights, pad_mask, lo[], size[])"""
    n, (_, s, k) = index.numel(), tokens.shape
    if n * s * k >= 1 << 31:
        raise ValueError(f"{fn}: {n} positions x {s} slots x {k} ids reach 2^31 contributions (the sort's payload is 32-bit): split the batch")
    index = _dev(index, "index", torch.int64)
    tokens, weights = _dev(tokens, "tokens", torch.int64), _dev(weights, "weights")
    pad_mask = _embed_mask_on_device(pad_mask)
    if not g.is_cuda:
        _dev(g, g_name, g.dtype)
    import ctypes as C
    arr = C.c_int64 * s
    return index, tokens, weights, pad_mask, arr(*[r[0] for r in regions]), arr(*[r[1] for r in regions])


def embed_codes_code_grad(g_out, index, tokens, weights, what_shape_or_what, regions=None, pad_mask=None):
    """Gradient of embed_codes w.r.t. the NORMALISED codebook, straight from the upstream gradient -> (g_what [n_codes, d], bins [n_codes]).

    g_out [*index.shape, slots * d] (a half-precision one is converted to fp32 first); index, tokens, weights, regions, pad_mask as
    embed_codes; what_shape_or_what: the normalised codebook or its shape (n_codes, d) -- its values are not read.  Contribution
    (p, s, j) is live exactly when the forward mixes that (position, slot): not padded, 0 <= index[p] < num_codes, every id of the
    slot inside its region.  It adds weights[index[p], s, j] * g_out[p, s * d : (s + 1) * d] to row lo_s + tokens[index[p], s, j];
    bins counts a row's live contributions, a row without any is exactly zero.  The order is fixed (a row's contributions by
    increasing (p, s, j), one fmaf chain from +0 per EMBED_CODE_GRAD_CHUNK of them, the chunk sums added in order; no float atomics):
    two calls give the same bits.  No [n * slots * k, d] buffer is made and nothing is read back.
    `normalize_backward(g_what, what, weight, live=bins)` takes the result to the codebook weight."""
    fn = "embed_codes_code_grad"
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"{fn}: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
    pad_mask = _embed_mask(fn, pad_mask, index)
    if isinstance(what_shape_or_what, torch.Tensor):
        what = what_shape_or_what
    else:
        shape = tuple(int(v) for v in what_shape_or_what)
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError(f"{fn}: the codebook's shape must be (n_codes, d), got {shape}")
        what = torch.empty(shape, dtype=torch.float32, device="meta")          # (shape checks only: no storage)
    tokens, weights, regions = _decode_shapes(fn, tokens, weights, what, regions)
    num_codes, s, k = tokens.shape
    if num_codes < 1:
        raise ValueError(f"{fn}: the token table is empty")
    n_codes, d = what.shape
    n, width = index.numel(), s * d
    if (not isinstance(g_out, torch.Tensor) or g_out.dtype not in EMBED_OUT_DTYPES or g_out.dim() < 1 or g_out.shape[-1] != width
            or g_out.numel() != n * width):
        raise ValueError(f"{fn}: g_out must be a floating [*{tuple(index.shape)}, {width}] tensor, got {getattr(g_out, 'dtype', type(g_out))} "
                         f"{tuple(getattr(g_out, 'shape', ()))}")
    index, tokens, weights, pad_mask, los, sizes = _embed_grad_prepare(fn, index, tokens, weights, regions, pad_mask, g_out, "g_out")
    g_out = g_out.reshape(n, width).float()
    if n and not (g_out.stride(1) == 1 and g_out.stride(0) >= width and g_out.stride(0) % 4 == 0 and g_out.data_ptr() % 16 == 0):
        g_out = g_out.contiguous()
    lib = _lib.load()
    dev = g_out.device
    g_what = torch.empty((n_codes, d), dtype=torch.float32, device=dev)
    bins = torch.empty(n_codes, dtype=torch.float32, device=dev)
    ws = _ws(lib.medtok_embed_code_grad_workspace_bytes(n, s, k, n_codes, d), g_out)
    with _on(dev):
        _lib.check(lib.medtok_embed_code_grad_f32(g_out.data_ptr(), g_out.stride(0) if n else 0, index.data_ptr(), _ptr(pad_mask), n, tokens.data_ptr(),
                                                  weights.data_ptr(), num_codes, s, k, n_codes, d, los, sizes, g_what.data_ptr(), bins.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream(g_out)), "medtok_embed_code_grad_f32")
    return g_what, bins


EMBED_G_DTYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}       # MEDTOK_EMBED_G_F32 / _F16 / _BF16


def embed_project_table_grad(g, index, tokens, weights, row_regions, pad_mask=None):
    """The upstream gradient of embed_project / embed_sequence's rows summed per row of the folded table -> (G [rows, Hp], bins [rows]),
    rows = the end of the last region.

    g [*index.shape, Hp], fp32, fp16 or bf16 (a 16-bit g goes to the kernel as it is and is widened in registers: exact), Hp % 4 == 0;
    a view with unit column stride and 16-byte aligned rows (a column block of a wider tensor) is read in place, anything else is made
    contiguous.  index, tokens, weights, pad_mask as embed_project; row_regions [(offset, size)] per slot as fold_projector returned
    them (size is also the range of the slot's ids; regions may coincide).  Contribution (p, s, j) is live exactly when the forward
    mixes that (position, slot) -- embed_codes_code_grad's rule; a miss position contributes nothing -- and adds
    weights[index[p], s, j] * g[p] (the whole row, the same for every slot) to row offset_s + tokens[index[p], s, j]; bins counts a row's
    live contributions, a row without any is exactly zero.  Order and chunking are embed_codes_code_grad's (EMBED_CODE_GRAD_CHUNK): that
    function gives the same bits on g tiled S times.  No float atomics, no [n * S, Hp] buffer, nothing read back.
    dW[:, s * e : (s + 1) * e] = G_s^T . what[region s] and d what[region s] += G_s . W_s follow by small_gemm."""
    fn = "embed_project_table_grad"
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"{fn}: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
    pad_mask = _embed_mask(fn, pad_mask, index)
    n = index.numel()
    if (not isinstance(g, torch.Tensor) or g.dtype not in EMBED_G_DTYPE_CODES or g.dim() < 1 or g.shape[-1] < 1 or g.shape[-1] % 4
            or g.numel() != n * g.shape[-1]):
        raise ValueError(f"{fn}: g must be an fp32, fp16 or bf16 [*{tuple(index.shape)}, Hp] tensor with Hp % 4 == 0, got "
                         f"{getattr(g, 'dtype', type(g))} {tuple(getattr(g, 'shape', ()))}")
    hp = int(g.shape[-1])
    try:
        row_regions = [(int(lo), int(size)) for lo, size in row_regions]
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: row_regions must be a sequence of (offset, size) pairs, got {row_regions!r}") from None
    if not row_regions or any(lo < 0 or size < 1 for lo, size in row_regions):
        raise ValueError(f"{fn}: every region needs offset >= 0 and size >= 1, got {row_regions}")
    rows = max(lo + size for lo, size in row_regions)
    if rows >= 1 << 31:
        raise ValueError(f"{fn}: {rows} table rows reach 2^31 (the sort's keys are 32-bit)")
    table = torch.empty((rows, hp), dtype=torch.float32, device="meta")          # (shape checks only: no storage)
    tokens, weights, row_regions = _decode_shapes(fn, tokens, weights, table, row_regions)
    num_codes, s, k = tokens.shape
    if num_codes < 1:
        raise ValueError(f"{fn}: the token table is empty")
    index, tokens, weights, pad_mask, los, sizes = _embed_grad_prepare(fn, index, tokens, weights, row_regions, pad_mask, g, "g")
    g = g.reshape(n, hp)
    if n and not (g.stride(1) == 1 and g.stride(0) >= hp and g.stride(0) * g.element_size() % 16 == 0 and g.data_ptr() % 16 == 0):
        g = g.contiguous()
    lib = _lib.load()
    dev = g.device
    G = torch.empty((rows, hp), dtype=torch.float32, device=dev)
    bins = torch.empty(rows, dtype=torch.float32, device=dev)
    ws = _ws(lib.medtok_embed_table_grad_workspace_bytes(n, s, k, rows, hp), g)
    with _on(dev):
        _lib.check(lib.medtok_embed_table_grad(g.data_ptr(), EMBED_G_DTYPE_CODES[g.dtype], g.stride(0) if n else 0, index.data_ptr(), _ptr(pad_mask), n,
                                               tokens.data_ptr(), weights.data_ptr(), num_codes, s, k, rows, hp, los, sizes, G.data_ptr(),
                                               bins.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g)), "medtok_embed_table_grad")
    return G, bins


EMBED_POOL_CHUNK = 16                       # positions per block of embed_pool_partial_kernel (MEDTOK_EMBED_POOL_CHUNK: part of the result's bits)
EMBED_POOL_MAX_WIDTH = 4096


def embed_pool(index, tokens, weights, what, regions=None, miss=None, pad_mask=None, normalize: bool = True, status=None):
    """The normalised mean of each bag of code indices, straight from the stored token table -> (pooled fp32 [B, slots * d],
    counts int32 [B, 2]).

    index int64 [B, L]; tokens, weights, what, regions, miss, status: as embed_codes; pad_mask: bool / uint8 [B, L], True = padded,
    any pattern.  With row(p) what embed_codes gives for position p,
        pooled[b] = (sum over the unpadded p of bag b, in a fixed order, of n(row(p))) / live_b,    n(v) = v / max(|v|_2, 1e-12) over the whole row
    (normalize=False: n(v) = v); live_b counts the unpadded positions (a bad index counts, as a row of zeros); a bag without one is a row
    of zeros; padded positions are not read.  counts[b] = (live_b, the unpadded miss positions of b): what embed_pool_miss_grad needs.
    The order is fixed but not strict position order (per EMBED_POOL_CHUNK positions: positions j, j + 4, .. per wavefront j % 4, then the
    four wavefronts, then the chunks; include/medtok_vq.h) and there are no float atomics: two runs give the same bits, and they depend on
    (index, pad_mask, L, the tables) only.
    slots * k <= 64 and slots * d <= EMBED_POOL_MAX_WIDTH.  Nothing is read back here."""
    fn = "embed_pool"
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"{fn}: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
    if index.dim() != 2:
        raise ValueError(f"{fn}: index must be [bags, bag_len], got {tuple(index.shape)}")
    pad_mask = _embed_mask(fn, pad_mask, index)
    tokens, weights, regions = _decode_shapes(fn, tokens, weights, what, regions)
    num_codes, s, k = tokens.shape
    if num_codes < 1:
        raise ValueError(f"{fn}: the token table is empty")
    d = what.shape[1]
    width = s * d
    if s * k > 64 or width > EMBED_POOL_MAX_WIDTH:
        raise ValueError(f"{fn}: {s} slots x {k} ids (at most 64 entries per code) and rows of {width} floats (at most {EMBED_POOL_MAX_WIDTH}) unsupported")
    _embed_miss(fn, miss, width)
    index = _dev(index, "index", torch.int64)
    tokens, weights, what, los, sizes = _decode_on_device(tokens, weights, what, regions)
    miss = None if miss is None else _dev(miss, "miss")
    pad_mask = _embed_mask_on_device(pad_mask)
    if status is not None:
        status = _dev(status, "status", torch.int32)
    bags, bag_len = index.shape
    pooled = torch.empty((bags, width), dtype=torch.float32, device=what.device)
    counts = torch.empty((bags, 2), dtype=torch.int32, device=what.device)
    lib = _lib.load()
    ws = _ws(lib.medtok_embed_pool_workspace_bytes(bags, bag_len, width), what)
    with _on(what.device):
        _lib.check(lib.medtok_embed_pool_f32(index.data_ptr(), _ptr(pad_mask), bags, bag_len, tokens.data_ptr(), weights.data_ptr(), num_codes, s, k,
                                             what.data_ptr(), what.shape[0], d, los, sizes, _ptr(miss), int(bool(normalize)), pooled.data_ptr(),
                                             width, counts.data_ptr(), _ptr(status), ws.data_ptr(), ws.numel(), _stream(what)),
                   "medtok_embed_pool_f32")
    return pooled, counts


def embed_pool_miss_grad(g_out, counts):
    """What embed_pool's upstream gradient g_out [B, width] sends to the vector every miss position carries: the fp32 [width] sum over
    the bags of (miss_b / live_b) * g_out[b], counts [B, 2] int32 as embed_pool returned them, added in a fixed order (no float atomics:
    two runs give the same bits; bags with live_b == 0 or miss_b == 0 are skipped).  With normalize=False this is the gradient of the
    miss row; otherwise normalize_backward takes it there.  A half-precision g_out is converted to fp32 first."""
    fn = "embed_pool_miss_grad"
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != 2:
        raise ValueError(f"{fn}: counts must be an int32 [bags, 2] tensor, got {getattr(counts, 'dtype', type(counts))} "
                         f"{tuple(getattr(counts, 'shape', ()))}")
    bags = counts.shape[0]
    if (not isinstance(g_out, torch.Tensor) or g_out.dtype not in EMBED_OUT_DTYPES or g_out.dim() != 2 or g_out.shape[0] != bags
            or g_out.shape[1] < 1):
        raise ValueError(f"{fn}: g_out must be a floating [{bags}, width] tensor, got {tuple(getattr(g_out, 'shape', ()))}")
    counts = _dev(counts, "counts", torch.int32)
    width = g_out.shape[1]
    g_out = _dev(g_out.float(), "g_out")
    g_acc = torch.empty(width, dtype=torch.float32, device=g_out.device)
    lib = _lib.load()
    ws = _ws(lib.medtok_embed_pool_workspace_bytes(bags, 1, width), g_out)
    with _on(g_out.device):
        _lib.check(lib.medtok_embed_pool_miss_grad_f32(g_out.data_ptr(), width, counts.data_ptr(), bags, width, g_acc.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), _stream(g_out)), "medtok_embed_pool_miss_grad_f32")
    return g_acc


def embed_pool_segments(index, segment_id, n_segments, tokens, weights, what, regions=None, miss=None, pad_mask=None, normalize: bool = False,
                        status=None):
    """embed_pool with a bag per (batch row, segment): (out fp32 [B, V, slots * d], counts int32 [B, V, 2]), V = n_segments.

    index, segment_id int64 [B, L]; tokens, weights, what, regions, miss, status: as embed_codes; pad_mask: bool / uint8 [B, L], True =
    padded, any pattern.  Bag (b, v) is the unpadded positions p of row b with segment_id[b, p] == v (ids in any order along the row, not
    necessarily contiguous), and with row(p), n(v) as embed_pool
        out[b, v] = (sum over the bag, in a fixed order, of n(row(b, p))) / count[b, v]
    An empty bag is a row of zeros; counts[b, v] = (count, the bag's miss positions): what embed_pool_miss_grad takes as
    counts.reshape(B * V, 2).  A padded position reads neither its index nor its segment id; an unpadded id outside [0, V) joins no bag
    and sets bit EMBED_BAD_SEGMENT_BIT of `status`; a bad code index counts in its bag as a row of zeros (bit EMBED_BAD_INDEX_BIT).
    The order (include/medtok_vq.h): a bag's positions ascending, chunks of EMBED_POOL_CHUNK entries summed as embed_pool sums a chunk,
    chunk sums in chunk order from +0, a true division -- no float atomics, two runs give the same bits, and with V = 1, ids 0 and no
    mask the result is embed_pool's bit for bit.  normalize defaults to False here (embed_pool: True).
    slots * k <= 64, slots * d <= EMBED_POOL_MAX_WIDTH, B * L < 2^31, B * V + 1 < 2^31.  Every step is a kernel launch and nothing is read back."""
    fn = "embed_pool_segments"
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"{fn}: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
    if index.dim() != 2:
        raise ValueError(f"{fn}: index must be [batch, length], got {tuple(index.shape)}")
    batch, length = index.shape
    if not isinstance(segment_id, torch.Tensor) or segment_id.dtype != torch.int64 or segment_id.shape != index.shape:
        raise ValueError(f"{fn}: segment_id must be an int64 [{batch}, {length}] tensor, got {getattr(segment_id, 'dtype', type(segment_id))} "
                         f"{tuple(getattr(segment_id, 'shape', ()))}")
    n_segments = int(n_segments)
    if n_segments < 1:
        raise ValueError(f"{fn}: n_segments = {n_segments} must be >= 1")
    if batch * length >= 1 << 31:
        raise ValueError(f"{fn}: {batch} x {length} positions reach 2^31: split the batch")
    if batch * n_segments + 1 >= 1 << 31:
        raise ValueError(f"{fn}: {batch} x {n_segments} segments + 1 reach 2^31: split the batch")
    pad_mask = _embed_mask(fn, pad_mask, index)
    tokens, weights, regions = _decode_shapes(fn, tokens, weights, what, regions)
    num_codes, s, k = tokens.shape
    if num_codes < 1:
        raise ValueError(f"{fn}: the token table is empty")
    d = what.shape[1]
    width = s * d
    if s * k > 64 or width > EMBED_POOL_MAX_WIDTH:
        raise ValueError(f"{fn}: {s} slots x {k} ids (at most 64 entries per code) and rows of {width} floats (at most {EMBED_POOL_MAX_WIDTH}) unsupported")
    _embed_miss(fn, miss, width)
    index = _dev(index, "index", torch.int64)
    segment_id = _dev(segment_id, "segment_id", torch.int64)
    tokens, weights, what, los, sizes = _decode_on_device(tokens, weights, what, regions)
    miss = None if miss is None else _dev(miss, "miss")
    pad_mask = _embed_mask_on_device(pad_mask)
    if status is not None:
        status = _dev(status, "status", torch.int32)
    out = torch.empty((batch, n_segments, width), dtype=torch.float32, device=what.device)
    counts = torch.empty((batch, n_segments, 2), dtype=torch.int32, device=what.device)
    lib = _lib.load()
    ws = _ws(lib.medtok_embed_pool_segments_workspace_bytes(batch, length, n_segments, width), what)
    with _on(what.device):
        _lib.check(lib.medtok_embed_pool_segments_f32(index.data_ptr(), _ptr(pad_mask), segment_id.data_ptr(), batch, length, n_segments,
                                                      tokens.data_ptr(), weights.data_ptr(), num_codes, s, k, what.data_ptr(), what.shape[0], d,
                                                      los, sizes, _ptr(miss), int(bool(normalize)), out.data_ptr(), width, counts.data_ptr(),
                                                      _ptr(status), ws.data_ptr(), ws.numel(), _stream(what)), "medtok_embed_pool_segments_f32")
    return out, counts


def fold_projector(what, regions, W, b=None, miss=None, e_dim=None):
    """The consumer's projector applied to the codebook instead of to every position: what embed_project gathers from.

    what [n_codes, d]: the NORMALISED codebook (d % 4 == 0; its first e_dim columns count, default d); regions: per slot (lo, size) in
    rows of `what`; W fp32 [H, S * e_dim], b fp32 [H] or None: the nn.Linear that follows the lookup; miss fp32 [S * e_dim] (or
    [1, S * e_dim]) or None.  Returns (table, row_regions, bias, miss_row): table [sum of sizes, Hp] (Hp = H rounded up to 4, the added
    columns zeros) stacks P_s = what[lo_s : lo_s + size_s] @ W[:, s * e_dim : (s + 1) * e_dim]^T per slot, row_regions [(offset_s,
    size_s)] says where, bias [Hp], miss_row [Hp] = W @ miss + b (or None).  Every product is small_gemm's exact fp32 chain: 2 * sum of
    sizes * e_dim * H flops, once per version of the weights."""
    fn = "fold_projector"
    if not all(isinstance(t, torch.Tensor) for t in (what, W)) or what.dtype != torch.float32 or W.dtype != torch.float32 or what.dim() != 2 or W.dim() != 2:
        raise ValueError(f"{fn}: what and W must be fp32 matrices")
    d = what.shape[1]
    e = d if e_dim is None else int(e_dim)
    regions = [(int(lo), int(size)) for lo, size in regions]
    s = len(regions)
    if not 1 <= s <= DECODE_MAX_SLOTS or not 1 <= e <= d or d % 4 or W.shape[1] != s * e:
        raise ValueError(f"{fn}: W must be [H, {s} * {e}] for {s} slots over a [n_codes, {d}] codebook, got {tuple(W.shape)}")
    for lo, size in regions:
        if lo < 0 or size < 1 or lo + size > what.shape[0]:
            raise ValueError(f"{fn}: region [{lo}, +{size}) is not inside the {what.shape[0]} codes")
    h = W.shape[0]
    hp = pad_dim(h)
    if b is not None and (not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or tuple(b.shape) != (h,)):
        raise ValueError(f"{fn}: b must be fp32 [{h}]")
    if miss is not None and (not isinstance(miss, torch.Tensor) or miss.dtype != torch.float32 or miss.numel() != s * e):
        raise ValueError(f"{fn}: miss must be fp32 [{s * e}]")
    what, W = _dev(what, "what"), _dev(W.detach(), "W")
    total = sum(size for _, size in regions)
    if total >= 2 ** 31:
        raise ValueError(f"{fn}: {total} table rows exceed what one lookup addresses")
    table = torch.empty((total, hp), dtype=torch.float32, device=what.device)
    Wp = torch.nn.functional.pad(W, (0, 0, 0, hp - h)) if hp != h else W                     # [Hp, S * e]: zero rows for the added columns
    row_regions, at = [], 0
    for i, (lo, size) in enumerate(regions):
        Ws = Wp[:, i * e:(i + 1) * e]
        Ws = torch.nn.functional.pad(Ws, (0, d - e)) if d != e else Ws.contiguous()          # (the codebook's padding columns are zeros)
        small_gemm(what[lo:lo + size], Ws, trans_b=True, out=table[at:at + size])
        row_regions.append((at, size))
        at += size
    bias = torch.zeros(hp, dtype=torch.float32, device=what.device)
    if b is not None:
        bias[:h] = _dev(b.detach(), "b")
    miss_row = None
    if miss is not None:
        miss_row = small_gemm(_dev(miss.detach(), "miss").reshape(1, s * e), Wp, trans_b=True).reshape(hp) + bias
    return table, row_regions, bias, miss_row


def _folded_shapes(fn, index, index_dims, tokens, weights, table, row_regions, bias, miss_row, pad_mask, out_dtype, width=None):
    """The ValueError half of embed_project / embed_sequence (index_dims = 2: index must be [batch, length]): types and shapes of the
    index, the mask, the stored lists against the folded tables, the bias and the miss row -> (pad_mask, tokens [num_codes, s, k],
    weights, row_regions, width); nothing is moved or loaded.  width: the width of embed_sequence's additive tensors (default: the tables')."""
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"{fn}: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
    if index_dims is not None and index.dim() != index_dims:
        raise ValueError(f"{fn}: index must be [batch, length], got {tuple(index.shape)}")
    if out_dtype not in EMBED_OUT_DTYPES:
        raise ValueError(f"{fn}: out_dtype must be one of {EMBED_OUT_DTYPES}, got {out_dtype!r}")
    pad_mask = _embed_mask(fn, pad_mask, index)
    tokens, weights, row_regions = _decode_shapes(fn, tokens, weights, table, row_regions)
    num_codes, s, k = tokens.shape
    if num_codes < 1:
        raise ValueError(f"{fn}: the token table is empty")
    if s * k > 64:
        raise ValueError(f"{fn}: {s} slots of {k} ids are more than the 64 entries per code the kernel takes")
    hp = table.shape[1]
    width = hp if width is None else int(width)
    if pad_dim(width) != hp:
        raise ValueError(f"{fn}: width = {width} does not pad to the tables' {hp} columns")
    for name, t in (("bias", bias), ("miss_row", miss_row)):
        if (t is not None or name == "bias") and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (hp,)):
            raise ValueError(f"{fn}: {name} must be fp32 [{hp}], got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return pad_mask, tokens, weights, row_regions, width


def _folded_on_device(index, tokens, weights, table, row_regions, bias, miss_row, pad_mask):
    """the device half: contiguous device tensors (MedTokLibraryError for anything else) and the regions as C arrays"""
    index = _dev(index, "index", torch.int64)
    tokens, weights, table, los, sizes = _decode_on_device(tokens, weights, table, row_regions)
    bias = _dev(bias, "bias")
    miss_row = None if miss_row is None else _dev(miss_row, "miss_row")
    return index, tokens, weights, table, los, sizes, bias, miss_row, _embed_mask_on_device(pad_mask)


def embed_project(index, tokens, weights, table, row_regions, bias, miss_row=None, pad_mask=None, out=None, out_dtype=torch.float32,
                  status=None):
    """projector(embed_codes(index, ...)) in one launch, without the [positions, slots * d] activation: the lookup over the folded
    tables of fold_projector -> [*index.shape, Hp].

    index, tokens, weights, pad_mask, out_dtype, status: as embed_codes (slots * k <= 64).  table [rows, Hp], row_regions [(offset,
    size)] per slot, bias [Hp], miss_row [Hp] or None: what fold_projector returned.  Per column one fp32 chain: bias, then slots
    ascending, then list order.  Padded positions are the bias row whatever their index holds; index == num_codes gives miss_row; any
    other index outside [0, num_codes) gives the bias row and sets bit 4 of `status`; a slot with an id outside its region contributes
    nothing and sets bit s -- nothing is read back here.  `out`: a [index.numel(), Hp] device view of out_dtype with unit column stride."""
    fn = "embed_project"
    pad_mask, tokens, weights, row_regions, _ = _folded_shapes(fn, index, None, tokens, weights, table, row_regions, bias, miss_row, pad_mask,
                                                               out_dtype)
    num_codes, s, k = tokens.shape
    hp = table.shape[1]
    n = index.numel()
    if out is not None:
        align = 16 if out_dtype == torch.float32 else 8
        if not (isinstance(out, torch.Tensor) and out.dtype == out_dtype and tuple(out.shape) == (n, hp) and out.stride(1) == 1
                and out.stride(0) % 4 == 0 and out.data_ptr() % align == 0):
            raise ValueError(f"{fn}: out must be a {out_dtype} [{n}, {hp}] view with unit column stride and {align}-byte aligned rows")
    index, tokens, weights, table, los, sizes, bias, miss_row, pad_mask = _folded_on_device(index, tokens, weights, table, row_regions, bias, miss_row,
                                                                                           pad_mask)
    if out is not None and not out.is_cuda:
        _dev(out, "out", out_dtype)
    if status is not None:
        status = _dev(status, "status", torch.int32)
    res = torch.empty((n, hp), dtype=out_dtype, device=table.device) if out is None else out
    stride = res.stride(0) if n else 0
    lib = _lib.load()
    with _on(table.device):
        head = (index.data_ptr(), _ptr(pad_mask), n, tokens.data_ptr(), weights.data_ptr(), num_codes, s, k, table.data_ptr(), table.shape[0], hp,
                los, sizes, bias.data_ptr(), _ptr(miss_row), res.data_ptr(), stride)
        if out_dtype == torch.float32:
            _lib.check(lib.medtok_embed_project_f32(*head, _ptr(status), _stream(table)), "medtok_embed_project_f32")
        else:
            _lib.check(lib.medtok_embed_project_f16(*head, int(out_dtype == torch.bfloat16), _ptr(status), _stream(table)), "medtok_embed_project_f16")
    return res.view(*index.shape, hp) if out is None else out


EMBED_BAD_SEGMENT_BIT = 5                   # MEDTOK_EMBED_BAD_SEGMENT_BIT: an unpadded position's segment id outside [0, V)
EMBED_SEQ_MAX_TERMS = 2                     # MEDTOK_EMBED_SEQ_MAX_TERMS: segment terms per call
EMBED_SEQ_MAX_SEGMENTS = 4096               # MEDTOK_EMBED_SEQ_MAX_SEGMENTS: V (the gradient keeps V x 4 columns of sums in 64 KiB of LDS)
EMBED_SEQ_GRAD_CHUNK = 256                  # positions per partial sum of embed_sequence_segment_grad (MEDTOK_EMBED_SEQ_GRAD_CHUNK: part of the bits)


def _sequence_parts(fn, batch, length, width, position_rows, segment_id, segment_rows, prefix):
    """The shape and dtype checks of the parts embed_sequence / embed_sequence_rows add to the [batch, length, width] rows ->
    (position_rows, segment_id, terms, prefix, n_segments, n_prefix); nothing here looks at a device."""
    def fp32(t, name, dims):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != dims or t.shape[-1] != width:
            raise ValueError(f"{fn}: {name} must be an fp32 {dims}-D tensor of width {width}, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    if position_rows is not None:
        fp32(position_rows, "position_rows", 2)
        if position_rows.shape[0] < length:
            raise ValueError(f"{fn}: position_rows holds {position_rows.shape[0]} rows, fewer than the {length} positions")
    terms = ()
    if segment_rows is not None:
        terms = (segment_rows,) if isinstance(segment_rows, torch.Tensor) else tuple(segment_rows)
        if not 1 <= len(terms) <= EMBED_SEQ_MAX_TERMS:
            raise ValueError(f"{fn}: segment_rows must be one tensor or a sequence of 1 .. {EMBED_SEQ_MAX_TERMS} tensors, got {len(terms)} terms")
    if terms and segment_id is None:
        raise ValueError(f"{fn}: segment_rows without segment_id")
    if segment_id is not None and not terms:
        raise ValueError(f"{fn}: segment_id without segment_rows")
    n_segments = 0
    if terms:
        if not isinstance(segment_id, torch.Tensor) or segment_id.dtype != torch.int64 or tuple(segment_id.shape) != (batch, length):
            raise ValueError(f"{fn}: segment_id must be an int64 [{batch}, {length}] tensor, got {getattr(segment_id, 'dtype', type(segment_id))} "
                             f"{tuple(getattr(segment_id, 'shape', ()))}")
        for i, t in enumerate(terms):
            fp32(t, f"segment_rows[{i}]", 3)
            if t.shape[0] != batch or t.shape[1] != terms[0].shape[1]:
                raise ValueError(f"{fn}: segment_rows[{i}] must be [{batch}, V, {width}] with one V for all terms, got {tuple(t.shape)}")
        n_segments = int(terms[0].shape[1])
        if not 1 <= n_segments <= EMBED_SEQ_MAX_SEGMENTS:
            raise ValueError(f"{fn}: V = {n_segments} segments unsupported (1 .. {EMBED_SEQ_MAX_SEGMENTS})")
    n_prefix = 0
    if prefix is not None:
        fp32(prefix, "prefix", 3)
        if prefix.shape[0] != batch:
            raise ValueError(f"{fn}: prefix must be [{batch}, P, {width}], got {tuple(prefix.shape)}")
        n_prefix = int(prefix.shape[1])
    if batch * (n_prefix + length) >= 1 << 31:
        raise ValueError(f"{fn}: {batch} x ({n_prefix} + {length}) rows reach 2^31: split the batch")
    return position_rows, segment_id, terms, prefix, n_segments, n_prefix


def _sequence_parts_on_device(position_rows, segment_id, terms, prefix, columns=0):
    """the parts as contiguous device tensors; columns > 0: that many zero columns are appended (the folded tables' rows are hp wide)"""
    def dev(t, name):
        t = _dev(t.detach(), name)
        return torch.nn.functional.pad(t, (0, columns)) if columns else t
    position_rows = None if position_rows is None else dev(position_rows, "position_rows")
    segment_id = None if segment_id is None else _dev(segment_id, "segment_id", torch.int64)
    terms = tuple(dev(t, f"segment_rows[{i}]") for i, t in enumerate(terms))
    prefix = None if prefix is None or prefix.shape[1] == 0 else dev(prefix, "prefix")
    return position_rows, segment_id, terms, prefix


def embed_sequence(index, tokens, weights, table, row_regions, bias, miss_row=None, pad_mask=None, position_rows=None, segment_id=None,
                   segment_rows=None, prefix=None, width=None, out_dtype=torch.float32, status=None):
    """embed_project's rows with the consumer's sequence assembly in the same launch -> (seq [B, P + L, Hp]).

    index int64 [B, L]; tokens .. pad_mask, out_dtype: as embed_project.  With r0 the row embed_project gives for position (b, p):
      padded position      seq[b, P + p] = r0 (the bias row); nothing is added; neither index[b, p] nor segment_id[b, p] is read
      unpadded position    seq[b, P + p] = ((r0 + position_rows[p]) + segment_rows[0][b, g]) + segment_rows[1][b, g],  g = segment_id[b, p]
      seq[b, :P]           prefix[b]
    plain fp32 additions in that order on the fp32 value of the lookup's chain: in fp32 the bits of torch adding the tensors to
    embed_project's result one after the other.  position_rows fp32 [>= L, width]; segment_id int64 [B, L]; segment_rows: one fp32
    [B, V, width] tensor or a sequence of at most EMBED_SEQ_MAX_TERMS, V <= EMBED_SEQ_MAX_SEGMENTS; prefix fp32 [B, P, width]; each may be
    None.  width (default Hp): the width of these tensors, Hp or the projector's H with pad_dim(H) == Hp (zero columns are appended
    here).  A g outside [0, V) adds no segment term and sets bit EMBED_BAD_SEGMENT_BIT of `status`; a miss position and a bad code index
    take the adds like any unpadded position.  Nothing is read back here."""
    fn = "embed_sequence"
    pad_mask, tokens, weights, row_regions, width = _folded_shapes(fn, index, 2, tokens, weights, table, row_regions, bias, miss_row, pad_mask,
                                                                   out_dtype, width)
    num_codes, s, k = tokens.shape
    hp = table.shape[1]
    batch, length = index.shape
    parts = _sequence_parts(fn, batch, length, width, position_rows, segment_id, segment_rows, prefix)
    n_segments, n_prefix = parts[4:]
    index, tokens, weights, table, los, sizes, bias, miss_row, pad_mask = _folded_on_device(index, tokens, weights, table, row_regions, bias, miss_row,
                                                                                           pad_mask)
    position_rows, segment_id, terms, prefix = _sequence_parts_on_device(*parts[:4], columns=hp - width)
    if status is not None:
        status = _dev(status, "status", torch.int32)
    res = torch.empty((batch, n_prefix + length, hp), dtype=out_dtype, device=table.device)
    lib = _lib.load()
    with _on(table.device):
        head = (index.data_ptr(), _ptr(pad_mask), batch, length, tokens.data_ptr(), weights.data_ptr(), num_codes, s, k, table.data_ptr(),
                table.shape[0], hp, los, sizes, bias.data_ptr(), _ptr(miss_row), _ptr(position_rows),
                0 if position_rows is None else position_rows.shape[0], _ptr(segment_id), _ptr(terms[0] if terms else None),
                _ptr(terms[1] if len(terms) > 1 else None), n_segments, _ptr(prefix), n_prefix, res.data_ptr(), hp)
        if out_dtype == torch.float32:
            _lib.check(lib.medtok_embed_sequence_f32(*head, _ptr(status), _stream(table)), "medtok_embed_sequence_f32")
        else:
            _lib.check(lib.medtok_embed_sequence_f16(*head, int(out_dtype == torch.bfloat16), _ptr(status), _stream(table)), "medtok_embed_sequence_f16")
    return res


def embed_sequence_rows(rows, pad_mask=None, position_rows=None, segment_id=None, segment_rows=None, prefix=None, out_dtype=torch.float32,
                        status=None):
    """embed_sequence over dense rows: rows fp32 [B, L, W] (what a lookup that does not run over folded tables returned, any W >= 1) in
    place of the tables -> seq [B, P + L, W] of out_dtype.  pad_mask bool / uint8 [B, L]; the parts, the order of the additions, the
    padded positions (rows[b, p] as it stands), the status bit and the single rounding of a 16-bit output: as embed_sequence, every
    tensor W wide.  Elementwise: place, add, cast."""
    fn = "embed_sequence_rows"
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] < 1:
        raise ValueError(f"{fn}: rows must be an fp32 [batch, length, width] tensor, got {getattr(rows, 'dtype', type(rows))} "
                         f"{tuple(getattr(rows, 'shape', ()))}")
    if out_dtype not in EMBED_OUT_DTYPES:
        raise ValueError(f"{fn}: out_dtype must be one of {EMBED_OUT_DTYPES}, got {out_dtype!r}")
    batch, length, width = rows.shape
    pad_mask = _embed_mask(fn, pad_mask, rows[:, :, 0])
    parts = _sequence_parts(fn, batch, length, width, position_rows, segment_id, segment_rows, prefix)
    n_segments, n_prefix = parts[4:]
    rows = _dev(rows.detach(), "rows")
    pad_mask = _embed_mask_on_device(pad_mask)
    position_rows, segment_id, terms, prefix = _sequence_parts_on_device(*parts[:4])
    if status is not None:
        status = _dev(status, "status", torch.int32)
    res = torch.empty((batch, n_prefix + length, width), dtype=out_dtype, device=rows.device)
    lib = _lib.load()
    with _on(rows.device):
        head = (rows.data_ptr(), _ptr(pad_mask), batch, length, width, _ptr(position_rows), 0 if position_rows is None else position_rows.shape[0],
                _ptr(segment_id), _ptr(terms[0] if terms else None), _ptr(terms[1] if len(terms) > 1 else None), n_segments, _ptr(prefix), n_prefix,
                res.data_ptr())
        if out_dtype == torch.float32:
            _lib.check(lib.medtok_embed_sequence_rows_f32(*head, _ptr(status), _stream(rows)), "medtok_embed_sequence_rows_f32")
        else:
            _lib.check(lib.medtok_embed_sequence_rows_f16(*head, int(out_dtype == torch.bfloat16), _ptr(status), _stream(rows)),
                       "medtok_embed_sequence_rows_f16")
    return res


def _sequence_grad_args(fn, g, pad_mask, n_prefix):
    """g floating [B, P + L, W] and pad_mask [B, L] of the sequence gradients -> (g fp32 contiguous on its device, pad_mask, B, L, W)"""
    n_prefix = int(n_prefix)
    if (not isinstance(g, torch.Tensor) or g.dtype not in EMBED_OUT_DTYPES or g.dim() != 3 or g.shape[2] < 1 or n_prefix < 0
            or g.shape[1] < n_prefix):
        raise ValueError(f"{fn}: g must be a floating [batch, {n_prefix} + length, width] tensor, got {getattr(g, 'dtype', type(g))} "
                         f"{tuple(getattr(g, 'shape', ()))}")
    batch, length, width = g.shape[0], g.shape[1] - n_prefix, g.shape[2]
    if pad_mask is not None and (not isinstance(pad_mask, torch.Tensor) or pad_mask.dtype not in (torch.bool, torch.uint8)
                                 or tuple(pad_mask.shape) != (batch, length)):
        raise ValueError(f"{fn}: pad_mask must be a bool or uint8 [{batch}, {length}] tensor, got {getattr(pad_mask, 'dtype', type(pad_mask))} "
                         f"{tuple(getattr(pad_mask, 'shape', ()))}")
    if batch * (n_prefix + length) >= 1 << 31:
        raise ValueError(f"{fn}: {batch} x ({n_prefix} + {length}) rows reach 2^31: split the batch")
    return batch, length, width


def embed_sequence_segment_grad(g, segment_id, n_segments, pad_mask=None, n_prefix=0):
    """Gradient of embed_sequence's segment rows -> fp32 [B, V, W] (every segment term receives this tensor): G[b, v] = the sum of
    g[b, P + p] over the unpadded p with segment_id[b, p] == v.  g floating [B, P + L, W] (a 16-bit one is converted to fp32 first:
    exact); segment_id int64 [B, L]; pad_mask bool / uint8 [B, L].  Fixed order, no float atomics: per EMBED_SEQ_GRAD_CHUNK consecutive
    positions of a batch row in ascending position order, then the chunk sums in chunk order -- two calls give the same bits.  Ids outside
    [0, V) and padded positions contribute nothing.  V <= EMBED_SEQ_MAX_SEGMENTS.  Nothing is read back."""
    fn = "embed_sequence_segment_grad"
    batch, length, width = _sequence_grad_args(fn, g, pad_mask, n_prefix)
    n_segments = int(n_segments)
    if not 1 <= n_segments <= EMBED_SEQ_MAX_SEGMENTS:
        raise ValueError(f"{fn}: V = {n_segments} segments unsupported (1 .. {EMBED_SEQ_MAX_SEGMENTS})")
    if not isinstance(segment_id, torch.Tensor) or segment_id.dtype != torch.int64 or tuple(segment_id.shape) != (batch, length):
        raise ValueError(f"{fn}: segment_id must be an int64 [{batch}, {length}] tensor, got {getattr(segment_id, 'dtype', type(segment_id))} "
                         f"{tuple(getattr(segment_id, 'shape', ()))}")
    if not g.is_cuda:
        _dev(g, "g", g.dtype)
    g = g.float().contiguous()
    segment_id = _dev(segment_id, "segment_id", torch.int64)
    pad_mask = _embed_mask_on_device(pad_mask)
    out = torch.empty((batch, n_segments, width), dtype=torch.float32, device=g.device)
    lib = _lib.load()
    ws = _ws(lib.medtok_embed_sequence_grad_workspace_bytes(batch, length, n_segments, width), g)
    with _on(g.device):
        _lib.check(lib.medtok_embed_sequence_segment_grad_f32(g.data_ptr(), _ptr(pad_mask), segment_id.data_ptr(), batch, length, int(n_prefix),
                                                              n_segments, width, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g)),
                   "medtok_embed_sequence_segment_grad_f32")
    return out


def embed_sequence_position_grad(g, n_rows, pad_mask=None, n_prefix=0):
    """Gradient of embed_sequence's position rows -> fp32 [n_rows, W]: dpos[p] = the sum over b ascending of g[b, P + p] at the unpadded
    (b, p) for p < L; the rows L <= p < n_rows (rows of the table the call did not use) are zeros.  g, pad_mask: as
    embed_sequence_segment_grad.  Fixed order, no float atomics.  Nothing is read back."""
    fn = "embed_sequence_position_grad"
    batch, length, width = _sequence_grad_args(fn, g, pad_mask, n_prefix)
    n_rows = int(n_rows)
    if n_rows < length or n_rows >= 1 << 31:
        raise ValueError(f"{fn}: n_rows = {n_rows} must be at least the {length} positions (and below 2^31)")
    if not g.is_cuda:
        _dev(g, "g", g.dtype)
    g = g.float().contiguous()
    pad_mask = _embed_mask_on_device(pad_mask)
    out = torch.empty((n_rows, width), dtype=torch.float32, device=g.device)
    lib = _lib.load()
    with _on(g.device):
        _lib.check(lib.medtok_embed_sequence_position_grad_f32(g.data_ptr(), _ptr(pad_mask), batch, length, int(n_prefix), width, n_rows,
                                                               out.data_ptr(), _stream(g)), "medtok_embed_sequence_position_grad_f32")
    return out


def soft_vq_backward(x, xhat, what, idx, w, g_zq=None, g_xhat=None, g_out=None, g_vq=None, g_commit=None,
                     vq_scale: float = 0.0, commit_scale: float = 0.0, want_gx: bool = True, want_g_code: bool = True):
    """Sparse backward of the soft top-k assignment: (gx [n, d], g_code [n*k, d]).

    g_zq / g_xhat / g_out: [n, d] upstream gradients w.r.t. the code mix, the normalised rows and the
    straight-through output (None = zero); g_vq / g_commit: 0-dim DEVICE tensors, the upstream gradients of
    mean((zq - x)^2) seen from zq and from x, scaled by vq_scale / commit_scale inside the kernel.
    g_code[r*k + j] is the gradient w.r.t. the normalised code what[idx[r, j]]."""
    x, xhat, what, w = _dev(x, "x"), _dev(xhat, "xhat"), _dev(what, "what"), _dev(w, "w")
    idx = _dev(idx, "idx", torch.int64)
    n, d = x.shape
    topk = idx.shape[1]
    opt = [None if t is None else _dev(t, nm) for t, nm in ((g_zq, "g_zq"), (g_xhat, "g_xhat"), (g_out, "g_out"),
                                                            (g_vq, "g_vq"), (g_commit, "g_commit"))]
    gx = torch.empty((n, d), dtype=torch.float32, device=x.device) if want_gx else None
    g_code = torch.empty((n * topk, d), dtype=torch.float32, device=x.device) if want_g_code else None
    lib = _lib.load()
    with _on(x.device):
        _lib.check(lib.medtok_soft_vq_backward_f32(x.data_ptr(), xhat.data_ptr(), what.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                                   n, d, topk, *[_ptr(t) for t in opt], float(vq_scale), float(commit_scale),
                                                   _ptr(gx), _ptr(g_code), _stream(x)), "medtok_soft_vq_backward_f32")
    return gx, g_code


def normalize_backward(g, vhat, v, live=None):
    """Backward of F.normalize(v, dim=-1): (g - vhat (vhat . g)) / max(|v|, 1e-12), row-wise.  live ([n] fp32): rows with a 0 there are
    known to hold an all-zero g and are written as zeros without being read (the same bits)."""
    g, vhat, v = _dev(g, "g"), _dev(vhat, "vhat"), _dev(v, "v")
    n, d = v.shape
    out = torch.empty_like(v)
    lib = _lib.load()
    with _on(v.device):
        if live is not None:
            live = _dev(live, "live")
            if live.numel() != n:
                raise ValueError("normalize_backward: live must have one entry per row")
            _lib.check(lib.medtok_normalize_backward_sparse_f32(g.data_ptr(), vhat.data_ptr(), v.data_ptr(), live.data_ptr(), n, d, out.data_ptr(), _stream(v)),
                       "medtok_normalize_backward_sparse_f32")
        else:
            _lib.check(lib.medtok_normalize_backward_f32(g.data_ptr(), vhat.data_ptr(), v.data_ptr(), n, d, out.data_ptr(), _stream(v)),
                       "medtok_normalize_backward_f32")
    return out


def info_nce_forward(q, k, temperature: float):
    """(loss 0-dim, prob [b, b], ws): InfoNCE of loss.py:40-56; prob and ws feed info_nce_backward."""
    q, k = _dev(q, "q"), _dev(k, "k")
    b, d = q.shape
    if k.shape != q.shape:
        raise ValueError("info_nce: q and k must have the same shape")
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=q.device)
    prob = torch.empty((b, b), dtype=torch.float32, device=q.device)
    ws = _ws(lib.medtok_info_nce_workspace_bytes(b, d), q)
    with _on(q.device):
        _lib.check(lib.medtok_info_nce_forward_f32(q.data_ptr(), k.data_ptr(), b, d, float(temperature), loss.data_ptr(),
                                                   prob.data_ptr(), ws.data_ptr(), ws.numel(), _stream(q)), "medtok_info_nce_forward_f32")
    return loss, prob, ws


def info_nce_backward(q, k, prob, ws, g_loss, temperature: float):
    """(gq, gk) [b, d] from the forward's prob / ws and the upstream 0-dim device gradient."""
    q, k, prob, g_loss = _dev(q, "q"), _dev(k, "k"), _dev(prob, "prob"), _dev(g_loss, "g_loss")
    b, d = q.shape
    gq, gk = torch.empty_like(q), torch.empty_like(k)
    lib = _lib.load()
    with _on(q.device):
        _lib.check(lib.medtok_info_nce_backward_f32(q.data_ptr(), k.data_ptr(), prob.data_ptr(), g_loss.data_ptr(), b, d,
                                                    float(temperature), gq.data_ptr(), gk.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    _stream(q)), "medtok_info_nce_backward_f32")
    return gq, gk


def row_dot(a, b):
    """out[r] = <a[r], b[r]> (fp32, the rownorm summation order)."""
    a, b = _dev(a, "a"), _dev(b, "b")
    n, d = a.shape
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    with _on(a.device):
        _lib.check(_lib.load().medtok_row_dot_f32(a.data_ptr(), b.data_ptr(), n, d, out.data_ptr(), _stream(a)), "medtok_row_dot_f32")
    return out


def small_gemm(A, B, trans_a: bool = False, trans_b: bool = False, out=None):
    """op(A) @ op(B) in exact fp32 (one fmaf chain per entry, k ascending).  A, B: contiguous fp32 matrices; the transposes
    are strides, nothing is copied.  out: a contiguous fp32 [m, n] device tensor to fill (e.g. a row block of a larger one)."""
    A, B = _dev(A, "A"), _dev(B, "B")
    (m, k), (sam, sak) = ((A.shape[1], A.shape[0]), (1, A.shape[1])) if trans_a else ((A.shape[0], A.shape[1]), (A.shape[1], 1))
    (k2, n), (sbk, sbn) = ((B.shape[1], B.shape[0]), (1, B.shape[1])) if trans_b else ((B.shape[0], B.shape[1]), (B.shape[1], 1))
    if k != k2:
        raise ValueError(f"small_gemm: inner dimensions differ ({k} vs {k2})")
    if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (m, n)
                                and out.is_contiguous()):
        raise ValueError(f"small_gemm: out must be a contiguous fp32 [{m}, {n}] device tensor")
    C = torch.empty((m, n), dtype=torch.float32, device=A.device) if out is None else out
    with _on(A.device):
        _lib.check(_lib.load().medtok_small_gemm_f32(A.data_ptr(), sam, sak, B.data_ptr(), sbk, sbn, m, n, k, C.data_ptr(), _stream(A)),
                   "medtok_small_gemm_f32")
    return C


def frobenius(x):
    """0-dim fp32 tensor ||x||_F of a contiguous [rows, d] matrix (d % 4 == 0)."""
    x = _dev(x, "x")
    rows, d = x.shape
    lib = _lib.load()
    out = torch.empty((), dtype=torch.float32, device=x.device)
    ws = _ws(lib.medtok_frobenius_workspace_bytes(rows), x)
    with _on(x.device):
        _lib.check(lib.medtok_frobenius_f32(x.data_ptr(), rows, d, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)), "medtok_frobenius_f32")
    return out


def split_half(x, dp: int = None, scale: float = 1.0, seg_len=None, seg_rows: int = 0):
    """(hi, lo) fp16 images [n, dp] of the fp32 matrix x [n, d] (last dim contiguous; a row-strided view is fine): x * scale =
    hi + lo to ~2^-22 relative.  dp (default: d rounded up to 8) pads with zero columns.  seg_len (int64 [n / seg_rows] on the
    device): only the first seg_len[b] rows of every segment of seg_rows rows are converted (the rest stay uninitialised)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise _lib.MedTokLibraryError("split_half: expected an fp32 [n, d] matrix with contiguous rows on an MI355X device")
    n, d = x.shape
    dp = (d + 7) // 8 * 8 if dp is None else int(dp)
    hi = torch.empty((n, dp), dtype=torch.float16, device=x.device)
    lo = torch.empty((n, dp), dtype=torch.float16, device=x.device)
    with _on(x.device):
        _lib.check(_lib.load().medtok_split_half_f32(x.data_ptr(), n, d, x.stride(0) if n > 1 else d, dp, float(scale), hi.data_ptr(), lo.data_ptr(),
                                                     _ptr(None if seg_len is None else _dev(seg_len, "seg_len", torch.int64)), int(seg_rows), _stream(x)),
                   "medtok_split_half_f32")
    return hi, lo


def split_gemm(a, b, n_g: int, k_g: int, groups: int = 1, a_group_cols: int = 0, b_group_rows: int = 0, bias=None, unscale: float = 1.0,
               want_f32: bool = True, want_split: bool = False):
    """unscale * (A . B^T) + bias on three fp16 MFMA passes (medtok_split_gemm_f16).  a = (hi, lo) [m, lda], b = (hi, lo)
    [b_rows, ldb] fp16 images; see include/medtok_vq.h for the grouped form.  Returns (c fp32 [m, groups * n_g] or None,
    (c_hi, c_lo) or None)."""
    a_hi, a_lo = a
    b_hi, b_lo = b
    for t in (a_hi, a_lo, b_hi, b_lo):
        if not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and t.dim() == 2):
            raise _lib.MedTokLibraryError("split_gemm: operands must be contiguous fp16 matrices on an MI355X device")
    m, lda = a_hi.shape
    b_rows, ldb = b_hi.shape
    n_out = groups * n_g
    bias = None if bias is None else _dev(bias, "bias")
    c = torch.empty((m, n_out), dtype=torch.float32, device=a_hi.device) if want_f32 else None
    ch = torch.empty((m, n_out), dtype=torch.float16, device=a_hi.device) if want_split else None
    cl = torch.empty((m, n_out), dtype=torch.float16, device=a_hi.device) if want_split else None
    with _on(a_hi.device):
        _lib.check(_lib.load().medtok_split_gemm_f16(a_hi.data_ptr(), a_lo.data_ptr(), m, lda, int(a_group_cols), b_hi.data_ptr(), b_lo.data_ptr(),
                                                     b_rows, ldb, int(b_group_rows), int(n_g), int(k_g), int(groups), _ptr(bias), float(unscale),
                                                     _ptr(c), n_out, _ptr(ch), _ptr(cl), n_out, _stream(a_hi)), "medtok_split_gemm_f16")
    return c, ((ch, cl) if want_split else None)


def half_gemm(a, b, n_g: int, k_g: int, groups: int = 1, a_group_cols: int = 0, b_group_rows: int = 0, bias=None, unscale: float = 1.0):
    """c [m, groups * n_g] fp32 = unscale * (A . B^T) + bias in ONE half-precision pass with fp32 accumulation (medtok_half_gemm_f32):
    a [m, lda], b [b_rows, ldb] both torch.float16 or both torch.bfloat16, contiguous; grouped as split_gemm."""
    if a.dtype != b.dtype or a.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError("half_gemm: operands must both be float16 or both bfloat16")
    for t in (a, b):
        if not (t.is_cuda and t.is_contiguous() and t.dim() == 2):
            raise _lib.MedTokLibraryError("half_gemm: operands must be contiguous 2-d matrices on an MI355X device")
    m, lda = a.shape
    b_rows, ldb = b.shape
    bias = None if bias is None else _dev(bias, "bias")
    c = torch.empty((m, groups * n_g), dtype=torch.float32, device=a.device)
    with _on(a.device):
        _lib.check(_lib.load().medtok_half_gemm_f32(a.data_ptr(), m, lda, int(a_group_cols), b.data_ptr(), b_rows, ldb, int(b_group_rows), int(n_g), int(k_g),
                                                    int(groups), _ptr(bias), float(unscale), c.data_ptr(), groups * n_g, int(a.dtype == torch.bfloat16),
                                                    _stream(a)), "medtok_half_gemm_f32")
    return c


def half_image(x, dp: int, dtype, transpose: bool = False, group_cols: int = 0, col_sums: bool = False):
    """the fp16 / bf16 image of the fp32 matrix x [n, d] (unit column stride): [n, dp] with zero columns past d, or (transpose) of x^T,
    [d, dp] with dp >= n, stacked as dp / group_cols groups of [d, group_cols] (medtok_half_image_f32)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise _lib.MedTokLibraryError("half_image: expected an fp32 [n, d] matrix with contiguous rows on an MI355X device")
    n, d = x.shape
    if transpose:
        gc = int(group_cols) or int(dp)
        shape = (int(dp) // gc * d, gc)
    else:
        shape = (n, int(dp))
    out = torch.empty(shape, dtype=dtype, device=x.device)
    if col_sums:            # (transposed image + the column sums of x from the same pass: medtok_half_image_t_sums_f32)
        if not transpose:
            raise ValueError("half_image: col_sums comes with the transposed image")
        partials = torch.empty(((int(dp) + 63) // 64, d), dtype=torch.float32, device=x.device)
        with _on(x.device):
            _lib.check(_lib.load().medtok_half_image_t_sums_f32(x.data_ptr(), n, d, x.stride(0) if n > 1 else d, int(dp), int(group_cols),
                                                                int(dtype == torch.bfloat16), out.data_ptr(), partials.data_ptr(), _stream(x)),
                       "medtok_half_image_t_sums_f32")
        return out, partials.sum(0)
    with _on(x.device):
        _lib.check(_lib.load().medtok_half_image_f32(x.data_ptr(), n, d, x.stride(0) if n > 1 else d, int(dp), int(bool(transpose)), int(group_cols),
                                                     int(dtype == torch.bfloat16), out.data_ptr(), _stream(x)), "medtok_half_image_f32")
    return out


def half_image_pair(x, dp: int, np_: int, dtype, group_cols: int = 0, col_sums: bool = False):
    """(half_image(x, dp), half_image(x, np_, transpose=True, group_cols)) from ONE pass over x (medtok_half_image_pair_f32), bit for bit.
    Both images are written completely: columns d .. dp - 1 of the plain image and columns n .. np_ - 1 of the transposed one (whole
    64-row tiles of padding included) are +0 -- the weight-gradient product multiplies that padding.  col_sums: + the fp32 column sums
    of x, the sum over the 64-row tiles of the kernel's partials (tests/test_gpu_operand_images.py)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise _lib.MedTokLibraryError("half_image_pair: expected an fp32 [n, d] matrix with contiguous rows on an MI355X device")
    n, d = x.shape
    if n == 0 or int(dp) > (d + 63) // 64 * 64:
        pair = half_image(x, dp, dtype), half_image(x, np_, dtype, transpose=True, group_cols=group_cols)
        return (*pair, x.sum(0)) if col_sums else pair
    gc = int(group_cols) or int(np_)
    plain = torch.empty((n, int(dp)), dtype=dtype, device=x.device)
    t = torch.empty((int(np_) // gc * d, gc), dtype=dtype, device=x.device)
    if col_sums:            # (+ the column sums of x from the same pass: per 64-row tile in the kernel, over the tiles here)
        partials = torch.empty(((int(np_) + 63) // 64, d), dtype=torch.float32, device=x.device)
        with _on(x.device):
            _lib.check(_lib.load().medtok_half_image_pair_sums_f32(x.data_ptr(), n, d, x.stride(0) if n > 1 else d, int(dp), int(np_), int(group_cols),
                                                                   int(dtype == torch.bfloat16), plain.data_ptr(), t.data_ptr(), partials.data_ptr(),
                                                                   _stream(x)), "medtok_half_image_pair_sums_f32")
        return plain, t, partials.sum(0)
    with _on(x.device):
        _lib.check(_lib.load().medtok_half_image_pair_f32(x.data_ptr(), n, d, x.stride(0) if n > 1 else d, int(dp), int(np_), int(group_cols),
                                                          int(dtype == torch.bfloat16), plain.data_ptr(), t.data_ptr(), _stream(x)), "medtok_half_image_pair_f32")
    return plain, t


def absmax(x):
    """0-dim device fp32 tensor max |x| (no host read): feeds the power-of-two prescale of training-mode split operands."""
    x = _dev(x, "x")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    with _on(x.device):
        _lib.check(_lib.load().medtok_absmax_f32(x.data_ptr(), x.numel(), out.data_ptr(), _stream(x)), "medtok_absmax_f32")
    return out


def split_half_scaled(x, dp: int, amax=None, transpose: bool = False, group_cols: int = 0):
    """(hi, lo) fp16 images of the fp32 matrix x [n, d], prescaled by the power of two that `amax` (0-dim device tensor, from absmax;
    None: 1) selects.  transpose=False: [n, dp], dp >= d; transpose=True: the images of x^T, [d, dp], dp >= n -- with group_cols (a
    multiple of 64 dividing dp) stacked as [dp / group_cols * d, group_cols]: group g holds columns [g group_cols, + group_cols)."""
    x = _dev(x, "x")
    n, d = x.shape
    if transpose:
        gc = int(group_cols) or int(dp)
        shape = (int(dp) // gc * d, gc)
    else:
        shape = (n, int(dp))
    hi = torch.empty(shape, dtype=torch.float16, device=x.device)
    lo = torch.empty(shape, dtype=torch.float16, device=x.device)
    with _on(x.device):
        _lib.check(_lib.load().medtok_split_half_scaled_f32(x.data_ptr(), n, d, d, int(dp), _ptr(amax), int(bool(transpose)), int(group_cols),
                                                            hi.data_ptr(), lo.data_ptr(), _stream(x)), "medtok_split_half_scaled_f32")
    return hi, lo


def split_gemm_scaled(a, b, n_g: int, k_g: int, bias=None, unscale: float = 1.0, amax_a=None, amax_b=None, groups: int = 1, a_group_cols: int = 0,
                      b_group_rows: int = 0):
    """c [m, groups * n_g] fp32 = unscale / (pow2(amax_a) pow2(amax_b)) * A . B^T + bias from (hi, lo) images made by split_half_scaled
    (grouped as medtok_split_gemm_f16)."""
    (a_hi, a_lo), (b_hi, b_lo) = a, b
    m, lda = a_hi.shape
    b_rows, ldb = b_hi.shape
    c = torch.empty((m, groups * n_g), dtype=torch.float32, device=a_hi.device)
    bias = None if bias is None else _dev(bias, "bias")
    with _on(a_hi.device):
        _lib.check(_lib.load().medtok_split_gemm_scaled_f16(a_hi.data_ptr(), a_lo.data_ptr(), m, lda, int(a_group_cols), b_hi.data_ptr(), b_lo.data_ptr(),
                                                            b_rows, ldb, int(b_group_rows), int(n_g), int(k_g), int(groups), _ptr(bias), float(unscale),
                                                            _ptr(amax_a), _ptr(amax_b), c.data_ptr(), groups * n_g, _stream(a_hi)),
                   "medtok_split_gemm_scaled_f16")
    return c


def residual_layernorm(a, b, gamma, beta, eps: float, split_dp: int = 0):
    """LayerNorm(a + b) * gamma + beta per row of the contiguous fp32 matrices a, b [n, d] (the tail of CrossAttentionLayer,
    vector_quantization_soft_one_new.py:47-50); d % 4 == 0, d <= 4096.  split_dp > 0: returns (y, (y_hi, y_lo)) with the (hi, lo)
    fp16 images [n, split_dp] of y that split_half(y, dp=split_dp) would make, written by the same kernel."""
    a, b, gamma, beta = _dev(a, "a"), _dev(b, "b"), _dev(gamma, "gamma"), _dev(beta, "beta")
    if a.shape != b.shape or a.dim() != 2 or gamma.shape != (a.shape[1],) or beta.shape != (a.shape[1],):
        raise ValueError(f"residual_layernorm: shapes a={tuple(a.shape)} b={tuple(b.shape)} gamma={tuple(gamma.shape)} beta={tuple(beta.shape)}")
    n, d = a.shape
    y = torch.empty_like(a)
    hi = lo = None
    if split_dp:
        hi = torch.empty((n, split_dp), dtype=torch.float16, device=a.device)
        lo = torch.empty((n, split_dp), dtype=torch.float16, device=a.device)
    with _on(a.device):
        _lib.check(_lib.load().medtok_residual_layernorm_split_f32(a.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), n, d, float(eps),
                                                                   y.data_ptr(), _ptr(hi), _ptr(lo), int(split_dp), _stream(a)),
                   "medtok_residual_layernorm_split_f32")
    return (y, (hi, lo)) if split_dp else y


def pack_codes(mask, batch, heads: int, lpt: bool, count_bound: int = 0, status=None):
    """The prologue of the batched cross-attention in three small launches (include/medtok_vq.h: medtok_pack_codes_checked): mask [B, L]
    (bool / int32 / int64), batch [n_nodes] int64 -> dict(valid_len, counts, starts, t_start, t_len, g_start, g_len, tok_start,
    g_kv_len: int64 [B] device tensors; stats: int64 [4] = largest count, id range, unsorted flag -- not yet read back).
    status (int32 device tensor, optional): what a caller that never reads stats back needs flagged -- bit 0 unsorted, bit 1 id out of
    range, bit 2 a code with more than count_bound nodes -- OR-ed into status[0] on the device."""
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dim() == 2):
        raise _lib.MedTokLibraryError("pack_codes: expected a [B, L] mask on an MI355X device")
    if mask.dtype not in (torch.bool, torch.uint8, torch.int32, torch.int64):
        mask = mask != 0
    mask = mask.contiguous()
    batch = _dev(batch.reshape(-1), "batch", torch.int64)
    bsz, seq_len = mask.shape
    dev = mask.device
    out = torch.empty((9, bsz), dtype=torch.int64, device=dev)
    stats = torch.empty(4, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = _ws(lib.medtok_pack_codes_workspace_bytes(bsz), mask)
    with _on(dev):
        if status is not None and not (status.is_cuda and status.dtype == torch.int32 and status.device == dev):
            raise _lib.MedTokLibraryError("pack_codes: status must be an int32 tensor on the mask's device")
        _lib.check(lib.medtok_pack_codes_checked(mask.data_ptr(), mask.element_size(), bsz, seq_len, batch.data_ptr(), batch.numel(), int(heads),
                                                 int(bool(lpt)), *[out[i].data_ptr() for i in range(9)], stats.data_ptr(), int(count_bound),
                                                 _ptr(status), ws.data_ptr(), ws.numel(), _stream(mask)),
                   "medtok_pack_codes")
    names = ("valid_len", "counts", "starts", "t_start", "t_len", "g_start", "g_len", "tok_start", "g_kv_len")
    r = {k: out[i] for i, k in enumerate(names)}
    r["stats"] = stats
    return r


def cross_attention_layer(rows, rows_images, w, q_start, q_len, max_q_len: int, kv, kv_split, kv_start, kv_len, scale: float, variant: int,
                          gamma, beta, eps: float, want_images: bool):
    """One CrossAttentionLayer at inference in one C call (include/medtok_vq.h: medtok_cross_attention_layer_f32).  rows [R, d] fp32;
    rows_images: their (hi, lo) images [R, dw] or None; w: the dict of CrossAttention._split_weights; kv fp32 [Rk, dw] or kv_split =
    (hi, lo | None) images, or kv_split = the fp32 rows themselves (split inside the kernel: shared_kv_attention_split).  Returns y [R, d] (and its images [R, dw] when want_images)."""
    rows = _dev(rows, "rows")
    n_rows, d = rows.shape
    heads, hp, dw = w["heads"], w["hp"], w["dw"]
    dev = rows.device
    y = torch.empty_like(rows)
    yh = torch.empty((n_rows, dw), dtype=torch.float16, device=dev) if want_images else None
    yl = torch.empty((n_rows, dw), dtype=torch.float16, device=dev) if want_images else None
    lib = _lib.load()
    ws = _ws(lib.medtok_cross_attention_layer_workspace_bytes(n_rows, d, dw, heads, hp), rows)
    (wq, wq_u), (wk, wk_u), (wv, wv_u), (wo, wo_u) = w["wq"], w["wk"], w["wv"], w["wo"]
    xh, xl = rows_images if rows_images is not None else (None, None)
    if torch.is_tensor(kv_split):               # fp32 key rows, turned into their images inside the attention kernel
        kh, kl, variant = _dev(kv_split, "kv"), None, int(variant) | ATTENTION_F32_KEYS
    else:
        kh, kl = kv_split if kv_split is not None else (None, None)
    with _on(dev):
        _lib.check(lib.medtok_cross_attention_layer_f32(
            rows.data_ptr(), _ptr(xh), _ptr(xl), n_rows, d, dw, heads, hp,
            wq[0].data_ptr(), wq[1].data_ptr(), float(wq_u), w["bq"].data_ptr(), wk[0].data_ptr(), wk[1].data_ptr(), float(wk_u),
            wv[0].data_ptr(), wv[1].data_ptr(), float(wv_u), w["bv"].data_ptr(), wo[0].data_ptr(), wo[1].data_ptr(), float(wo_u), w["bo"].data_ptr(),
            q_start.data_ptr(), q_len.data_ptr(), q_start.numel(), int(max_q_len), _ptr(kv if kv_split is None else None), _ptr(kh), _ptr(kl),
            kv_start.data_ptr(), kv_len.data_ptr(), float(scale), int(variant), gamma.data_ptr(), beta.data_ptr(), float(eps),
            y.data_ptr(), _ptr(yh), _ptr(yl), ws.data_ptr(), ws.numel(), _stream(rows)), "medtok_cross_attention_layer_f32")
    return (y, (yh, yl)) if want_images else y


SMALL_ATTENTION_LAYER_FLOATS = 4 * 64 * 64 + 6 * 64


def cross_attention_small(text, mask, nodes, batch, weights, layers: int, scale: float, ln_eps: float, pooled, status, exact_f32: bool = False):
    """CrossAttention.pooled at e_dim = 64 with 4 heads in two launches and no host read (include/medtok_vq.h:
    medtok_cross_attention_small_f32).  text [B, L, 64] fp32, mask [B, L] (bool / int32 / int64), nodes [N, 64] fp32 with a sorted
    batch vector [N] int64, weights [layers, SMALL_ATTENTION_LAYER_FLOATS] (CrossAttention._small_weights), pooled [B, 2, 64] fp32
    (written: [:, 0] the attended CLS rows, [:, 1] the node means), status int32 [4] (zeroed once by its owner).
    exact_f32 (tests only): the attention core on the fp32 matrix pipe instead of the product's split-fp16 core."""
    text, nodes, weights = _dev(text, "text"), _dev(nodes, "nodes"), _dev(weights, "weights")
    batch = _dev(batch.reshape(-1), "batch", torch.int64)
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dim() == 2):
        raise _lib.MedTokLibraryError("cross_attention_small: expected a [B, L] mask on an MI355X device")
    if mask.dtype not in (torch.bool, torch.uint8, torch.int32, torch.int64):
        mask = mask != 0
    mask = mask.contiguous()
    bsz, seq_len, d = text.shape
    n_nodes = nodes.shape[0]
    if pooled.shape != (bsz, 2, d) or pooled.dtype != torch.float32 or not pooled.is_contiguous():
        raise ValueError("cross_attention_small: pooled must be a contiguous fp32 [B, 2, d] tensor")
    y_nodes = torch.empty((max(n_nodes, 1), d), dtype=torch.float32, device=text.device)
    with _on(text.device):
        lib = _lib.load()
        _lib.check((lib.medtok_debug_cross_attention_small_exact_f32 if exact_f32 else lib.medtok_cross_attention_small_f32)(
            text.data_ptr(), mask.data_ptr(), mask.element_size(), bsz, seq_len, nodes.data_ptr() if n_nodes else 0, batch.data_ptr() if n_nodes else 0,
            n_nodes, d, 4, int(layers), weights.data_ptr(), float(scale), float(ln_eps), y_nodes.data_ptr(), pooled.data_ptr(), 2 * d, d,
            status.data_ptr(), _stream(text)), "medtok_cross_attention_small_f32")
    return pooled


def segment_mean(x, seg_start, seg_len):
    """out[b] = mean of rows [seg_start[b], seg_start[b] + seg_len[b]) of the contiguous fp32 matrix x [rows, d] (rows added in
    order; an empty segment gives zeros) -- the `.mean(dim=0)` over a code's graph nodes (:140-141).  seg_* int64 device vectors."""
    x = _dev(x, "x")
    seg_start, seg_len = _dev(seg_start, "seg_start", torch.int64), _dev(seg_len, "seg_len", torch.int64)
    n_seg, d = seg_start.numel(), x.shape[1]
    if seg_len.numel() != n_seg:
        raise ValueError("segment_mean: seg_start and seg_len differ in length")
    out = torch.empty((n_seg, d), dtype=torch.float32, device=x.device)
    with _on(x.device):
        _lib.check(_lib.load().medtok_segment_mean_f32(x.data_ptr(), seg_start.data_ptr(), seg_len.data_ptr(), n_seg, d, out.data_ptr(), _stream(x)),
                   "medtok_segment_mean_f32")
    return out


def scale_by_device_scalar(x, num, den=None, c: float = 1.0):
    """x * (c * num / den) with num / den 0-dim device tensors (no host sync)."""
    x, num = _dev(x, "x"), _dev(num, "num")
    den = None if den is None else _dev(den, "den")
    out = torch.empty_like(x)
    with _on(x.device):
        _lib.check(_lib.load().medtok_scale_by_device_scalar_f32(x.data_ptr(), x.numel(), num.data_ptr(), _ptr(den), float(c), out.data_ptr(),
                                                                 _stream(x)), "medtok_scale_by_device_scalar_f32")
    return out


def _attention_outputs(q, split_out):
    """fp32 result, or its (hi, lo) fp16 images (rows that belong to no code stay uninitialised either way)"""
    if not split_out:
        return torch.empty_like(q), None, None
    return None, torch.empty(q.shape, dtype=torch.float16, device=q.device), torch.empty(q.shape, dtype=torch.float16, device=q.device)


def shared_kv_attention(q, q_start, q_len, kv, kv_start, kv_len, max_q_len: int, scale: float, exact_f32: bool = False, split_out: bool = False):
    """out[r] = softmax_j(scale * <q[r], kv[j]>) . kv over each code's own (ragged) query and key rows.
    q [Rq, d], kv [Rk, d] fp32; *_start / *_len int64 [n_codes] on the device; d = 64 or a multiple of 128 up to 768.
    Default: both products as three fp16 MFMAs over (hi, lo) pairs (fp32-accurate, 16/3 the fp32 pipe's rate); exact_f32: the
    fp32-MFMA kernel the training forward uses.  split_out: return the (hi, lo) fp16 images of the result instead (written by the
    kernel for the dense product that follows)."""
    q, kv = _dev(q, "q"), _dev(kv, "kv")
    qs, ql = _dev(q_start, "q_start", torch.int64), _dev(q_len, "q_len", torch.int64)
    ks, kl = _dev(kv_start, "kv_start", torch.int64), _dev(kv_len, "kv_len", torch.int64)
    out, oh, ol = _attention_outputs(q, split_out)
    lib = _lib.load()
    with _on(q.device):
        _lib.check(lib.medtok_shared_kv_attention_f32(q.data_ptr(), qs.data_ptr(), ql.data_ptr(), kv.data_ptr(), ks.data_ptr(),
                                                      kl.data_ptr(), qs.numel(), int(max_q_len), q.shape[1], float(scale),
                                                      _ptr(out), _ptr(oh), _ptr(ol), int(bool(exact_f32)), _stream(q)), "medtok_shared_kv_attention_f32")
    return (oh, ol) if split_out else out


ATTENTION_SPLIT_WIDTHS = (128, 256, 384, 512, 768, 1024)
ATTENTION_HALF_KEY_WIDTHS = (256, 512, 768)        # widths at which fp16 keys are taken as they stand (variant 2, no lo image)


ATTENTION_F32_KEYS = 0x100                 # MEDTOK_ATTENTION_F32_KEYS (include/medtok_vq.h)


def shared_kv_attention_split(q, q_start, q_len, kv_split, kv_start, kv_len, max_q_len: int, scale: float, split_out: bool = False, variant: int = 0):
    """shared_kv_attention for wide batches: the keys as the (hi, lo) fp16 images of split_half (made once per forward), 64 query
    rows per block, keys copied into LDS by DMA.  d in ATTENTION_SPLIT_WIDTHS."""
    q = _dev(q, "q")
    if torch.is_tensor(kv_split):               # fp32 key rows, turned into their images inside the kernel (variant 2, d = 256 / 512 / 768)
        kh, kl_ = _dev(kv_split, "kv"), None
        if kh.dim() != 2 or kh.shape[1] != q.shape[1]:
            raise _lib.MedTokLibraryError("shared_kv_attention_split: fp32 keys must be [Rk, d]")
        variant = int(variant) | ATTENTION_F32_KEYS
    else:
        kh, kl_ = kv_split                      # kl_ = None: fp16 keys as they stand (no lo image; variant 2, d = 256 / 512 / 768)
        for t in (kh, kl_):
            if t is not None and not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == q.shape[1]):
                raise _lib.MedTokLibraryError("shared_kv_attention_split: the key images must be contiguous fp16 [Rk, d] device tensors")
    qs, ql = _dev(q_start, "q_start", torch.int64), _dev(q_len, "q_len", torch.int64)
    ks, kl = _dev(kv_start, "kv_start", torch.int64), _dev(kv_len, "kv_len", torch.int64)
    out, oh, ol = _attention_outputs(q, split_out)
    with _on(q.device):
        _lib.check(_lib.load().medtok_shared_kv_attention_split_f32(q.data_ptr(), qs.data_ptr(), ql.data_ptr(), kh.data_ptr(), _ptr(kl_),
                                                                    ks.data_ptr(), kl.data_ptr(), qs.numel(), int(max_q_len), q.shape[1], float(scale),
                                                                    _ptr(out), _ptr(oh), _ptr(ol), int(variant), _stream(q)), "medtok_shared_kv_attention_split_f32")
    return (oh, ol) if split_out else out


ATTENTION_TRAIN_SPLIT_WIDTHS = (256, 512, 768)


def _into(buf, name, shape, like):
    """a caller's output buffer (a contiguous fp32 tensor -- e.g. a row range of a larger one -- that a kernel writes into)"""
    t = _dev(buf, name)
    if t is not buf:
        raise ValueError(f"{name} must be contiguous (the kernel writes into it)")
    if tuple(t.shape) != tuple(shape) or t.device != like.device:
        raise ValueError(f"{name} {tuple(t.shape)} on {t.device} does not match {tuple(shape)} on {like.device}")
    return t


def shared_kv_attention_train(q, q_start, q_len, kv, kv_start, kv_len, max_q_len: int, scale: float, dropout_p: float = 0.0, seed: int = 0,
                              split: bool = False, out=None, lse=None):
    """(out, lse): the attention core with dropout on the probabilities (stateless hash mask) and the log-sum-exp per query row.
    split=True (widths ATTENTION_TRAIN_SPLIT_WIDTHS): on the three-pass fp16 products instead of the exact fp32 matrix pipe -- the
    same mask bits, outputs within ~1e-6 relative, a third of the time at D = 768 (the autocast trainer's form).
    out / lse: the caller's buffers ([rows, d] zeros / [rows] -inf where rows may belong to no code), e.g. row ranges of larger ones."""
    q, kv = _dev(q, "q"), _dev(kv, "kv")
    qs, ql = _dev(q_start, "q_start", torch.int64), _dev(q_len, "q_len", torch.int64)
    ks, kl = _dev(kv_start, "kv_start", torch.int64), _dev(kv_len, "kv_len", torch.int64)
    out = torch.zeros_like(q) if out is None else _into(out, "out", q.shape, q)              # rows that belong to no code stay zero
    lse = (torch.full((q.shape[0],), float("-inf"), dtype=torch.float32, device=q.device) if lse is None else _into(lse, "lse", (q.shape[0],), q))
    lib = _lib.load()
    fn, name = ((lib.medtok_shared_kv_attention_train_split_f32, "medtok_shared_kv_attention_train_split_f32") if split else
                (lib.medtok_shared_kv_attention_train_f32, "medtok_shared_kv_attention_train_f32"))
    with _on(q.device):
        _lib.check(fn(q.data_ptr(), qs.data_ptr(), ql.data_ptr(), kv.data_ptr(), ks.data_ptr(), kl.data_ptr(), qs.numel(), int(max_q_len), q.shape[1],
                      float(scale), float(dropout_p), int(seed) & 0xFFFFFFFF, out.data_ptr(), lse.data_ptr(), _stream(q)), name)
    return out, lse


def shared_kv_attention_backward(q, q_start, q_len, kv, kv_start, kv_len, max_q_len: int, max_kv_len: int, scale: float, dropout_p: float,
                                 seed: int, out, lse, d_out, half=None, dkv_into=None, accumulate=False, dq_into=None):
    """(dq, dkv) of shared_kv_attention_train for the upstream gradient d_out.  half = torch.float16 / torch.bfloat16: the four matrix
    products in one half-precision pass with fp32 accumulation (autocast callers); None: exact fp32 MFMA.
    dkv_into: a contiguous fp32 [kv_rows, d] buffer that receives dkv (returned as dkv); with accumulate=True the key gradient is
    ADDED to what it holds (the layers of CrossAttention share their keys: one buffer, no add pass).  dq_into: the buffer for dq."""
    q, kv, out, lse, d_out = _dev(q, "q"), _dev(kv, "kv"), _dev(out, "out"), _dev(lse, "lse"), _dev(d_out, "d_out")
    qs, ql = _dev(q_start, "q_start", torch.int64), _dev(q_len, "q_len", torch.int64)
    ks, kl = _dev(kv_start, "kv_start", torch.int64), _dev(kv_len, "kv_len", torch.int64)
    dq = torch.empty_like(q) if dq_into is None else _into(dq_into, "dq_into", q.shape, q)
    if dkv_into is None:
        if accumulate:
            raise ValueError("shared_kv_attention_backward: accumulate=True needs the buffer to add to (dkv_into)")
        dkv = torch.empty_like(kv)
    else:
        dkv = _dev(dkv_into, "dkv_into")
        if dkv is not dkv_into:
            raise ValueError("shared_kv_attention_backward: dkv_into must be contiguous (the kernel writes into it)")
        if dkv.shape != kv.shape or dkv.device != kv.device:
            raise ValueError(f"shared_kv_attention_backward: dkv_into {tuple(dkv.shape)} on {dkv.device} does not match kv {tuple(kv.shape)} on {kv.device}")
    lib = _lib.load()
    ws = _ws(lib.medtok_shared_kv_attention_backward_workspace_bytes(q.shape[0]), q)
    args = (q.data_ptr(), qs.data_ptr(), ql.data_ptr(), kv.data_ptr(), ks.data_ptr(), kl.data_ptr(), qs.numel(), int(max_q_len), int(max_kv_len),
            q.shape[0], kv.shape[0], q.shape[1], float(scale), float(dropout_p), int(seed) & 0xFFFFFFFF, out.data_ptr(), lse.data_ptr(),
            d_out.data_ptr(), dq.data_ptr(), dkv.data_ptr(), ws.data_ptr(), ws.numel())
    with _on(q.device):
        if accumulate:
            mode = 1 if half == torch.float16 else (2 if half == torch.bfloat16 else 0)
            _lib.check(lib.medtok_shared_kv_attention_backward_acc_f32(*args, mode, 1, _stream(q)), "medtok_shared_kv_attention_backward_acc_f32")
        elif half in (torch.float16, torch.bfloat16):
            _lib.check(lib.medtok_shared_kv_attention_backward_half_f32(*args, int(half == torch.bfloat16), _stream(q)), "medtok_shared_kv_attention_backward_half_f32")
        else:
            _lib.check(lib.medtok_shared_kv_attention_backward_f32(*args, _stream(q)), "medtok_shared_kv_attention_backward_f32")
    return dq, dkv


def shared_kv_attention_backward_dq(q, q_start, q_len, kv, kv_start, kv_len, max_q_len: int, max_kv_len: int, scale: float, dropout_p: float,
                                    seed: int, out, lse, d_out, half=None, dq_into=None):
    """(dq, delta): the query gradient alone (medtok_shared_kv_attention_backward_acc_f32, accumulate_dkv = 2) and delta = <d_out, out> per
    query row -- what shared_kv_attention_dkv_multi takes, with the call's other tensors, as one of its sources."""
    q, kv, out, lse, d_out = _dev(q, "q"), _dev(kv, "kv"), _dev(out, "out"), _dev(lse, "lse"), _dev(d_out, "d_out")
    qs, ql = _dev(q_start, "q_start", torch.int64), _dev(q_len, "q_len", torch.int64)
    ks, kl = _dev(kv_start, "kv_start", torch.int64), _dev(kv_len, "kv_len", torch.int64)
    dq = torch.empty_like(q) if dq_into is None else _into(dq_into, "dq_into", q.shape, q)
    delta = torch.empty((max(q.shape[0], 1),), dtype=torch.float32, device=q.device)
    mode = 1 if half == torch.float16 else (2 if half == torch.bfloat16 else 0)
    with _on(q.device):
        _lib.check(_lib.load().medtok_shared_kv_attention_backward_acc_f32(
            q.data_ptr(), qs.data_ptr(), ql.data_ptr(), kv.data_ptr(), ks.data_ptr(), kl.data_ptr(), qs.numel(), int(max_q_len), int(max_kv_len),
            q.shape[0], kv.shape[0], q.shape[1], float(scale), float(dropout_p), int(seed) & 0xFFFFFFFF, out.data_ptr(), lse.data_ptr(),
            d_out.data_ptr(), dq.data_ptr(), 0, delta.data_ptr(), delta.numel() * 4, mode, 2, _stream(q)), "medtok_shared_kv_attention_backward_acc_f32")
    return dq, delta


def shared_kv_attention_dkv_multi(sources, kv, kv_start, kv_len, max_kv_len: int, half=None):
    """dkv [kv_rows, d]: the key gradient of several attention calls over the same keys in ONE launch (medtok_shared_kv_attention_dkv_multi_f32).
    sources: dicts with q, d_out, lse, delta (of shared_kv_attention_backward_dq), q_start, q_len, scale, dropout_p, seed."""
    kv = _dev(kv, "kv")
    ks, kl = _dev(kv_start, "kv_start", torch.int64), _dev(kv_len, "kv_len", torch.int64)
    count = len(sources)
    if not 1 <= count <= _lib.DKV_SOURCES_MAX:
        raise ValueError(f"shared_kv_attention_dkv_multi: 1..{_lib.DKV_SOURCES_MAX} sources per call")
    descs = (_lib.DkvSource * count)()
    keep = []
    for i, src in enumerate(sources):
        t = [_dev(src[k], k) for k in ("q", "d_out", "lse", "delta")] + [_dev(src[k], k, torch.int64) for k in ("q_start", "q_len")]
        if t[0].shape[1] != kv.shape[1] or t[1].shape != t[0].shape or t[2].numel() < t[0].shape[0] or t[3].numel() < t[0].shape[0] or t[4].numel() != ks.numel():
            raise ValueError("shared_kv_attention_dkv_multi: a source's tensors do not fit together")
        keep.append(t)
        descs[i] = _lib.DkvSource(*[x.data_ptr() for x in t], float(src["scale"]), float(src["dropout_p"]), int(src["seed"]) & 0xFFFFFFFF, 0)
    dkv = torch.empty_like(kv)
    mode = 1 if half == torch.float16 else (2 if half == torch.bfloat16 else 0)
    with _on(kv.device):
        _lib.check(_lib.load().medtok_shared_kv_attention_dkv_multi_f32(descs, count, kv.data_ptr(), ks.data_ptr(), kl.data_ptr(), ks.numel(), int(max_kv_len),
                                                                        kv.shape[0], kv.shape[1], dkv.data_ptr(), mode, _stream(kv)),
                   "medtok_shared_kv_attention_dkv_multi_f32")
    return dkv


def sum_scale(vals: torch.Tensor, scale: float) -> torch.Tensor:
    """0-dim fp32 tensor = scale * sum(vals) (fp64 accumulation, fixed order)."""
    vals = _dev(vals, "vals")
    out = torch.empty((), dtype=torch.float32, device=vals.device)
    lib = _lib.load()
    with _on(vals.device):
        _lib.check(lib.medtok_sum_scale_f32(vals.data_ptr(), vals.numel(), float(scale), out.data_ptr(),
                                            _stream(vals)), "medtok_sum_scale_f32")
    return out


def ema_stats(zhat, idx, k_codes: int, fused: bool = False):
    """(bins [K] fp32, embed_sum [K, D] fp32).  With fused=True both are views of ONE buffer
    [embed_sum | bins], returned as a third value, so a single all-reduce covers both statistics
    (embed_sum first keeps it 16-byte aligned)."""
    zhat = _dev(zhat, "zhat")
    idx = _dev(idx, "idx", torch.int64)
    n, d = zhat.shape
    lib = _lib.load()
    stats = torch.empty(k_codes * (d + 1), dtype=torch.float32, device=zhat.device)
    es = stats[: k_codes * d].view(k_codes, d)
    bins = stats[k_codes * d:]
    ws = _ws(lib.medtok_ema_stats_workspace_bytes(n, k_codes), zhat)
    with _on(zhat.device):
        _lib.check(lib.medtok_ema_stats_f32(zhat.data_ptr(), idx.data_ptr(), n, d, k_codes, bins.data_ptr(),
                                            es.data_ptr(), ws.data_ptr(), ws.numel(), _stream(zhat)),
                   "medtok_ema_stats_f32")
    return (bins, es, stats) if fused else (bins, es)


def code_histogram(idx, k_codes: int) -> torch.Tensor:
    """bins [K] fp32: number of rows assigned to each code (exact)."""
    idx = _dev(idx.reshape(-1), "idx", torch.int64)
    lib = _lib.load()
    bins = torch.empty(k_codes, dtype=torch.float32, device=idx.device)
    ws = _ws(lib.medtok_code_histogram_workspace_bytes(k_codes), idx)
    with _on(idx.device):
        _lib.check(lib.medtok_code_histogram_f32(idx.data_ptr(), idx.numel(), k_codes, bins.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), _stream(idx)), "medtok_code_histogram_f32")
    return bins


def ema_apply_(E, cluster_size, bins, embed_sum, decay: float) -> None:
    """In-place codebook + cluster_size update."""
    for name, t in (("E", E), ("cluster_size", cluster_size)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.MedTokLibraryError(f"ema_apply_: {name} must be a contiguous fp32 device tensor")
    bins, embed_sum = _dev(bins, "bins"), _dev(embed_sum, "embed_sum")
    k, d = E.shape
    lib = _lib.load()
    with _on(E.device):
        _lib.check(lib.medtok_ema_apply_f32(E.data_ptr(), cluster_size.data_ptr(), bins.data_ptr(), embed_sum.data_ptr(),
                                            k, d, float(decay), float(1 - decay), _stream(E)), "medtok_ema_apply_f32")


def ema_cluster_size_(cluster_size, bins, decay: float) -> None:
    if not (cluster_size.is_cuda and cluster_size.dtype == torch.float32 and cluster_size.is_contiguous()):
        raise _lib.MedTokLibraryError("ema_cluster_size_: cluster_size must be a contiguous fp32 device tensor")
    bins = _dev(bins, "bins")
    lib = _lib.load()
    with _on(bins.device):
        _lib.check(lib.medtok_ema_cluster_size_f32(cluster_size.data_ptr(), bins.data_ptr(), cluster_size.numel(),
                                                   float(decay), float(1 - decay), _stream(bins)),
                   "medtok_ema_cluster_size_f32")


def usage_update_(window: torch.Tensor, ids: torch.Tensor, n_codes: int) -> torch.Tensor:
    """Slide `window` (fp32, in place) by ids.numel(), append ids, return the
    distinct-value count as a device int32 scalar (no host sync)."""
    if not (window.is_cuda and window.dtype == torch.float32 and window.is_contiguous()):
        raise _lib.MedTokLibraryError("usage_update_: window must be a contiguous fp32 device tensor")
    ids = _dev(ids.reshape(-1), "ids", torch.int64)
    lib = _lib.load()
    count = torch.empty((), dtype=torch.int32, device=window.device)
    ws = _ws(lib.medtok_usage_workspace_bytes(window.numel(), n_codes), window)
    with _on(window.device):
        _lib.check(lib.medtok_usage_update(window.data_ptr(), window.numel(), ids.data_ptr(), ids.numel(), n_codes,
                                           count.data_ptr(), ws.data_ptr(), ws.numel(), _stream(window)),
                   "medtok_usage_update")
    return count


def multi_search_eligible(n: int, k_codes: int, d: int, topk: int) -> bool:
    """may this search go into a soft_vq_forward_multi call (small: the exact fp32-MFMA path, at most 4096 rows)?"""
    return bool(_lib.load().medtok_soft_vq_multi_eligible(int(n), int(k_codes), int(d), int(topk)))


def soft_vq_forward_multi(searches, topk: int, want_sqerr: bool = False):
    """Several small soft top-k searches in one C call and three launches (include/medtok_vq.h: medtok_soft_vq_forward_multi_f32).
    searches: list of dict(x [n, d] fp32, what [K, d], wsq [K], out = optional [n, d] view for zq); every entry must be
    multi_search_eligible.  Returns a list of dict(xhat, idx, dist, w, zq, row_sqerr) -- the bits of soft_vq_forward per entry
    (row_sqerr: None unless want_sqerr, the training forward)."""
    import ctypes as C
    lib = _lib.load()
    count = len(searches)
    if not 1 <= count <= _lib.MULTI_SEARCH_MAX:
        raise ValueError(f"soft_vq_forward_multi: 1..{_lib.MULTI_SEARCH_MAX} searches per call")
    descs = (_lib.SearchDesc * count)()
    outs, keep = [], []
    d = None
    for i, q in enumerate(searches):
        x, what, wsq = q["x"], _dev(q["what"], "what"), _dev(q["wsq"], "wsq")
        # (x may be a column block of a wider row-major matrix: its row stride travels in the descriptor)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0
                and x.stride(0) >= x.shape[1] and x.data_ptr() % 16 == 0):
            x = _dev(x, "x")
        n, di = x.shape
        d = di if d is None else d
        if di != d or what.shape[1] != d:
            raise ValueError("soft_vq_forward_multi: all searches share one width")
        dev = x.device
        xhat = torch.empty((n, d), dtype=torch.float32, device=dev)
        idx = torch.empty((n, topk), dtype=torch.int64, device=dev)
        dist = torch.empty((n, topk), dtype=torch.float32, device=dev)
        w = torch.empty((n, topk), dtype=torch.float32, device=dev)
        zq, zstride = _zq_out(q.get("out"), n, d, x)
        sqerr = torch.empty((n,), dtype=torch.float32, device=dev) if want_sqerr else None
        keep.append((x, what, wsq))
        descs[i] = _lib.SearchDesc(x.data_ptr(), n, what.data_ptr(), wsq.data_ptr(), what.shape[0], xhat.data_ptr(), idx.data_ptr(), dist.data_ptr(),
                                   w.data_ptr(), zq.data_ptr(), zstride, x.stride(0) if n > 1 else d, _ptr(sqerr))
        outs.append(dict(xhat=xhat, idx=idx, dist=dist, w=w, zq=zq, row_sqerr=sqerr))
    ws = _ws(lib.medtok_soft_vq_forward_multi_workspace_bytes(descs, count, d, topk), keep[0][0])
    with _on(keep[0][0].device):
        _lib.check(lib.medtok_soft_vq_forward_multi_f32(descs, count, d, topk, ws.data_ptr(), ws.numel(), _stream(keep[0][0])),
                   "medtok_soft_vq_forward_multi_f32")
    return outs


def usage_update_multi_(window: torch.Tensor, ids_list, n_codes: int, extra_word=None) -> torch.Tensor:
    """usage_update_ for several id sets appended in order, in two launches: int32 [len(ids_list)] device tensor of the distinct-value
    counts after each update (no host sync).  extra_word (int32 device tensor): its first element is copied behind the counts (the
    result has one more entry), so that the caller's one host read brings it along; while it is non-zero the window is NOT written
    (include/medtok_vq.h: the caller repeats the forward on repaired inputs)."""
    import ctypes as C
    if not (window.is_cuda and window.dtype == torch.float32 and window.is_contiguous()):
        raise _lib.MedTokLibraryError("usage_update_multi_: window must be a contiguous fp32 device tensor")
    count = len(ids_list)
    if not 1 <= count <= _lib.USAGE_MULTI_MAX:
        raise ValueError(f"usage_update_multi_: 1..{_lib.USAGE_MULTI_MAX} updates per call")
    ids = [_dev(t.reshape(-1), "ids", torch.int64) for t in ids_list]
    ptrs = (C.c_void_p * count)(*[t.data_ptr() for t in ids])
    ms = (C.c_int64 * count)(*[t.numel() for t in ids])
    lib = _lib.load()
    if extra_word is not None and not (extra_word.is_cuda and extra_word.dtype == torch.int32 and extra_word.device == window.device):
        raise _lib.MedTokLibraryError("usage_update_multi_: extra_word must be an int32 tensor on the window's device")
    counts = torch.empty(count + (extra_word is not None), dtype=torch.int32, device=window.device)
    ws = _ws(lib.medtok_usage_multi_workspace_bytes(window.numel(), n_codes, count), window)
    with _on(window.device):
        _lib.check(lib.medtok_usage_update_multi_word(window.data_ptr(), window.numel(), ptrs, ms, count, n_codes, counts.data_ptr(), _ptr(extra_word),
                                                      ws.data_ptr(), ws.numel(), _stream(window)), "medtok_usage_update_multi")
    return counts


def normalized_search(z, what, wsq, topk: int = 1, path: int = PATH_AUTO):
    """(zhat, |zhat|^2, idx [n, topk], dist [n, topk]): F.normalize(z) and its nearest codes in one C call -- the head of
    NormEMAVectorQuantizer.forward (norm_ema_quantizer.py:169-179).  Same bits as rownorm() + topk_search()."""
    z, what, wsq = _dev(z, "z"), _dev(what, "what"), _dev(wsq, "wsq")
    n, d = z.shape
    k = what.shape[0]
    lib = _lib.load()
    dev = z.device
    zhat = torch.empty_like(z)
    zsq = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty((n, topk), dtype=torch.int64, device=dev)
    dist = torch.empty((n, topk), dtype=torch.float32, device=dev)
    ws = _ws(lib.medtok_normalized_search_workspace_bytes(n, k, d, topk, path), z)
    with _on(dev):
        _lib.check(lib.medtok_normalized_search_f32(z.data_ptr(), n, d, what.data_ptr(), wsq.data_ptr(), k, topk, path, zhat.data_ptr(),
                                                    zsq.data_ptr(), idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(), _stream(z)),
                   "medtok_normalized_search_f32")
    return zhat, zsq, idx, dist


def takes_filter_path(n: int, k_codes: int, d: int, topk: int, path: int = PATH_AUTO) -> bool:
    """does a search of this shape run the fp16 shortlist (and so profit from a prepared codebook)?"""
    return _lib.load().medtok_search_resolved_path(int(n), int(k_codes), int(d), int(topk), int(path)) == PATH_F16_FILTER


def prepare_codebook(weight: torch.Tensor, regions, normalised=None):
    """normalize(weight) plus everything the fp16-filter searches derive from it, once per weight version (include/medtok_vq.h:
    medtok_rownorm_image_f32 + medtok_codebook_prepare_f32; two launches): (what [K, d], wsq [K], {region name: prepared}) for
    regions = {name: (lo, hi)}.  A `prepared` entry goes to soft_vq_forward(..., prepared=...) together with what[lo:hi] / wsq[lo:hi].
    normalised = (what, wsq) of an earlier rownorm(weight): only the image and the regions' values are made (weight is not read)."""
    import ctypes as C
    w = _dev(weight if normalised is None else normalised[0], "weight")
    n, d = w.shape
    if not 1 <= len(regions) <= _lib.PREP_MAX_REGIONS:
        raise ValueError(f"prepare_codebook: 1..{_lib.PREP_MAX_REGIONS} regions")
    lib = _lib.load()
    dp = lib.medtok_filter_image_width(d)
    dev = w.device
    rows = n + 256
    what = torch.empty_like(w) if normalised is None else None
    wsq = torch.empty(n, dtype=torch.float32, device=dev) if normalised is None else None
    image = torch.empty((rows, dp), dtype=torch.float16, device=dev)
    descs = (_lib.RegionDesc * len(regions))()
    prepared = {}
    for i, (name, (lo, hi)) in enumerate(regions.items()):
        k = hi - lo
        if not 0 <= lo < hi <= n:
            raise ValueError(f"prepare_codebook: region {name} = [{lo}, {hi}) outside the codebook")
        wsqp = torch.empty((k + 255) // 256 * 256, dtype=torch.float32, device=dev)
        en_max = torch.empty(1, dtype=torch.float32, device=dev)
        descs[i] = _lib.RegionDesc(lo, k, wsqp.data_ptr(), en_max.data_ptr())
        prepared[name] = dict(image=image[lo:], wsqp=wsqp, en_max=en_max, k=k, d=d)
    with _on(dev):
        if normalised is None:
            _lib.check(lib.medtok_rownorm_image_f32(w.data_ptr(), n, d, what.data_ptr(), wsq.data_ptr(), image.data_ptr(), rows, dp, _stream(w)),
                       "medtok_rownorm_image_f32")
        else:
            what, wsq = w, _dev(normalised[1], "wsq")
            _lib.check(lib.medtok_codebook_image_f32(what.data_ptr(), n, d, image.data_ptr(), rows, dp, _stream(w)), "medtok_codebook_image_f32")
        _lib.check(lib.medtok_codebook_prepare_f32(wsq.data_ptr(), descs, len(regions), _stream(w)), "medtok_codebook_prepare_f32")
    return what, wsq, prepared


# Measurement hook (bench.py, tests; never set in product code): while this is a list, every soft_vq_forward that takes the fp16
# shortlist appends (its workspace, n, K, d, topk, path) -- the workspace stays alive with the entry, nothing is read back;
# filter_stats(entry) reduces it on the device afterwards.
FILTER_STATS = None


def filter_stats(entry) -> dict:
    """What the shortlist pass of the finished search behind `entry` (an element of FILTER_STATS) left behind: candidates per row,
    share of full candidate lists, rows handed to the exact kernel (include/medtok_vq.h: medtok_debug_filter_stats).  One host read."""
    ws, n, k, d, topk, path = entry
    out = torch.zeros(4, dtype=torch.int64, device=ws.device)
    with _on(ws.device):
        _lib.check(_lib.load().medtok_debug_filter_stats(ws.data_ptr(), ws.numel(), 1, n, k, d, topk, path, out.data_ptr(), _stream(ws)),
                   "medtok_debug_filter_stats")
    cand, full, fb, lists = out.cpu().tolist()
    return dict(rows=n, codes=k, candidates_per_row=cand / n, full_lists_share=full / max(lists, 1), lists_per_row=lists / n, fallback_rows=fb)


def _note_filter_stats(ws, n, k, d, topk, path):
    if FILTER_STATS is not None and n > 0 and takes_filter_path(n, k, d, topk, path):
        FILTER_STATS.append((ws, n, k, d, topk, path))


def soft_vq_forward(x, what, wsq, topk: int, path: int = PATH_AUTO, want_sqerr: bool = True, out=None, prepared=None):
    """rownorm -> search -> soft assign in one C call.
    Returns dict(xhat, idx, dist, w, zq, row_sqerr); `out` as in soft_assign.  prepared (inference, want_sqerr = False): the region's
    entry of prepare_codebook -- the same bits without the search's own passes over the codebook."""
    x, what, wsq = _dev(x, "x"), _dev(what, "what"), _dev(wsq, "wsq")
    n, d = x.shape
    k = what.shape[0]
    if prepared is not None and not want_sqerr and SEARCH_TIMER is None and n > 0:
        if prepared["k"] != k or prepared["d"] != d or prepared["image"].device != x.device:
            raise ValueError("soft_vq_forward: `prepared` belongs to another region / width / device")
        lib = _lib.load()
        dev = x.device
        xhat = torch.empty_like(x)
        idx = torch.empty((n, topk), dtype=torch.int64, device=dev)
        dist = torch.empty((n, topk), dtype=torch.float32, device=dev)
        w = torch.empty((n, topk), dtype=torch.float32, device=dev)
        zq, zstride = _zq_out(out, n, d, x)
        ws = _ws(lib.medtok_soft_vq_workspace_bytes(n, k, d, topk, path), x)
        with _on(dev):
            _lib.check(lib.medtok_soft_vq_forward_prepared_f32(x.data_ptr(), n, d, what.data_ptr(), wsq.data_ptr(), k, topk, path,
                                                               prepared["image"].data_ptr(), prepared["wsqp"].data_ptr(), prepared["en_max"].data_ptr(),
                                                               xhat.data_ptr(), idx.data_ptr(), dist.data_ptr(), w.data_ptr(),
                                                               zq.data_ptr(), zstride, ws.data_ptr(), ws.numel(), _stream(x)),
                       "medtok_soft_vq_forward_prepared_f32")
        _note_filter_stats(ws, n, k, d, topk, path)
        return dict(xhat=xhat, idx=idx, dist=dist, w=w, zq=zq, row_sqerr=None)
    if SEARCH_TIMER is not None:         # same kernels, launched piecewise so the search can be bracketed
        xhat, xsq = rownorm(x)
        idx, dist = topk_search(xhat, xsq, what, wsq, topk, path)
        w, zq, se = soft_assign(x, what, idx, dist, want_sqerr=want_sqerr, out=out)
        return dict(xhat=xhat, idx=idx, dist=dist, w=w, zq=zq, row_sqerr=se)
    lib = _lib.load()
    dev = x.device
    xhat = torch.empty_like(x)
    idx = torch.empty((n, topk), dtype=torch.int64, device=dev)
    dist = torch.empty((n, topk), dtype=torch.float32, device=dev)
    w = torch.empty((n, topk), dtype=torch.float32, device=dev)
    zq, zstride = _zq_out(out, n, d, x)
    se = torch.empty(n, dtype=torch.float32, device=dev) if want_sqerr else None
    ws = _ws(lib.medtok_soft_vq_workspace_bytes(n, k, d, topk, path), x)
    with _on(dev):
        _lib.check(lib.medtok_soft_vq_forward_f32(x.data_ptr(), n, d, what.data_ptr(), wsq.data_ptr(), k, topk, path,
                                                  xhat.data_ptr(), idx.data_ptr(), dist.data_ptr(), w.data_ptr(),
                                                  zq.data_ptr(), zstride, _ptr(se), ws.data_ptr(), ws.numel(), _stream(x)),
                   "medtok_soft_vq_forward_f32")
    _note_filter_stats(ws, n, k, d, topk, path)
    return dict(xhat=xhat, idx=idx, dist=dist, w=w, zq=zq, row_sqerr=se)
