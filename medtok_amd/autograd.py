"""The autograd layer of the quantiser: torch.autograd.Function nodes around the library's training kernels.

Everything here depends on torch and medtok_amd.ops only; the modules of vector_quantization_soft_one_new (CrossAttention,
VectorQuantizer) and the tokenizer call it, and that module re-exports every name below for callers that knew them there.
  - _SplitLinearFunction / split_linear: y = x W^T + b with forward, dX and dW on the library's own GEMM (three fp16 MFMA passes over
    (hi, lo) images for fp32 callers, ONE half-precision pass under torch.autocast);
  - _RaggedAttentionFunction / _TwoSidedAttentionFunction: the ragged attention core (HIP forward with dropout, HIP dQ / dKV backward);
  - fan_out_text / _TextFanOut / _KeyGradSink: the text rows of a training step behind ONE gradient buffer;
  - _SegmentMeanFunction, _HeadBlockDiag: the node mean of a code, the block-diagonal per-head weights;
  - _SoftVQFunction / _SoftVQMultiFunction / _DecodeFunction: a search, all searches of a forward, and decode under autograd
    (sparse backward; the code gradients summed per code without atomics);
  - _EmbedCodesFunction: the embedding lookup over the stored token table (MedTokEmbedding) and the gradient of its miss row;
  - _EmbedProjectFunction: that lookup with the consumer's projector folded into the tables (forward on embed_folded_kernel; dW, db
    and the miss row's gradient in a fixed order); _SmallLinearFunction / small_linear: y = x W^T + b on the exact fp32 product.
"""
from __future__ import annotations

import torch

from . import ops

# The switches of this module: each is read here and nowhere else, and a test runs both positions.
#
# training: the text rows are read three ways -- as the keys of every cross-attention layer (:83,86: always the ORIGINAL text), as the
# CLS query of the text side, as the CLS half of h (tokenizer.py:162) -- and autograd would sum their four [B L, D] gradients with a
# zero fill and an add pass each (0.8 ms of a 12 ms step at B = 256, L = 512).  On: the layers' dQ kernels leave their sources with
# the sink and the node that collects the key gradient turns them into the [rows, D] matrix with ONE dKV launch over all layers'
# queries (per-layer launches -- the first stores, the others add -- only for keys that differ or more layers than
# ops.DKV_SOURCES_MAX); the CLS gradients are added to its B rows in place (_TextFanOut).
# Both positions: tests/test_gpu_train_step.py::test_key_gradient_sink_gives_the_gradients_of_plain_autograd
KEY_GRADIENT_SINK = True
# training: all searches of a forward run under one autograd node, so that the codebook receives ONE dense gradient
# (_SoftVQMultiFunction).  On: their forward as ONE batched call too (three launches: ops.soft_vq_forward_multi with per-row squared
# errors) where every search takes the exact path with at most 4096 rows.  Off: measured SLOWER at cfg 4 (six searches of 256 rows
# over 49 152 / 16 384 codes: 10.5 -> 10.9 ms per step, tools/r05/ab_cfg4_switch.py TRAIN_BATCHED_SEARCHES) -- the batched kernel's
# split plan is made for the few hundred codes of the reference's default codebook; it pays at e_dim = 64, n_e = 600 (fewer
# launches), not here.
# Both positions: tests/test_gpu_train_step.py::test_batched_training_searches_switch_gives_the_same_bits
TRAIN_BATCHED_SEARCHES = False
# ... the searches that share a region (the two shared ones; text and its aug view; graph and its aug view) as ONE search on their rows stacked.
# Both positions: tests/test_gpu_train_step.py::test_batched_training_searches_switch_gives_the_same_bits (its second half)
TRAIN_STACK_SEARCHES_OF_A_REGION = True


class _SegmentMeanFunction(torch.autograd.Function):
    """Mean of the attended nodes of every code (:140-141) under autograd: forward = the library's ordered segment mean (rows of a code
    are adjacent), backward = each node row receives its code's gradient / node count (one division, one gather).  The training path
    used to scatter the rows into a zero [B, max_nodes, D] tensor and sum it (157 MB at B = 256, max 200 nodes, D = 768)."""

    @staticmethod
    def forward(ctx, g, starts, counts, batch_sorted):
        ctx.save_for_backward(counts, batch_sorted)
        ctx.in_dtype = g.dtype
        return ops.segment_mean(g.detach().float().contiguous(), starts, counts)

    @staticmethod
    def backward(ctx, d_out):
        counts, batch_sorted = ctx.saved_tensors
        per_code = d_out.float() / counts.clamp(min=1).unsqueeze(-1).to(torch.float32)
        return per_code[batch_sorted].to(ctx.in_dtype), None, None, None


class _KeyGradSink:
    """Where the layers that share one key matrix leave its gradient during a backward (see _TextFanOut): as `pending` sources (a
    layer's queries, upstream gradient, row statistics, mask parameters) that the collecting node turns into the gradient with ONE
    launch, or -- keys that differ from the pending sources', more sources than ops.DKV_SOURCES_MAX -- written by the layer's own dKV
    kernel at once (`buf`: the first stores, the others add)."""
    __slots__ = ("buf", "node", "pending", "common")

    def __init__(self):
        self.buf = None         # the [rows, D] gradient while a backward is under way
        self.node = None        # weak reference to the autograd node that collects it
        self.pending = []       # sources of ops.shared_kv_attention_dkv_multi
        self.common = None      # (kv, kv_start, kv_len, max_kv_len, half) of the pending sources


def _sink_key_gradient(sink, q, q_start, q_len, kv, kv_start, kv_len, max_q_len, max_kv_len, scale, dropout_p, seed, out, lse, d_out, half, dq_into=None):
    """dq of one attention call whose key gradient goes to `sink`: deferred as a source of the collecting node's one dKV launch where
    the keys are those of the sources already there, else written / added by this call's own dKV kernel."""
    common = (kv, kv_start, kv_len, max_kv_len, half)
    same = sink.common is not None and all(a is b or (torch.is_tensor(a) and torch.is_tensor(b) and a.data_ptr() == b.data_ptr() and a.shape == b.shape)
                                           or (not torch.is_tensor(a) and a == b) for a, b in zip(common, sink.common))
    if sink.buf is None and len(sink.pending) < ops.DKV_SOURCES_MAX and (not sink.pending or same):
        dq, delta = ops.shared_kv_attention_backward_dq(q, q_start, q_len, kv, kv_start, kv_len, max_q_len, max_kv_len, scale, dropout_p, seed, out, lse,
                                                        d_out, half=half, dq_into=dq_into)
        sink.pending.append(dict(q=q, d_out=d_out, lse=lse, delta=delta, q_start=q_start, q_len=q_len, scale=scale, dropout_p=dropout_p, seed=seed))
        sink.common = common
        return dq
    first = sink.buf is None
    if first:
        sink.buf = torch.empty_like(kv)
    dq, _ = ops.shared_kv_attention_backward(q, q_start, q_len, kv, kv_start, kv_len, max_q_len, max_kv_len, scale, dropout_p, seed, out, lse, d_out,
                                             half=half, dkv_into=sink.buf, accumulate=not first, dq_into=dq_into)
    return dq


class _TextFan:
    """carried by a text tensor that went through fan_out_text(): the CLS rows and the gradient sink of its keys"""
    __slots__ = ("sink", "cls")

    def __init__(self, sink, cls):
        self.sink, self.cls = sink, cls


class _TextFanOut(torch.autograd.Function):
    """text [B, L, D] -> (the same rows, their CLS rows [B, D]) with ONE gradient buffer behind both: the attention layers whose keys
    these rows are add their dKV into `sink` during the backward (and hand autograd no gradient for them), this node -- which the
    engine runs after every consumer of its outputs -- adds the CLS gradient to the buffer's B first rows and passes it on."""

    @staticmethod
    def forward(ctx, text, sink):
        ctx.sink = sink
        ctx.seq_len = text.shape[1]
        ctx.set_materialize_grads(False)
        return text.view_as(text), text[:, 0].contiguous()

    @staticmethod
    def backward(ctx, g_rows, g_cls):
        sink = ctx.sink
        buf, sink.buf = sink.buf, None
        pending, common, sink.pending, sink.common = sink.pending, sink.common, [], None
        if pending:                         # the deferred key gradients of all layers: one launch, one store of the [rows, D] matrix
            d = ops.shared_kv_attention_dkv_multi(pending, common[0], common[1], common[2], common[3], half=common[4])
            buf = d if buf is None else buf.add_(d)
        if g_rows is not None:              # (a consumer outside the sink protocol)
            g_rows = g_rows.float()
            buf = g_rows.clone() if buf is None else buf.view_as(g_rows).add_(g_rows)
        if g_cls is not None:
            if buf is None:
                buf = g_cls.new_zeros((g_cls.shape[0], ctx.seq_len, g_cls.shape[1]), dtype=torch.float32)
            buf = buf.view(g_cls.shape[0], -1, g_cls.shape[1])
            buf[:, 0].add_(g_cls)
        return (None if buf is None else buf.view(-1, ctx.seq_len, buf.shape[-1])), None


def fan_out_text(text):
    """The text rows [B, L, D] of a training step behind one gradient buffer (KEY_GRADIENT_SINK): returns the same values as a tensor
    that carries `_medtok_fan` = (sink, CLS rows).  CrossAttention.pooled() and MultimodalTokenizer.quant() read the CLS rows from
    there and route the key gradients of the attention layers into the sink; any other use of the returned tensor is ordinary
    autograd.  Anything it does not apply to (no autograd, not an fp32 [B, L, D] tensor on an MI355X) is returned as it came."""
    if getattr(text, "_medtok_fan", None) is not None:
        return text
    if not (KEY_GRADIENT_SINK and torch.is_tensor(text) and text.is_cuda and text.dim() == 3 and text.dtype == torch.float32
            and text.requires_grad and torch.is_grad_enabled() and text.is_contiguous() and text.shape[1] > 0
            and hasattr(torch._C, "_will_engine_execute_node")):
        return text
    import weakref
    sink = _KeyGradSink()
    rows, cls = _TextFanOut.apply(text, sink)
    sink.node = weakref.ref(rows.grad_fn)
    rows._medtok_fan = _TextFan(sink, cls)
    return rows


def _autocast_half():
    """the half-precision dtype of the attention backward's products under torch.autocast (None: exact fp32 kernels)"""
    if torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") in (torch.float16, torch.bfloat16):
        return torch.get_autocast_dtype("cuda")
    return None


def _split_forward(half, width, max_q_len, q_rows, kv_rows):
    """the training forward on the three-pass fp16 kernel? (autocast callers, many query rows per code: see _RaggedAttentionFunction)"""
    return half is not None and width in ops.ATTENTION_TRAIN_SPLIT_WIDTHS and max_q_len > 8 and q_rows > 0 and kv_rows > 0


def _live_sink(sink, needs_kv_grad):
    """the sink if THIS backward will run the node that collects it (torch.autograd.grad() for other inputs does not), else None"""
    if sink is None or not needs_kv_grad:
        return None
    node = sink.node() if sink.node is not None else None
    return sink if (node is not None and torch._C._will_engine_execute_node(node)) else None


class _TwoSidedAttentionFunction(torch.autograd.Function):
    """Both directions of a training layer in ONE autograd node: query rows [0, cut) (the graph side: nodes x heads) attend to kv_a
    (the text rows), rows [cut, n) (the text side: CLS x heads) to kv_b (the nodes) -- the two launches of _RaggedAttentionFunction
    writing into row ranges of one output (and, backward, of one dQ) instead of a split in front and a concatenation behind, each a
    copy of the [R heads, D] matrix forward and backward.  la / lb = (q_start, q_len, kv_start, kv_len, max_q_len, max_kv_len) per side."""

    @staticmethod
    def forward(ctx, qf, kv_a, kv_b, la, lb, cut, scale, dropout_p, seed_a, seed_b, sink):
        q = qf.detach().float().contiguous()
        ka, kb = kv_a.detach().float().contiguous(), kv_b.detach().float().contiguous()
        ctx.half = _autocast_half()
        n = q.shape[0]
        out = torch.zeros_like(q)
        lse = torch.full((n,), float("-inf"), dtype=torch.float32, device=q.device)
        for lo, hi, kv, l, seed in ((0, cut, ka, la, seed_a), (cut, n, kb, lb, seed_b)):
            if hi > lo:
                ops.shared_kv_attention_train(q[lo:hi], l[0], l[1], kv, l[2], l[3], l[4], scale, dropout_p, seed,
                                              split=_split_forward(ctx.half, q.shape[1], l[4], hi - lo, kv.shape[0]), out=out[lo:hi], lse=lse[lo:hi])
        ctx.save_for_backward(q, ka, kb, out, lse, *la[:4], *lb[:4])
        ctx.cfg = (cut, la[4], la[5], lb[4], lb[5], scale, dropout_p, seed_a, seed_b, qf.dtype, kv_a.dtype, kv_b.dtype)
        ctx.sink = sink
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, ka, kb, out, lse, *lists = ctx.saved_tensors
        cut, mq_a, mk_a, mq_b, mk_b, scale, dropout_p, seed_a, seed_b, qd, kad, kbd = ctx.cfg
        n = q.shape[0]
        d = d_out.float().contiguous()
        dq = torch.empty_like(q)
        dka = dkb = None
        sink = _live_sink(ctx.sink, ctx.needs_input_grad[1])
        if cut > 0:
            a = lists[:4]
            if sink is not None:
                _sink_key_gradient(sink, q[:cut], a[0], a[1], ka, a[2], a[3], mq_a, mk_a, scale, dropout_p, seed_a, out[:cut], lse[:cut], d[:cut], ctx.half,
                                   dq_into=dq[:cut])
            else:
                _, dka = ops.shared_kv_attention_backward(q[:cut], a[0], a[1], ka, a[2], a[3], mq_a, mk_a, scale, dropout_p, seed_a, out[:cut], lse[:cut],
                                                          d[:cut], half=ctx.half, dq_into=dq[:cut])
                dka = dka.to(kad)
        elif ctx.needs_input_grad[1] and sink is None:
            dka = torch.zeros_like(ka).to(kad)
        if n > cut:
            b = lists[4:]
            _, dkb = ops.shared_kv_attention_backward(q[cut:], b[0], b[1], kb, b[2], b[3], mq_b, mk_b, scale, dropout_p, seed_b, out[cut:], lse[cut:], d[cut:],
                                                      half=ctx.half, dq_into=dq[cut:])
            dkb = dkb.to(kbd)
        else:
            dkb = torch.zeros_like(kb).to(kbd)
        return dq.to(qd), dka, dkb, None, None, None, None, None, None, None, None


class _RaggedAttentionFunction(torch.autograd.Function):
    """The ragged attention core under autograd: forward = medtok_shared_kv_attention_train_f32 (dropout on the probabilities by
    a stateless hash mask, log-sum-exp kept per row), backward = medtok_shared_kv_attention_backward_f32 (dQ and dKV kernels that
    rebuild probabilities and mask; nothing of size rows x keys is stored).  fp32 whatever autocast says.
    `sink` (a _KeyGradSink, or None): the key gradient goes into the sink's buffer instead of back to autograd."""

    @staticmethod
    def forward(ctx, q, kv, q_start, q_len, kv_start, kv_len, max_q_len, max_kv_len, scale, dropout_p, seed, sink=None):
        qf, kvf = q.detach().float().contiguous(), kv.detach().float().contiguous()
        # under torch.autocast the backward's four matrix products run as ONE half-precision pass (the reference's class there) and
        # the forward on the three-pass fp16 products (fp32-accurate to ~1e-6: its log-sum-exp feeds the backward's softmax
        # rebuild) where more than a few query rows share a code's keys; fp32 callers keep the exact fp32 kernels on both sides
        ctx.half = _autocast_half()
        split = _split_forward(ctx.half, qf.shape[1], max_q_len, qf.shape[0], kvf.shape[0])
        out, lse = ops.shared_kv_attention_train(qf, q_start, q_len, kvf, kv_start, kv_len, max_q_len, scale, dropout_p, seed, split=split)
        ctx.save_for_backward(qf, kvf, out, lse, q_start, q_len, kv_start, kv_len)
        ctx.cfg = (max_q_len, max_kv_len, scale, dropout_p, seed, q.dtype, kv.dtype)
        ctx.sink = sink
        return out

    @staticmethod
    def backward(ctx, d_out):
        qf, kvf, out, lse, q_start, q_len, kv_start, kv_len = ctx.saved_tensors
        max_q_len, max_kv_len, scale, dropout_p, seed, qd, kd = ctx.cfg
        sink = _live_sink(ctx.sink, ctx.needs_input_grad[1])
        if sink is not None:
            dq = _sink_key_gradient(sink, qf, q_start, q_len, kvf, kv_start, kv_len, max_q_len, max_kv_len, scale, dropout_p, seed, out, lse,
                                    d_out.float().contiguous(), ctx.half)
            return dq.to(qd), None, None, None, None, None, None, None, None, None, None, None
        dq, dkv = ops.shared_kv_attention_backward(qf, q_start, q_len, kvf, kv_start, kv_len, max_q_len, max_kv_len, scale, dropout_p, seed,
                                                   out, lse, d_out.float().contiguous(), half=ctx.half)
        return dq.to(qd), dkv.to(kd), None, None, None, None, None, None, None, None, None, None


# split-K of the weight-gradient products (dW = dY^T X, contraction over the rows): at least this many rows per group.  A cfg 4 layer
# has ~5 600 rows: at 2048 its [768, 768] gradients ran as 18 blocks of 256 x 256 on 256 CUs (56 us), its block-diagonal ones as 72 (146 us)
SPLIT_K_MIN_ROWS = 512


def _pad32(n):
    return (int(n) + 31) // 32 * 32


class _SplitLinearFunction(torch.autograd.Function):
    """y = x W^T + b under autograd on the library's own dense product (medtok_split_gemm_scaled_f16: three fp16 MFMA passes over
    (hi, lo) pairs, fp32-accurate) -- forward, data gradient dX = dY W and weight gradient dW = dY^T X are all "A . B^T" products of
    split operands; the operands whose magnitude the host does not know (activations, upstream gradients) are prescaled by a power
    of two taken from a device-side |.|_max, so nothing is read back.  fp32 in and out whatever autocast says (the reference's
    projections, vector_quantization_soft_one_new.py:30,45, run in the autocast dtype: this is at least as accurate)."""

    @staticmethod
    def _weight_images(w, wf, npad_t):
        """(amax, images [n, pad32(k)], transposed images [k, pad32(n)]) of a weight, per (storage, version): a parameter is used by
        both attention directions of a step and by forward and backward -- one |w|_max and one split each instead of four.  Tensors
        built inside the graph (the block-diagonal per-head weights) are new objects every forward and are simply split again."""
        # (a slice of a parameter -- the q / k / v thirds of in_proj_weight -- is cached on the parameter it views)
        holder = w if isinstance(w, torch.nn.Parameter) else (w._base if isinstance(getattr(w, "_base", None), torch.nn.Parameter) else None)
        key = (w.data_ptr(), w._version, tuple(w.shape))
        cache = getattr(holder, "_medtok_train_images", None) if holder is not None else None
        if cache is not None and key[0] in cache and cache[key[0]][0] == key:
            return cache[key[0]][1]
        aw = ops.absmax(wf)
        val = (aw, ops.split_half_scaled(wf, _pad32(wf.shape[1]), aw), ops.split_half_scaled(wf, npad_t, aw, transpose=True))
        if holder is not None:
            if cache is None:
                cache = holder._medtok_train_images = {}
            cache[key[0]] = (key, val)
        return val

    @staticmethod
    def _half_images(w, dt, kp, npad):
        """(w [n, pad32(k)], w^T [k, pad32(n)]) as dt (fp16 / bf16) matrices, per (storage, version, dtype) for parameters"""
        holder = w if isinstance(w, torch.nn.Parameter) else (w._base if isinstance(getattr(w, "_base", None), torch.nn.Parameter) else None)
        key = (w.data_ptr(), w._version, tuple(w.shape), dt)
        cache = getattr(holder, "_medtok_half_images", None) if holder is not None else None
        if cache is not None and (key[0], dt) in cache and cache[(key[0], dt)][0] == key:
            return cache[(key[0], dt)][1]
        w16 = w.detach().to(dt)
        n, k = w16.shape
        val = (torch.nn.functional.pad(w16, (0, kp - k)).contiguous() if kp != k else w16.contiguous(),
               torch.nn.functional.pad(w16.t(), (0, npad - n)).contiguous())
        if holder is not None:
            if cache is None:
                cache = holder._medtok_half_images = {}
            cache[(key[0], dt)] = (key, val)
        return val

    @staticmethod
    def _forward_half(ctx, x, w, b, dt):
        """the autocast form: y = x16 w16^T + b, one half-precision pass with fp32 accumulation; the 16-bit operand images (and, in
        the backward, their transposes) come from the library's own cast / transpose kernels"""
        m, k = x.shape
        n = w.shape[0]
        kp, npad = _pad32(k), _pad32(n)
        xf = x.detach().float()
        xf = xf if xf.stride(1) == 1 and xf.stride(0) % 4 == 0 and xf.data_ptr() % 16 == 0 else xf.contiguous()
        w16, wt16 = _SplitLinearFunction._half_images(w, dt, kp, npad)
        # the weight gradient contracts over the rows: it reads x TRANSPOSED (split over the rows into `groups` chunks: see backward);
        # that image comes out of the same pass over x as the forward's operand, and is what the backward keeps of x
        groups, chunk, mp = _SplitLinearFunction._row_split(m, n, k)
        if ctx.needs_input_grad[1]:
            x16, xt16 = ops.half_image_pair(xf, kp, mp, dt, group_cols=chunk)
        else:
            x16, xt16 = ops.half_image(xf, kp, dt), None
        y = ops.half_gemm(x16, w16, n_g=n, k_g=kp, bias=None if b is None else b.detach().float().contiguous())
        ctx.save_for_backward(xt16, wt16)
        ctx.shape = (m, k, n)
        ctx.half = dt
        ctx.dtypes = (x.dtype, w.dtype, None if b is None else b.dtype)
        return y

    @staticmethod
    def _row_split(m, n, k):
        """split-K of the weight-gradient product: (groups, rows per group (a multiple of 64), padded row count)"""
        tiles = ((n + 255) // 256) * ((k + 255) // 256)
        groups = max(1, min(256 // max(tiles, 1), m // SPLIT_K_MIN_ROWS))
        chunk = (-(-m // groups) + 63) // 64 * 64
        groups = -(-m // chunk)
        return groups, chunk, groups * chunk

    @staticmethod
    def _backward_half(ctx, dy):
        xt16, wt16 = ctx.saved_tensors
        dxt, dwt, dbt = ctx.dtypes
        m, k, n = ctx.shape
        dt = ctx.half
        npad = wt16.shape[1]
        dyf = dy.detach().float().contiguous()
        dx = dw = db = None
        groups, chunk, mp = _SplitLinearFunction._row_split(m, n, k)
        want_dx, want_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and xt16 is not None
        want_db = dbt is not None and ctx.needs_input_grad[2]
        if want_dx and want_dw:                                   # both images of dY (and the bias gradient) from one pass over it
            if want_db:
                dy16, dyt16, db = ops.half_image_pair(dyf, npad, mp, dt, col_sums=True)
                db = db.to(dbt)
            else:
                dy16, dyt16 = ops.half_image_pair(dyf, npad, mp, dt)
        else:                                                     # (only one of dX / dW is wanted)
            dy16 = ops.half_image(dyf, npad, dt) if want_dx else None
            if want_dw and want_db and m > 0:
                dyt16, db = ops.half_image(dyf, mp, dt, transpose=True, col_sums=True)
                db = db.to(dbt)
            else:
                dyt16 = ops.half_image(dyf, mp, dt, transpose=True) if want_dw else None
        if want_dx:                          # dX [m, k] = dY [m, n] . (W^T [k, n])^T
            dx = ops.half_gemm(dy16, wt16, n_g=k, k_g=npad).to(dxt)
        if want_dw:                          # dW [n, k] = dY^T [n, m] . (X^T [k, m])^T, split over the rows in one grouped launch
            dw = ops.half_gemm(dyt16, xt16, n_g=k, k_g=chunk, groups=groups, a_group_cols=chunk, b_group_rows=k)
            dw = (dw.view(n, groups, k).sum(1) if groups > 1 else dw).to(dwt)
        if want_db and db is None:
            db = dyf.sum(0).to(dbt)
        return dx, dw, db

    @staticmethod
    def forward(ctx, x, w, b):
        m, k = x.shape
        n = w.shape[0]
        ctx.half = None
        if (torch.is_autocast_enabled() and m > 0 and k % 8 == 0 and n % 4 == 0 and k % 4 == 0
                and torch.get_autocast_dtype("cuda") in (torch.float16, torch.bfloat16)):
            return _SplitLinearFunction._forward_half(ctx, x, w, b, torch.get_autocast_dtype("cuda"))
        xf, wf = x.detach().float().contiguous(), w.detach().float().contiguous()
        m, k = xf.shape
        n = wf.shape[0]
        kp = _pad32(k)
        if m == 0:
            ctx.shape = (0, k, n)
            ctx.dtypes = (x.dtype, w.dtype, None if b is None else b.dtype)
            return xf.new_zeros(0, n)
        ax = ops.absmax(xf)
        aw, w_img, wt_img = _SplitLinearFunction._weight_images(w, wf, _pad32(n))
        y = ops.split_gemm_scaled(ops.split_half_scaled(xf, kp, ax), w_img, n_g=n, k_g=kp,
                                  bias=None if b is None else b.detach().float().contiguous(), amax_a=ax, amax_b=aw)
        ctx.save_for_backward(xf, ax, aw, *wt_img)
        ctx.shape = (m, k, n)
        ctx.dtypes = (x.dtype, w.dtype, None if b is None else b.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.half is not None:
            return _SplitLinearFunction._backward_half(ctx, dy)
        dxt, dwt, dbt = ctx.dtypes
        dyf = dy.float().contiguous()
        m, k, n = ctx.shape
        if m == 0:                           # no rows (a batch without graph nodes, an empty z): empty / zero gradients, like F.linear
            return (dyf.new_zeros(0, k).to(dxt) if ctx.needs_input_grad[0] else None,
                    dyf.new_zeros(n, k).to(dwt) if ctx.needs_input_grad[1] else None,
                    dyf.new_zeros(n).to(dbt) if (dbt is not None and ctx.needs_input_grad[2]) else None)
        xf, ax, aw, wt_hi, wt_lo = ctx.saved_tensors
        ad = ops.absmax(dyf)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:          # dX [m, k] = dY [m, n] . (W^T [k, n])^T
            npad = _pad32(n)
            dx = ops.split_gemm_scaled(ops.split_half_scaled(dyf, npad, ad), (wt_hi, wt_lo), n_g=k, k_g=npad, amax_a=ad, amax_b=aw).to(dxt)
        if ctx.needs_input_grad[1]:          # dW [n, k] = dY^T [n, m] . (X^T [k, m])^T: both operands transposed, contraction over the rows
            # split-K in one grouped launch: the rows are cut into G chunks, group g multiplies chunk g of both operands into its own
            # [n, k] block, the G blocks are summed (a [768, 768] gradient is nine 256 x 256 tiles: alone they would walk all the
            # rows on nine CUs)
            groups, chunk, mp = _SplitLinearFunction._row_split(m, n, k)
            dw = ops.split_gemm_scaled(ops.split_half_scaled(dyf, mp, ad, transpose=True),
                                       ops.split_half_scaled(xf, mp, ax, transpose=True, group_cols=chunk),
                                       n_g=k, k_g=chunk, amax_a=ad, amax_b=ax, groups=groups, a_group_cols=chunk, b_group_rows=k)
            dw = (dw.view(n, groups, k).sum(1) if groups > 1 else dw).to(dwt)
        if dbt is not None and ctx.needs_input_grad[2]:
            db = dyf.sum(0).to(dbt)
        return dx, dw, db


def split_linear(x, w, b=None):
    return _SplitLinearFunction.apply(x, w, b)


class _HeadBlockDiag(torch.autograd.Function):
    """The block-diagonal matrix of a [H hd, D] projection weight's per-head blocks -- transposed: blocks w_h^T, [H D, H hd] (the fold
    of W_k into the queries); else blocks w_h, [H hd, H D] (W_v on the per-head contexts) -- in two launches (zero fill + one
    strided copy) with a one-launch backward (the diagonal blocks of the gradient, gathered).  torch.block_diag over H slices is
    the same matrix in 5 launches forward and 11 backward (a zero [D, D] tensor, a copy and an add per slice)."""

    @staticmethod
    def forward(ctx, w, heads, transposed):
        hd, dim = w.shape[0] // heads, w.shape[1]
        ctx.cfg = (heads, hd, dim, transposed)
        blocks = w.detach().view(heads, hd, dim)
        if transposed:
            out = w.new_zeros(heads * dim, heads * hd)
            out.view(heads, dim, heads, hd).diagonal(dim1=0, dim2=2).copy_(blocks.permute(2, 1, 0))
        else:
            out = w.new_zeros(heads * hd, heads * dim)
            out.view(heads, hd, heads, dim).diagonal(dim1=0, dim2=2).copy_(blocks.permute(1, 2, 0))
        return out

    @staticmethod
    def backward(ctx, g):
        heads, hd, dim, transposed = ctx.cfg
        if transposed:
            gw = g.view(heads, dim, heads, hd).diagonal(dim1=0, dim2=2).permute(2, 1, 0)
        else:
            gw = g.view(heads, hd, heads, dim).diagonal(dim1=0, dim2=2).permute(2, 0, 1)
        return gw.reshape(heads * hd, dim), None, None


class _SoftVQFunction(torch.autograd.Function):
    """One search in train mode: (zq_ste, vq, commit, xhat, idx, w) from projected rows x and a codebook region.

    Forward is the fused gfx950 path (rownorm -> search -> soft assign, medtok_soft_vq_forward_f32) plus the
    fixed-order loss reduction.  Backward is ONE sparse kernel (medtok_soft_vq_backward_f32): per row only the k
    selected codes carry gradient -- the dense N x K matrix the reference's autograd graph differentiates
    (:120-125,157-182,203-214) is exactly zero everywhere else.  The per-(row, slot) code gradients are summed per
    code in row order by the EMA-statistics kernels (no atomics: bit-reproducible), then taken through F.normalize.
    The upstream gradients of vq / commit stay on the device (0-dim tensors); nothing synchronises the host."""

    @staticmethod
    def forward(ctx, x, weight, what, wsq, topk, path, beta):
        ctx.set_materialize_grads(False)
        r = ops.soft_vq_forward(x.detach(), what, wsq, topk, path, want_sqerr=True)
        n, d = x.shape
        vq = ops.sum_scale(r["row_sqerr"], (1.0 / (n * d)) if n else float("nan"))      # mean of nothing: nan, like F.mse_loss
        commit = ops.sum_scale(r["row_sqerr"], beta / (n * d))
        ctx.save_for_backward(x, weight, r["xhat"], what, r["idx"], r["w"])
        ctx.beta = beta
        ctx.mark_non_differentiable(r["idx"], r["w"])
        return r["zq"], vq, commit, r["xhat"], r["idx"], r["w"]

    @staticmethod
    def backward(ctx, g_zq_ste, g_vq, g_commit, g_xhat, _gi, _gw):
        x, weight, xhat, what, idx, w = ctx.saved_tensors
        n, d = x.shape
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        as_f32 = lambda t: None if t is None else t.float()
        gx, g_code = ops.soft_vq_backward(x.detach(), xhat, what, idx, w, g_xhat=as_f32(g_xhat), g_out=as_f32(g_zq_ste),
                                          g_vq=as_f32(g_vq), g_commit=as_f32(g_commit),
                                          vq_scale=2.0 / (n * d), commit_scale=2.0 * ctx.beta / (n * d),
                                          want_gx=want_x, want_g_code=want_w)
        gw = None
        if want_w:
            bins, g_what = ops.ema_stats(g_code, idx.reshape(-1), what.shape[0])
            gw = ops.normalize_backward(g_what, what, weight.detach(), live=bins)
        return gx, gw, None, None, None, None, None


class _DecodeFunction(torch.autograd.Function):
    """VectorQuantizer.decode under autograd: embedding [N, S * d] from stored (tokens, weights) and the codebook weight.

    Forward is the decode kernel (medtok_decode_tokens_f32).  Backward is ONE kernel (medtok_decode_tokens_backward_f32) for the
    gradient of the weights and the per-(row, slot, j) gradients of the normalised codes; those are summed per code in row order
    by the EMA-statistics kernels and taken through F.normalize exactly as _SoftVQFunction's code gradient is (no float atomics:
    two runs give the same bits).  Nothing flows to the token ids."""

    @staticmethod
    def forward(ctx, weights, weight, tokens, what, regions, status):
        out = ops.decode_tokens(tokens, weights.detach(), what, regions, status=status)
        ctx.save_for_backward(weights, weight, tokens, what)
        ctx.regions = regions
        return out

    @staticmethod
    def backward(ctx, g):
        weights, weight, tokens, what = ctx.saved_tensors
        want_w, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_w or want_c):
            return None, None, None, None, None, None
        g_w, g_code, g_ids = ops.decode_tokens_backward(g.float(), tokens, weights.detach(), what, ctx.regions, want_g_w=want_w, want_g_code=want_c)
        gw = None
        if want_c:
            bins, g_what = ops.ema_stats(g_code, g_ids, what.shape[0])
            gw = ops.normalize_backward(g_what, what, weight.detach(), live=bins)
        if g_w is not None:
            g_w = g_w.view(weights.shape)
        return g_w, gw, None, None, None, None


class _EmbedCodesFunction(torch.autograd.Function):
    """MedTokEmbedding.forward with a frozen codebook under autograd: the lookup kernel (medtok_embed_codes_*), whose one
    differentiable input is the miss row.  Backward is the fixed-order sum of the upstream rows at the unpadded miss positions
    (medtok_embed_codes_miss_grad_f32: no float atomics, two runs give the same bits); a half-precision upstream gradient is summed in
    fp32."""

    @staticmethod
    def forward(ctx, miss, index, pad_mask, tokens, weights, what, regions, out_dtype, status):
        out = ops.embed_codes(index, tokens, weights, what, regions, miss=miss.detach(), pad_mask=pad_mask, out_dtype=out_dtype, status=status)
        ctx.save_for_backward(index, pad_mask)
        ctx.num_codes = tokens.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        index, pad_mask = ctx.saved_tensors
        g_miss = ops.embed_codes_miss_grad(g, index, ctx.num_codes, pad_mask) if ctx.needs_input_grad[0] else None
        return g_miss, None, None, None, None, None, None, None, None


class _EmbedCodesTrainFunction(torch.autograd.Function):
    """MedTokEmbedding.forward with a codebook that trains (freeze_codebook=False): the SAME lookup kernel as the frozen path, so the
    same rows in every out_dtype, with two differentiable inputs, the codebook weight and the miss row.  Backward, straight from the
    upstream gradient: ops.embed_codes_code_grad sums w * g per codebook row in a fixed order (medtok_embed_code_grad_f32: a sort of 8
    bytes per contribution and chunked fmaf chains; no [positions * S * k, d] buffer, no float atomics, nothing read back), then
    F.normalize's backward exactly as _DecodeFunction finishes (rows no live position selected: bins = 0, zeros), and
    ops.embed_codes_miss_grad for the miss row.  `what` is the normalised codebook the forward used: a quantizer in train() mode
    renormalises on every call.  A half-precision upstream gradient is summed in fp32.  Two runs give the same bits."""

    @staticmethod
    def forward(ctx, weight, miss, index, pad_mask, tokens, weights, what, regions, out_dtype, status):
        out = ops.embed_codes(index, tokens, weights, what, regions, miss=None if miss is None else miss.detach(), pad_mask=pad_mask,
                              out_dtype=out_dtype, status=status)
        ctx.save_for_backward(weight, index, pad_mask, tokens, weights, what)
        ctx.regions = regions
        ctx.miss_shape = None if miss is None else miss.shape
        return out

    @staticmethod
    def backward(ctx, g):
        weight, index, pad_mask, tokens, weights, what = ctx.saved_tensors
        gw = g_miss = None
        if g.dtype != torch.float32:
            g = g.float()                                          # (once, for both sums)
        if ctx.needs_input_grad[0]:
            g_what, bins = ops.embed_codes_code_grad(g, index, tokens, weights, what.shape, ctx.regions, pad_mask)
            gw = ops.normalize_backward(g_what, what, weight.detach(), live=bins)
        if ctx.miss_shape is not None and ctx.needs_input_grad[1]:
            g_miss = ops.embed_codes_miss_grad(g, index, tokens.shape[0], pad_mask).reshape(ctx.miss_shape)
        return (gw, g_miss) + (None,) * 8


class _EmbedPoolFunction(torch.autograd.Function):
    """MedTokEmbedding.pooled and .pooled_segments with a frozen codebook under autograd: the pooling kernels (medtok_embed_pool_f32, or
    medtok_embed_pool_segments_f32 where segment_id is given: a bag per (batch row, segment), out [B, V, width]), whose one
    differentiable input is the miss row (the table is a constant).  Every unpadded miss position of bag b adds n(miss) / live_b to
    pooled[b], so backward is G = sum_b (miss_b / live_b) g[b] in bag order (medtok_embed_pool_miss_grad_f32: fixed order, no float
    atomics, two runs give the same bits) and, with normalisation, G taken through n by ops.normalize_backward."""

    @staticmethod
    def forward(ctx, miss, index, pad_mask, tokens, weights, what, regions, normalize, status, segment_id=None, n_segments=0):
        if segment_id is None:
            out, counts = ops.embed_pool(index, tokens, weights, what, regions, miss=miss.detach(), pad_mask=pad_mask, normalize=normalize,
                                         status=status)
        else:
            out, counts = ops.embed_pool_segments(index, segment_id, n_segments, tokens, weights, what, regions, miss=miss.detach(),
                                                  pad_mask=pad_mask, normalize=normalize, status=status)
            ctx.mark_non_differentiable(counts)
        ctx.save_for_backward(miss, counts)
        ctx.normalize = bool(normalize)
        return out if segment_id is None else (out, counts)

    @staticmethod
    def backward(ctx, g, *_):
        miss, counts = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 11
        g_acc = ops.embed_pool_miss_grad(g.reshape(-1, g.shape[-1]), counts.reshape(-1, 2))
        if ctx.normalize:
            v = miss.detach().reshape(1, -1).contiguous()
            g_acc = ops.normalize_backward(g_acc.view(1, -1), torch.nn.functional.normalize(v, dim=-1), v)
        return (g_acc.reshape(miss.shape),) + (None,) * 10


class _SegmentSumFunction(torch.autograd.Function):
    """sums[b, v] = the sum of rows[b, p] over the unpadded p with segment_id[b, p] == v, rows fp32 [B, L, W] -> [B, V, W]: the composed
    route of MedTokEmbedding.pooled_segments (a training codebook).  Forward is the fixed-order ops.embed_sequence_segment_grad (no float
    atomics, V <= ops.EMBED_SEQ_MAX_SEGMENTS); backward is the masked gather g[b, segment_id[b, p]] (zeros at padded positions and at ids
    outside [0, V))."""

    @staticmethod
    def forward(ctx, rows, segment_id, n_segments, pad_mask):
        ctx.save_for_backward(segment_id, pad_mask)
        ctx.n_segments = int(n_segments)
        return ops.embed_sequence_segment_grad(rows.detach(), segment_id, n_segments, pad_mask)

    @staticmethod
    def backward(ctx, g):
        segment_id, pad_mask = ctx.saved_tensors
        on = (segment_id >= 0) & (segment_id < ctx.n_segments)
        if pad_mask is not None:
            on = on & (pad_mask == 0)
        at = torch.where(on, segment_id, torch.zeros_like(segment_id))
        rows = torch.gather(g, 1, at.unsqueeze(-1).expand(-1, -1, g.shape[-1]))
        return rows * on.unsqueeze(-1).to(rows.dtype), None, None, None


class _SmallLinearFunction(torch.autograd.Function):
    """y = x W^T + b under autograd on the library's exact fp32 product (ops.small_gemm: one fmaf chain per entry, any shape): what
    MedTokEmbedding puts behind the lookup where the projector is not folded into the tables.  dX = dY W, dW = dY^T X, db = the column
    sum of dY; fp32 in and out; no float atomics anywhere (two runs give the same bits)."""

    @staticmethod
    def forward(ctx, x, w, b):
        xf, wf = x.detach().float().contiguous(), w.detach().float().contiguous()
        ctx.save_for_backward(xf, wf)
        ctx.has_bias = b is not None
        if xf.shape[0] == 0:
            return xf.new_zeros(0, wf.shape[0])
        y = ops.small_gemm(xf, wf, trans_b=True)
        return y if b is None else y.add_(b.detach().float())

    @staticmethod
    def backward(ctx, dy):
        xf, wf = ctx.saved_tensors
        dyf = dy.float().contiguous()
        if xf.shape[0] == 0:
            return (torch.zeros_like(xf) if ctx.needs_input_grad[0] else None, torch.zeros_like(wf) if ctx.needs_input_grad[1] else None,
                    wf.new_zeros(wf.shape[0]) if ctx.has_bias and ctx.needs_input_grad[2] else None)
        dx = ops.small_gemm(dyf, wf) if ctx.needs_input_grad[0] else None
        dw = ops.small_gemm(dyf, xf, trans_a=True) if ctx.needs_input_grad[1] else None
        db = dyf.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db


def small_linear(x, w, b=None):
    return _SmallLinearFunction.apply(x, w, b)


EMBED_PROJECT_GRAD_CHUNK = 16384          # positions per recomputed block of embeddings in _EmbedProjectFunction.backward


class _EmbedProjectFunction(torch.autograd.Function):
    """projector(MedTokEmbedding lookup) under autograd.  Forward: embed_folded_kernel over the folded tables (`folded` =
    ops.fold_projector's result, built from detached tensors: constants of this node), the same bits in either gradient form.
    `weight`: the codebook weight (padded to the normalised codebook's width) where it trains, which only the scatter form can serve,
    else None.  `scatter` (not a tensor) chooses the backward, both deterministic and without float atomics:
      dense (MedTokEmbedding's default), from g [n, Hp] converted to fp32 (the padding columns dropped), _embed_project_grads:
        dW        blocks of EMBED_PROJECT_GRAD_CHUNK positions in order: emb = embed_codes(...) fp32 recomputed (the only temporary:
                  chunk x S * d floats), dW += g_block^T . emb by the exact fp32 product;
        db        the column sum of g (padded positions are the bias row: they count);
        d miss    (sum of g over the unpadded miss positions, embed_codes_miss_grad at width H) . W.
      scatter (grad_form="scatter"), _embed_project_scatter_grads: dW as G_s^T . what_s over the folded tables' rows, and the codebook's
        gradient; a 16-bit upstream gradient goes to the sums as it is."""

    @staticmethod
    def forward(ctx, w, b, miss, weight, index, pad_mask, tokens, weights, what, regions, e_dim, folded, out_dtype, status, scatter):
        table, row_regions, bias, miss_row = folded
        out = ops.embed_project(index, tokens, weights, table, row_regions, bias, miss_row=miss_row, pad_mask=pad_mask, out_dtype=out_dtype,
                                status=status)
        ctx.save_for_backward(w, miss, weight, index, pad_mask, tokens, weights, what)
        ctx.cfg = (tuple(regions), tuple(row_regions), int(e_dim), b is not None, bool(scatter))
        return out

    @staticmethod
    def backward(ctx, g):
        w, miss, weight, index, pad_mask, tokens, weights, what = ctx.saved_tensors
        regions, row_regions, e, has_bias, scatter = ctx.cfg
        needs = ctx.needs_input_grad
        if scatter:
            grads = _embed_project_scatter_grads(g, w, miss, index, pad_mask, tokens, weights, what, regions, row_regions, e, has_bias, needs[:4],
                                                 weight)
        else:
            grads = _embed_project_grads(g, w, miss, index, pad_mask, tokens, weights, what, regions, e, has_bias, needs[:3]) + (None,)
        return grads + (None,) * 11


def _embed_project_grads(g, w, miss, index, pad_mask, tokens, weights, what, regions, e, has_bias, needs):
    """(dW, db, d miss) of the folded lookup in the DENSE form, from the upstream gradient g [n, >= H] of its rows: the arithmetic
    _EmbedProjectFunction documents, shared with _EmbedSequenceFunction (which feeds it g[:, P:])"""
    h, s, d = w.shape[0], len(regions), what.shape[1]
    n = index.numel()
    g = g.reshape(n, g.shape[-1])[:, :h].float().contiguous()          # (not -1: n may be 0)
    index = index.reshape(-1)
    pad_mask = None if pad_mask is None else pad_mask.reshape(-1)
    wf = w.detach().float().contiguous()
    dw = db = dmiss = None
    if needs[0]:
        miss_d = None
        if miss is not None:
            miss_d = miss.detach().reshape(s, e)
            miss_d = (torch.nn.functional.pad(miss_d, (0, d - e)) if d != e else miss_d).reshape(-1).contiguous()
        dw = torch.zeros_like(wf)
        for r0 in range(0, n, EMBED_PROJECT_GRAD_CHUNK):
            r1 = min(n, r0 + EMBED_PROJECT_GRAD_CHUNK)
            emb = ops.embed_codes(index[r0:r1], tokens, weights, what, regions, miss=miss_d,
                                  pad_mask=None if pad_mask is None else pad_mask[r0:r1])
            if d != e:
                emb = emb.view(r1 - r0, s, d)[:, :, :e].reshape(r1 - r0, s * e)
            dw.add_(ops.small_gemm(g[r0:r1], emb, trans_a=True))
    if has_bias and needs[1]:
        db = g.sum(0)
    if miss is not None and needs[2]:
        g_rows = ops.embed_codes_miss_grad(g, index, tokens.shape[0], pad_mask) if n else g.new_zeros(h)
        dmiss = ops.small_gemm(g_rows.view(1, h), wf).reshape(miss.shape)
    return dw, db, dmiss


def _embed_project_scatter_grads(g, w, miss, index, pad_mask, tokens, weights, what, regions, row_regions, e, has_bias, needs, weight=None):
    """(dW, db, d miss, d codebook weight) of the folded lookup in the SCATTER form, from the upstream gradient g [n, Hp] (fp32, fp16 or
    bf16) of its rows; needs: which of the four are wanted.  No [n, S * e] tensor exists: ops.embed_project_table_grad sums g per row of
    the folded table in a fixed order, (G [rows, Hp], bins), and then, exact fp32 products (ops.small_gemm) throughout,
      dW        dW[:, s * e : (s + 1) * e] = G_s^T . what[lo_s : lo_s + size_s, :e] per slot (2 * sum of sizes * e * H flops instead of
                2 * n * S * e * H), plus the miss positions' outer product (sum of g over them) x miss_emb, which the dense form gets from
                its recomputed rows;
      db, d miss  as _embed_project_grads;
      d weight  g_what = zeros; slots ascending: g_what[lo_s : lo_s + size_s] += G_s . W[:, s * e : (s + 1) * e] (zero columns appended
                where the codebook is padded; two slots over one region add in slot order); live[r] = the bins of the slots that map to
                codebook row r, summed; then F.normalize's backward, ops.normalize_backward(g_what, what, weight, live=live), as
                _EmbedCodesTrainFunction finishes: rows no live contribution reaches are exactly zero.
    Deterministic and without float atomics: two runs give the same bits."""
    h, s, d = w.shape[0], len(regions), what.shape[1]
    n = index.numel()
    hp = ops.pad_dim(h)
    g = g.reshape(n, hp)                                               # (the folded forward's rows are Hp wide; not -1: n may be 0)
    index = index.reshape(-1)
    pad_mask = None if pad_mask is None else pad_mask.reshape(-1)
    wf = w.detach().float().contiguous()
    dw = db = dmiss = dweight = None
    want_w, want_b, want_miss, want_code = needs[0], has_bias and needs[1], miss is not None and needs[2], weight is not None and needs[3]
    gf = g[:, :h].float().contiguous() if want_b or ((want_w or want_miss) and miss is not None) else None
    g_rows = None
    if gf is not None and miss is not None and (want_w or want_miss):
        g_rows = ops.embed_codes_miss_grad(gf, index, tokens.shape[0], pad_mask) if n else gf.new_zeros(h)
    if want_w or want_code:
        G, bins = ops.embed_project_table_grad(g, index, tokens, weights, row_regions, pad_mask)
    if want_w:
        dw = torch.empty_like(wf)
        for i, ((lo, size), (at, _)) in enumerate(zip(regions, row_regions)):
            dw[:, i * e:(i + 1) * e] = ops.small_gemm(G[at:at + size], what[lo:lo + size, :e], trans_a=True)[:h]
        if g_rows is not None:
            dw.add_(ops.small_gemm(g_rows.view(h, 1), miss.detach().float().reshape(1, s * e)))
    if want_b:
        db = gf.sum(0)
    if want_miss:
        dmiss = ops.small_gemm(g_rows.view(1, h), wf).reshape(miss.shape)
    if want_code:
        wp = torch.nn.functional.pad(wf, (0, 0, 0, hp - h)) if hp != h else wf         # [Hp, S * e]: zero rows for the added columns
        g_what = torch.zeros_like(what)
        live = torch.zeros(what.shape[0], dtype=torch.float32, device=what.device)
        for i, ((lo, size), (at, _)) in enumerate(zip(regions, row_regions)):
            ws = wp[:, i * e:(i + 1) * e]
            ws = torch.nn.functional.pad(ws, (0, d - e)) if d != e else ws.contiguous()
            g_what[lo:lo + size].add_(ops.small_gemm(G[at:at + size], ws))
            live[lo:lo + size].add_(bins[at:at + size])
        dweight = ops.normalize_backward(g_what, what, weight.detach().float().contiguous(), live=live)
    return dw, db, dmiss, dweight


def _sequence_part_grads(g, needs, n_rows, segment_id, n_segments, pad_mask, n_prefix):
    """(d position_rows, d segment_rows[0], d segment_rows[1], d prefix) from g fp32 [B, P + L, W]; needs: which of the four are wanted"""
    dpos = dseg = dprefix = None
    if needs[0]:
        dpos = ops.embed_sequence_position_grad(g, n_rows, pad_mask, n_prefix)
    if needs[1] or needs[2]:
        dseg = ops.embed_sequence_segment_grad(g, segment_id, n_segments, pad_mask, n_prefix)
    if needs[3]:
        dprefix = g[:, :n_prefix].contiguous()
    return dpos, dseg if needs[1] else None, dseg if needs[2] else None, dprefix


class _EmbedSequenceFunction(torch.autograd.Function):
    """MedTokEmbedding.sequence over the folded tables under autograd: one launch forward (ops.embed_sequence).  `weight` and `scatter`
    as in _EmbedProjectFunction.  Backward from g [B, P + L, Hp], deterministic and without float atomics:
      d prefix                g[:, :P]
      d position_rows         ops.embed_sequence_position_grad (b ascending)
      d segment_rows[0], [1]  ops.embed_sequence_segment_grad, the same tensor for both terms (chunks of 256 positions, then chunk order)
                              -- these three from g converted to fp32 (exact), the padding columns dropped;
      dW, db, d miss          dense: _embed_project_grads on a contiguous copy of that fp32 g[:, P:] (padded positions are the bias row:
                              they count in db, as there); scatter: with the codebook's gradient, _embed_project_scatter_grads on a
                              contiguous copy of g[:, P:] in g's own dtype."""

    @staticmethod
    def forward(ctx, w, b, miss, weight, position_rows, seg0, seg1, prefix, index, pad_mask, segment_id, tokens, weights, what, regions, e_dim,
                folded, out_dtype, status, scatter):
        table, row_regions, bias, miss_row = folded
        terms = tuple(t for t in (seg0, seg1) if t is not None)
        out = ops.embed_sequence(index, tokens, weights, table, row_regions, bias, miss_row=miss_row, pad_mask=pad_mask,
                                 position_rows=position_rows, segment_id=segment_id, segment_rows=terms or None, prefix=prefix, width=w.shape[0],
                                 out_dtype=out_dtype, status=status)
        ctx.save_for_backward(w, miss, weight, index, pad_mask, segment_id, tokens, weights, what)
        ctx.cfg = (tuple(regions), tuple(row_regions), int(e_dim), b is not None, bool(scatter),
                   None if position_rows is None else position_rows.shape[0], 0 if seg0 is None else seg0.shape[1],
                   0 if prefix is None else prefix.shape[1])
        return out

    @staticmethod
    def backward(ctx, g):
        w, miss, weight, index, pad_mask, segment_id, tokens, weights, what = ctx.saved_tensors
        regions, row_regions, e, has_bias, scatter, n_rows, n_segments, n_prefix = ctx.cfg
        needs = ctx.needs_input_grad
        gf = g[:, :, :w.shape[0]].float().contiguous() if not scatter or any(needs[4:8]) else None
        grads = (None, None, None, None)
        if scatter and any(needs[:4]):
            grads = _embed_project_scatter_grads(g[:, n_prefix:].contiguous(), w, miss, index, pad_mask, tokens, weights, what, regions,
                                                 row_regions, e, has_bias, needs[:4], weight)
        elif not scatter and any(needs[:3]):
            grads = _embed_project_grads(gf[:, n_prefix:].contiguous(), w, miss, index, pad_mask, tokens, weights, what, regions, e, has_bias,
                                         needs[:3]) + (None,)
        parts = (None, None, None, None)
        if any(needs[4:8]):
            parts = _sequence_part_grads(gf, needs[4:8], n_rows, segment_id, n_segments, pad_mask, n_prefix)
        return grads + parts + (None,) * 12


class _EmbedSequenceRowsFunction(torch.autograd.Function):
    """MedTokEmbedding.sequence over dense rows under autograd (ops.embed_sequence_rows): the lookup's fp32 rows [B, L, W] are an input,
    so d rows = g[:, P:] flows on into the nodes that made them (the codebook's and the miss row's gradients, the unfolded projector's).
    The additive parts' gradients are _EmbedSequenceFunction's."""

    @staticmethod
    def forward(ctx, rows, position_rows, seg0, seg1, prefix, pad_mask, segment_id, out_dtype, status):
        terms = tuple(t for t in (seg0, seg1) if t is not None)
        out = ops.embed_sequence_rows(rows, pad_mask=pad_mask, position_rows=position_rows, segment_id=segment_id, segment_rows=terms or None,
                                      prefix=prefix, out_dtype=out_dtype, status=status)
        ctx.save_for_backward(pad_mask, segment_id)
        ctx.cfg = (None if position_rows is None else position_rows.shape[0], 0 if seg0 is None else seg0.shape[1],
                   0 if prefix is None else prefix.shape[1])
        return out

    @staticmethod
    def backward(ctx, g):
        pad_mask, segment_id = ctx.saved_tensors
        n_rows, n_segments, n_prefix = ctx.cfg
        g = g.float().contiguous()
        needs = ctx.needs_input_grad
        drows = g[:, n_prefix:].contiguous() if needs[0] else None
        return (drows,) + _sequence_part_grads(g, needs[1:5], n_rows, segment_id, n_segments, pad_mask, n_prefix) + (None,) * 4


def _lib_multi_max():
    return ops._lib.MULTI_SEARCH_MAX


class _SoftVQMultiFunction(torch.autograd.Function):
    """All searches of a training forward under ONE autograd node: (zq_ste, vq, commit, xhat, idx, w) per search from its rows and its
    region of the codebook -- the per-search forward of _SoftVQFunction, search by search.  What changes is the BACKWARD of the codebook:
    the per-(row, slot) code gradients of all searches are summed per code in ONE segmented sum over global code ids and taken through
    F.normalize once, so the weight receives ONE dense gradient.  (Six _SoftVQFunction nodes on six slices of the weight hand autograd
    six dense [n_e, D] gradients -- a zero fill and a copy each for the slices -- that it then adds up: 1.9 ms of fills and adds per
    step at n_e = 49152, D = 768.)"""

    @staticmethod
    def forward(ctx, weight, what, wsq, topk, path, beta, regions, *xs):
        ctx.set_materialize_grads(False)
        outs, saved, nondiff = [], [], []
        # a per-GPU batch of searches (at most 4096 rows each, the exact path): ONE call of three launches for all of them
        # (ops.soft_vq_forward_multi: the per-search bits) instead of five launches per search
        batched = None
        if (TRAIN_BATCHED_SEARCHES and path in (ops.PATH_AUTO, ops.PATH_F32_MFMA) and 1 <= len(xs) <= _lib_multi_max() and topk <= 8
                and all(x.is_cuda and x.shape[0] > 0 and ops.multi_search_eligible(x.shape[0], hi - lo, x.shape[1], topk) for x, (lo, hi) in zip(xs, regions))):
            batched = ops.soft_vq_forward_multi([dict(x=x.detach().float(), what=what[lo:hi], wsq=wsq[lo:hi].contiguous()) for x, (lo, hi) in zip(xs, regions)],
                                                topk, want_sqerr=True)
        # the searches of ONE region (both shared ones; a modality's two views) as one call on their rows stacked: the region's codes are
        # streamed once for both and five launches serve two searches (any row count gives every row the same bits: the library's plans
        # only cut the code axis, and the per-split lists are joined in the (distance, index) total order)
        stacked = {}
        if batched is None and TRAIN_STACK_SEARCHES_OF_A_REGION and all(x.is_cuda and x.dim() == 2 for x in xs):
            by_region = {}
            for i, reg in enumerate(regions):
                by_region.setdefault((tuple(reg), xs[i].shape[1], xs[i].dtype), []).append(i)
            for (reg, _, _), members in by_region.items():
                if len(members) > 1 and all(xs[i].shape[0] > 0 for i in members):
                    lo, hi = reg
                    r = ops.soft_vq_forward(torch.cat([xs[i].detach() for i in members]), what[lo:hi], wsq[lo:hi].contiguous(), topk, path, want_sqerr=True)
                    a = 0
                    for i in members:
                        b = a + xs[i].shape[0]
                        stacked[i] = {k: (v[a:b] if torch.is_tensor(v) else v) for k, v in r.items()}
                        a = b
        for i, (x, (lo, hi)) in enumerate(zip(xs, regions)):
            r = (batched[i] if batched is not None else stacked[i] if i in stacked else
                 ops.soft_vq_forward(x.detach(), what[lo:hi], wsq[lo:hi].contiguous(), topk, path, want_sqerr=True))
            n, d = x.shape
            outs += [r["zq"], ops.sum_scale(r["row_sqerr"], (1.0 / (n * d)) if n else float("nan")), ops.sum_scale(r["row_sqerr"], beta / (n * d) if n else float("nan")),
                     r["xhat"], r["idx"], r["w"]]
            saved += [x, r["xhat"], r["idx"], r["w"]]
            nondiff += [r["idx"], r["w"]]
        ctx.save_for_backward(weight, what, *saved)
        ctx.regions, ctx.beta, ctx.m = tuple(regions), beta, len(xs)
        ctx.mark_non_differentiable(*nondiff)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        weight, what, *saved = ctx.saved_tensors
        want_w = ctx.needs_input_grad[0]
        as_f32 = lambda t: None if t is None else t.float()
        gxs, g_codes, ids = [], [], []
        for i in range(ctx.m):
            x, xhat, idx, w = saved[4 * i: 4 * i + 4]
            lo, hi = ctx.regions[i]
            g_zq, g_vq, g_commit, g_xhat = grads[6 * i: 6 * i + 4]
            n, d = x.shape
            gx, g_code = ops.soft_vq_backward(x.detach(), xhat, what[lo:hi], idx, w, g_xhat=as_f32(g_xhat), g_out=as_f32(g_zq), g_vq=as_f32(g_vq),
                                              g_commit=as_f32(g_commit), vq_scale=2.0 / (n * d), commit_scale=2.0 * ctx.beta / (n * d),
                                              want_gx=ctx.needs_input_grad[7 + i], want_g_code=want_w)
            gxs.append(gx)
            if want_w and n:
                g_codes.append(g_code)
                ids.append(idx.reshape(-1) + lo if lo else idx.reshape(-1))
        gw = None
        if want_w:
            if g_codes:
                bins, g_what = ops.ema_stats(torch.cat(g_codes), torch.cat(ids), what.shape[0])
                # (codes no row selected: bins = 0, their gradient rows are zeros -- written without reading the codebook)
                gw = ops.normalize_backward(g_what, what, weight.detach(), live=bins)
            else:
                gw = torch.zeros_like(weight)
        return (gw, None, None, None, None, None, None, *gxs)
