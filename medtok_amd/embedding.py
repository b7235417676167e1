"""MedTokEmbedding: what a downstream model does with embeddings_all.npy, without the table.

The reference's consumers load the [num_codes, 4 * e_dim] table onto the device, append a learned "missing code" row and index the
result with a [B, max_medical_code] batch of code indices (MedTok_EHR_Tutorial/EHRModel_token.py:128-141,214-215; padding and
code_mask in dataloader.py:79-88):

    self.emb          = torch.from_numpy(np.load(pre_trained_embedding)).cuda()
    self.miss_emb     = torch.nn.Parameter(torch.randn(1, 256)).cuda()
    self.med_code_emb = torch.concat([self.emb, self.miss_emb], dim=0)
    src_emb           = self.med_code_emb[data.x].squeeze()

This module answers the same index tensor from tokens_all.npy / weights_all.npy (12 k bytes per code and slot instead of 4 e_dim)
and a VectorQuantizer's codebook: one kernel goes from the indices through the stored ids and weights to the embedding
(ops.embed_codes, medtok_amd/csrc/embed_kernels.h).  The one semantic difference: a position under the padding mask is a row of
zeros, not code 0's embedding (the reference masks those positions in its attention anyway).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .autograd import (_EmbedCodesFunction, _EmbedCodesTrainFunction, _EmbedPoolFunction, _EmbedProjectFunction,
                       _EmbedSequenceFunction, _EmbedSequenceRowsFunction, _SegmentSumFunction, small_linear)

DEFAULT_TYPES = ("text", "graph", "shared", "shared")


def _autocast_dtype():
    """the dtype an active device autocast asks for, or None"""
    if hasattr(torch, "get_autocast_dtype"):
        return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    return torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else None


class MedTokEmbedding(nn.Module):
    """`med_code_emb[index]` over the table `quantizer.decode(tokens, weights)` would build, plus a learned miss row.

    quantizer: a VectorQuantizer; it is REFERENCED (its codebook is read on every call), not copied and not a submodule: it is
    neither in this module's state dict nor moved by .to().  tokens int64 / weights fp32 [num_codes, S, k], numpy or tensor, slot s
    searched over the region types[s]: persistent buffers (they travel in the state dict and with .to(); they start on the
    codebook's device).  Ids are region-local as every forward returns them; global_ids=True takes rows of codebook.weight and
    subtracts the region offsets once, here.  miss_row: keep `miss_emb`, an nn.Parameter [1, S * e_dim] initialised randn as the
    reference's, served at index num_codes (`miss_index`); without it that index is an error.  freeze_codebook=True (the
    reference's table is a constant): the only gradient is miss_emb's; False: the table follows the codebook and codebook.weight gets
    its gradient too, where it requires one: the same lookup kernel forward, and backward the per-row sums of the upstream gradient in
    a fixed order (ops.embed_codes_code_grad: no row-per-contribution buffer, no float atomics, no host read -- with validate=False a
    fine-tuning step can be captured in a HIP graph like every frozen path).

    projector: the nn.Linear(S * e_dim, H) every consumer of the reference puts behind the lookup (`projector(med_code_emb[data.x])`,
    EHRModel_token.py:143,215-217); it becomes a submodule (its parameters train and travel with this module) and forward returns
    projector(embedding) [..., H].  The lookup is linear in the codebook rows, so the projector can be applied to the codebook once
    per weight version instead of to every position (ops.fold_projector / ops.embed_project: the [positions, S * e_dim] activation
    never exists).  fold=True / False forces that path / the lookup followed by the dense product; fold=None folds when the
    projector narrows (H < S * e_dim), the tables fit FOLD_MAX_BYTES and either the cached tables are valid or positions * S >= 3 x the
    tables' rows (fold_rule, where the measurements behind it are given).  The folded tables are
    cached per (normalised codebook entry, version and storage of projector.weight, projector.bias and miss_emb); `fold_builds`
    counts how often they were built.  The quantizer caches its normalised codebook in eval mode only: while it is in train() mode
    (e.g. as a submodule of a model that was sent .train()) every call normalises afresh, so the key changes and the tables are
    refolded on every call, and fold=None never sees a valid cache; keep a frozen quantizer in eval().  Without a projector nothing
    here changes.

    grad_form: how a call that takes the folded route is differentiated.  "dense" (the default) recomputes the embeddings in blocks and
    multiplies them with the upstream gradient (autograd._embed_project_grads), and a codebook that trains (freeze_codebook=False)
    switches the fold off.  "scatter" sums the upstream rows per row of the folded tables in a fixed order
    (ops.embed_project_table_grad: a sort of 8 bytes per contribution, no float atomics, nothing read back) and takes dW = G_s^T . what_s
    and the codebook's gradient G_s . W_s from those sums: no [positions, S * e_dim] tensor exists in either direction, and
    freeze_codebook=False no longer forces fold=False (fold=True folds, fold=None applies fold_rule; the tables are refolded per
    weight version as said above, i.e. once per optimiser step with the quantizer in eval()).  The forward is the same kernel over the
    same tables in both forms, hence the same bits; where the folded route is not taken (fold_rule says no, fold=False, or a training
    codebook with e_dim % 4 != 0) nothing changes, and `pooled` is untouched.  The default stays "dense" until the measurement of
    DESIGN.md section 7.1h is in; flipping it is a separate change."""

    # The memory budget of the folded tables (sum of the slots' region sizes x H rounded up to 4 x 4 bytes; 134 MB for a 256-wide
    # projector over cfg 3's 49,152 codes): above it fold=None takes the lookup followed by the dense product.  Chosen by size alone:
    # no table near it has been timed.
    FOLD_MAX_BYTES = 1 << 30
    # fold=None builds the tables for a call only from positions * S >= FOLD_COLD_FACTOR * rows (measured, section 7.1d: see fold_rule)
    FOLD_COLD_FACTOR = 3

    def __init__(self, quantizer, tokens, weights, types=DEFAULT_TYPES, miss_row: bool = True, freeze_codebook: bool = True,
                 global_ids: bool = False, projector=None, fold=None, grad_form: str = "dense"):
        super().__init__()
        kinds = (types,) if isinstance(types, str) else tuple(types)
        if not 1 <= len(kinds) <= ops.DECODE_MAX_SLOTS or any(t not in quantizer.DECODE_TYPES for t in kinds):
            raise ValueError(f"MedTokEmbedding: types must name 1 .. {ops.DECODE_MAX_SLOTS} of {quantizer.DECODE_TYPES}, got {types!r}")
        dev = quantizer.codebook.weight.device
        tokens = torch.as_tensor(np.ascontiguousarray(tokens) if isinstance(tokens, np.ndarray) else tokens)
        weights = torch.as_tensor(np.ascontiguousarray(weights) if isinstance(weights, np.ndarray) else weights)
        if tokens.dtype != torch.int64 or weights.dtype != torch.float32:
            raise ValueError(f"MedTokEmbedding: expected int64 tokens and fp32 weights, got {tokens.dtype} and {weights.dtype}")
        if tokens.dim() != 3 or tokens.shape != weights.shape or tokens.shape[1] != len(kinds) or tokens.shape[0] < 1:
            raise ValueError(f"MedTokEmbedding: tokens and weights must both be [num_codes, {len(kinds)}, k] for types={types!r}; got "
                             f"{tuple(tokens.shape)} and {tuple(weights.shape)}")
        if not 1 <= tokens.shape[2] <= ops.MAX_TOPK:
            raise ValueError(f"MedTokEmbedding: k={tokens.shape[2]} ids per slot unsupported (1 .. {ops.MAX_TOPK})")
        self.__dict__["quantizer"] = quantizer            # (a plain attribute: nn.Module would register it as a submodule)
        self.types = kinds
        self.freeze_codebook = bool(freeze_codebook)
        tokens = tokens.detach().to(dev, copy=True).contiguous()      # (copies: load_state_dict writes into the buffers in place)
        if global_ids:
            tokens -= torch.tensor([quantizer._region(t)[0] for t in kinds], dtype=torch.int64, device=dev).view(1, -1, 1)
        self.register_buffer("tokens", tokens)
        self.register_buffer("weights", weights.detach().to(dev, copy=True).contiguous())
        self.num_codes = int(tokens.shape[0])
        self.embedding_dim = len(kinds) * int(quantizer.e_dim)
        self.miss_index = self.num_codes if miss_row else None
        self.num_embeddings = self.num_codes + (1 if miss_row else 0)
        if miss_row:
            self.miss_emb = nn.Parameter(torch.randn(1, self.embedding_dim, device=dev))
        else:
            self.register_parameter("miss_emb", None)
        if fold is not None and not isinstance(fold, bool):
            raise ValueError(f"MedTokEmbedding: fold must be None, True or False, got {fold!r}")
        if fold is not None and projector is None:
            raise ValueError(f"MedTokEmbedding: fold={fold!r} without a projector: there is nothing to fold")
        if grad_form not in ("dense", "scatter"):
            raise ValueError(f"MedTokEmbedding: grad_form must be 'dense' or 'scatter', got {grad_form!r}")
        if grad_form == "scatter" and projector is None:
            raise ValueError("MedTokEmbedding: grad_form='scatter' without a projector: only the folded route has a scatter form")
        self.grad_form = grad_form
        if projector is not None:
            if not isinstance(projector, nn.Linear) or projector.in_features != self.embedding_dim:
                raise ValueError(f"MedTokEmbedding: projector must be an nn.Linear with in_features = S * e_dim = {self.embedding_dim}, got "
                                 f"{projector!r}")
            if projector.weight.dtype != torch.float32:
                raise ValueError(f"MedTokEmbedding: the projector must be fp32 (every product behind the lookup is), got {projector.weight.dtype}")
            self.projector = projector
            self.fold = fold
            self.fold_builds = 0
            self.__dict__["_fold_cache"] = None           # (key, the normalised-codebook entry it was built from, folded tensors)

    @classmethod
    def from_dir(cls, path, quantizer, **kw):
        """From the arrays run_inference wrote; reads tokens_all.npy and weights_all.npy only (never embeddings_all.npy)."""
        p = Path(path)
        return cls(quantizer, np.load(p / "tokens_all.npy"), np.load(p / "weights_all.npy"), **kw)

    def extra_repr(self):
        return (f"num_embeddings={self.num_embeddings}, embedding_dim={self.embedding_dim}, k={self.tokens.shape[2]}, types={self.types}, "
                f"freeze_codebook={self.freeze_codebook}")

    def _regions(self):
        return [(lo, hi - lo) for lo, hi in (self.quantizer._region(t) for t in self.types)]

    def forward(self, index, padding_mask=None, validate: bool = True, out_dtype=None, out=None):
        """index int64 [...] -> [..., S * e_dim].  padding_mask: bool / uint8 of index's shape, True = padded (the sense of the
        reference's code_mask): those rows are zeros whatever the index holds.  Without a mask and in fp32 the result is what
        `med_code_emb[index]` gives over the decoded table.

        validate=True reads ONE status word back and raises ValueError naming the "code index" (an unmasked index outside
        [0, num_embeddings)) or the first slot of the table that holds a token id outside its region; validate=False reads nothing
        (such rows are zeros), so the call can be captured in a HIP graph.  out_dtype: torch.float32 / float16 / bfloat16; None =
        fp32, or the autocast dtype where autocast is active.  `out`: a [index.numel(), S * e_dim] device view of that dtype to fill
        (e.g. a column block of a wider tensor); such a call is not differentiable.

        With a projector the result is projector(embedding) [..., H] (`out`: [index.numel(), H]); padded positions and, with
        validate=False, positions with a bad index are then the projector's bias row (the projector applied to a row of zeros)."""
        if getattr(self, "projector", None) is not None:
            return self._forward_projected(index, padding_mask, validate, out_dtype, out)
        return self._lookup(index, padding_mask, validate, out_dtype, out)

    def _checked(self, index, padding_mask, out_dtype, out, width):
        """the argument checks of both forwards -> (padding_mask, out_dtype); `out`, if given, must be [index.numel(), width]"""
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
            raise ValueError(f"MedTokEmbedding: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
        if out_dtype is None:
            out_dtype = (out.dtype if out is not None else None) or _autocast_dtype() or torch.float32
        if out_dtype not in ops.EMBED_OUT_DTYPES:
            raise ValueError(f"MedTokEmbedding: out_dtype must be one of {ops.EMBED_OUT_DTYPES}, got {out_dtype!r}")
        padding_mask = ops._embed_mask("MedTokEmbedding", padding_mask, index)
        n = index.numel()
        if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == out_dtype and tuple(out.shape) == (n, width)):
            raise ValueError(f"MedTokEmbedding: out must be a {out_dtype} [{n}, {width}] tensor")
        return padding_mask, out_dtype

    def _lookup(self, index, padding_mask, validate, out_dtype, out):
        """forward without a projector"""
        q = self.quantizer
        s, e, pad = len(self.types), int(q.e_dim), getattr(q, "_pad", 0)
        padding_mask, out_dtype = self._checked(index, padding_mask, out_dtype, out, s * e)
        n = index.numel()
        grad_on = out is None and torch.is_grad_enabled()
        want_codebook = grad_on and not self.freeze_codebook and q.codebook.weight.requires_grad
        regions = self._regions()
        what = q._normalised_codebook()[0]
        miss = self.miss_emb
        want_miss = grad_on and miss is not None and miss.requires_grad
        if miss is not None:
            if not want_miss:
                miss = miss.detach()
            miss = (torch.nn.functional.pad(miss.view(s, e), (0, pad)) if pad else miss).reshape(-1)
        status = torch.zeros(1, dtype=torch.int32, device=self.tokens.device) if validate else None
        if want_codebook:
            # the same kernel and rows; the codebook's gradient comes straight from the upstream gradient (ops.embed_codes_code_grad).  The
            # columns appended for e_dim % 4 != 0 are handled as VectorQuantizer.decode does: padded here, under autograd
            wt = q.codebook.weight
            wp = torch.nn.functional.pad(wt.float(), (0, pad)) if pad else wt.float()
            res = _EmbedCodesTrainFunction.apply(wp, miss, index, padding_mask, self.tokens, self.weights, what, tuple(regions), out_dtype, status)
        elif want_miss:
            res = _EmbedCodesFunction.apply(miss, index, padding_mask, self.tokens, self.weights, what, tuple(regions), out_dtype, status)
        else:
            res = ops.embed_codes(index, self.tokens, self.weights, what, regions, miss=miss, pad_mask=padding_mask,
                                  out=None if pad else out, out_dtype=out_dtype, status=status)
        if pad:
            res = res.reshape(n, s, e + pad)[:, :, :e].reshape(n, s * e)
            if out is not None:
                out.copy_(res)
        if validate:
            self._raise_on(int(status.item()), regions)
        return out if out is not None else res.reshape(*index.shape, s * e)

    def _raise_on(self, word, regions):
        if not word:
            return
        if word >> ops.EMBED_BAD_INDEX_BIT & 1:
            raise ValueError(f"MedTokEmbedding: a code index outside [0, {self.num_embeddings}) at a position the padding mask does not cover"
                             + ("" if self.miss_index is not None else f" (no miss row: {self.num_codes} is not an index)"))
        bad = (word & -word).bit_length() - 1
        raise ValueError(f"MedTokEmbedding: slot {bad} ({self.types[bad]!r}) of the token table holds an id outside [0, {regions[bad][1]}); "
                         f"slots with bad ids: {[i for i in range(len(regions)) if word >> i & 1]}")

    # ------------------------------------------------------------------ the consumer's input sequence
    def sequence(self, index, padding_mask=None, *, position_rows=None, segment_id=None, segment_rows=None, prefix=None, validate: bool = True,
                 out_dtype=None):
        """index int64 [B, L] -> (seq [B, P + L, W], key_padding_mask bool [B, P + L]): the input sequence the reference's EHR model
        assembles from `forward`'s rows before its first transformer layer (EHRModel_token.py:220-232, PositionalEncoding.forward
        :65-78), in the lookup's launch.  W is what `forward` returns per position (H with a projector, S * e_dim without).

        position_rows fp32 [>= L, W]: the consumer's pe[:L], or a learned table.  segment_id int64 [B, L] (the consumer's
        visit_id[:, :, 0]) with segment_rows, one fp32 [B, V, W] tensor or a sequence of at most ops.EMBED_SEQ_MAX_TERMS of them: the time
        embeddings computed per VISIT (embedding the gathered timestamps equals gathering the embedded timestamps, value for value, and
        [B, V, W] is L / V times smaller than what the reference gathers); V <= ops.EMBED_SEQ_MAX_SEGMENTS.  prefix fp32 [B, P, W]: the
        rows the consumer puts in front (cls, gender, ethnicity), copied into seq[:, :P].  Every part may be absent; with none of them seq
        is forward(index, padding_mask).  With r = forward(index, padding_mask, out_dtype=torch.float32)[b, p]:

            padded position      seq[b, P + p] = r (the bias row, or zeros without a projector); nothing is added, and neither
                                 index[b, p] nor segment_id[b, p] is read
            unpadded position    seq[b, P + p] = ((r + position_rows[p]) + segment_rows[0][b, g]) + segment_rows[1][b, g],  g = segment_id[b, p]

        plain fp32 additions in that order (the reference's ((x + pe) + t_within) + t_between), continuing from the fp32 value of the
        lookup: in fp32 seq[:, P:] is bit for bit torch.where(mask, r, ((r + pe) + R0[b, g]) + R1[b, g]).  A miss position and, with
        validate=False, a bad code index take the adds like any unpadded position.  A 16-bit output rounds the finished fp32 value once.
        key_padding_mask is padding_mask with P False columns in front (all False without a mask).  Deviation from the reference: it
        adds the terms at padded positions too; those positions are masked as keys and only the CLS row is read, so nothing downstream
        sees the difference.  Dropout stays outside: PositionalEncoding's dropout(0.2) is torch's, applied by the caller to seq[:, P:].

        validate=True reads the status back and raises the ValueErrors of `forward` first ("code index", then the first slot with a bad
        id), then one naming the "segment id" for an unpadded g outside [0, V); validate=False reads nothing (such a position gets no
        segment term), so a step -- forward and backward -- can be captured in a HIP graph.  Gradients: prefix, position_rows and
        segment_rows get theirs from fixed-order sums without float atomics (ops.embed_sequence_position_grad / _segment_grad: two
        backward runs give the same bits); the projector, miss_emb and a training codebook get what `forward` gives them from
        g[:, P:].  Over folded tables (the rule of `forward`) the whole row is made in one launch (ops.embed_sequence); otherwise the
        lookup's fp32 rows go through one elementwise launch (ops.embed_sequence_rows)."""
        name = "MedTokEmbedding.sequence"
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
            raise ValueError(f"MedTokEmbedding: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
        if index.dim() != 2:
            raise ValueError(f"{name} takes index [B, L], got {tuple(index.shape)}")
        p, q = getattr(self, "projector", None), self.quantizer
        width = self.embedding_dim if p is None else p.out_features
        padding_mask, out_dtype = self._checked(index, padding_mask, out_dtype, None, width)
        batch, length = index.shape
        position_rows, segment_id, terms, prefix, n_segments, n_prefix = ops._sequence_parts(name, batch, length, width, position_rows, segment_id,
                                                                                             segment_rows, prefix)
        seg0, seg1 = (terms + (None, None))[:2]
        parts = (position_rows, seg0, seg1, prefix)
        grad_on = torch.is_grad_enabled()
        parts_grad = grad_on and any(t is not None and t.requires_grad for t in parts)
        dev = self.tokens.device
        regions = self._regions()
        fold = False
        if p is not None:
            if p.weight.dtype != torch.float32:
                raise ValueError(f"MedTokEmbedding: the projector must be fp32 (every product behind the lookup is), got {p.weight.dtype}")
            want_codebook, _, norm, fold = self._route(grad_on, index.numel())
        status = torch.zeros(1, dtype=torch.int32, device=dev) if validate else None
        if fold:
            folded = self._folded(norm)
            scatter = self.grad_form == "scatter"
            if parts_grad or (scatter and want_codebook) or (grad_on and any(
                    t is not None and t.requires_grad for t in (p.weight, p.bias, self.miss_emb))):
                seq = _EmbedSequenceFunction.apply(p.weight, p.bias, self.miss_emb, self._codebook_input() if scatter and want_codebook else None,
                                                   position_rows, seg0, seg1, prefix, index, padding_mask, segment_id, self.tokens, self.weights,
                                                   norm[0], tuple(regions), int(q.e_dim), folded, out_dtype, status, scatter)
            else:
                seq = ops.embed_sequence(index, self.tokens, self.weights, *folded[:3], miss_row=folded[3], pad_mask=padding_mask,
                                         position_rows=position_rows, segment_id=segment_id, segment_rows=terms or None, prefix=prefix,
                                         width=width, out_dtype=out_dtype, status=status)
            if seq.shape[2] != width:
                seq = seq[:, :, :width].contiguous()
        else:
            rows = self.forward(index, padding_mask, validate=validate, out_dtype=torch.float32)     # (raises its own errors first)
            if parts_grad or rows.requires_grad:
                seq = _EmbedSequenceRowsFunction.apply(rows, position_rows, seg0, seg1, prefix, padding_mask, segment_id, out_dtype, status)
            else:
                seq = ops.embed_sequence_rows(rows, pad_mask=padding_mask, position_rows=position_rows, segment_id=segment_id,
                                              segment_rows=terms or None, prefix=prefix, out_dtype=out_dtype, status=status)
        if validate:
            word = int(status.item())
            self._raise_on(word & ~(1 << ops.EMBED_BAD_SEGMENT_BIT), regions)
            if word >> ops.EMBED_BAD_SEGMENT_BIT & 1:
                raise ValueError(f"MedTokEmbedding: a segment id outside [0, {n_segments}) at a position the padding mask does not cover")
        keys = torch.zeros((batch, n_prefix + length), dtype=torch.bool, device=seq.device)
        if padding_mask is not None:
            keys[:, n_prefix:] = padding_mask.to(seq.device) != 0
        return seq, keys

    # ------------------------------------------------------------------ bag pooling
    def pooled(self, index, padding_mask=None, normalize: bool = True, validate: bool = True):
        """index int64 [B, L] -> fp32 [B, S * e_dim]: the mean over each bag's unpadded positions of the L2-normalised rows `forward`
        would give, in one pass and without the [B, L, S * e_dim] rows (ops.embed_pool).  What the reference's QA adapter computes per
        sample in a Python loop over embeddings_all.npy (MedTok_QA_Tutorial/review.py:50-64: gather the sample's codes, F.normalize
        each 256-wide row, mean over the set):

            pooled[b] = (sum over the unpadded p of bag b, in a fixed order, of n(row(p))) / live_b,     n(v) = v / max(|v|_2, 1e-12)

        The norm runs over the whole row (all slots), not per slot; normalize=False: n(v) = v (the default here is True, the QA
        adapter's form; pooled_segments, the EHR form, defaults to False).  padding_mask: bool / uint8 [B, L],
        True = padded, any pattern (not only a prefix); padded positions are not read.  live_b counts the unpadded positions: a
        position with a bad index counts (validate=False: as a row of zeros).  Deviation from the reference: a bag without an unpadded
        position is a row of ZEROS (the reference's mean over an empty set is NaN); a row of norm 0 contributes zeros.  The sum has a
        fixed order (not strict position order: ops.embed_pool says which) and uses no float atomics: two calls give the same bits, and with normalize=False a bag with one unpadded position
        holds that position's `forward` row.

        validate=True reads ONE status word back and raises the ValueErrors of `forward` ("code index", or the first slot with a bad
        id); validate=False reads nothing, so the call can be captured in a HIP graph.  With a frozen codebook the only gradient is
        miss_emb's (fixed order: two backward runs give the same bits); freeze_codebook=False composes the result from `forward`'s rows
        (the lookup kernel and its codebook gradient), F.normalize and a masked mean: the [B, L, S * e_dim] rows exist on that route.

        With a projector the result is projector(pooled) [B, H] by the exact fp32 dense product on the B pooled rows.  The projector is
        NOT folded into the tables here: the normalisation sits between the lookup and the projector, and it is not linear."""
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
            raise ValueError(f"MedTokEmbedding: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
        if index.dim() != 2:
            raise ValueError(f"MedTokEmbedding: pooled takes index [bags, bag_len], got {tuple(index.shape)}")
        padding_mask = ops._embed_mask("MedTokEmbedding", padding_mask, index)
        q = self.quantizer
        s, e, pad = len(self.types), int(q.e_dim), getattr(q, "_pad", 0)
        grad_on = torch.is_grad_enabled()
        if grad_on and not self.freeze_codebook and q.codebook.weight.requires_grad:
            res = self._pooled_composed(index, padding_mask, normalize, validate)
        else:
            regions = self._regions()
            what = q._normalised_codebook()[0]
            miss = self.miss_emb
            want_miss = grad_on and miss is not None and miss.requires_grad
            if miss is not None:
                if not want_miss:
                    miss = miss.detach()
                miss = (torch.nn.functional.pad(miss.view(s, e), (0, pad)) if pad else miss).reshape(-1)
            status = torch.zeros(1, dtype=torch.int32, device=self.tokens.device) if validate else None
            if want_miss:
                res = _EmbedPoolFunction.apply(miss, index, padding_mask, self.tokens, self.weights, what, tuple(regions), bool(normalize), status,
                                               None, 0)
            else:
                res = ops.embed_pool(index, self.tokens, self.weights, what, regions, miss=miss, pad_mask=padding_mask, normalize=normalize,
                                     status=status)[0]
            if pad:                                               # (the padding columns are zeros: they change no norm)
                res = res.reshape(-1, s, e + pad)[:, :, :e].reshape(-1, s * e)
            if validate:
                self._raise_on(int(status.item()), regions)
        p = getattr(self, "projector", None)
        return res if p is None else small_linear(res, p.weight, p.bias)

    def _pooled_composed(self, index, padding_mask, normalize, validate):
        """freeze_codebook=False: the same function from the lookup's rows (_lookup: the kernel forward, ops.embed_codes_code_grad
        backward), torch's normalise and a masked mean, so that codebook.weight gets its gradient"""
        rows = self._lookup(index, padding_mask, validate, torch.float32, None)
        if normalize:
            rows = torch.nn.functional.normalize(rows, dim=-1)
        if padding_mask is None:
            keep = torch.ones(index.shape, dtype=torch.float32, device=rows.device)
        else:
            keep = (padding_mask.to(rows.device) == 0).float()
        live = keep.sum(1, keepdim=True)
        return torch.where(live > 0, (rows * keep.unsqueeze(-1)).sum(1) / live.clamp(min=1.0), torch.zeros_like(live))

    # ------------------------------------------------------------------ a row per visit
    def pooled_segments(self, index, segment_id, n_segments, padding_mask=None, normalize: bool = False, validate: bool = True):
        """index, segment_id int64 [B, L] -> (out fp32 [B, V, S * e_dim], empty bool [B, V]), V = n_segments: one row per (batch row,
        segment) -- the mean of `forward`'s rows over the unpadded positions of row b whose segment id is v -- in one pass and without the
        [B, L, S * e_dim] rows (ops.embed_pool_segments).  With the dataloader's visit_id[:, :, 0] as segment_id this is the visit-level
        input of the reference's patientEncoder_old (EHRModel_token.py:249-272: a transformer over [B, max_visit_num, dim] visit embeddings),
        and `empty` is its src_key_padding_mask (the sense of pad_sequence's mask, :279-292: True where there is no visit):

            out[b, v] = (sum over the unpadded p with segment_id[b, p] == v, in a fixed order, of n(row(b, p))) / count[b, v]

        n(v) = v / max(|v|_2, 1e-12) over the whole row with normalize=True, else v.  normalize defaults to False here: the EHR path
        never normalises, and `sequence` does not either (`pooled`, the QA adapter's form, defaults to True).  padding_mask: bool / uint8
        [B, L], True = padded, any pattern; a padded position reads neither its index nor its segment id.  Segment ids may come in any
        order along a row (ascending runs are the dataloader's form) and need not be contiguous.  An empty (b, v) is a row of zeros.  A
        position with a bad code index counts towards its segment as a row of zeros (validate=False), as in `pooled`; an unpadded
        position whose segment id is outside [0, V) joins no segment.  The order is fixed (include/medtok_vq.h: positions ascending,
        chunks of ops.EMBED_POOL_CHUNK summed as `pooled` sums a chunk, chunk sums in order from +0, a true division) and there are no
        float atomics: two calls give the same bits, relabelling the segments permutes the rows bit for bit, with V = 1, every id 0 and
        no mask out[:, 0] is `pooled`'s, and with normalize=False a segment of one position holds that position's `forward` row.

        validate=True reads ONE status word back and raises the ValueErrors of `forward` first ("code index", then the first slot with a
        bad id), then `sequence`'s, naming the "segment id"; validate=False reads nothing, and every step is a kernel launch, so the call
        -- forward and backward -- can be captured in a HIP graph.  With a frozen codebook the only gradient is miss_emb's (`pooled`'s
        arithmetic over B * V bags; two backward runs give the same bits).  freeze_codebook=False composes the result from `forward`'s
        rows, F.normalize, the fixed-order per-segment sum of ops.embed_sequence_segment_grad (V <= ops.EMBED_SEQ_MAX_SEGMENTS on this
        route) and a division by integer counts: the [B, L, S * e_dim] rows exist on that route.

        With a projector the result is projector(out) [B, V, H] by the exact fp32 dense product on the B * V pooled rows (an empty
        segment: the bias row, as in `pooled`).  The projector is not folded into the tables here."""
        name = "MedTokEmbedding.pooled_segments"
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
            raise ValueError(f"MedTokEmbedding: index must be an int64 tensor, got {getattr(index, 'dtype', type(index))}")
        if index.dim() != 2:
            raise ValueError(f"{name} takes index [B, L], got {tuple(index.shape)}")
        batch, length = index.shape
        if not isinstance(segment_id, torch.Tensor) or segment_id.dtype != torch.int64 or segment_id.shape != index.shape:
            raise ValueError(f"{name}: segment_id must be an int64 [{batch}, {length}] tensor, got {getattr(segment_id, 'dtype', type(segment_id))} "
                             f"{tuple(getattr(segment_id, 'shape', ()))}")
        n_segments = int(n_segments)
        if n_segments < 1:
            raise ValueError(f"{name}: n_segments = {n_segments} must be >= 1")
        padding_mask = ops._embed_mask("MedTokEmbedding", padding_mask, index)
        q = self.quantizer
        s, e, pad = len(self.types), int(q.e_dim), getattr(q, "_pad", 0)
        grad_on = torch.is_grad_enabled()
        regions = self._regions()
        if grad_on and not self.freeze_codebook and q.codebook.weight.requires_grad:
            res, empty = self._pooled_segments_composed(index, segment_id, n_segments, padding_mask, normalize, validate)
        else:
            what = q._normalised_codebook()[0]
            miss = self.miss_emb
            want_miss = grad_on and miss is not None and miss.requires_grad
            if miss is not None:
                if not want_miss:
                    miss = miss.detach()
                miss = (torch.nn.functional.pad(miss.view(s, e), (0, pad)) if pad else miss).reshape(-1)
            status = torch.zeros(1, dtype=torch.int32, device=self.tokens.device) if validate else None
            if want_miss:
                res, counts = _EmbedPoolFunction.apply(miss, index, padding_mask, self.tokens, self.weights, what, tuple(regions), bool(normalize),
                                                       status, segment_id, n_segments)
            else:
                res, counts = ops.embed_pool_segments(index, segment_id, n_segments, self.tokens, self.weights, what, regions, miss=miss,
                                                      pad_mask=padding_mask, normalize=normalize, status=status)
            if pad:                                               # (the padding columns are zeros: they change no norm)
                res = res.reshape(batch, n_segments, s, e + pad)[..., :e].reshape(batch, n_segments, s * e)
            empty = counts[..., 0] == 0
            if validate:
                self._raise_on_segments(int(status.item()), regions, n_segments)
        p = getattr(self, "projector", None)
        if p is not None:
            res = small_linear(res.reshape(batch * n_segments, -1), p.weight, p.bias).reshape(batch, n_segments, -1)
        return res, empty

    def _raise_on_segments(self, word, regions, n_segments):
        """`forward`'s two errors first, then `sequence`'s "segment id" error"""
        self._raise_on(word & ~(1 << ops.EMBED_BAD_SEGMENT_BIT), regions)
        if word >> ops.EMBED_BAD_SEGMENT_BIT & 1:
            raise ValueError(f"MedTokEmbedding: a segment id outside [0, {n_segments}) at a position the padding mask does not cover")

    def _pooled_segments_composed(self, index, segment_id, n_segments, padding_mask, normalize, validate):
        """freeze_codebook=False: the same function from the lookup's rows (_lookup: the kernel forward, ops.embed_codes_code_grad
        backward), torch's normalise, the fixed-order per-segment sum (_SegmentSumFunction) and integer counts made in torch, so that
        codebook.weight gets its gradient.  No index_add_."""
        rows = self._lookup(index, padding_mask, validate, torch.float32, None)
        if normalize:
            rows = torch.nn.functional.normalize(rows, dim=-1)
        segment_id = segment_id.to(rows.device)
        mask = None if padding_mask is None else padding_mask.to(rows.device)
        on = (segment_id >= 0) & (segment_id < n_segments)
        if mask is not None:
            on = on & (mask == 0)
            if validate and bool(((mask == 0) & ~on).any()):
                raise ValueError(f"MedTokEmbedding: a segment id outside [0, {n_segments}) at a position the padding mask does not cover")
        elif validate and not bool(on.all()):
            raise ValueError(f"MedTokEmbedding: a segment id outside [0, {n_segments}) at a position the padding mask does not cover")
        sums = _SegmentSumFunction.apply(rows, segment_id, n_segments, mask)
        hit = torch.arange(n_segments, device=rows.device).view(1, 1, -1) == torch.where(on, segment_id, -1).unsqueeze(-1)   # [B, L, V]
        count = hit.sum(1)                                                                                                   # integers
        empty = count == 0
        return torch.where(empty.unsqueeze(-1), torch.zeros_like(sums), sums / count.clamp(min=1).unsqueeze(-1).float()), empty

    # ------------------------------------------------------------------ the projector behind the lookup
    def fold_table_shape(self):
        """(rows, columns) of the folded tables: the slots' region sizes summed, H rounded up to 4"""
        return sum(size for _, size in self._regions()), ops.pad_dim(self.projector.out_features)

    def fold_rule(self, positions: int, cache_valid: bool) -> bool:
        """fold=None: fold when the projector narrows (H < S * e_dim), the tables fit FOLD_MAX_BYTES and either they are already built
        for the current weights or positions * S >= FOLD_COLD_FACTOR * rows.

        Measured at 96,000 positions, H = 256, against F.linear(lookup) (profiles/embed_bench.json "project"):
        at H = S * e_dim = 256 the lookup over warm tables is 0.98x the composition (k rows of H floats per slot are 4x the rows of e_dim
        floats the plain lookup gathers), so such a projector is not folded; at e_dim = 768 it is 9.4x.  The flop break-even positions *
        S >= rows (2 * rows * e_dim * H against 2 * positions * S * e_dim * H) did not hold for a call that has to build its tables:
        0.98x at positions * S = 2.9 rows (cfg 3: the fold takes 1.51 ms, which the call repays at 1.54 us per 100 positions, i.e.
        from 97,900 positions = 3.0 rows / S), hence the factor; it comes from that one shape and a time taken as linear in the
        positions.  The module's own unfolded path (small_linear, not F.linear) has not been timed."""
        rows, hp = self.fold_table_shape()
        if self.projector.out_features >= self.embedding_dim or rows * hp * 4 > self.FOLD_MAX_BYTES:
            return False
        return bool(cache_valid) or positions * len(self.types) >= self.FOLD_COLD_FACTOR * rows

    def _route(self, grad_on, positions):
        """Which way a call with a projector goes -> (want_codebook, unfolded, norm, fold).  want_codebook: the codebook trains in this
        call; unfolded: it does and the gradient form cannot serve it over the folded tables, so the lookup runs as it stands and the
        dense product follows; norm: the normalised codebook (None where unfolded: the lookup makes its own, under autograd); fold: the
        folded route is taken -- the module's setting, or fold_rule for this many positions."""
        q = self.quantizer
        want_codebook = grad_on and not self.freeze_codebook and q.codebook.weight.requires_grad
        unfolded = want_codebook and not self._scatter_trains()
        norm = None if unfolded else q._normalised_codebook()
        fold = False if unfolded else self.fold
        if fold is None:
            cache = self._fold_cache
            fold = self.fold_rule(positions, cache is not None and cache[0] == self._fold_key(norm))
        return want_codebook, unfolded, norm, fold

    def _scatter_trains(self):
        """whether a codebook that trains may stay on the folded route: grad_form="scatter" (e_dim % 4 != 0 keeps the unfolded route)"""
        return self.grad_form == "scatter" and not getattr(self.quantizer, "_pad", 0)

    def _codebook_input(self):
        """codebook.weight as the scatter nodes take it: fp32, under autograd"""
        return self.quantizer.codebook.weight.float()

    def _fold_key(self, norm):
        tensors = (self.projector.weight, self.projector.bias, self.miss_emb)
        return (id(norm),) + tuple(None if t is None else (t._version, t.data_ptr(), t.device) for t in tensors)

    def _folded(self, norm):
        """the folded tables of the current weights: (table, row_regions, bias, miss_row), rebuilt only when the key changes"""
        key = self._fold_key(norm)
        cache = self._fold_cache
        if cache is None or cache[0] != key:
            p, e = self.projector, int(self.quantizer.e_dim)
            with torch.no_grad():
                folded = ops.fold_projector(norm[0], self._regions(), p.weight.detach(), None if p.bias is None else p.bias.detach(),
                                            None if self.miss_emb is None else self.miss_emb.detach().reshape(-1), e_dim=e)
            self.fold_builds += 1
            cache = self.__dict__["_fold_cache"] = (key, norm, folded)     # (the entry is kept: its id cannot be handed out again)
        return cache[2]

    def _forward_projected(self, index, padding_mask, validate, out_dtype, out):
        """forward with a projector: [..., H].  Folded: one launch over the cached tables (ops.embed_project); else the lookup as it
        stands, in fp32, followed by the exact fp32 dense product (autograd.small_linear)."""
        p, q = self.projector, self.quantizer
        if p.weight.dtype != torch.float32:
            raise ValueError(f"MedTokEmbedding: the projector must be fp32 (every product behind the lookup is), got {p.weight.dtype}")
        h, hp, n = p.out_features, ops.pad_dim(p.out_features), index.numel()
        padding_mask, out_dtype = self._checked(index, padding_mask, out_dtype, out, h)
        grad_on = out is None and torch.is_grad_enabled()
        want_codebook, _, norm, fold = self._route(grad_on, n)
        if not fold:
            # the lookup (its own validation, miss-row and codebook gradients), then the dense product; `out` cannot take the fp32 rows
            with torch.set_grad_enabled(grad_on):                  # (a call that fills `out` is not differentiable: no graph is built)
                emb = self._lookup(index, padding_mask, validate, torch.float32, None)
                res = small_linear(emb.reshape(n, self.embedding_dim), p.weight, p.bias).to(out_dtype)
            if out is not None:
                out.copy_(res)
                return out
            return res.reshape(*index.shape, h)
        folded = self._folded(norm)
        regions = self._regions()
        status = torch.zeros(1, dtype=torch.int32, device=self.tokens.device) if validate else None
        wants = [t is not None and t.requires_grad for t in (p.weight, p.bias, self.miss_emb)]
        scatter = self.grad_form == "scatter"
        if grad_on and (any(wants) or (scatter and want_codebook)):
            res = _EmbedProjectFunction.apply(p.weight, p.bias, self.miss_emb, self._codebook_input() if scatter and want_codebook else None, index,
                                              padding_mask, self.tokens, self.weights, norm[0], tuple(regions), int(q.e_dim), folded, out_dtype,
                                              status, scatter)
        else:
            res = ops.embed_project(index, self.tokens, self.weights, *folded[:3], miss_row=folded[3], pad_mask=padding_mask,
                                    out=out if hp == h else None, out_dtype=out_dtype, status=status)
        if hp != h:
            res = res.reshape(n, hp)[:, :h]
            if out is not None:
                out.copy_(res)
        if validate:
            self._raise_on(int(status.item()), regions)
        return out if out is not None else res.reshape(*index.shape, h)
