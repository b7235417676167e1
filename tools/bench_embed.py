"""Time MedTokEmbedding -- code indices -> embeddings through the stored token table -- on one MI355X against the two ways a
downstream model had before it.

    python tools/bench_embed.py [--codes 600000] [--batch 32] [--length 3000] [--reps 20] [--warmup 3] [--out profiles/embed_bench.json]

Prints ONE JSON line.  A [batch, length] index tensor over num_codes codes (S = 4 slots, k = 5), about 40 % of the positions under
the padding mask and 1 % at the miss index, at two shapes: the reference's (e_dim 64, n_e 21000) and cfg 3 (e_dim 768, n_e 49152).
Per shape:

  kernel_f32 / kernel_bf16   MedTokEmbedding.forward(index, padding_mask, validate=False): one launch, fp32 or bf16 rows
  composition                what the parent commit offered: quantizer.decode(tokens[idx], weights[idx]) on the gathered rows, the miss
                             row put in with torch.where and the padded rows zeroed with masked_fill (no host read either)
  table_gather               the reference's way: med_code_emb[index] over the materialised fp32 table with the miss row appended
                             (EHRModel_token.py:128-141,214-215; its padded positions hold code 0's row).  The table has --table-rows
                             rows (default: all num_codes where they fit into a quarter of the free memory, else as many as do; the
                             indices are folded into them) -- `table_rows` in the result says how many

--project H: the lookup followed by the consumers' nn.Linear(S * e_dim, H) instead (MedTokEmbedding(projector=...)), the same two
workloads; four cases per shape, compared before anything is timed (1e-5 of the output's scale):

  folded_warm                module(index, padding_mask, validate=False), fold=True, the folded tables cached: one launch
  folded_cold                the same call with the cached tables dropped before it: the fold (2 * rows * e_dim * H flops) included
  forward_backward           the folded forward under autograd and its backward (dW, db, d miss_emb) from a fixed upstream gradient
  composition                what the parent commit offered: F.linear(module(index, padding_mask, validate=False), W, b)

The result goes under the key "project" of --out (the other keys of an existing file are kept).

--pool: bag pooling (MedTokEmbedding.pooled: the normalised mean of each bag's unpadded codes, what the reference's QA adapter computes
per sample, MedTok_QA_Tutorial/review.py:50-64) at two bag shapes per store shape -- the adapter's, 16 bags x 256 left-padded
positions, and a throughput shape, 4096 bags x 64 -- with --padded of the positions under the mask and --miss at the miss index; three
cases, compared before anything is timed (1e-5 of the result's scale):

  pooled                     module.pooled(index, padding_mask, validate=False): two launches, [bags, S * e_dim] and the partial sums
  composition                what the parent commit offered: module(index, padding_mask, validate=False) -> F.normalize -> sum over the
                             bag / the unmasked count (the padded rows are zeros already); the [bags, L, S * e_dim] rows are written
  reference_loop             the reference's own loop over the materialised fp32 table: per sample a boolean selection of its codes
                             (a host read, as its .item()), the gather, F.normalize, mean (table_rows as above)

The result goes under the key "pool" of --out (the other keys are kept).

--codebook-grad: forward + backward with freeze_codebook=False (the table follows the tokenizer's codebook during fine-tuning) from a
fixed upstream gradient, at the same two workloads and in a "hot" variant of each with half the live positions on ONE code (real code
frequencies are heavy-tailed); the gradients of codebook.weight are compared before anything is timed (1e-5 of their scale):

  kernel                     module(index, padding_mask, validate=False).backward(g): the lookup kernel, then the per-row sums straight
                             from the upstream gradient (ops.embed_codes_code_grad: sort of 8 bytes per contribution, chunked chains)
  parent_composition         what the parent commit ran, restated here: boolean selections and nonzero() (host reads), quantizer.decode
                             on the gathered rows of the live positions, index_put; its backward writes one [d] row per (position, slot,
                             j) and sorts and sums those
  torch_table                torch autograd over the materialised table: (weights * F.normalize(W)[tokens + lo]).sum -> table[index]; the
                             table has --table-rows rows (default 20000: the [rows, S, k, d] gather is 1.2 GB at cfg 3, 37 GB for all 600,000) and the
                             indices are folded into them

Per case also `peak_bytes`: the rise of torch.cuda.max_memory_allocated() over one forward + backward.  The result goes under the key
"codebook_grad" of --out (the other keys are kept).

--sequence H: the EHR model's input sequence (MedTokEmbedding.sequence: the folded lookup, a positional row per position, two time rows
per position carried from its visit, three prefix rows in front; EHRModel_token.py:215-232) at the reference's own shape (MedTok_EHR.py:
49,77-80) -- --batch 256 --length 2000, 100 visits, 3 prefix rows -- over the reference store shape, visits in ascending order along a
row; compared before anything is timed (fp32: bit for bit at the unpadded positions and the prefix, the bias row at the padded ones):

  sequence_f32 / _bf16       module.sequence(index, mask, position_rows=, segment_id=, segment_rows=[t0, t1], prefix=, validate=False)
  composition_f32 / _bf16    what a user writes today: module(index, mask, validate=False) + pe[:L] + the two [B, L, H] gathers of the
                             per-visit rows, added, torch.cat behind the prefix (bf16: converted at the end)
  sequence_step / composition_step   forward + backward of the fp32 forms from a fixed upstream gradient, the additive tensors, the
                             projector and miss_emb requiring gradients

`spread` of a case = (ms_max - ms_min) / ms_median over its samples.  The result goes under the key "sequence" of --out (the other keys
are kept).

--segments: one row per visit (MedTokEmbedding.pooled_segments: the mean of `forward`'s rows over the unpadded positions of each (batch
row, visit); the input of the reference's patientEncoder_old, EHRModel_token.py:249-292) at the --sequence shape -- --batch 256 --length
2000, --visits 100, the reference store shape, no projector, normalize=False -- with the visit ids in ascending runs along a row (the
dataloader's form) and, as a second case, the same ids shuffled along the row; compared at the timed size before anything is timed (1e-5
of the result's scale, and the `empty` masks equal):

  pooled_segments            module.pooled_segments(index, segment_id, V, mask, validate=False): keys, sort, pooling over listed positions
  composition_segment_grad   what a user writes today without atomics: module(index, mask, validate=False) rows [B, L, S * e_dim], then
                             ops.embed_sequence_segment_grad(rows, segment_id, V, mask) / the counts
  composition_index_add      the same rows, then zeros(B * V + 1, W).index_add_(0, b * V + id, rows) / the counts (float atomics: the
                             bits change from run to run)

Per side the timing statistics, `spread` and `peak_bytes` (the rise of torch.cuda.max_memory_allocated() over one call); per case
`pooled_segments_not_slower_within_spread` against each composition: the fused median <= the composition's median + (its max - its
min).  The result goes under the key "segments" of --out (the other keys are kept).

--grad-form (with --project H or --sequence H): forward + backward of the folded route with MedTokEmbedding(grad_form="scatter") against
grad_form="dense" (the parent commit's arithmetic unchanged), both modules over one projector and one miss row, from a fixed upstream
gradient; outputs (bit for bit) and gradients (1e-5 of their scale between the sides; dW, whose entries sum over every position, 1e-4
of its fp64 restatement on both sides, both errors recorded) are compared at the timed size before anything is timed:

  --project H --grad-form                    frozen codebook, fold=True on both sides, the two workloads of --project
  --sequence H --grad-form                   the --sequence step (--batch 256 --length 2000), the additive tensors requiring gradients too
  --project H --grad-form --train-codebook   freeze_codebook=False: scatter stays folded, dense unfolds (the lookup's [n, S * e_dim] rows and
                                             small_linear); a random store and the "hot" store of --codebook-grad per workload; a third
                                             side, scatter_refold, drops the cached tables before every step (what a step that
                                             follows an optimiser step pays)

Per side the timing statistics, `spread` and `peak_bytes` (the rise of torch.cuda.max_memory_allocated() over one step); per case
`table_grad_ms`, ops.embed_project_table_grad alone on the same upstream gradient (its sort and its sums are not separated: that takes
a kernel trace), and `scatter_not_slower_within_dense_spread`: scatter's median <= dense's median + (dense's max - dense's min).  The
result goes under the key "table_grad" of --out, one sub-key per invocation form (the other keys are kept).

Discipline (bench_decode.py's): all sides are warmed up at the timed shape, compared before anything is timed, timed with device
events over samples of >= 50 ms of back-to-back calls that ALTERNATE between the sides, at least 20 samples each; the shader clock
(ops.ClockProbe) is read over further kernel samples right behind the timed region.  Algorithmic bytes of the kernel = per position
the index and the mask byte, per live position S * 12 k of ids and weights, per position the written row, plus the codebook once;
their rate is given as a fraction of the 6.29 TB/s a float4 copy reaches on this chip (8.0 TB/s is the HBM3E spec).
`device_bytes_held` is what each approach keeps resident between calls.
"""
from __future__ import annotations

import argparse
import datetime
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_MEASURED_TBS = 6.29       # float4 copy
HBM_SPEC_TBS = 8.0
SHAPES = {"reference": dict(d=64, n_e=21000), "cfg3": dict(d=768, n_e=49152)}
TYPES = ("text", "graph", "shared", "shared")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", type=int, default=600000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--padded", type=float, default=0.40)
    ap.add_argument("--miss", type=float, default=0.01)
    ap.add_argument("--table-rows", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="reference,cfg3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--project", type=int, default=0, metavar="H", help="time the lookup with a folded nn.Linear(S * e_dim, H) instead")
    ap.add_argument("--pool", action="store_true", help="time bag pooling (MedTokEmbedding.pooled) instead")
    ap.add_argument("--codebook-grad", action="store_true", help="time forward + backward with freeze_codebook=False instead")
    ap.add_argument("--sequence", type=int, default=0, metavar="H", help="time MedTokEmbedding.sequence against the torch composition instead")
    ap.add_argument("--segments", action="store_true", help="time MedTokEmbedding.pooled_segments (a row per visit) against the compositions instead")
    ap.add_argument("--visits", type=int, default=100, help="--sequence / --segments: segments (visits) per batch row")
    ap.add_argument("--prefix", type=int, default=3, help="--sequence: rows in front of each batch row")
    ap.add_argument("--grad-form", action="store_true", help="with --project / --sequence: time grad_form='scatter' against 'dense' instead")
    ap.add_argument("--train-codebook", action="store_true", help="--project H --grad-form: with freeze_codebook=False")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_embed needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def inner_for(fn):
        t = timed(fn, 1)
        return max(1, min(200, math.ceil(50.0 / max(t, 1e-3))))

    def stats(ms):
        return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), ms_mean=statistics.fmean(ms), samples=len(ms))

    if args.grad_form:
        if not (args.project or args.sequence) or (args.train_codebook and not args.project):
            ap.error("--grad-form goes with --project H or --sequence H; --train-codebook with --project H")
        return grad_form_mode(args, dev, timed, inner_for, stats)
    if args.project:
        return project_mode(args, dev, timed, inner_for, stats)
    if args.pool:
        return pool_mode(args, dev, timed, stats)
    if args.codebook_grad:
        return codebook_grad_mode(args, dev, timed, inner_for, stats)
    if args.sequence:
        return sequence_mode(args, dev, timed, inner_for, stats)
    if args.segments:
        return segments_mode(args, dev, timed, inner_for, stats)

    result = {"tool": "tools/bench_embed.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
              "num_codes": args.codes, "positions": [args.batch, args.length], "slots": 4, "k": args.k, "padded_fraction": args.padded,
              "miss_fraction": args.miss, "hbm_roof_tb_s": HBM_MEASURED_TBS, "hbm_spec_tb_s": HBM_SPEC_TBS, "shapes": {}}
    for name in args.shapes.split(","):
        d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
        k, num_codes, width = args.k, args.codes, 4 * SHAPES[name]["d"]
        n_pos = args.batch * args.length
        torch.manual_seed(0)
        vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
        with torch.no_grad():
            vq.codebook.weight.normal_()
        vq = vq.to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(1)
        sizes = [hi - lo for lo, hi in (vq._region(t) for t in TYPES)]
        tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen, device=dev) for s in sizes], 1).contiguous()
        weights = torch.softmax(torch.randn(num_codes, 4, k, generator=gen, device=dev), -1).contiguous()
        module = MedTokEmbedding(vq, tokens, weights).to(dev)
        del tokens, weights
        tokens, weights, miss = module.tokens, module.weights, module.miss_emb.detach()
        index = torch.randint(0, num_codes, (args.batch, args.length), generator=gen, device=dev)
        u = torch.rand(args.batch, args.length, generator=gen, device=dev)
        index[u < args.miss] = num_codes
        mask = u > 1.0 - args.padded
        index[mask] = 0                                     # (the reference's dataloader pads with code 0 under its code_mask)
        live = int((~mask & (index < num_codes)).sum())
        n_miss = int((~mask & (index == num_codes)).sum())

        # the reference's table: decoded in chunks, the miss row appended; as many rows as fit comfortably
        free = torch.cuda.mem_get_info(dev)[0]
        fit = int(free // 4 // (width * 4))
        table_rows = min(num_codes, args.table_rows or fit)
        table = torch.empty(table_rows + 1, width, device=dev)
        with torch.no_grad():
            for r0 in range(0, table_rows, 65536):
                r1 = min(table_rows, r0 + 65536)
                vq.decode(tokens[r0:r1], weights[r0:r1], out=table[r0:r1], validate=False)
            table[table_rows] = miss[0]
        table_index = torch.where(index == num_codes, table_rows, index % table_rows)
        is_miss = (index == num_codes).unsqueeze(-1)
        safe = torch.where(index < num_codes, index, 0).reshape(-1)
        outs = {}

        def kernel_f32():
            outs["kernel_f32"] = module(index, padding_mask=mask, validate=False)

        def kernel_bf16():
            outs["kernel_bf16"] = module(index, padding_mask=mask, validate=False, out_dtype=torch.bfloat16)

        def composition():
            rows = vq.decode(tokens[safe], weights[safe], validate=False).view(args.batch, args.length, width)
            outs["composition"] = torch.where(is_miss, miss[0], rows).masked_fill_(mask.unsqueeze(-1), 0.0)

        def table_gather():
            outs["table_gather"] = table[table_index]

        sides = {"kernel_f32": kernel_f32, "kernel_bf16": kernel_bf16, "composition": composition, "table_gather": table_gather}
        with torch.no_grad():
            for _ in range(args.warmup):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            if not torch.equal(outs["kernel_f32"], outs["composition"]):
                raise SystemExit(f"{name}: kernel and torch composition disagree")
            if not torch.equal(outs["kernel_bf16"], outs["kernel_f32"].to(torch.bfloat16)):
                raise SystemExit(f"{name}: the bf16 output is not the rounded fp32 output")
            if table_rows == num_codes and not torch.equal(outs["table_gather"][~mask], outs["kernel_f32"][~mask]):
                raise SystemExit(f"{name}: kernel and table gather disagree on the unpadded positions")
            inner = {s: inner_for(fn) for s, fn in sides.items()}
            ms = {s: [] for s in sides}
            for _ in range(args.reps):                      # the sides alternate
                for s, fn in sides.items():
                    ms[s].append(timed(fn, inner[s]))
            with ops.ClockProbe(dev, max_seconds=10.0) as probe:
                for _ in range(max(2, args.reps // 4)):
                    timed(kernel_f32, inner["kernel_f32"])
            clock = probe.result()
        st = {s: stats(v) for s, v in ms.items()}
        table_bytes = live * 4 * 12 * k + n_pos * 9 + n_e * d * 4
        alg = {"kernel_f32": table_bytes + n_pos * width * 4, "kernel_bf16": table_bytes + n_pos * width * 2,
               "table_gather": n_pos * 8 + 2 * n_pos * width * 4}
        held = {"kernel": tokens.numel() * 8 + weights.numel() * 4 + 2 * n_e * d * 4 + width * 4,
                "composition": tokens.numel() * 8 + weights.numel() * 4 + 2 * n_e * d * 4 + width * 4,
                "table_gather": table.numel() * 4, "table_gather_at_all_codes": (num_codes + 1) * width * 4}
        entry = {"d": d, "n_e": n_e, "k": k, "num_codes": num_codes, "positions": n_pos, "live_positions": live, "miss_positions": n_miss,
                 "padded_positions": int(mask.sum()), "output_gb_f32": n_pos * width * 4 / 1e9, "table_rows": table_rows,
                 "table_is_complete": table_rows == num_codes, "device_bytes_held": held,
                 "composition_temporaries_bytes": n_pos * 4 * k * 12 + 2 * n_pos * width * 4,
                 "clock_ghz": clock.get("ghz_mean"), "clock_ghz_min": clock.get("ghz_min"), "clock_ghz_max": clock.get("ghz_max"),
                 "clock_region": "further kernel_f32 samples right behind the timed region"}
        for s in sides:
            e = dict(st[s], calls_per_sample=inner[s], positions_per_s=n_pos / (st[s]["ms_median"] * 1e-3))
            if s in alg:
                tbs = alg[s] / (st[s]["ms_median"] * 1e-3) / 1e12
                e.update(algorithmic_bytes=alg[s], algorithmic_tb_s=tbs, frac_of_hbm_roof=tbs / HBM_MEASURED_TBS, frac_of_hbm_spec=tbs / HBM_SPEC_TBS)
            entry[s] = e
        entry["kernel_f32_speedup_over_composition"] = st["composition"]["ms_median"] / st["kernel_f32"]["ms_median"]
        entry["kernel_f32_speedup_over_table_gather"] = st["table_gather"]["ms_median"] / st["kernel_f32"]["ms_median"]
        entry["kernel_bf16_speedup_over_kernel_f32"] = st["kernel_f32"]["ms_median"] / st["kernel_bf16"]["ms_median"]
        entry["kernel_at_least_as_fast_as_composition"] = st["kernel_f32"]["ms_median"] <= st["composition"]["ms_median"]
        result["shapes"][name] = entry
        del table, outs, module, tokens, weights, index, mask, table_index, safe, is_miss
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(line)


def project_mode(args, dev, timed, inner_for, stats):
    import torch
    import torch.nn.functional as F
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    h = args.project
    result = {"tool": "tools/bench_embed.py --project", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
              "num_codes": args.codes, "positions": [args.batch, args.length], "slots": 4, "k": args.k, "H": h,
              "padded_fraction": args.padded, "miss_fraction": args.miss, "shapes": {}}
    for name in args.shapes.split(","):
        d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
        k, num_codes, n_pos = args.k, args.codes, args.batch * args.length
        torch.manual_seed(0)
        vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
        with torch.no_grad():
            vq.codebook.weight.normal_()
        vq = vq.to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(1)
        sizes = [hi - lo for lo, hi in (vq._region(t) for t in TYPES)]
        tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen, device=dev) for s in sizes], 1).contiguous()
        weights = torch.softmax(torch.randn(num_codes, 4, k, generator=gen, device=dev), -1).contiguous()
        proj = torch.nn.Linear(4 * d, h).to(dev)
        module = MedTokEmbedding(vq, tokens, weights, projector=proj, fold=True)
        plain = MedTokEmbedding(vq, tokens, weights)
        plain.tokens, plain.weights, plain.miss_emb = module.tokens, module.weights, module.miss_emb
        del tokens, weights
        index = torch.randint(0, num_codes, (args.batch, args.length), generator=gen, device=dev)
        u = torch.rand(args.batch, args.length, generator=gen, device=dev)
        index[u < args.miss] = num_codes
        mask = u > 1.0 - args.padded
        index[mask] = 0
        g_out = torch.randn(args.batch, args.length, h, generator=gen, device=dev)
        outs = {}

        def folded_warm():
            with torch.no_grad():
                outs["folded_warm"] = module(index, padding_mask=mask, validate=False)

        def folded_cold():
            module.__dict__["_fold_cache"] = None
            with torch.no_grad():
                outs["folded_cold"] = module(index, padding_mask=mask, validate=False)

        def forward_backward():
            module.zero_grad(set_to_none=True)
            module(index, padding_mask=mask, validate=False).backward(g_out)

        def composition():
            with torch.no_grad():
                outs["composition"] = F.linear(plain(index, padding_mask=mask, validate=False), proj.weight, proj.bias)

        sides = {"folded_warm": folded_warm, "folded_cold": folded_cold, "forward_backward": forward_backward, "composition": composition}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        scale = float(outs["composition"].abs().max())
        err = float((outs["folded_warm"] - outs["composition"]).abs().max()) / scale
        if not err <= 1e-5 or not torch.equal(outs["folded_warm"], outs["folded_cold"]):
            raise SystemExit(f"{name}: folded lookup and composition disagree (rel {err})")
        inner = {s: inner_for(fn) for s, fn in sides.items()}
        ms = {s: [] for s in sides}
        for _ in range(args.reps):                          # the sides alternate
            for s, fn in sides.items():
                ms[s].append(timed(fn, inner[s]))
        with ops.ClockProbe(dev, max_seconds=10.0) as probe:
            for _ in range(max(2, args.reps // 4)):
                timed(folded_warm, inner["folded_warm"])
        clock = probe.result()
        st = {s: stats(v) for s, v in ms.items()}
        rows, hp = module.fold_table_shape()
        live = int((~mask & (index < num_codes)).sum())
        entry = {"d": d, "n_e": n_e, "k": k, "H": h, "num_codes": num_codes, "positions": n_pos, "live_positions": live,
                 "table_rows": rows, "table_bytes": rows * hp * 4, "fold_flops": 2 * rows * d * h, "per_position_product_flops": 2 * n_pos * 4 * d * h,
                 "activation_bytes_not_written": n_pos * 4 * d * 4, "rel_folded_vs_composition": err,
                 "folded_warm_algorithmic_bytes": live * 4 * 12 * k + n_pos * 9 + n_pos * hp * 4 + rows * hp * 4,
                 "clock_ghz": clock.get("ghz_mean"), "clock_region": "further folded_warm samples right behind the timed region"}
        for s in sides:
            entry[s] = dict(st[s], calls_per_sample=inner[s], positions_per_s=n_pos / (st[s]["ms_median"] * 1e-3))
        entry["folded_warm_speedup_over_composition"] = st["composition"]["ms_median"] / st["folded_warm"]["ms_median"]
        entry["folded_cold_speedup_over_composition"] = st["composition"]["ms_median"] / st["folded_cold"]["ms_median"]
        result["shapes"][name] = entry
        del module, plain, outs, index, mask, g_out
        torch.cuda.empty_cache()
    if args.out:
        path = Path(args.out)
        whole = json.loads(path.read_text()) if path.exists() else {}
        whole["project"] = result
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(result))


POOL_BAGS = {"adapter": (16, 256), "throughput": (4096, 64)}


def pool_mode(args, dev, timed, stats):
    import torch
    import torch.nn.functional as F
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    result = {"tool": "tools/bench_embed.py --pool", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
              "num_codes": args.codes, "slots": 4, "k": args.k, "padded_fraction": args.padded, "miss_fraction": args.miss,
              "chunk": ops.EMBED_POOL_CHUNK, "samples_of_at_least_ms": 50.0, "shapes": {}}

    def inner_for(fn):                                      # samples of >= 50 ms (aimed at 65): calls of tens of microseconds need
        inner = 10                                          # thousands, and the first calls are slower than the steady ones, so the
        for _ in range(6):                                  # count is corrected on samples of its own size until one is long enough
            sample = timed(fn, inner) * inner
            if sample >= 60.0 or inner >= 50000:
                break
            inner = max(inner + 1, min(50000, math.ceil(inner * 65.0 / max(sample, 1e-3))))
        return inner

    for name in args.shapes.split(","):
        d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
        k, num_codes, width = args.k, args.codes, 4 * d
        torch.manual_seed(0)
        vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
        with torch.no_grad():
            vq.codebook.weight.normal_()
        vq = vq.to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(1)
        sizes = [hi - lo for lo, hi in (vq._region(t) for t in TYPES)]
        tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen, device=dev) for s in sizes], 1).contiguous()
        weights = torch.softmax(torch.randn(num_codes, 4, k, generator=gen, device=dev), -1).contiguous()
        module = MedTokEmbedding(vq, tokens, weights).to(dev)
        del tokens, weights
        tokens, weights, miss = module.tokens, module.weights, module.miss_emb.detach()
        free = torch.cuda.mem_get_info(dev)[0]
        table_rows = min(num_codes, args.table_rows or int(free // 4 // (width * 4)))
        table = torch.empty(table_rows + 1, width, device=dev)
        with torch.no_grad():
            for r0 in range(0, table_rows, 65536):
                r1 = min(table_rows, r0 + 65536)
                vq.decode(tokens[r0:r1], weights[r0:r1], out=table[r0:r1], validate=False)
            table[table_rows] = miss[0]
        for bag_name, (bags, length) in POOL_BAGS.items():
            index = torch.randint(0, num_codes, (bags, length), generator=gen, device=dev)
            index[torch.rand(bags, length, generator=gen, device=dev) < args.miss] = num_codes
            # left-padded: bag b's first pad_b positions, pad_b uniform in [0, 2 * padded * L) (at most L - 1)
            pads = (torch.rand(bags, generator=gen, device=dev) * 2 * args.padded * length).long().clamp_(max=length - 1)
            mask = torch.arange(length, device=dev).expand(bags, length) < pads.view(-1, 1)
            index[mask] = 0
            table_index = torch.where(index == num_codes, table_rows, index % table_rows)
            n_pos, live = bags * length, int((~mask).sum())
            n_miss = int((~mask & (index == num_codes)).sum())
            outs = {}

            def pooled():
                outs["pooled"] = module.pooled(index, padding_mask=mask, validate=False)

            def composition():
                rows = F.normalize(module(index, padding_mask=mask, validate=False), dim=-1)
                outs["composition"] = rows.sum(1) / (~mask).sum(1, keepdim=True).clamp(min=1)

            def reference_loop():
                res = []
                for b in range(bags):
                    codes = table_index[b][~mask[b]]
                    res.append(F.normalize(table[codes], p=2, dim=-1).mean(0))
                outs["reference_loop"] = torch.stack(res)

            sides = {"pooled": pooled, "composition": composition, "reference_loop": reference_loop}
            with torch.no_grad():
                for _ in range(args.warmup):
                    for fn in sides.values():
                        fn()
                torch.cuda.synchronize()
                scale = float(outs["composition"].abs().max())
                err = float((outs["pooled"] - outs["composition"]).abs().max()) / scale
                err_ref = float((outs["pooled"] - outs["reference_loop"]).abs().max()) / scale if table_rows == num_codes else None
                if not err <= 1e-5 or (err_ref is not None and not err_ref <= 1e-5):
                    raise SystemExit(f"{name}/{bag_name}: pooled disagrees with the composition ({err}) or the reference loop ({err_ref})")
                inner = {s: inner_for(fn) for s, fn in sides.items()}
                ms = {s: [] for s in sides}
                for _ in range(args.reps):                  # the sides alternate
                    for s, fn in sides.items():
                        ms[s].append(timed(fn, inner[s]))
                with ops.ClockProbe(dev, max_seconds=10.0) as probe:
                    for _ in range(max(2, args.reps // 4)):
                        timed(pooled, inner["pooled"])
                clock = probe.result()
            st = {s: stats(v) for s, v in ms.items()}
            chunks = (length + ops.EMBED_POOL_CHUNK - 1) // ops.EMBED_POOL_CHUNK
            # what the kernels move: per position the index and the mask byte, per live code its ids and weights and k rows of the
            # codebook per slot (from the caches: n_e * d * 4 bytes are the distinct ones), the partial sums written and read, the result
            gathered = (live - n_miss) * 4 * k * d * 4
            entry = {"d": d, "n_e": n_e, "k": k, "bags": bags, "bag_len": length, "positions": n_pos, "live_positions": live,
                     "miss_positions": n_miss, "table_rows": table_rows, "table_is_complete": table_rows == num_codes,
                     "rel_pooled_vs_composition": err, "rel_pooled_vs_reference_loop": err_ref,
                     "bytes_held": {"pooled": bags * width * 4 + int(ops._lib.load().medtok_embed_pool_workspace_bytes(bags, length, width)),
                                    "pooled_result": bags * width * 4, "pooled_partial_sums_and_counts": bags * chunks * (width * 4 + 8),
                                    "composition": 2 * n_pos * width * 4 + bags * width * 4,
                                    "reference_loop_table": (table_rows + 1) * width * 4},
                     "pooled_traffic_bytes": {"index_and_mask": n_pos * 9, "ids_and_weights": (live - n_miss) * 4 * k * 12,
                                              "codebook_rows_gathered": gathered, "codebook_distinct": n_e * d * 4,
                                              "partial_sums_written_and_read": 2 * bags * chunks * width * 4, "result": bags * width * 4},
                     "composition_traffic_bytes": {"rows_written": n_pos * width * 4, "rows_read_and_normalised_written": 2 * n_pos * width * 4,
                                                   "normalised_read": n_pos * width * 4},
                     "clock_ghz": clock.get("ghz_mean"), "clock_ghz_min": clock.get("ghz_min"), "clock_ghz_max": clock.get("ghz_max"),
                     "clock_region": "further pooled samples right behind the timed region"}
            for s in sides:
                entry[s] = dict(st[s], calls_per_sample=inner[s], sample_ms=st[s]["ms_median"] * inner[s], sample_ms_min=st[s]["ms_min"] * inner[s],
                                positions_per_s=n_pos / (st[s]["ms_median"] * 1e-3))
            entry["pooled_speedup_over_composition"] = st["composition"]["ms_median"] / st["pooled"]["ms_median"]
            entry["pooled_speedup_over_reference_loop"] = st["reference_loop"]["ms_median"] / st["pooled"]["ms_median"]
            entry["pooled_no_slower_than_composition"] = st["pooled"]["ms_median"] <= st["composition"]["ms_median"]
            result["shapes"][f"{name}/{bag_name}"] = entry
            del outs, index, mask, table_index
        del table, module, tokens, weights
        torch.cuda.empty_cache()
    if args.out:
        path = Path(args.out)
        whole = json.loads(path.read_text()) if path.exists() else {}
        whole["pool"] = result
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(result))


def codebook_grad_mode(args, dev, timed, inner_for, stats):
    import torch
    import torch.nn.functional as F
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    result = {"tool": "tools/bench_embed.py --codebook-grad", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
              "num_codes": args.codes, "positions": [args.batch, args.length], "slots": 4, "k": args.k, "padded_fraction": args.padded,
              "miss_fraction": args.miss, "chunk": ops.EMBED_CODE_GRAD_CHUNK, "shapes": {}}
    for name in args.shapes.split(","):
        d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
        k, num_codes, n_pos, width = args.k, args.codes, args.batch * args.length, 4 * SHAPES[name]["d"]
        torch.manual_seed(0)
        vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
        with torch.no_grad():
            vq.codebook.weight.normal_()
        vq = vq.to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(1)
        regions = [vq._region(t) for t in TYPES]
        tokens = torch.stack([torch.randint(0, hi - lo, (num_codes, k), generator=gen, device=dev) for lo, hi in regions], 1).contiguous()
        weights = torch.softmax(torch.randn(num_codes, 4, k, generator=gen, device=dev), -1).contiguous()
        module = MedTokEmbedding(vq, tokens, weights, freeze_codebook=False)
        del tokens, weights
        tokens, weights, W, miss = module.tokens, module.weights, vq.codebook.weight, module.miss_emb
        table_rows = min(num_codes, args.table_rows or 20000)
        lo = torch.tensor([r[0] for r in regions], device=dev).view(1, -1, 1)
        g_out = torch.randn(args.batch, args.length, width, generator=gen, device=dev)
        for variant in ("random", "hot"):
            index = torch.randint(0, num_codes, (args.batch, args.length), generator=gen, device=dev)
            u = torch.rand(args.batch, args.length, generator=gen, device=dev)
            if variant == "hot":                                # half the live positions on one code
                index[torch.rand(args.batch, args.length, generator=gen, device=dev) < 0.5] = 7
            index[u < args.miss] = num_codes
            mask = u > 1.0 - args.padded
            index[mask] = 0
            table_index = torch.where(index == num_codes, table_rows, index % table_rows)
            grads = {}

            def finish(case, out):
                W.grad = miss.grad = None
                out.backward(g_out)
                grads[case] = W.grad

            def kernel():
                finish("kernel", module(index, padding_mask=mask, validate=False))

            def parent_composition():
                flat = index.reshape(-1)
                padded = mask.reshape(-1)
                live = ~padded & (flat >= 0) & (flat < num_codes)
                is_miss = ~padded & (flat == num_codes)
                out = torch.zeros(n_pos, width, dtype=torch.float32, device=dev)
                at = live.nonzero().squeeze(1)
                if at.numel():
                    sel = flat[at]
                    out = out.index_put((at,), vq.decode(tokens[sel], weights[sel], types=TYPES, validate=False))
                at = is_miss.nonzero().squeeze(1)
                if at.numel():
                    out = out.index_put((at,), miss.expand(at.numel(), -1))
                finish("parent_composition", out.reshape(args.batch, args.length, width))

            def torch_table():
                table = (weights[:table_rows].unsqueeze(-1) * F.normalize(W, dim=-1)[tokens[:table_rows] + lo]).sum(2).reshape(table_rows, width)
                out = torch.cat([table, miss], 0)[table_index] * (~mask).unsqueeze(-1)
                finish("torch_table", out)

            sides = {"kernel": kernel, "parent_composition": parent_composition, "torch_table": torch_table}
            peak = {}
            for _ in range(args.warmup):
                for s, fn in sides.items():
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    fn()
                    torch.cuda.synchronize()
                    peak[s] = torch.cuda.max_memory_allocated() - before
            scale = float(grads["parent_composition"].abs().max())
            err = float((grads["kernel"] - grads["parent_composition"]).abs().max()) / scale
            if not err <= 1e-5:
                raise SystemExit(f"{name}/{variant}: the kernel's codebook gradient and the parent composition's disagree (rel {err})")
            inner = {s: inner_for(fn) for s, fn in sides.items()}
            ms = {s: [] for s in sides}
            for _ in range(args.reps):                          # the sides alternate
                for s, fn in sides.items():
                    ms[s].append(timed(fn, inner[s]))
            with ops.ClockProbe(dev, max_seconds=10.0) as probe:
                for _ in range(max(2, args.reps // 4)):
                    timed(kernel, inner["kernel"])
            clock = probe.result()
            st = {s: stats(v) for s, v in ms.items()}
            live = int((~mask & (index < num_codes)).sum())
            entry = {"d": d, "n_e": n_e, "k": k, "num_codes": num_codes, "positions": n_pos, "live_positions": live, "table_rows": table_rows,
                     "contribution_rows_bytes": live * 4 * k * d * 4, "codebook_bytes": n_e * d * 4, "rel_kernel_vs_parent_composition": err,
                     "clock_ghz": clock.get("ghz_mean"), "clock_region": "further kernel samples right behind the timed region"}
            for s in sides:
                entry[s] = dict(st[s], calls_per_sample=inner[s], peak_bytes=peak[s], positions_per_s=n_pos / (st[s]["ms_median"] * 1e-3))
            entry["kernel_speedup_over_parent_composition"] = st["parent_composition"]["ms_median"] / st["kernel"]["ms_median"]
            entry["kernel_speedup_over_torch_table"] = st["torch_table"]["ms_median"] / st["kernel"]["ms_median"]
            entry["kernel_no_slower_than_parent_composition"] = st["kernel"]["ms_median"] <= st["parent_composition"]["ms_median"]
            entry["kernel_peak_smaller_than_parent_composition"] = peak["kernel"] < peak["parent_composition"]
            result["shapes"][f"{name}/{variant}"] = entry
            W.grad = miss.grad = None
            del grads, index, mask, table_index
            torch.cuda.empty_cache()
        del module, tokens, weights, g_out
        torch.cuda.empty_cache()
    if args.out:
        path = Path(args.out)
        whole = json.loads(path.read_text()) if path.exists() else {}
        whole["codebook_grad"] = result
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(result))


def sequence_mode(args, dev, timed, inner_for, stats):
    import torch
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    h, n_seg, n_prefix = args.sequence, args.visits, args.prefix
    batch, length = args.batch, args.length
    name = "reference"
    d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
    k, num_codes, n_pos = args.k, args.codes, batch * length
    torch.manual_seed(0)
    vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
    with torch.no_grad():
        vq.codebook.weight.normal_()
    vq = vq.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    sizes = [hi - lo for lo, hi in (vq._region(t) for t in TYPES)]
    tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen, device=dev) for s in sizes], 1).contiguous()
    weights = torch.softmax(torch.randn(num_codes, 4, k, generator=gen, device=dev), -1).contiguous()
    module = MedTokEmbedding(vq, tokens, weights, projector=torch.nn.Linear(4 * d, h).to(dev), fold=True)
    del tokens, weights
    index = torch.randint(0, num_codes, (batch, length), generator=gen, device=dev)
    u = torch.rand(batch, length, generator=gen, device=dev)
    index[u < args.miss] = num_codes
    mask = u > 1.0 - args.padded
    index[mask] = 0                                         # (the reference's dataloader pads with code 0 under its code_mask)
    seg = torch.randint(0, n_seg, (batch, length), generator=gen, device=dev).sort(1).values      # visits in time order
    rnd = lambda *shape: torch.randn(*shape, generator=gen, device=dev)
    pe, t0, t1, prefix = rnd(length, h), rnd(batch, n_seg, h), rnd(batch, n_seg, h), rnd(batch, n_prefix, h)
    g_out = rnd(batch, n_prefix + length, h)
    gather_at = seg.unsqueeze(-1).expand(-1, -1, h)
    leaves = [pe, t0, t1, prefix]
    outs = {}

    def sequence(dtype):
        return module.sequence(index, mask, position_rows=pe, segment_id=seg, segment_rows=[t0, t1], prefix=prefix, validate=False, out_dtype=dtype)[0]

    def composition():
        x = module(index, padding_mask=mask, validate=False)
        x = x + pe[:length]
        x = x + t0.gather(1, gather_at)
        x = x + t1.gather(1, gather_at)
        return torch.cat([prefix, x], 1)

    def sequence_f32():
        with torch.no_grad():
            outs["sequence_f32"] = sequence(torch.float32)

    def sequence_bf16():
        with torch.no_grad():
            outs["sequence_bf16"] = sequence(torch.bfloat16)

    def composition_f32():
        with torch.no_grad():
            outs["composition_f32"] = composition()

    def composition_bf16():
        with torch.no_grad():
            outs["composition_bf16"] = composition().to(torch.bfloat16)

    def step(fn):
        module.zero_grad(set_to_none=True)
        for t in leaves:
            t.grad = None
        fn().backward(g_out)

    def sequence_step():
        step(lambda: sequence(torch.float32))

    def composition_step():
        step(composition)

    sides = {"sequence_f32": sequence_f32, "composition_f32": composition_f32, "sequence_bf16": sequence_bf16, "composition_bf16": composition_bf16}
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    live = ~mask
    got, want = outs["sequence_f32"], outs["composition_f32"]
    bias_rows = module.projector.bias.detach().expand(int(mask.sum()), -1)
    equal = (torch.equal(got[:, :n_prefix], want[:, :n_prefix]) and torch.equal(got[:, n_prefix:][live], want[:, n_prefix:][live])
             and torch.equal(got[:, n_prefix:][mask], bias_rows) and torch.equal(outs["sequence_bf16"], got.to(torch.bfloat16)))
    if not equal:
        raise SystemExit("sequence and the composition disagree at the timed size")
    for t in leaves:
        t.requires_grad_(True)
    sides.update(sequence_step=sequence_step, composition_step=composition_step)
    grads = {}
    for _ in range(args.warmup):
        for s in ("sequence_step", "composition_step"):
            sides[s]()
            grads[s] = [t.grad.clone() for t in leaves]
    torch.cuda.synchronize()
    # the composition's gradients also hold the padded positions' contributions (it adds there too) and come from atomics: reported, not asserted
    grad_rel = [float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) for a, b in zip(grads["sequence_step"], grads["composition_step"])]
    inner = {s: inner_for(fn) for s, fn in sides.items()}
    ms = {s: [] for s in sides}
    for _ in range(args.reps):                              # the sides alternate
        for s, fn in sides.items():
            ms[s].append(timed(fn, inner[s]))
    with ops.ClockProbe(dev, max_seconds=10.0) as probe:
        for _ in range(max(2, args.reps // 4)):
            timed(sequence_f32, inner["sequence_f32"])
    clock = probe.result()
    st = {s: stats(v) for s, v in ms.items()}
    rows, hp = module.fold_table_shape()
    tensor_bytes = n_pos * h * 4
    entry = {"d": d, "n_e": n_e, "k": k, "H": h, "num_codes": num_codes, "batch": batch, "length": length, "visits": n_seg, "prefix_rows": n_prefix,
             "positions": n_pos, "live_positions": int((live & (index < num_codes)).sum()), "padded_fraction": args.padded,
             "miss_fraction": args.miss, "table_rows": rows, "activation_bytes": tensor_bytes,
             "outputs_bit_equal_fp32": equal, "step_grad_rel_vs_composition": dict(zip(("position_rows", "segment_rows0", "segment_rows1", "prefix"), grad_rel)),
             "step_grad_note": "the composition adds the terms at padded positions too, so its gradients of the additive rows hold those positions' "
                               "upstream rows as well: the two differ by design",
             "clock_ghz": clock.get("ghz_mean"), "clock_region": "further sequence_f32 samples right behind the timed region"}
    for s in sides:
        entry[s] = dict(st[s], calls_per_sample=inner[s], spread=(st[s]["ms_max"] - st[s]["ms_min"]) / st[s]["ms_median"],
                        positions_per_s=n_pos / (st[s]["ms_median"] * 1e-3))
    for a, b in (("sequence_f32", "composition_f32"), ("sequence_bf16", "composition_bf16"), ("sequence_step", "composition_step")):
        entry[f"{a}_speedup_over_composition"] = st[b]["ms_median"] / st[a]["ms_median"]
        entry[f"{a}_not_slower_within_spread"] = st[a]["ms_median"] <= st[b]["ms_median"] + (st[b]["ms_max"] - st[b]["ms_min"])
    result = {"tool": "tools/bench_embed.py --sequence", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
              "shapes": {name: entry}}
    if args.out:
        path = Path(args.out)
        whole = json.loads(path.read_text()) if path.exists() else {}
        whole["sequence"] = result
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(result))


def segments_mode(args, dev, timed, inner_for, stats):
    import torch
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    n_seg, batch, length = args.visits, args.batch, args.length
    name = "reference"
    d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
    k, num_codes, n_pos, width = args.k, args.codes, batch * length, 4 * d
    torch.manual_seed(0)
    vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
    with torch.no_grad():
        vq.codebook.weight.normal_()
    vq = vq.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    sizes = [hi - lo for lo, hi in (vq._region(t) for t in TYPES)]
    tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen, device=dev) for s in sizes], 1).contiguous()
    weights = torch.softmax(torch.randn(num_codes, 4, k, generator=gen, device=dev), -1).contiguous()
    module = MedTokEmbedding(vq, tokens, weights)
    del tokens, weights
    index = torch.randint(0, num_codes, (batch, length), generator=gen, device=dev)
    u = torch.rand(batch, length, generator=gen, device=dev)
    index[u < args.miss] = num_codes
    mask = u > 1.0 - args.padded
    index[mask] = 0                                         # (the reference's dataloader pads with code 0 under its code_mask)
    ascending = torch.randint(0, n_seg, (batch, length), generator=gen, device=dev).sort(1).values      # visits in time order
    shuffled = ascending.gather(1, torch.rand(batch, length, generator=gen, device=dev).argsort(1))
    live = ~mask
    row_base = (torch.arange(batch, device=dev) * n_seg).view(-1, 1)
    result = {"tool": "tools/bench_embed.py --segments", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
              "chunk": ops.EMBED_POOL_CHUNK, "samples_of_at_least_ms": 50.0,
              "expectation": "stated before measuring: pooled_segments is not slower than either composition by more than that composition's "
                             "own run-to-run spread (median <= median + (max - min)); no speed-up is fixed in advance",
              "shapes": {}}

    def inner_for(fn):                                      # pool_mode's: samples of >= 50 ms (aimed at 65), the count corrected on samples
        inner = 10                                          # of its own size (the first calls are slower than the steady ones)
        for _ in range(6):
            sample = timed(fn, inner) * inner
            if sample >= 60.0 or inner >= 50000:
                break
            inner = max(inner + 1, min(50000, math.ceil(inner * 65.0 / max(sample, 1e-3))))
        return inner

    for case, seg in (("ascending", ascending), ("shuffled", shuffled)):
        key = torch.where(live, row_base + seg, torch.full_like(seg, batch * n_seg)).reshape(-1)        # dead: one bin past the bags
        outs = {}

        def counts():
            return torch.zeros(batch * n_seg + 1, device=dev).index_add_(0, key, live.reshape(-1).float())[:-1].view(batch, n_seg, 1)

        def finish(sums):
            c = counts()
            return torch.where(c > 0, sums / c.clamp(min=1.0), torch.zeros_like(sums)), c.squeeze(-1) == 0

        def pooled_segments():
            with torch.no_grad():
                outs["pooled_segments"] = module.pooled_segments(index, seg, n_seg, padding_mask=mask, validate=False)

        def composition_segment_grad():
            with torch.no_grad():
                rows = module(index, padding_mask=mask, validate=False)
                outs["composition_segment_grad"] = finish(ops.embed_sequence_segment_grad(rows, seg, n_seg, mask))

        def composition_index_add():
            with torch.no_grad():
                rows = module(index, padding_mask=mask, validate=False)
                sums = torch.zeros(batch * n_seg + 1, width, device=dev).index_add_(0, key, rows.view(-1, width))[:-1]
                outs["composition_index_add"] = finish(sums.view(batch, n_seg, width))

        sides = {"pooled_segments": pooled_segments, "composition_segment_grad": composition_segment_grad,
                 "composition_index_add": composition_index_add}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        got, empty = outs["pooled_segments"]
        rel = {}
        for s in ("composition_segment_grad", "composition_index_add"):
            want, want_empty = outs[s]
            rel[s] = float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))
            if rel[s] > 1e-5 or not torch.equal(empty, want_empty):
                raise SystemExit(f"pooled_segments and {s} disagree at the timed size ({case}): rel {rel[s]:.3e}")
        peak = {}
        for s, fn in sides.items():
            outs.clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[s] = torch.cuda.max_memory_allocated() - before
        inner = {s: inner_for(fn) for s, fn in sides.items()}
        ms = {s: [] for s in sides}
        for _ in range(args.reps):                          # the sides alternate
            for s, fn in sides.items():
                ms[s].append(timed(fn, inner[s]))
        with ops.ClockProbe(dev, max_seconds=10.0) as probe:
            for _ in range(max(2, args.reps // 4)):
                timed(pooled_segments, inner["pooled_segments"])
        clock = probe.result()
        st = {s: stats(v) for s, v in ms.items()}
        seg_len = (~empty).sum().clamp(min=1)
        entry = {"d": d, "n_e": n_e, "k": k, "num_codes": num_codes, "batch": batch, "length": length, "visits": n_seg, "width": width,
                 "positions": n_pos, "live_positions": int(live.sum()), "padded_fraction": args.padded, "miss_fraction": args.miss,
                 "normalize": False, "non_empty_segments": int((~empty).sum()), "mean_positions_per_non_empty_segment": float(live.sum() / seg_len),
                 "rows_bytes": n_pos * width * 4, "out_bytes": batch * n_seg * width * 4,
                 "workspace_bytes": int(ops._lib.load().medtok_embed_pool_segments_workspace_bytes(batch, length, n_seg, width)),
                 "rel_vs": rel, "empty_masks_equal": True, "shortest_sample_ms": min(min(ms[s_]) * inner[s_] for s_ in sides),
                 "clock_ghz": clock.get("ghz_mean"), "clock_region": "further pooled_segments samples right behind the timed region"}
        for s in sides:
            entry[s] = dict(st[s], calls_per_sample=inner[s], spread=(st[s]["ms_max"] - st[s]["ms_min"]) / st[s]["ms_median"], peak_bytes=peak[s],
                            positions_per_s=n_pos / (st[s]["ms_median"] * 1e-3))
        a = "pooled_segments"
        for b in ("composition_segment_grad", "composition_index_add"):
            entry[f"speedup_over_{b}"] = st[b]["ms_median"] / st[a]["ms_median"]
            entry[f"pooled_segments_not_slower_within_spread_of_{b}"] = st[a]["ms_median"] <= st[b]["ms_median"] + (st[b]["ms_max"] - st[b]["ms_min"])
            entry[f"peak_bytes_saved_vs_{b}"] = peak[b] - peak[a]
        result["shapes"][case] = entry
    if args.out:
        path = Path(args.out)
        whole = json.loads(path.read_text()) if path.exists() else {}
        whole["segments"] = result
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(result))


def grad_form_mode(args, dev, timed, inner_for, stats):
    import torch
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    seq, train = bool(args.sequence), args.train_codebook
    h = args.sequence or args.project
    form = "sequence" if seq else "project_training" if train else "project_frozen"
    batch, length, k, num_codes, n_pos = args.batch, args.length, args.k, args.codes, args.batch * args.length
    result = {"tool": f"tools/bench_embed.py --{'sequence' if seq else 'project'} {h} --grad-form" + (" --train-codebook" if train else ""),
              "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "num_codes": num_codes,
              "positions": [batch, length], "slots": 4, "k": k, "H": h, "padded_fraction": args.padded, "miss_fraction": args.miss,
              "chunk": ops.EMBED_CODE_GRAD_CHUNK, "cases": {}}
    for name in (["reference"] if seq else args.shapes.split(",")):
        d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
        torch.manual_seed(0)
        vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
        with torch.no_grad():
            vq.codebook.weight.normal_()
        vq = vq.to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(1)
        sizes = [hi - lo for lo, hi in (vq._region(t) for t in TYPES)]
        tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen, device=dev) for s in sizes], 1).contiguous()
        weights = torch.softmax(torch.randn(num_codes, 4, k, generator=gen, device=dev), -1).contiguous()
        proj = torch.nn.Linear(4 * d, h).to(dev)
        kw = dict(projector=proj, fold=True, freeze_codebook=not train)
        mods = {"scatter": MedTokEmbedding(vq, tokens, weights, grad_form="scatter", **kw)}
        mods["dense"] = MedTokEmbedding(vq, tokens, weights, grad_form="dense", **kw)
        mods["dense"].tokens, mods["dense"].weights, mods["dense"].miss_emb = mods["scatter"].tokens, mods["scatter"].weights, mods["scatter"].miss_emb
        plain = MedTokEmbedding(vq, tokens, weights)            # (the fp64 restatement of dW takes its rows from the lookup kernel)
        plain.tokens, plain.weights, plain.miss_emb = mods["scatter"].tokens, mods["scatter"].weights, mods["scatter"].miss_emb
        del tokens, weights
        rnd = lambda *shape: torch.randn(*shape, generator=gen, device=dev)
        n_prefix = args.prefix if seq else 0
        g_out = rnd(batch, n_prefix + length, h)
        leaves = []
        if seq:
            seg = torch.randint(0, args.visits, (batch, length), generator=gen, device=dev).sort(1).values
            leaves = [rnd(length, h), rnd(batch, args.visits, h), rnd(batch, args.visits, h), rnd(batch, n_prefix, h)]
            for t in leaves:
                t.requires_grad_(True)
        params = [proj.weight, proj.bias, mods["scatter"].miss_emb] + ([vq.codebook.weight] if train else [])
        for variant in (("random", "hot") if train else ("random",)):
            index = torch.randint(0, num_codes, (batch, length), generator=gen, device=dev)
            u = torch.rand(batch, length, generator=gen, device=dev)
            if variant == "hot":                                # half the live positions on one code
                index[torch.rand(batch, length, generator=gen, device=dev) < 0.5] = 7
            index[u < args.miss] = num_codes
            mask = u > 1.0 - args.padded
            index[mask] = 0
            outs, grads = {}, {}

            def step(side):
                m = mods[side]
                for t in params + leaves:
                    t.grad = None
                if seq:
                    out = m.sequence(index, mask, position_rows=leaves[0], segment_id=seg, segment_rows=leaves[1:3], prefix=leaves[3], validate=False)[0]
                else:
                    out = m(index, padding_mask=mask, validate=False)
                out.backward(g_out)
                outs[side] = out.detach()
                grads[side] = [t.grad for t in params + leaves]

            def scatter_refold():                               # what a step after an optimiser step pays: the tables folded again
                mods["scatter"].__dict__["_fold_cache"] = None
                step("scatter")

            sides = {"scatter": lambda: step("scatter"), "dense": lambda: step("dense")}
            if train:
                sides["scatter_refold"] = scatter_refold
            peak = {}
            for _ in range(args.warmup):
                for s, fn in sides.items():
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    fn()
                    torch.cuda.synchronize()
                    peak[s] = torch.cuda.max_memory_allocated() - before
            out_rel = float((outs["scatter"] - outs["dense"]).abs().max() / outs["dense"].abs().max())
            if not (out_rel <= 1e-5 and (train or torch.equal(outs["scatter"], outs["dense"]))):
                raise SystemExit(f"{name}/{variant}: the outputs of the two forms disagree (rel {out_rel})")
            names = ["dW", "db", "d_miss"] + (["d_codebook"] if train else []) + (["d_position_rows", "d_segment_rows0", "d_segment_rows1", "d_prefix"] if seq else [])
            grad_rel = {nm: float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) for nm, a, b in zip(names, grads["scatter"], grads["dense"])}
            # dW against its fp64 restatement g^T . emb (emb: the lookup kernel's fp32 rows).  An entry of dW sums up to n_pos products, in
            # two different fp32 orders on the two sides: their rounding alone reaches sqrt(n_pos) * 2^-24 ~ 2e-5 to 4e-5 of the scale
            # at these sizes, so dW is held to 1e-4 of the fp64 result (a wrong gradient is off by order 1) and both errors are
            # recorded; every other gradient is held to 1e-5 between the sides.
            with torch.no_grad():
                dw64 = torch.zeros(h, 4 * d, dtype=torch.float64, device=dev)
                flat_i, flat_m, flat_g = index.reshape(-1), mask.reshape(-1), g_out[:, n_prefix:].reshape(n_pos, h)
                for r0 in range(0, n_pos, 32768):
                    emb = plain(flat_i[r0:r0 + 32768], padding_mask=flat_m[r0:r0 + 32768], validate=False).double()
                    dw64 += flat_g[r0:r0 + 32768].double().t() @ emb
                dw_rel64 = {s: float((grads[s][0] - dw64).abs().max() / dw64.abs().max()) for s in ("scatter", "dense")}
                del dw64, emb
            if not max(v for nm, v in grad_rel.items() if nm != "dW") <= 1e-5 or not max(dw_rel64.values()) <= 1e-4:
                raise SystemExit(f"{name}/{variant}: the gradients of the two forms disagree: {grad_rel}; dW against fp64: {dw_rel64}")
            folded = mods["scatter"]._folded(vq._normalised_codebook())
            g_rows = g_out[:, n_prefix:].contiguous()
            if g_rows.shape[-1] != folded[0].shape[1]:
                g_rows = torch.nn.functional.pad(g_rows, (0, folded[0].shape[1] - g_rows.shape[-1]))
            sides["table_grad"] = lambda: ops.embed_project_table_grad(g_rows, index, mods["scatter"].tokens, mods["scatter"].weights, folded[1], pad_mask=mask)
            sides["table_grad"]()
            inner = {s: inner_for(fn) for s, fn in sides.items()}
            ms = {s: [] for s in sides}
            for _ in range(args.reps):                          # the sides alternate
                for s, fn in sides.items():
                    ms[s].append(timed(fn, inner[s]))
            with ops.ClockProbe(dev, max_seconds=10.0) as probe:
                for _ in range(max(2, args.reps // 4)):
                    timed(sides["scatter"], inner["scatter"])
            clock = probe.result()
            st = {s: stats(v) for s, v in ms.items()}
            rows, hp = mods["scatter"].fold_table_shape()
            entry = {"d": d, "n_e": n_e, "k": k, "H": h, "num_codes": num_codes, "positions": n_pos,
                     "live_positions": int((~mask & (index < num_codes)).sum()), "table_rows": rows,
                     "dense_weight_grad_flops": 2 * n_pos * 4 * d * h, "scatter_weight_grad_flops": 2 * rows * d * h,
                     "activation_bytes": n_pos * 4 * d * 4, "table_grad_workspace_bytes": ops._lib.load().medtok_embed_table_grad_workspace_bytes(n_pos, 4, k, rows, hp),
                     "out_rel_scatter_vs_dense": out_rel, "outputs_bit_equal": bool(torch.equal(outs["scatter"], outs["dense"])),
                     "grad_rel_scatter_vs_dense": grad_rel, "dW_rel_vs_fp64": dw_rel64, "fold_builds": {s: mods[s].fold_builds for s in mods},
                     "table_grad_ms": st["table_grad"]["ms_median"], "sort_share_of_table_grad": None,
                     "clock_ghz": clock.get("ghz_mean"), "clock_region": "further scatter samples right behind the timed region"}
            for s in (s for s in sides if s != "table_grad"):
                entry[s] = dict(st[s], calls_per_sample=inner[s], spread=(st[s]["ms_max"] - st[s]["ms_min"]) / st[s]["ms_median"],
                                peak_bytes=peak[s], positions_per_s=n_pos / (st[s]["ms_median"] * 1e-3))
            entry["scatter_speedup_over_dense"] = st["dense"]["ms_median"] / st["scatter"]["ms_median"]
            entry["scatter_not_slower_within_dense_spread"] = st["scatter"]["ms_median"] <= st["dense"]["ms_median"] + (st["dense"]["ms_max"] - st["dense"]["ms_min"])
            entry["scatter_peak_smaller_than_dense"] = peak["scatter"] < peak["dense"]
            if train:
                entry["scatter_refold_not_slower_within_dense_spread"] = (st["scatter_refold"]["ms_median"] <= st["dense"]["ms_median"]
                                                                          + (st["dense"]["ms_max"] - st["dense"]["ms_min"]))
            result["cases"][f"{name}/{variant}" if train else name] = entry
            for t in params + leaves:
                t.grad = None
            del outs, grads, index, mask, sides, g_rows, folded
            torch.cuda.empty_cache()
        del mods, plain, g_out, leaves, params
        torch.cuda.empty_cache()
    if args.out:
        path = Path(args.out)
        whole = json.loads(path.read_text()) if path.exists() else {}
        whole.setdefault("table_grad", {})[form] = result
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
