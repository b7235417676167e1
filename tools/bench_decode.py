"""Time decode -- (token ids, weights) -> embeddings -- on one MI355X against the same decode written as a torch expression.

    python tools/bench_decode.py [--rows 600000] [--reps 20] [--warmup 3] [--out profiles/decode_bench.json]

Prints ONE JSON line.  Two shapes (S = 4 slots, k = 5): cfg 3 (D = 768, n_e = 49152; the output is rows x 3072 floats, 7.4 GB at
600k rows) and the reference shape (D = 64, n_e = 21000).  Per shape and per side:

  kernel   VectorQuantizer.decode(tokens, weights, out=..., validate=False): one launch for all four slots
  torch    per slot  out[:, s] = (w.unsqueeze(-1) * what[ids]).sum(1)  on the same GPU, same process, same inputs, chunked over the
           rows (the expression materialises [rows, k, D] twice; --chunk-rows, default 131072, keeps that at 2 x 2 GB at D = 768)

Discipline (bench.py's): warm-up of both sides at the timed shape, device events around every timed sample, a sample is `inner`
back-to-back calls so that it lasts >= 50 ms, the two sides ALTERNATE sample by sample, at least 20 samples each; the shader clock
(ops.ClockProbe) of further kernel samples right behind the timed region.  Algorithmic bytes = rows * S * (12 k + 4 D) + the codebook
once; their rate is given as a fraction of the 6.29 TB/s a float4 copy reaches on this chip (8.0 TB/s is the HBM3E spec).  The
outputs of the two sides are compared before anything is timed.

Backward (time only): decode + sum-of-products loss + backward through the library's kernels against the same expression under
torch autograd (fp32), at --backward-rows rows (default 65536: the per-(row, slot, j) code-gradient buffer is rows * S * k * D floats).
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
SHAPES = {"cfg3": dict(d=768, n_e=49152), "reference": dict(d=64, n_e=21000)}
TYPES = ("text", "graph", "shared", "shared")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=600000)
    ap.add_argument("--backward-rows", type=int, default=65536)
    ap.add_argument("--chunk-rows", type=int, default=131072)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="cfg3,reference")
    ap.add_argument("--no-backward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    import torch.nn.functional as F
    from medtok_amd import ops
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode needs an MI355X: there is nothing to time without one")
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
        return max(1, min(50, math.ceil(50.0 / max(t, 1e-3))))

    def stats(ms):
        return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), ms_mean=statistics.fmean(ms), samples=len(ms))

    def inputs(vq, rows, k, seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        sizes = [hi - lo for lo, hi in (vq._region(t) for t in TYPES)]
        tokens = torch.stack([torch.randint(0, s, (rows, k), generator=gen, device=dev) for s in sizes], 1).contiguous()
        weights = torch.softmax(torch.randn(rows, 4, k, generator=gen, device=dev), -1).contiguous()
        return tokens, weights

    result = {"tool": "tools/bench_decode.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
              "slots": 4, "k": args.k, "hbm_roof_tb_s": HBM_MEASURED_TBS, "hbm_spec_tb_s": HBM_SPEC_TBS, "shapes": {}}
    for name in args.shapes.split(","):
        d, n_e = SHAPES[name]["d"], SHAPES[name]["n_e"]
        rows, k = args.rows, args.k
        torch.manual_seed(0)
        vq = VectorQuantizer(n_e, d, 0.25, 0.0, True, False, [d, d], k=k)
        with torch.no_grad():
            vq.codebook.weight.normal_()
        vq = vq.to(dev).eval()
        los = [vq._region(t)[0] for t in TYPES]
        tokens, weights = inputs(vq, rows, k, 1)
        out_k = torch.empty(rows, 4 * d, device=dev)
        out_t = torch.empty(rows, 4 * d, device=dev)
        with torch.no_grad():
            what = vq._normalised_codebook()[0]

        def kernel():
            vq.decode(tokens, weights, out=out_k, validate=False)

        def expression():
            for r0 in range(0, rows, args.chunk_rows):
                r1 = min(rows, r0 + args.chunk_rows)
                for s in range(4):
                    out_t[r0:r1, s * d:(s + 1) * d] = (weights[r0:r1, s].unsqueeze(-1) * what[tokens[r0:r1, s] + los[s]]).sum(1)

        with torch.no_grad():
            for _ in range(args.warmup):
                kernel(), expression()
            torch.cuda.synchronize()
            diff = float((out_k[:65536] - out_t[:65536]).abs().max() / out_t[:65536].abs().max())
            if not diff <= 1e-5:
                raise SystemExit(f"{name}: kernel and torch expression disagree (rel {diff})")
            ik, it = inner_for(kernel), inner_for(expression)
            ms_k, ms_t = [], []
            for _ in range(args.reps):                  # the two sides alternate
                ms_k.append(timed(kernel, ik))
                ms_t.append(timed(expression, it))
            with ops.ClockProbe(dev, max_seconds=10.0) as probe:
                for _ in range(max(2, args.reps // 4)):
                    timed(kernel, ik)
            clock = probe.result()
        alg_bytes = rows * 4 * (12 * k + 4 * d) + n_e * d * 4
        sk, st = stats(ms_k), stats(ms_t)
        tbs = alg_bytes / (sk["ms_median"] * 1e-3) / 1e12
        entry = {"rows": rows, "d": d, "n_e": n_e, "k": k, "output_gb": rows * 4 * d * 4 / 1e9, "algorithmic_bytes": alg_bytes,
                 "kernel": dict(sk, calls_per_sample=ik, rows_per_s=rows / (sk["ms_median"] * 1e-3), algorithmic_tb_s=tbs,
                                frac_of_hbm_roof=tbs / HBM_MEASURED_TBS, frac_of_hbm_spec=tbs / HBM_SPEC_TBS,
                                kernel_chunked=False),
                 "torch_expression": dict(st, calls_per_sample=it, rows_per_s=rows / (st["ms_median"] * 1e-3), chunk_rows=args.chunk_rows),
                 "speedup_over_torch_expression": st["ms_median"] / sk["ms_median"],
                 "kernel_at_least_as_fast": sk["ms_median"] <= st["ms_median"],
                 "max_rel_diff_kernel_vs_torch": diff,
                 "clock_ghz": clock.get("ghz_mean"), "clock_ghz_min": clock.get("ghz_min"), "clock_ghz_max": clock.get("ghz_max"),
                 "clock_region": "further kernel samples right behind the timed region"}
        del out_k, out_t, tokens, weights
        torch.cuda.empty_cache()

        if not args.no_backward:
            rb = min(args.backward_rows, rows)
            tokens, weights = inputs(vq, rb, k, 2)
            probe_t = torch.randn(rb, 4 * d, device=dev)
            W = vq.codebook.weight
            lo_t = torch.tensor(los, device=dev).view(1, 4, 1)
            ids = tokens + lo_t

            def lib_step():
                W.grad = None
                w = weights.detach().requires_grad_(True)
                (vq.decode(tokens, w, validate=False) * probe_t).sum().backward()

            def torch_step():
                W.grad = None
                w = weights.detach().requires_grad_(True)
                ((w.unsqueeze(-1) * F.normalize(W, dim=-1)[ids]).sum(2).reshape(rb, -1) * probe_t).sum().backward()

            for _ in range(args.warmup):
                lib_step(), torch_step()
            torch.cuda.synchronize()
            il, ib = inner_for(lib_step), inner_for(torch_step)
            ms_l, ms_b = [], []
            for _ in range(args.reps):
                ms_l.append(timed(lib_step, il))
                ms_b.append(timed(torch_step, ib))
            sl, sb = stats(ms_l), stats(ms_b)
            entry["forward_backward"] = {"rows": rb, "what": "decode + sum-of-products loss + backward to weights and codebook.weight",
                                         "kernels": dict(sl, calls_per_sample=il), "torch_autograd_fp32": dict(sb, calls_per_sample=ib),
                                         "speedup_over_torch_autograd": sb["ms_median"] / sl["ms_median"]}
            W.grad = None
            del tokens, weights, probe_t, ids
            torch.cuda.empty_cache()
        result["shapes"][name] = entry
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
