"""Dev tool: VALUE mutants of the half-precision attention backward (attention_backward.h: shared_kv_attention_dq_kernel and
shared_kv_attention_dkv_kernel with HM = 1 / 2, att_accumulate_hh, att_cvt16, att_pack8), made by text substitution on a copy of the
sources (tools/mutants_operand_images.py's pattern), into devlib/<name>/libmedtok_vq.so (git-ignored), and bound for a test session
through MEDTOK_TEST_LIB (tests/conftest.py).

    python tools/mutants_attention_half.py build [name ...]      # compile (all by default)
    python tools/mutants_attention_half.py run [name ...]        # on the GPU box: the test selections once against each built mutant

Every mutant changes VALUES only: none changes a global or LDS address outside what the original reads, widens an access, or touches a
launch shape or a barrier (lse_row / del_row read another entry of the same 32-entry statistic array the original reads) -- a mutated
library can compute wrong numbers, never fault.  tests/test_gpu_attention_half_backward.py must FAIL on each of them (DESIGN.md,
section 6, has the table); what the older 4e-3 / 4e-2 tests of tests/test_gpu_kernels.py made of them is recorded beside it.

  cvt_trunc      att_cvt16<true> and att_pack8<true>: bf16 by truncation instead of round-to-nearest-even
  ds_keepscale   dKV half loop: dp = keep ? dp : 0 -- the kept entries of dP lose their 1 / (1 - p)
  dq_keepscale   dQ kernel: the same
  lse_row        dKV half loop: every query column of a thread reads lse_s[qc] instead of lse_s[qc + j]
  del_row        dKV half loop: the same for del_s
  tail_p         dKV half loop: "key < kl && qr < ql" -> "key < kl": the clamped tail query rows of a chunk contribute
  acc_half_k     att_accumulate_hh: zeros as the A operand of st == 1 -- the upper 16 of a chunk's 32 contraction rows are dropped
  src_scale      multi-source loop: sources after the first keep source 0's scale
"""
import os
import shutil
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from medtok_amd.csrc import build as B

_TRUNC_PACK = ("if constexpr (BF) { const __bf16 b = (__bf16)v[e]; r[e] = __builtin_bit_cast(unsigned short, b); }",
               "if constexpr (BF) { r[e] = (unsigned short)(__float_as_uint(v[e]) >> 16); }")
_TRUNC_CVT = ("if constexpr (BF) { const __bf16 b = (__bf16)v; return __builtin_bit_cast(unsigned short, b); }",
              "if constexpr (BF) { return (unsigned short)(__float_as_uint(v) >> 16); }")
# (the half loop of the dKV kernel is indented four columns deeper than the fp32 loop: the leading newline + 16 blanks pick it)
_HALF_P = "\n                p[j] = (key < kl && qr < ql) ? expf(a * scale - lse_s[qc + j]) : 0.f;"
MUTANTS = {
    "cvt_trunc": [_TRUNC_PACK, _TRUNC_CVT],
    "ds_keepscale": [("\n                dp = keep[j] ? dp * keep_scale : 0.f;", "\n                dp = keep[j] ? dp : 0.f;")],
    "dq_keepscale": [("if (drop_thresh) dp = att_keep(seed, qs + qt * 32 + row, key, drop_thresh) ? dp * keep_scale : 0.f;",
                      "if (drop_thresh) dp = att_keep(seed, qs + qt * 32 + row, key, drop_thresh) ? dp : 0.f;")],
    "lse_row": [(_HALF_P, _HALF_P.replace("lse_s[qc + j]", "lse_s[qc]"))],
    "del_row": [("\n                ds[qc + j][krow_t] = p[j] * (dp - del_s[qc + j]) * scale;",
                 "\n                ds[qc + j][krow_t] = p[j] * (dp - del_s[qc]) * scale;")],
    "tail_p": [(_HALF_P, _HALF_P.replace("key < kl && qr < ql", "key < kl"))],
    "acc_half_k": [("        const half8 a = att_pack8<BF>(av);\n#pragma unroll\n        for (int t = 0; t < NT; ++t) {\n            // (rows + 16 st:",
                    "        if (st == 1) {\n#pragma unroll\n            for (int e = 0; e < 8; ++e) av[e] = 0.f;\n        }\n"
                    "        const half8 a = att_pack8<BF>(av);\n#pragma unroll\n        for (int t = 0; t < NT; ++t) {\n            // (rows + 16 st:")],
    "src_scale": [("scale = src.scale; keep_scale = src.keep_scale;", "if (si == 0) scale = src.scale; keep_scale = src.keep_scale;")],
}
# (test file, -k selection): the new module, and the tests that ran the half-precision backward before it
SELECTIONS = (("tests/test_gpu_attention_half_backward.py", None),
              ("tests/test_gpu_kernels.py", "one_half_precision_pass or several_attention_calls or accumulates_key_gradient"))


def build(names):
    for name in names:
        out = ROOT / "devlib" / name
        src = out / "src" / "medtok_amd" / "csrc"
        if out.exists():
            shutil.rmtree(out)
        src.mkdir(parents=True)
        for p in B.HERE.glob("*.h"):
            shutil.copy(p, src / p.name)
        shutil.copy(B.SRC, src / B.SRC.name)
        (out / "src" / "include").mkdir()
        shutil.copy(B.HEADER, out / "src" / "include" / B.HEADER.name)
        f = src / "attention_backward.h"
        text = f.read_text()
        for old, new in MUTANTS[name]:
            assert text.count(old) == 1, f"{name}: pattern found {text.count(old)} times: {old[:60]!r}"
            text = text.replace(old, new)
        f.write_text(text)
        so = out / "libmedtok_vq.so"
        subprocess.check_call([B.hipcc(), *B.FLAGS, str(src / B.SRC.name), "-o", str(so)])
        shutil.rmtree(out / "src")
        print("built", so, flush=True)


def run(names, limit=300):
    """each selection once against each mutant, each session under its own time limit; a session that did not end as a pytest
    session ends (0: nothing failed, 1: tests failed) ends the whole run: nothing more is started on that GPU"""
    for name in names:
        so = ROOT / "devlib" / name / "libmedtok_vq.so"
        if not so.exists():
            raise SystemExit(f"{so}: not built")
        for tf, pick in SELECTIONS:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", tf, "-m", "gpu", "-q", "-rf", "--tb=no", "-p", "no:cacheprovider"]
            r = subprocess.run(cmd + (["-k", pick] if pick else []), cwd=ROOT, env=dict(os.environ, MEDTOK_TEST_LIB=str(so)),
                               capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("FAILED ")]
            failed = sorted({ln.split(" ")[1].split("::")[1].split("[")[0] for ln in lines})
            cases = sorted({ln.split(" ")[1].split("::")[1] for ln in lines})
            tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
            print(f"MUTANT {name} | {tf} | exit {r.returncode} | {tail} | failed: {', '.join(failed) or '-'}", flush=True)
            print(f"MUTANT_CASES {name} | {tf} | {' '.join(cases) or '-'}", flush=True)
            if r.returncode not in (0, 1):
                print(r.stdout[-3000:], r.stderr[-3000:])
                raise SystemExit(f"{name} / {tf}: the session ended with status {r.returncode}; stopping")


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("build", "run"):
        raise SystemExit(__doc__)
    picked = sys.argv[2:] or list(MUTANTS)
    for n_ in picked:
        if n_ not in MUTANTS:
            raise SystemExit(f"unknown mutant {n_}; known: {', '.join(MUTANTS)}")
    (build if sys.argv[1] == "build" else run)(picked)
