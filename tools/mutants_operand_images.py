"""Dev tool: VALUE mutants of the operand-image kernels (split_gemm.h: half_image_kernel, half_image_t_kernel, split_half_t_kernel,
absmax_kernel, pow2_prescale), made by text substitution on a copy of the sources (tools/r05/build_mutants.py's pattern), into
devlib/<name>/libmedtok_vq.so (git-ignored), and bound for a test session through MEDTOK_TEST_LIB (tests/conftest.py).

    python tools/mutants_operand_images.py build [name ...]      # compile (all by default)
    python tools/mutants_operand_images.py run [name ...]        # on the GPU box: both test files once against each built mutant

Every mutant changes VALUES only: none changes an address, widens an access, or touches a launch shape or a barrier -- a mutated
library can compute wrong numbers, never fault.  tests/test_gpu_operand_images.py must FAIL on each of them (DESIGN.md has the
table); what tests/test_gpu_split_gemm.py made of them is recorded beside it.

  bf16_trunc     half_bits<BF>: the bf16 image by truncation instead of round-to-nearest-even
  img_drop4      half_image_kernel: the first float4 of a group of 8 is read only where the second one starts below d ("c + 4 < d" in
                 place of "c < d"): the last four columns are zero when d % 8 == 4
  img_c8_equiv   half_image_kernel: "c + 4 < d" -> "c + 8 <= d" on the second float4.  EQUIVALENT, kept as a record: c is a multiple of
                 8 and the entry point requires d % 4 == 0, so both conditions hold for exactly the same (c, d); no test can fail on it
  sums_noshfl2   half_image_t_kernel: the column sums combine two of the four 16-row sums only
  tile_fill1     half_image_t_kernel: rows past n and columns past d of the tile are 1.f, not 0.f
  clamp127       pow2_prescale: upper clamp of the exponent 127 instead of 126
  absmax_tail    absmax_kernel: the scalar tail stops one element early
  t_lo_zero      split_half_t_kernel: the lo image is written as zero
"""
import os
import shutil
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from medtok_amd.csrc import build as B

MUTANTS = {
    "bf16_trunc": ("if constexpr (BF) { const __bf16 b = (__bf16)x; return __builtin_bit_cast(unsigned short, b); }",
                   "if constexpr (BF) { return (unsigned short)(__float_as_uint(x) >> 16); }"),
    "img_drop4": ("        if (c < d) va = *reinterpret_cast<const g_f4 *>(src + r * src_stride + c);\n        if (c + 4 < d) vb =",
                  "        if (c + 4 < d) va = *reinterpret_cast<const g_f4 *>(src + r * src_stride + c);\n        if (c + 4 < d) vb ="),
    "img_c8_equiv": ("        if (c + 4 < d) vb = *reinterpret_cast<const g_f4 *>(src + r * src_stride + c + 4);",
                     "        if (c + 8 <= d) vb = *reinterpret_cast<const g_f4 *>(src + r * src_stride + c + 4);"),
    "sums_noshfl2": ("        a += __shfl_xor(a, 2, 64);\n", ""),
    "tile_fill1": ("        g_f4 v = (g_f4){0.f, 0.f, 0.f, 0.f};\n"
                   "        if (r0 + r < n && c0 + c < d) v = *reinterpret_cast<const g_f4 *>(src + (r0 + r) * src_stride + c0 + c);\n"
                   "        tile[r][c] = v[0]",
                   "        g_f4 v = (g_f4){1.f, 1.f, 1.f, 1.f};\n"
                   "        if (r0 + r < n && c0 + c < d) v = *reinterpret_cast<const g_f4 *>(src + (r0 + r) * src_stride + c0 + c);\n"
                   "        tile[r][c] = v[0]"),
    "clamp127": ("se = se > 126 ? 126 : (se < -126 ? -126 : se);", "se = se > 127 ? 127 : (se < -126 ? -126 : se);"),
    "absmax_tail": ("for (long j = i; j < count; ++j) m = max(", "for (long j = i; j + 1 < count; ++j) m = max("),
    "t_lo_zero": ("ll[j] = (_Float16)(x - (float)hh[j]);", "ll[j] = (_Float16)0.f;"),
}
TEST_FILES = ("tests/test_gpu_operand_images.py", "tests/test_gpu_split_gemm.py")


def build(names):
    for name in names:
        old, new = MUTANTS[name]
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
        f = src / "split_gemm.h"
        text = f.read_text()
        assert text.count(old) == 1, f"{name}: pattern found {text.count(old)} times: {old[:60]!r}"
        f.write_text(text.replace(old, new))
        so = out / "libmedtok_vq.so"
        subprocess.check_call([B.hipcc(), *B.FLAGS, str(src / B.SRC.name), "-o", str(so)])
        shutil.rmtree(out / "src")
        print("built", so, flush=True)


def run(names, limit=600):
    """both test files once against each mutant, each session under its own time limit; a session that did not end as a pytest
    session ends (0: nothing failed, 1: tests failed) ends the whole run: nothing more is started on that GPU"""
    for name in names:
        so = ROOT / "devlib" / name / "libmedtok_vq.so"
        if not so.exists():
            raise SystemExit(f"{so}: not built")
        for tf in TEST_FILES:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", tf, "-m", "gpu", "-q", "-rf",
                                "--tb=no", "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, MEDTOK_TEST_LIB=str(so)),
                               capture_output=True, text=True)
            failed = sorted({ln.split(" ")[1].split("::")[1].split("[")[0] for ln in r.stdout.splitlines() if ln.startswith("FAILED ")})
            tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
            print(f"MUTANT {name} | {tf} | exit {r.returncode} | {tail} | failed: {', '.join(failed) or '-'}", flush=True)
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
