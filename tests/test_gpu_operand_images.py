"""GPU: the conversion kernels in front of every dense product of a training step (split_gemm.h: split_half_kernel,
split_half_t_kernel, absmax_kernel with pow2_prescale, half_image_kernel, half_image_t_kernel) BIT FOR BIT against a few lines of CPU
arithmetic on the same fp32 input.  Each of them is an exact function -- one round-to-nearest-even per element, zero padding, a fixed
summation order of the column partials, an exponent-only prescale -- so nothing here has a tolerance except section 5, the autocast
split_linear end to end, whose only inexact step is the fp32 accumulation of half_gemm.

The C entry points are called with outputs this module owns: every output lies at a 16-byte aligned offset inside a larger allocation
that is prefilled with a sentinel bit pattern.  The elements in front of and behind the output must keep the sentinel (no write out of
bounds), no element inside it may (no write missing; the inputs are chosen so that no image contains the pattern), and padding must be
bit-zero.  The ops.* wrappers are called with the same data and must return the same bits."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT16 = 0x5a5a                 # fp16 203.25, bf16 1.5e16
SENT32 = 0x5a5a5a5b             # fp32 1.5e16 (odd)
GUARD = 512                     # sentinel elements in front of and behind every output
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


# ---------------------------------------------------------------------------------------------------------------- harness
class _Guarded:
    """an output of `numel` 16-bit (or, wide, 32-bit) elements inside a sentinel-filled allocation"""

    def __init__(self, numel, dev, wide=False):
        self.sent = SENT32 if wide else SENT16
        self.n = int(numel)
        self.buf = torch.full((2 * GUARD + self.n,), self.sent, dtype=torch.int32 if wide else torch.int16, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        assert self.ptr % 16 == 0

    def inner(self):
        """the output as a CPU integer tensor, after the guards were found untouched"""
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.sent).all()), "the kernel wrote in front of its output"
        assert bool((b[GUARD + self.n:] == self.sent).all()), "the kernel wrote past the end of its output"
        return b[GUARD:GUARD + self.n]


def _bits(t):
    """integer bit view of a CPU or device tensor (fp16 / bf16 -> int16, fp32 -> int32), flat, on the CPU"""
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).reshape(-1).cpu()


def _no_sentinel(ref, sent=SENT16):
    assert not bool((ref == sent).any()), "test input: the reference image contains the sentinel pattern"


def _same_bits(got, ref, what, sent=SENT16, rows=None):
    """got == ref as integers, element by element (and so: nothing left unwritten, padding bit-zero where ref is)"""
    ref = ref.reshape(-1)
    assert got.numel() == ref.numel(), (what, got.numel(), ref.numel())
    if rows is not None:
        got, ref = got.reshape(rows.numel(), -1)[rows], ref.reshape(rows.numel(), -1)[rows]
        got, ref = got.reshape(-1), ref.reshape(-1)
    assert not bool((got == sent).any()), f"{what}: {int((got == sent).sum())} elements were never written"
    bad = (got != ref).nonzero().reshape(-1)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {ref.numel()} elements differ; first at {i}: "
                             f"got {int(got[i]) & 0xffffffff:#x}, want {int(ref[i]) & 0xffffffff:#x}")


def _lib_and_stream():
    from medtok_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- inputs
def _specials():
    """what a rounding kernel gets wrong first: ties, the subnormal range of fp16, the top of fp16, signed zeros, infinities"""
    f = np.float32
    up, down = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    v = [0.0, -0.0, 1.0, -1.0, 0.1, -3.3,
         # exact ties of fp16 (11 significant bits) and their neighbours; the same for bf16 (8 bits)
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), up(1 + 2.0 ** -11), down(1 + 2.0 ** -11), up(1 + 3 * 2.0 ** -11),
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8), up(1 + 2.0 ** -8), down(1 + 2.0 ** -8), down(1 + 3 * 2.0 ** -8),
         1000.25, 1000.75, 2049.0, 2051.0, 257.0, 259.0,
         # fp16 subnormals: step 2^-24, ties at odd multiples of 2^-25
         2.0 ** -24, 2.0 ** -25, up(2.0 ** -25), down(2.0 ** -25), 3 * 2.0 ** -25, -(3 * 2.0 ** -25), 5 * 2.0 ** -25, 2.0 ** -26,
         2.0 ** -14, down(2.0 ** -14), 2.0 ** -14 - 2.0 ** -25, 1023.5 * 2.0 ** -24, 3.1e-7, -4.7e-6, 6.0e-5, 1e-9,
         # the top of fp16: 65504 is the largest finite value, 65520 the tie that rounds to inf
         65504.0, 65505.0, down(65520.0), 65520.0, up(65520.0), 65536.0, -65504.0, -down(65520.0), -65520.0, 1e5, -3e7,
         np.finfo(f).max, -np.finfo(f).max, 3.38e38, np.inf, -np.inf]
    return np.array(v, dtype=f)


def _avoid_sentinel(x):
    """(elements whose fp16 or bf16 image would be the sentinel pattern: replaced)"""
    for dt in DTYPES.values():
        x[x.to(dt).view(torch.int16) == SENT16] = 0.5
    return x


def _matrix(n, d, seed, specials=True):
    """fp32 [n, d] on the CPU: normal values over eight decades, and (specials) the list above at random places"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-5, 3, (n, d))).astype(np.float32)
    flat = x.reshape(-1)
    flat[rng.permutation(flat.size)[:max(1, flat.size // 50)]] *= np.float32(-0.0)          # some signed zeros everywhere
    if specials:
        s = _specials()
        if flat.size <= s.size:
            flat[:] = s[:flat.size]
        else:
            reps = min(4, flat.size // s.size)
            flat[rng.permutation(flat.size)[:reps * s.size]] = np.tile(s, reps)
    return _avoid_sentinel(torch.from_numpy(x))


# ---------------------------------------------------------------------------------------------------------------- references
def ref_image(x, dt, dp):
    """[n, dp] image bits: round to nearest even, zero columns past d"""
    n, d = x.shape
    out = torch.zeros(n, dp, dtype=dt)
    out[:, :d] = x.to(dt)
    return out.view(torch.int16)


def _grouped(full, gc):
    """[d, np] -> [np / gc * d, gc]: column chunk g of the transposed image is row block g"""
    return torch.cat([full[:, g * gc:(g + 1) * gc] for g in range(full.shape[1] // gc)], 0).contiguous()


def ref_image_t(x, dt, np_, gc):
    n, d = x.shape
    full = torch.zeros(d, np_, dtype=dt)
    full[:, :n] = x.t().to(dt)
    return _grouped(full, gc or np_).view(torch.int16)


def ref_partials(x, np_):
    """[(np + 63) // 64, d] fp32: per column and 64-row tile, four sequential sums of 16 rows from 0.f, then (s0 + s1) + (s2 + s3)"""
    n, d = x.shape
    tiles = (np_ + 63) // 64
    xp = np.zeros((tiles * 64, d), np.float32)
    xp[:n] = x.numpy()
    xp = xp.reshape(tiles, 4, 16, d)
    s = np.zeros((tiles, 4, d), np.float32)
    for j in range(16):
        s = s + xp[:, :, j, :]
    out = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def ref_split(x, s, dp=None, transpose=False, np_=0, gc=0):
    """(hi, lo) bits: xs = x * s in fp32, hi = fp16(xs), lo = fp16(xs - fp32(hi)); padded / transposed / grouped like the images"""
    n, d = x.shape
    xs = x * torch.tensor(s, dtype=torch.float32)
    assert xs.dtype == torch.float32
    hi = xs.to(torch.float16)
    lo = (xs - hi.float()).to(torch.float16)
    outs = []
    for img in (hi, lo):
        if transpose:
            full = torch.zeros(d, np_, dtype=torch.float16)
            full[:, :n] = img.t()
            outs.append(_grouped(full, gc or np_).view(torch.int16))
        else:
            full = torch.zeros(n, dp, dtype=torch.float16)
            full[:, :d] = img
            outs.append(full.view(torch.int16))
    return outs[0], outs[1], xs


def ref_prescale(amax):
    """2^clamp(11 - floor(log2 amax), -126, 126); 1 for amax zero or non-finite"""
    if amax == 0.0 or not math.isfinite(amax):
        return 1.0
    e = math.frexp(amax)[1] - 1                      # floor(log2 amax)
    return 2.0 ** min(126, max(-126, 11 - e))


def test_the_references_themselves():
    """(no kernel: the CPU rules above on hand-made values, so that a wrong reference cannot agree with a wrong kernel unnoticed)"""
    x = torch.tensor([[1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65520.0, -0.0], [2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]])
    h = ref_image(x, torch.float16, 8)
    assert [v & 0xffff for v in h[0].tolist()] == [0x3c00, 0x3c02, 0x7c00, 0x8000, 0, 0, 0, 0]
    assert [v & 0xffff for v in h[1].tolist()[:2]] == [0x0000, 0x0002]
    b = ref_image(x, torch.bfloat16, 8)
    assert [v & 0xffff for v in b[1].tolist()[2:4]] == [0x3f80, 0x3f82]
    t = ref_image_t(torch.arange(8.0).reshape(2, 4), torch.float16, 128, 64)
    assert t.shape == (8, 64) and t[1, 1] == ref_image(torch.tensor([[5.0]]), torch.float16, 1)[0, 0] and not t[4:].any()
    assert [ref_prescale(a) for a in (0.0, math.inf, 1.0, 3e4, 2.0 ** -126, 1.5 * 2.0 ** 127, 1e-45)] == \
           [1.0, 1.0, 2.0 ** 11, 2.0 ** -3, 2.0 ** 126, 2.0 ** -116, 2.0 ** 126]
    p = ref_partials(torch.ones(65, 4), 72)
    assert p.tolist() == [[64.0] * 4, [1.0] * 4]


# ---------------------------------------------------------------------------------------------------------------- 1. single images
def _run_half_image(x_dev, dt, dp, transpose=0, np_=0, gc=0):
    """medtok_half_image_f32 into a guarded buffer -> CPU bits"""
    _lib, lib, stream = _lib_and_stream()
    n, d = x_dev.shape
    numel = d * np_ if transpose else n * dp
    out = _Guarded(numel, x_dev.device)
    _lib.check(lib.medtok_half_image_f32(x_dev.data_ptr(), n, d, x_dev.stride(0) if n > 1 else d, np_ if transpose else dp, transpose, gc,
                                         int(dt == torch.bfloat16), out.ptr, stream), "medtok_half_image_f32")
    return out.inner()


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("n,d,dp", [(1, 4, 8), (3, 12, 16), (70, 100, 128), (257, 768, 768)])
def test_single_image_is_round_to_nearest_even_with_zero_padding(dev, dtn, n, d, dp):
    from medtok_amd import ops
    dt = DTYPES[dtn]
    x = _matrix(n, d, seed=n * 1000 + d)
    ref = ref_image(x, dt, dp)
    _no_sentinel(ref)
    xd = x.to(dev)
    _same_bits(_run_half_image(xd, dt, dp), ref, f"half_image {dtn} ({n}, {d}, {dp})")
    _same_bits(_bits(ops.half_image(xd, dp, dt)), ref, "ops.half_image")


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_single_image_of_a_row_strided_source(dev, dtn):
    from medtok_amd import ops
    dt = DTYPES[dtn]
    wide = _matrix(64, 300, seed=11)
    x = wide[:, 100:164]
    ref = ref_image(x, dt, 64)
    _no_sentinel(ref)
    xd = wide.to(dev)[:, 100:164]
    assert xd.stride(0) == 300
    _same_bits(_run_half_image(xd, dt, 64), ref, f"half_image {dtn}, strided")
    _same_bits(_bits(ops.half_image(xd, 64, dt)), ref, "ops.half_image, strided")


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_single_image_second_grid_stride_trip(dev, dtn):
    """n dp / 8 > 8192 x 256 threads: the last rows are converted in a second trip of the grid-stride loop.  The reference of this one
    case is torch's own conversion on the device, after the same conversion was shown to give the CPU's bits on the special values."""
    dt = DTYPES[dtn]
    small = _matrix(70, 100, seed=5)
    assert torch.equal(_bits(small.to(dev).to(dt)), ref_image(small, dt, 100).reshape(-1))
    n, d = 32800, 512
    assert n * d // 8 > 8192 * 256
    g = torch.Generator(device=dev).manual_seed(12)
    x = torch.randn(n, d, device=dev, generator=g) * torch.logspace(-6, 3, d, device=dev)
    sp = _specials()
    x[-8:].reshape(-1)[:sp.size] = torch.from_numpy(sp).to(dev)              # (in the rows of the second trip)
    x[:8].reshape(-1)[:sp.size] = torch.from_numpy(sp).to(dev)
    ref = x.to(dt).view(torch.int16)
    x[ref == SENT16] = 0.5
    ref = x.to(dt).view(torch.int16).reshape(-1)
    assert not bool((ref == SENT16).any())
    _lib, lib, stream = _lib_and_stream()
    out = _Guarded(n * d, dev)
    _lib.check(lib.medtok_half_image_f32(x.data_ptr(), n, d, d, d, 0, 0, int(dt == torch.bfloat16), out.ptr, stream), "medtok_half_image_f32")
    assert bool((out.buf[:GUARD] == SENT16).all()) and bool((out.buf[GUARD + n * d:] == SENT16).all())
    got = out.buf[GUARD:GUARD + n * d]
    nbad = int((got != ref).sum())
    assert nbad == 0, f"{nbad} elements differ, first at {int((got != ref).nonzero()[0])}"


# ---------------------------------------------------------------------------------------------------------------- 2. transposed / paired / sums
def _r(v, q):
    return (v + q - 1) // q * q


#            n    d    np                 gc   dp_plain
T_CASES = [(1, 4, _r(1, 8), 0, _r(4, 8)),
           (63, 60, _r(63, 64), 64, _r(60, 32)),
           (64, 64, _r(64, 64) + 64, 128, _r(64, 64)),
           (65, 68, _r(65, 8), 0, _r(68, 8)),
           (130, 132, _r(130, 64), 64, _r(132, 32)),
           (130, 60, _r(130, 64) + 64, 128, _r(60, 64)),
           (65, 132, _r(65, 64) + 64, 64, _r(132, 64)),
           (1, 64, _r(1, 64) + 64, 64, _r(64, 8)),
           (63, 4, _r(63, 8), 0, _r(4, 32)),
           (64, 68, _r(64, 64), 0, _r(68, 64))]


@functools.lru_cache(maxsize=None)
def _t_case(i):
    n, d, np_, gc, dpp = T_CASES[i]
    x = _matrix(n, d, seed=100 + i, specials=False)                # (finite: the column sums must not meet inf - inf)
    flat = x.reshape(-1)
    fin = _specials()
    fin = torch.from_numpy(fin[np.abs(fin) < 1e30])
    if flat.numel() > fin.numel():
        flat[torch.from_numpy(np.random.default_rng(i).permutation(flat.numel())[:fin.numel()])] = fin
    x = _avoid_sentinel(x)
    part = ref_partials(x, np_)
    _no_sentinel(part.view(torch.int32), SENT32)
    return x, part


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("case", range(len(T_CASES)))
def test_transposed_paired_images_and_column_partials(dev, dtn, case):
    from medtok_amd import ops
    _lib, lib, stream = _lib_and_stream()
    dt, bf = DTYPES[dtn], int(dtn == "bf16")
    n, d, np_, gc, dpp = T_CASES[case]
    x, ref_p = _t_case(case)
    ref_t, ref_pl = ref_image_t(x, dt, np_, gc), ref_image(x, dt, dpp)
    _no_sentinel(ref_t), _no_sentinel(ref_pl)
    tiles = (np_ + 63) // 64
    assert ref_t.shape == (np_ // (gc or np_) * d, gc or np_) and ref_p.shape == (tiles, d)
    ref_pb = ref_p.view(torch.int32)
    xd = x.to(dev)
    stride = d
    tag = f"{dtn} n={n} d={d} np={np_} gc={gc} dp_plain={dpp}"

    # the transposed image alone
    _same_bits(_run_half_image(xd, dt, 0, transpose=1, np_=np_, gc=gc), ref_t, "half_image(transpose) " + tag)
    # ... with the column partials
    o_t, o_p = _Guarded(d * np_, dev), _Guarded(tiles * d, dev, wide=True)
    _lib.check(lib.medtok_half_image_t_sums_f32(xd.data_ptr(), n, d, stride, np_, gc, bf, o_t.ptr, o_p.ptr, stream), "medtok_half_image_t_sums_f32")
    _same_bits(o_t.inner(), ref_t, "half_image_t_sums image " + tag)
    _same_bits(o_p.inner(), ref_pb, "half_image_t_sums partials " + tag, SENT32)
    # both images from one pass
    o_pl, o_t = _Guarded(n * dpp, dev), _Guarded(d * np_, dev)
    _lib.check(lib.medtok_half_image_pair_f32(xd.data_ptr(), n, d, stride, dpp, np_, gc, bf, o_pl.ptr, o_t.ptr, stream), "medtok_half_image_pair_f32")
    _same_bits(o_pl.inner(), ref_pl, "half_image_pair plain " + tag)
    _same_bits(o_t.inner(), ref_t, "half_image_pair transposed " + tag)
    # ... with the column partials
    o_pl, o_t, o_p = _Guarded(n * dpp, dev), _Guarded(d * np_, dev), _Guarded(tiles * d, dev, wide=True)
    _lib.check(lib.medtok_half_image_pair_sums_f32(xd.data_ptr(), n, d, stride, dpp, np_, gc, bf, o_pl.ptr, o_t.ptr, o_p.ptr, stream),
               "medtok_half_image_pair_sums_f32")
    _same_bits(o_pl.inner(), ref_pl, "half_image_pair_sums plain " + tag)
    _same_bits(o_t.inner(), ref_t, "half_image_pair_sums transposed " + tag)
    got_p = o_p.inner()
    _same_bits(got_p, ref_pb, "half_image_pair_sums partials " + tag, SENT32)
    if tiles * 64 >= n + 64:                                          # the all-padding row tile: +0, every bit
        assert not bool(got_p.reshape(tiles, d)[(n + 63) // 64:].any())
    # the plain image of the pair is the single-image kernel's
    _same_bits(_run_half_image(xd, dt, dpp), ref_pl, "half_image (row-major) " + tag)

    # the wrappers: the same bits; db = the sum of the partials (fp32 summation of `tiles` terms: exact for one tile)
    db_ref = ref_p.double().sum(0)
    db_tol = tiles * 2.0 ** -24 * ref_p.double().abs().sum(0)
    _same_bits(_bits(ops.half_image(xd, np_, dt, transpose=True, group_cols=gc)), ref_t, "ops.half_image(transpose)")
    t, db = ops.half_image(xd, np_, dt, transpose=True, group_cols=gc, col_sums=True)
    _same_bits(_bits(t), ref_t, "ops.half_image(transpose, col_sums)")
    assert db.shape == (d,) and bool(((db.cpu().double() - db_ref).abs() <= (0 if tiles == 1 else 1) * db_tol).all())
    pl, t = ops.half_image_pair(xd, dpp, np_, dt, group_cols=gc)
    _same_bits(_bits(pl), ref_pl, "ops.half_image_pair plain"), _same_bits(_bits(t), ref_t, "ops.half_image_pair transposed")
    pl, t, db = ops.half_image_pair(xd, dpp, np_, dt, group_cols=gc, col_sums=True)
    _same_bits(_bits(pl), ref_pl, "ops.half_image_pair(col_sums) plain"), _same_bits(_bits(t), ref_t, "ops.half_image_pair(col_sums) transposed")
    assert db.shape == (d,) and bool(((db.cpu().double() - db_ref).abs() <= (0 if tiles == 1 else 1) * db_tol).all())


def test_transposed_image_of_a_row_strided_source(dev):
    """a column block of a wider matrix through the transposed kernel, pair and sums"""
    _lib, lib, stream = _lib_and_stream()
    wide = _matrix(70, 300, seed=21, specials=False)
    x = wide[:, 100:168].contiguous()
    n, d, np_, dpp = 70, 68, 128, 96
    ref_t, ref_pl, ref_p = ref_image_t(x, torch.bfloat16, np_, 64), ref_image(x, torch.bfloat16, dpp), ref_partials(x, np_)
    _no_sentinel(ref_t), _no_sentinel(ref_pl)
    xd = wide.to(dev)[:, 100:168]
    o_pl, o_t, o_p = _Guarded(n * dpp, dev), _Guarded(d * np_, dev), _Guarded(2 * d, dev, wide=True)
    _lib.check(lib.medtok_half_image_pair_sums_f32(xd.data_ptr(), n, d, 300, dpp, np_, 64, 1, o_pl.ptr, o_t.ptr, o_p.ptr, stream),
               "medtok_half_image_pair_sums_f32")
    _same_bits(o_pl.inner(), ref_pl, "plain"), _same_bits(o_t.inner(), ref_t, "transposed")
    _same_bits(o_p.inner(), ref_p.view(torch.int32), "partials", SENT32)


# ---------------------------------------------------------------------------------------------------------------- 3. split pairs
def _split_input(n, d, seed):
    """values whose (hi, lo) pair under the scales of this section stays finite"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-4, 1, (n, d))).astype(np.float32)
    x.reshape(-1)[rng.permutation(x.size)[:max(1, x.size // 40)]] *= np.float32(-0.0)
    return torch.from_numpy(x)


def _split_clean(x, s):
    """(elements whose hi part under the scale s would be the sentinel pattern: zeroed; a lo part is too small to be it)"""
    x[(x * torch.tensor(s, dtype=torch.float32)).to(torch.float16).view(torch.int16) == SENT16] = 0.0
    return x


def _check_split(got_hi, got_lo, ref_hi, ref_lo, what, rows=None):
    _same_bits(got_hi, ref_hi, what + " hi", rows=rows)
    _same_bits(got_lo, ref_lo, what + " lo", rows=rows)


def _run_split_half(xd, dp, scale, seg_len=None, seg_rows=0):
    _lib, lib, stream = _lib_and_stream()
    n, d = xd.shape
    hi, lo = _Guarded(n * dp, xd.device), _Guarded(n * dp, xd.device)
    _lib.check(lib.medtok_split_half_f32(xd.data_ptr(), n, d, xd.stride(0) if n > 1 else d, dp, float(scale), hi.ptr, lo.ptr,
                                         0 if seg_len is None else seg_len.data_ptr(), seg_rows, stream), "medtok_split_half_f32")
    return hi.inner(), lo.inner()


@pytest.mark.parametrize("n,d,dp,scale", [(513, 100, 128, 1.0), (37, 100, 128, 2.0 ** -7), (37, 100, 104, 2.0 ** 9), (3, 12, 16, 1.0)])
def test_split_half_bits(dev, n, d, dp, scale):
    from medtok_amd import ops
    x = _split_clean(_split_input(n, d, seed=n + d), scale)
    rh, rl, xs = ref_split(x, scale, dp=dp)
    _no_sentinel(rh), _no_sentinel(rl)
    assert bool(torch.isfinite(rh.view(torch.float16).float()).all())
    xd = x.to(dev)
    gh, gl = _run_split_half(xd, dp, scale)
    _check_split(gh, gl, rh, rl, f"split_half ({n}, {d}, {dp}) x {scale}")
    back = gh.view(torch.float16).double() + gl.view(torch.float16).double()
    want = torch.zeros(n, dp, dtype=torch.float64)
    want[:, :d] = xs.double()
    assert bool(((back.reshape(n, dp) - want).abs() <= 2.0 ** -21 * want.abs() + 2.0 ** -24).all())
    oh, ol = ops.split_half(xd, dp=dp, scale=scale)
    _check_split(_bits(oh), _bits(ol), rh, rl, "ops.split_half")


def test_split_half_of_a_row_strided_source(dev):
    wide = _split_input(64, 300, seed=31)
    x = wide[:, 100:164]
    rh, rl, _ = ref_split(x, 1.0, dp=72)
    _no_sentinel(rh), _no_sentinel(rl)
    gh, gl = _run_split_half(wide.to(dev)[:, 100:164], 72, 1.0)
    _check_split(gh, gl, rh, rl, "split_half, strided")


def test_split_half_segmented_converts_the_leading_rows_of_every_segment(dev):
    """seg_rows = 8, seg_len = 0, 1, 7, 8: rows below seg_len exactly; the rows at or past it are not part of the contract (the kernel
    leaves them unwritten); nothing outside the images is touched"""
    from medtok_amd import ops
    seg = [0, 1, 7, 8, 3, 0]
    n, d, dp = 8 * len(seg), 36, 40
    x = _split_input(n, d, seed=41)
    rh, rl, _ = ref_split(x, 1.0, dp=dp)
    _no_sentinel(rh), _no_sentinel(rl)
    rows = torch.tensor([r % 8 < seg[r // 8] for r in range(n)])
    xd, sl = x.to(dev), torch.tensor(seg, dtype=torch.int64, device=dev)
    gh, gl = _run_split_half(xd, dp, 1.0, sl, 8)
    _check_split(gh, gl, rh, rl, "split_half, segmented", rows=rows)
    oh, ol = ops.split_half(xd, dp=dp, seg_len=sl, seg_rows=8)
    _check_split(_bits(oh), _bits(ol), rh, rl, "ops.split_half, segmented", rows=rows)


AMAX_KINDS = {"2^-126": 2.0 ** -126, "1": 1.0, "3e4": 3e4, "1.5*2^127": 1.5 * 2.0 ** 127, "zero": 0.0, "inf": math.inf}
#               layout         n    d    dp / np  gc
S_LAYOUTS = [("plain", 70, 100, 128, 0), ("plain", 3, 12, 16, 0),
             ("t", 65, 68, 72, 0), ("t", 63, 60, 64, 64), ("t", 130, 132, 256, 128), ("t", 1, 4, 8, 0), ("t", 64, 64, 192, 64)]


def _scaled_input(n, d, kind, seed):
    """fp32 [n, d] whose largest magnitude is exactly AMAX_KINDS[kind] (inf: moderate values and one +inf)"""
    target = AMAX_KINDS[kind]
    rng = np.random.default_rng(seed)
    base = (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-3, 0, (n, d))).astype(np.float32)
    base = base / np.abs(base).max()                                  # |.| <= 1
    pos = int(rng.integers(base.size))
    if kind == "zero":
        x = base * np.float32(0.0)                                    # (signed zeros)
    elif kind == "inf":
        x = base * np.float32(100.0)
        x.reshape(-1)[pos] = np.inf
    else:
        x = base * np.float32(target)
        x.reshape(-1)[pos] = -target if seed % 2 else target
    assert x.dtype == np.float32
    return torch.from_numpy(x)


@pytest.mark.parametrize("kind", list(AMAX_KINDS))
def test_split_half_scaled_bits_and_the_prescale_rule(dev, kind):
    """the device-side |x|max and the power of two it selects: s = 2^clamp(11 - floor(log2 amax), -126, 126), 1 for amax 0 or
    non-finite -- seen through the bits of the prescaled pair (a product undoes the scale with the same function, so a wrong rule
    cancels end to end)"""
    from medtok_amd import ops
    _lib, lib, stream = _lib_and_stream()
    for li, (layout, n, d, dp, gc) in enumerate(S_LAYOUTS):
        x = _scaled_input(n, d, kind, seed=li)
        amax = float(x.abs().max())
        assert amax == AMAX_KINDS[kind]
        s = ref_prescale(amax)
        x = _split_clean(x, s)
        assert float(x.abs().max()) == amax
        tr = layout == "t"
        rh, rl, xs = ref_split(x, s, dp=dp, transpose=tr, np_=dp, gc=gc)
        _no_sentinel(rh), _no_sentinel(rl)
        xd = x.to(dev)
        am = ops.absmax(xd)
        assert float(am) == amax
        numel = (d if tr else n) * dp
        hi, lo = _Guarded(numel, dev), _Guarded(numel, dev)
        _lib.check(lib.medtok_split_half_scaled_f32(xd.data_ptr(), n, d, d, dp, am.data_ptr(), int(tr), gc, hi.ptr, lo.ptr, stream),
                   "medtok_split_half_scaled_f32")
        gh, gl = hi.inner(), lo.inner()
        tag = f"split_half_scaled {layout} n={n} d={d} dp={dp} gc={gc} amax={kind}"
        # (inf - inf: the lo part of an infinite element is a NaN, whose payload is not part of the contract)
        nan = torch.isnan(rl.view(torch.float16)).reshape(-1)
        assert int(nan.sum()) == (1 if kind == "inf" else 0)
        assert bool(torch.isnan(gl.view(torch.float16)[nan]).all())
        keep = (~nan).nonzero().reshape(-1)
        _same_bits(gh, rh, tag + " hi")
        _same_bits(gl[keep], rl.reshape(-1)[keep], tag + " lo")
        # hi + lo = x s to 22 bits (or the fp16 subnormal step)
        if tr:
            want = torch.zeros(d, dp, dtype=torch.float64)
            want[:, :n] = xs.double().t()
            want = _grouped(want, gc or dp).reshape(-1)
        else:
            want = torch.zeros(n, dp, dtype=torch.float64)
            want[:, :d] = xs.double()
            want = want.reshape(-1)
        back = gh.view(torch.float16).double() + gl.view(torch.float16).double()
        assert bool(((back - want).abs()[keep] <= (2.0 ** -21 * want.abs() + 2.0 ** -24)[keep]).all()), tag
        oh, ol = ops.split_half_scaled(xd, dp, am, transpose=tr, group_cols=gc)
        _same_bits(_bits(oh), rh, "ops." + tag + " hi")
        _same_bits(_bits(ol)[keep], rl.reshape(-1)[keep], "ops." + tag + " lo")
        if li == 0 and kind in ("1", "zero"):                         # amax NULL: no prescale
            r1h, r1l, _ = ref_split(_split_clean(x, 1.0), 1.0, dp=dp)
            _no_sentinel(r1h)
            xd = x.to(dev)
            hi, lo = _Guarded(numel, dev), _Guarded(numel, dev)
            _lib.check(lib.medtok_split_half_scaled_f32(xd.data_ptr(), n, d, d, dp, 0, 0, 0, hi.ptr, lo.ptr, stream), "medtok_split_half_scaled_f32")
            _check_split(hi.inner(), lo.inner(), r1h, r1l, "split_half_scaled without amax")


def test_split_half_scaled_of_a_row_strided_source(dev):
    from medtok_amd import ops
    _lib, lib, stream = _lib_and_stream()
    wide = _split_input(70, 300, seed=51)
    x = wide[:, 100:168].contiguous()
    xd = wide.to(dev)[:, 100:168]
    am = ops.absmax(x.to(dev))
    s = ref_prescale(float(x.abs().max()))
    for tr, dp, gc in ((0, 72, 0), (1, 128, 64)):
        rh, rl, _ = ref_split(x, s, dp=dp, transpose=bool(tr), np_=dp, gc=gc)
        _no_sentinel(rh), _no_sentinel(rl)
        numel = (68 if tr else 70) * dp
        hi, lo = _Guarded(numel, dev), _Guarded(numel, dev)
        _lib.check(lib.medtok_split_half_scaled_f32(xd.data_ptr(), 70, 68, 300, dp, am.data_ptr(), tr, gc, hi.ptr, lo.ptr, stream),
                   "medtok_split_half_scaled_f32")
        _check_split(hi.inner(), lo.inner(), rh, rl, f"split_half_scaled, strided, transpose={tr}")


# ---------------------------------------------------------------------------------------------------------------- 4. absmax
ABS_STEP = 512 * 1024                      # elements between the four loads of a thread in the unrolled loop, at 512 blocks
ABS_BIG = 4 * ABS_STEP + 4 * 100 + 3       # one unrolled trip, a float4 tail of 100 threads and a scalar tail of 3 elements


def _abs_positions(count):
    if count <= 5:
        return list(range(count))
    pos = {0, count - 1, count - 2, count - 3, count // 2}
    if count == ABS_BIG:
        pos |= {u * ABS_STEP + 4 * 77 + (u + 1) % 4 for u in range(4)}      # each of the four unrolled slots
        pos |= {4 * ABS_STEP + 4 * 50 + 1, 4 * ABS_STEP - 1, ABS_STEP}       # the float4 tail; slot boundaries
    return sorted(pos)


@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 4095, 4096, 4097, ABS_BIG])
def test_absmax_is_exact_wherever_the_maximum_sits(dev, count):
    from medtok_amd import ops
    _lib, lib, stream = _lib_and_stream()
    assert ABS_BIG >= 3 * 512 * 1024 + 4 and ABS_BIG % 4 == 3
    rng = np.random.default_rng(count)
    base = torch.from_numpy(rng.uniform(-1.0, 1.0, max(count, 4)).astype(np.float32))
    base_max = float(base[:count].abs().max()) if count else 0.0
    xd = base.to(dev)
    runs = [(None, None, base_max)]
    for p in _abs_positions(count):
        runs += [(p, 7.5, 7.5), (p, -7.25, 7.25)]
    if count:
        runs += [(count - 1, math.inf, math.inf), (count // 2, -math.inf, math.inf), (count - 1, math.nan, None), (0, math.nan, None)]
    # every run writes its own 16-byte aligned slot of one guarded buffer; the three words behind a slot are guards too
    out = _Guarded(4 * len(runs) + 4, dev, wide=True)
    for i, (p, v, _) in enumerate(runs):
        if p is not None:
            xd[p] = v
        _lib.check(lib.medtok_absmax_f32(xd.data_ptr(), count, out.ptr + 16 * i, stream), "medtok_absmax_f32")
        if p is not None:
            xd[p] = float(base[p])
    # a second call on a smaller input overwrites, not accumulates: big maximum first, then a prefix without it
    last = len(runs)
    if count >= 4:
        xd[count - 1] = 9.0
        _lib.check(lib.medtok_absmax_f32(xd.data_ptr(), count, out.ptr + 16 * last, stream), "medtok_absmax_f32")
        _lib.check(lib.medtok_absmax_f32(xd.data_ptr(), count - 1, out.ptr + 16 * last, stream), "medtok_absmax_f32")
        xd[count - 1] = float(base[count - 1])
    got = out.inner().reshape(-1, 4)
    assert bool((got[:, 1:] == SENT32).all()), "absmax wrote more than one float"
    vals = got[:, 0].contiguous().view(torch.float32)
    for i, (p, v, want) in enumerate(runs):
        assert int(got[i, 0]) != SENT32, (count, p, v, "not written")
        if want is None:
            assert not math.isfinite(float(vals[i])), (count, p, v, float(vals[i]))
        else:
            assert float(vals[i]) == want and int(got[i, 0]) >= 0, (count, p, v, float(vals[i]), want)
    if count >= 4:
        assert float(vals[last]) == float(base[:count - 1].abs().max())
    if count:
        assert float(ops.absmax(xd[:count])) == base_max
        assert float(ops.absmax(torch.zeros(count, device=dev) * -1.0)) == 0.0
    else:
        assert int(got[0, 0]) == 0


# ---------------------------------------------------------------------------------------------------------------- 5. autocast split_linear
#                 m     k    n    x is a column block of a wider tensor
LINEAR_SHAPES = [(1, 8, 4, False), (63, 40, 36, False), (65, 96, 100, False), (130, 72, 260, False), (1100, 64, 64, False),
                 (1537, 264, 520, False), (65, 96, 100, True)]
#            name         x      w      bias: None = no bias, else whether its gradient is wanted
REQUESTS = [("x w b", True, True, True), ("w b", False, True, True), ("x", True, False, False), ("w, no bias", False, True, None),
            ("x w, no bias", True, True, None)]


@functools.lru_cache(maxsize=None)
def _linear_case(si, dtn):
    """inputs (fp32, CPU) and the fp64 products of the operands rounded to the autocast dtype"""
    m, k, n, block = LINEAR_SHAPES[si]
    dt = DTYPES[dtn]
    rng = np.random.default_rng(1000 + si)
    wide = torch.from_numpy(rng.standard_normal((m, k + 104 if block else k)).astype(np.float32))
    x = wide[:, 40:40 + k] if block else wide
    w = torch.from_numpy((rng.standard_normal((n, k)) / k ** 0.5).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((m, n)).astype(np.float32))
    x16, w16, dy16 = x.to(dt).double(), w.to(dt).double(), dy.to(dt).double()
    ref = dict(y=x16 @ w16.t() + b.double(), y_nobias=x16 @ w16.t(), dx=dy16 @ w16, dw=dy16.t() @ x16, db=dy.double().sum(0))
    return wide, w, b, dy, ref


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("si", range(len(LINEAR_SHAPES)))
def test_autocast_split_linear_against_fp64_of_the_rounded_operands(dev, dtn, si):
    """forward, dx, dw, db of split_linear under torch.autocast at the shapes where its glue branches (d % 8 == 4 paddings, row counts
    around 64, one to three row groups of the weight gradient, a strided x), for every set of requested gradients: once the images are
    exact, half_gemm's fp32 accumulation is the only inexact step -- 4e-6 of each result's largest magnitude (fuzz_split_gemm's bar for
    half_gemm against fp64 on rounded operands); db is an fp32 sum of at most 1537 terms: 2e-6."""
    from medtok_amd.vector_quantization_soft_one_new import split_linear
    from medtok_amd.autograd import _SplitLinearFunction
    m, k, n, block = LINEAR_SHAPES[si]
    dt = DTYPES[dtn]
    wide, w_c, b_c, dy_c, ref = _linear_case(si, dtn)
    groups = _SplitLinearFunction._row_split(m, n, k)[0]
    assert groups == {1100: 2, 1537: 3}.get(m, 1)
    wide_d, dy = wide.to(dev), dy_c.to(dev)
    for name, gx, gw, gb in REQUESTS:
        x = (wide_d[:, 40:40 + k] if block else wide_d).detach()
        assert (x.stride(0) != k) == block
        x.requires_grad_(gx)
        w = w_c.to(dev).requires_grad_(gw)
        b = None if gb is None else b_c.to(dev).requires_grad_(gb)
        with torch.autocast("cuda", dtype=dt):
            y = split_linear(x, w, b)
        assert y.dtype == torch.float32 and y.shape == (m, n)
        wanted = [(t, r) for t, r, on in ((x, "dx", gx), (w, "dw", gw), (b, "db", bool(gb))) if on]
        grads = torch.autograd.grad(y, [t for t, _ in wanted], dy)
        results = [("y" if b is not None else "y_nobias", y.detach())] + [(r, g) for (_, r), g in zip(wanted, grads)]
        for what, got in results:
            want = ref[what]
            assert got.shape == want.shape and got.dtype == torch.float32
            err = float((got.cpu().double() - want).abs().max()) / float(want.abs().max())
            print(f"{dtn} ({m}, {k}, {n}){' block' if block else ''} [{name}] {what}: {err:.3e}")
            assert err <= (2e-6 if what == "db" else 4e-6), (dtn, m, k, n, block, name, what, err)
