"""The half-precision form of the attention backward (shared_kv_attention_dq_kernel / shared_kv_attention_dkv_kernel, HM = 1 / 2:
16-bit swizzled chunk images, transposed LDS reads, two images resident in the dKV loop, woven loads, clamped tail rows, several
sources per launch) against an fp64 reference of the ROUNDED operands (tests/attention_half_reference.py), per code and per output.

The forward's out / lse come from the CPU oracle, the dropout mask from the oracle's hash: the backward is tested on its own.
Per code, e = max |gpu - ref64| over the code's rows / the code's scale (largest MAGNITUDE entry: the formulas in absolute values),

    e <= 4 spread + flip + 2e-6

spread: the same statistic between the reference's own fp32 and fp64 forms (what fp32 accumulation and exp legitimately move,
rounding flips of PM / dS entries included; the GPU's flipped set is an independent draw of the same process -- margin four);
flip: one half-precision ulp of the code's largest dS (PM) entry times its largest operand entry, over the scale (a code so
small that the fp32 reference flips nothing while the GPU flips one entry); 2e-6: fp32 storage and summation of the result.
Measured values: DESIGN.md, section 6.  tools/mutants_attention_half.py lists the value mutants this file must fail on."""
import functools

import numpy as np
import pytest
import torch

import attention_half_reference as R

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256, 384, 512, 640, 768)             # every (W, NT) instantiation of the backward
HALVES = (torch.float16, torch.bfloat16)
# long q meets short kv and the reverse; 0 / 1 / tile - 1 / tile / tile + 1 / two tiles / three tiles + 1 on both sides
Q_LEN = np.array([0, 1, 5, 31, 32, 33, 64, 97], np.int64)
KV_LEN = np.array([33, 100, 65, 0, 32, 31, 17, 1], np.int64)
KV_PAD = np.array([2, 0, 3, 4, 0, 1, 0, 5], np.int64)   # key slots longer than their valid keys
Q_LEN_2 = np.array([33, 0, 64, 2, 1, 40, 5, 31], np.int64)         # the second source of the multi-source launch
KV_START = np.cumsum(KV_LEN + KV_PAD) - (KV_LEN + KV_PAD)
NK = int((KV_LEN + KV_PAD).sum())
SOURCES = ((Q_LEN, 0.2, 0.1, 99), (Q_LEN_2, 0.15, 0.0, 5))         # (q_len, scale, dropout_p, seed) of sources 0 / 1


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def _inputs(d, source):
    """(q, d_out, q_start, nq) of source 0 / 1: random queries (0.3 N(0, 1)) and upstream gradients, + two query rows of no code"""
    q_len = SOURCES[source][0]
    rng = np.random.default_rng(d + 7 * source)
    nq = int(q_len.sum()) + 2
    return (rng.standard_normal((nq, d)) * 0.3).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32), np.cumsum(q_len) - q_len, nq


@functools.lru_cache(maxsize=None)
def _keys(d):
    """the keys every source attends to.  Two late keys are scaled copies of queries of source 0: a dominant softmax entry (S = 10)
    in a late chunk -- key 70 of code 1's 100 (third chunk) and key 64 of code 2's 65 (the lone row of a tail chunk)"""
    kv = np.random.default_rng(1000 + d).standard_normal((NK, d)).astype(np.float32)
    q, _, q_start, _ = _inputs(d, 0)
    for b, key, row in ((1, 70, 0), (2, 64, 3)):
        qr = q[q_start[b] + row].astype(np.float64)
        kv[KV_START[b] + key] = (qr * (10.0 / (SOURCES[0][1] * float(qr @ qr)))).astype(np.float32)
    return kv


@functools.lru_cache(maxsize=None)
def _case(d, p, source=0):
    """CPU inputs of one attention call over the shared keys + the oracle's forward (p = None: the source's own rate); cached, never
    modified"""
    q_len, scale, p_src, seed = SOURCES[source]
    p = p_src if p is None else p
    q, d_out, q_start, nq = _inputs(d, source)
    d_out, kv = d_out.copy(), _keys(d).copy()
    O = _oracle()
    out, lse = O.shared_kv_attention_train(q, q_start, q_len, kv, KV_START, KV_LEN, scale, p, seed)
    out[-2:] = d_out[-2:][:, ::-1]                                  # rows of no code: whatever the buffers hold must not matter
    masks = R.keep_masks(O, seed, q_start, q_len, KV_LEN, p)
    for a in (q, kv, d_out, out, lse, q_start):
        a.setflags(write=False)
    return dict(q=q, kv=kv, d_out=d_out, out=out, lse=lse, q_start=q_start, q_len=q_len, scale=scale, p=p, seed=seed, masks=masks, nq=nq)


@functools.lru_cache(maxsize=None)
def _reference(d, p, half, source=0):
    """(ref64, ref32) of a case"""
    c = _case(d, p, source)
    args = (c["q"], c["q_start"], c["q_len"], c["kv"], KV_START, KV_LEN, c["d_out"], c["out"], c["lse"], c["scale"], c["masks"],
            R.keep_scale_of(c["p"]))
    return R.backward(*args, half=half, acc=np.float64), R.backward(*args, half=half, acc=np.float32)


def _dev_args(c, dev):
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)                  # (a copy: the cached arrays are read-only)
    return dict(q=T(c["q"]), q_start=T(c["q_start"]), q_len=T(c["q_len"]), kv=T(c["kv"]), kv_start=T(KV_START), kv_len=T(KV_LEN),
                out=T(c["out"]), lse=T(c["lse"]), d_out=T(c["d_out"]))


def _call(fn, c, t, half, **kw):
    return fn(t["q"], t["q_start"], t["q_len"], t["kv"], t["kv_start"], t["kv_len"], int(c["q_len"].max()), int(KV_LEN.max()), c["scale"],
              c["p"], c["seed"], t["out"], t["lse"], t["d_out"], half=half, **kw)


def _own_rows(q_start, q_len, nq):
    """(query rows of codes with keys, key rows of codes with queries): everything else must be exactly zero"""
    own_q, own_k = np.zeros(nq, bool), np.zeros(NK, bool)
    for b in range(len(q_len)):
        if KV_LEN[b] > 0:
            own_q[q_start[b]: q_start[b] + q_len[b]] = True
        if q_len[b] > 0:
            own_k[KV_START[b]: KV_START[b] + KV_LEN[b]] = True
    return own_q, own_k


def _check_codes(tag, what, got, refs, starts, lens, half):
    """the per-code bound for one output (`what` = "dq" / "dkv") of one or several sources: e scale <= sum over the sources of
    (4 spread + flip) scale_source + 2e-6 scale, scale = the largest entry of the sources' summed magnitude over the code's rows"""
    ref = sum(r64[what] for r64, _ in refs)
    mag = sum(r64[what + "_mag"] for r64, _ in refs)
    fl = [R.flips(r64, half)[0 if what == "dq" else 1] for r64, _ in refs]
    worst = (0.0, 0.0, 0.0)
    failures = []
    for b in range(len(lens)):
        s, n = int(starts[b]), int(lens[b])
        if n == 0:
            continue
        scale = float(mag[s: s + n].max())
        e = R.code_error(got, ref, scale, s, n)
        allowed, spread = 2e-6, 0.0
        for (r64, r32), f in zip(refs, fl):
            sc_src = float(r64[what + "_scale"][b])
            sp = R.code_error(r32[what], r64[what], sc_src, s, n)
            if scale > 0:
                allowed += (4 * sp + float(f[b])) * sc_src / scale
                spread += sp * sc_src / scale
        print(f"ATT_HALF {tag} {what} code={b} rows={n} e={e:.3e} spread={spread:.3e} allowed={allowed:.3e}")
        if e > worst[0]:
            worst = (e, spread, allowed)
        if not e <= allowed:
            failures.append((b, e, spread, allowed))
    print(f"ATT_HALF_WORST {tag} {what} e={worst[0]:.3e} spread={worst[1]:.3e} allowed={worst[2]:.3e}")
    assert not failures, (tag, what, failures)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("half", HALVES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("d", WIDTHS)
def test_half_backward_matches_the_rounded_operand_reference(dev, d, half, p):
    """dQ and dKV of the full call, per code, against the fp64 reference of the rounded operands; rows outside every code, slots past
    a code's keys, keys of codes without queries and queries of codes without keys are exactly zero."""
    from medtok_amd import ops
    c, refs = _case(d, p), [_reference(d, p, half)]
    t = _dev_args(c, dev)
    dq, dkv = _call(ops.shared_kv_attention_backward, c, t, half)
    dq, dkv = dq.cpu().numpy(), dkv.cpu().numpy()
    tag = f"d={d} {str(half)[6:]} p={p}"
    _check_codes(tag, "dq", dq, refs, c["q_start"], c["q_len"], half)
    _check_codes(tag, "dkv", dkv, refs, KV_START, KV_LEN, half)
    own_q, own_k = _own_rows(c["q_start"], c["q_len"], c["nq"])
    assert not dq[~own_q].any() and not dkv[~own_k].any()
    assert np.isfinite(dq).all() and np.isfinite(dkv).all()


@pytest.mark.parametrize("d,half", [(64, torch.bfloat16), (128, torch.float16), (256, torch.bfloat16), (384, torch.float16), (512, torch.bfloat16),
                                    (640, torch.float16), (768, torch.bfloat16)], ids=lambda v: str(v).replace("torch.", ""))
def test_dq_only_entry_returns_the_full_call_dq_and_the_reference_delta(dev, d, half):
    """shared_kv_attention_backward_dq: dq bit for bit the full call's; delta = <d_out, out> of the unrounded fp32 rows within fp32
    round-off: a product passes 4 ceil(d / 256) fused multiply-adds of a lane and six butterfly additions, each 2^-24 relative, so
    |delta - ref| <= (4 ceil(d / 256) + 6) 2^-24 sum |d_out out| (row_dot_kernel); rows of no code included."""
    from medtok_amd import ops
    c = _case(d, 0.1)
    r64, _ = _reference(d, 0.1, half)
    t = _dev_args(c, dev)
    dq_full, _ = _call(ops.shared_kv_attention_backward, c, t, half)
    dq, delta = _call(ops.shared_kv_attention_backward_dq, c, t, half)
    assert torch.equal(dq, dq_full)
    delta = delta.cpu().numpy()[: c["nq"]].astype(np.float64)
    bound = (4 * -(-d // 256) + 6) * 2.0 ** -24 * r64["delta_mag"]
    err = np.abs(delta - r64["delta"])
    print(f"ATT_HALF_DELTA d={d} worst err/bound={float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    # (the bound is not vacuous: it is zero only where the forward output is -- no keys, or the code's one key dropped)
    assert np.count_nonzero(r64["delta_mag"]) >= int(0.8 * c["nq"])


@pytest.mark.parametrize("d,half", [(64, torch.float16), (128, torch.bfloat16), (256, torch.float16), (384, torch.bfloat16), (512, torch.float16),
                                    (640, torch.bfloat16), (768, torch.float16)], ids=lambda v: str(v).replace("torch.", ""))
def test_key_gradient_of_two_sources_in_one_launch_matches_the_sum_of_the_references(dev, d, half):
    """shared_kv_attention_dkv_multi: two sources over the same keys -- their own q_len vectors, seeds, dropout rates and scales --
    against the SUM of the two references, per code, the sources' spreads and flips added; a single source is the plain launch bit
    for bit; the accumulate=True form is held + plain bit for bit and touches no row it does not own."""
    from medtok_amd import ops
    sources, refs, plain = [], [], None
    kv = kv_start = kv_len = None
    for si in (0, 1):
        c = _case(d, None, si)
        t = _dev_args(c, dev)
        if si == 0:
            kv, kv_start, kv_len = t["kv"], t["kv_start"], t["kv_len"]
        else:
            t["kv"] = kv
        dq, delta = _call(ops.shared_kv_attention_backward_dq, c, t, half)
        sources.append(dict(q=t["q"], d_out=t["d_out"], lse=t["lse"], delta=delta, q_start=t["q_start"], q_len=t["q_len"], scale=c["scale"],
                            dropout_p=c["p"], seed=c["seed"]))
        refs.append(_reference(d, None, half, si))
        if si == 0:
            plain = _call(ops.shared_kv_attention_backward, c, t, half)[1]
            held = torch.from_numpy(np.random.default_rng(d).standard_normal((NK, d)).astype(np.float32)).to(dev)
            buf = held.clone()
            _, into = _call(ops.shared_kv_attention_backward, c, t, half, dkv_into=buf, accumulate=True)
            assert into is buf and torch.equal(buf, held + plain)
            own_k = torch.from_numpy(_own_rows(c["q_start"], c["q_len"], c["nq"])[1]).to(dev)
            assert torch.equal(buf[~own_k], held[~own_k])
    one = ops.shared_kv_attention_dkv_multi(sources[:1], kv, kv_start, kv_len, int(KV_LEN.max()), half=half)
    assert torch.equal(one, plain)
    both = ops.shared_kv_attention_dkv_multi(sources, kv, kv_start, kv_len, int(KV_LEN.max()), half=half).cpu().numpy()
    _check_codes(f"d={d} {str(half)[6:]} two-sources", "dkv", both, refs, KV_START, KV_LEN, half)
    own = _own_rows(SOURCES[0][0].cumsum() - SOURCES[0][0], SOURCES[0][0], 0)[1] | _own_rows(SOURCES[1][0].cumsum() - SOURCES[1][0], SOURCES[1][0], 0)[1]
    assert not both[~own].any()
