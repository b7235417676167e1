"""GPU: MedTokEmbedding.pooled_segments / ops.embed_pool_segments -- one row per (batch row, segment) from the token store
(embed_pool_segments_keys_kernel, the scan and stable radix sort, embed_pool_partial_kernel<.., LISTED>, embed_pool_finish_kernel) -- and
the gradients behind it.

Comparator: torch fp64 on the GPU over the rows `module(index, mask, validate=False)` returns (the existing lookup, never the code
under test): normalise each row over its full width if asked, sum per (b, v) with a dense 0 / 1 selector product (an id outside [0, V)
selects nothing), divide by the count, zeros for an empty segment.  Bar: the rel() <= 1e-5 of tests/test_gpu_embed_pool.py, of the
comparator's max magnitude; its derivation carries over because a bag here is at most L <= 300 rows of 8 .. 3072 floats: per row
~2^-24 relative from the squared norm's sum, its root, the reciprocal and the scaling, and the running sum of at most L rows adds at most
L * 2^-24 of a sum that the mean divides by the same count -- under 1e-6.  Every figure is printed before it is asserted.  The tables
are that file's: N_E = 96, regions text [0, 32), graph [64, 96), shared [0, 96), 50 codes."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
RTOL = 1e-5
N_E = 96
TYPES = {4: ("text", "graph", "shared", "shared"), 1: ("graph",)}        # one slot: a region that does not start at 0
NUM_CODES = 50
B = 3
GARBAGE = (-7, 2 ** 40)


def chunk():
    from medtok_amd import ops
    return ops.EMBED_POOL_CHUNK


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def table_case(e_dim, slots, k):
    """(tests/test_gpu_embed_pool.py::table_case) a VectorQuantizer(96, e_dim) with a random codebook and a random token table
    [NUM_CODES, slots, k] -- made once per shape and left unchanged"""
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    dev = torch.device("cuda:0")
    torch.manual_seed(e_dim * 100 + slots * 10 + k)
    v = VectorQuantizer(N_E, e_dim, 0.25, 0.0, True, True, [e_dim, e_dim], num_head=4 if e_dim % 4 == 0 else 2, k=k)
    with torch.no_grad():
        v.codebook.weight.normal_()
    v = v.to(dev).eval()
    types = TYPES[slots]
    gen = torch.Generator(device="cpu").manual_seed(k + 7)
    regions = [v._region(t) for t in types]
    tokens = torch.stack([torch.randint(0, hi - lo, (NUM_CODES, k), generator=gen) for lo, hi in regions], 1).to(dev)
    weights = torch.softmax(torch.randn(NUM_CODES, slots, k, generator=gen), -1).to(dev)
    return v, types, tokens, weights


def make_module(case, seed=0, **kw):
    from medtok_amd import MedTokEmbedding
    v, types, tokens, weights = case
    torch.manual_seed(seed)
    return MedTokEmbedding(v, tokens, weights, types=types, **kw)


def table64(v, types, tokens, weights, codebook=None):
    """(tests/test_gpu_embed_pool.py::table64) the fp64 embedding table [num_codes, S * e_dim], differentiable in `codebook`"""
    cb = v.codebook.weight.detach().double() if codebook is None else codebook
    lo = torch.tensor([v._region(t)[0] for t in types], device=tokens.device).view(1, -1, 1)
    return (weights.double()[..., None] * F.normalize(cb, dim=-1)[tokens + lo]).sum(2).reshape(tokens.shape[0], -1)


def segment_pool64(rows, seg, n_segments, mask, normalize):
    """the comparator's second half, fp64: rows [B, L, W] -> (out [B, V, W], count [B, V])"""
    rows = rows.double()
    if normalize:
        rows = rows / rows.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    select = seg.unsqueeze(-1) == torch.arange(n_segments, device=seg.device).view(1, 1, -1)          # [B, L, V]; a bad id selects nothing
    if mask is not None:
        select = select & ~mask.unsqueeze(-1)
    count = select.sum(1)
    sums = torch.einsum("blv,blw->bvw", select.double(), rows)
    out = torch.where(count.unsqueeze(-1) > 0, sums / count.clamp_min(1).unsqueeze(-1).double(), torch.zeros_like(sums))
    return out, count


def want_from_forward(module, index, seg, n_segments, mask, normalize):
    with torch.no_grad():
        return segment_pool64(module(index, padding_mask=mask, validate=False), seg, n_segments, mask, normalize)


def mask_patterns(rows, length, seed):
    """(tests/test_gpu_embed_pool.py::mask_patterns) none / a left-padded prefix per row / scattered / one row fully padded"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    at = torch.arange(length).expand(rows, length)
    prefix = at < (torch.tensor([0.0, 0.4, 0.9])[torch.arange(rows) % 3] * length).floor().long().view(-1, 1)
    scattered = torch.rand(rows, length, generator=gen) < 0.5
    full = scattered.clone()
    full[1 % rows] = True
    return {"none": None, "prefix": prefix, "scattered": scattered, "one row padded": full}


def index_patterns(rows, length, seed):
    """(tests/test_gpu_embed_pool.py::index_patterns)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    n = rows * length
    perm = torch.randperm(NUM_CODES, generator=gen).repeat(n // NUM_CODES + 1)[:n]
    mixed = torch.randint(0, NUM_CODES, (n,), generator=gen)
    mixed[torch.rand(n, generator=gen) < 0.2] = NUM_CODES
    return {"permutation": perm.view(rows, length), "one code": torch.full((rows, length), int(torch.randint(0, NUM_CODES, (1,), generator=gen))),
            "all miss": torch.full((rows, length), NUM_CODES), "mixed": mixed.view(rows, length)}


def with_garbage(t, mask):
    """garbage below the mask (code indices and segment ids alike): those positions must not be read"""
    if mask is None:
        return t
    t = t.clone()
    t[mask] = torch.tensor(GARBAGE)[torch.arange(int(mask.sum())) % 2]
    return t


def segment_lengths(c):
    """one segment of each length C - 1, C, C + 1, 3 C + 5, and one of a single position"""
    return [c - 1, c, c + 1, 3 * c + 5, 1]


def segment_patterns(n_segments, seed):
    """name -> segment_id [B, L].  V = 5, L = 6 C + 6, no mask: every row has one segment of each of segment_lengths()
    ("ascending", row r with the lengths rotated by r, so each segment id meets several lengths; in row 0 segment 4's only position is the
    row's last), "descending" the same runs reversed, "shuffled" the same multiset in random order along the row, "interleaved" segments 0
    and 1 taking turns position by position (3 C + 3 each, never contiguous) and the others empty, "all in one" every position in the last
    segment and the others empty.  V = 1: the one pattern there is; the lengths come from L."""
    c = chunk()
    lens = segment_lengths(c)
    length = sum(lens)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    asc = torch.stack([torch.repeat_interleave(torch.arange(5), torch.tensor(lens[-r:] + lens[:-r] if r else lens)) for r in range(B)])
    assert n_segments == 5 and asc.shape == (B, length)
    shuffled = torch.stack([row[torch.randperm(length, generator=gen)] for row in asc])
    return {"ascending": asc, "descending": asc.flip(1), "shuffled": shuffled, "interleaved": (torch.arange(length) % 2).expand(B, length).clone(),
            "all in one": torch.full((B, length), 4)}


def check_values(m, index, seg, n_segments, mask, label):
    """both normalize values against the comparator; two calls and both validate values give the same bits; `empty` is the comparator's"""
    worst = 0.0
    for normalize in (True, False):
        want, count = want_from_forward(m, index, seg, n_segments, mask, normalize)
        with torch.no_grad():
            got, empty = m.pooled_segments(index, seg, n_segments, padding_mask=mask, normalize=normalize)
            again, empty2 = m.pooled_segments(index, seg, n_segments, padding_mask=mask, normalize=normalize, validate=False)
        err = rel(got, want)
        worst = max(worst, err)
        print(f"{label} normalize={normalize}: rel {err:.3e}")
        assert got.shape == want.shape and got.dtype == torch.float32 and empty.shape == count.shape and empty.dtype == torch.bool
        assert torch.isfinite(got).all()
        assert err <= RTOL, (label, normalize, err)
        assert torch.equal(got, again) and torch.equal(empty, empty2)          # two calls, validate or not: the same bits
        assert torch.equal(empty, count == 0)
        assert not bool(got[empty].any())                                      # an empty segment: zeros
    return worst


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("n_segments", [1, 5])
@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("d,k", [(8, 1), (40, 9), (64, 5), (64, 16), (768, 5)])
def test_values(dev, d, k, slots, n_segments):
    m = make_module(table_case(d, slots, k), seed=d + k)
    c = chunk()
    if n_segments == 1:
        layouts = {f"L={length}": torch.zeros(B, length, dtype=torch.int64) for length in (c - 1, c, c + 1, 3 * c + 5)}
    else:
        layouts = segment_patterns(n_segments, seed=d)
    worst = 0.0
    for sname, seg in layouts.items():
        length = seg.shape[1]
        for mname, mask in mask_patterns(B, length, seed=length).items():
            for iname, index in index_patterns(B, length, seed=length + 1).items():
                index, ids = with_garbage(index, mask).to(dev), with_garbage(seg, mask).to(dev)
                mk = None if mask is None else mask.to(dev)
                worst = max(worst, check_values(m, index, ids, n_segments, mk, f"d={d} k={k} S={slots} V={n_segments} {sname} mask={mname} index={iname}"))
    print(f"d={d} k={k} S={slots} V={n_segments}: worst rel vs fp64 {worst:.3e}")


def test_padded_e_dim_and_a_projector(dev):
    """e_dim = 10 (the codebook is padded to 12 columns for the kernels, and the zero columns are sliced off); rows of 3200 floats (the
    widest instantiation); a projector on the B * V pooled rows, an empty segment giving the bias row"""
    for d, k, slots in ((10, 5, 4), (800, 9, 4)):
        m = make_module(table_case(d, slots, k), seed=5)
        seg = segment_patterns(5, seed=2)["shuffled"]
        mask = mask_patterns(B, seg.shape[1], seed=3)["scattered"]
        index = torch.randint(0, NUM_CODES + 1, seg.shape, generator=torch.Generator(device="cpu").manual_seed(d))
        check_values(m, with_garbage(index, mask).to(dev), with_garbage(seg, mask).to(dev), 5, mask.to(dev), f"d={d}")
    case = table_case(64, 4, 5)
    torch.manual_seed(3)
    proj = nn.Linear(256, 6).to(dev)
    m = make_module(case, seed=5, projector=proj)
    plain = make_module(case, seed=5)
    seg = segment_patterns(5, seed=4)["interleaved"].to(dev)
    index = index_patterns(B, seg.shape[1], seed=6)["mixed"].to(dev)
    with torch.no_grad():
        got, empty = m.pooled_segments(index, seg, 5)
        base, empty0 = plain.pooled_segments(index, seg, 5)
    want = F.linear(base.double(), proj.weight.double(), proj.bias.double())
    print(f"projector: rel {rel(got, want):.3e}")
    assert got.shape == (B, 5, 6) and rel(got, want) <= RTOL and torch.equal(empty, empty0) and bool(empty[:, 2:].all())
    assert torch.equal(got[empty], proj.bias.detach().expand(int(empty.sum()), 6))


# ------------------------------------------------------------------ 2. bit-level pins of the order
@pytest.mark.parametrize("d,k,slots", [(8, 1, 1), (64, 5, 4), (768, 5, 4)])
def test_one_segment_without_a_mask_is_pooled(dev, d, k, slots):
    m = make_module(table_case(d, slots, k), seed=1)
    c = chunk()
    for length in (c - 1, c, c + 1, 3 * c + 5):
        index = index_patterns(B, length, seed=length)["mixed"].to(dev)
        seg = torch.zeros(B, length, dtype=torch.int64, device=dev)
        for normalize in (True, False):
            with torch.no_grad():
                got, empty = m.pooled_segments(index, seg, 1, normalize=normalize)
                want = m.pooled(index, normalize=normalize)
            assert torch.equal(got[:, 0], want), (length, normalize)
            assert not bool(empty.any())


@pytest.mark.parametrize("d,k,slots", [(8, 1, 1), (64, 5, 4), (768, 5, 4)])
def test_a_segment_of_one_position_is_the_forward_row(dev, d, k, slots):
    m = make_module(table_case(d, slots, k), seed=1)
    length = chunk() + 3
    gen = torch.Generator(device="cpu").manual_seed(d)
    index = torch.randint(0, NUM_CODES + 1, (B, length), generator=gen)
    index[1, 2] = NUM_CODES                                                    # a miss row among them
    seg = torch.stack([torch.randperm(length, generator=gen) for _ in range(B)])   # every segment: exactly one position, in any order
    index, seg = index.to(dev), seg.to(dev)
    with torch.no_grad():
        rows = m(index)
        got, empty = m.pooled_segments(index, seg, length, normalize=False)
    want = torch.empty_like(rows)
    want[torch.arange(B).view(-1, 1), seg] = rows
    assert torch.equal(got, want) and not bool(empty.any())
    assert torch.equal(got[1, seg[1, 2]], m.miss_emb.detach()[0])


def test_relabelling_the_segments_permutes_the_rows(dev):
    m = make_module(table_case(64, 4, 5), seed=2)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for sname, seg in segment_patterns(5, seed=7).items():
        mask = mask_patterns(B, seg.shape[1], seed=8)["scattered"].to(dev)
        index = index_patterns(B, seg.shape[1], seed=9)["mixed"].to(dev)
        perm = torch.randperm(5, generator=gen)
        for normalize in (True, False):
            with torch.no_grad():
                got, empty = m.pooled_segments(index, seg.to(dev), 5, padding_mask=mask, normalize=normalize)
                moved, moved_empty = m.pooled_segments(index, perm[seg].to(dev), 5, padding_mask=mask, normalize=normalize)
            assert torch.equal(moved[:, perm], got) and torch.equal(moved_empty[:, perm], empty), sname


def test_counts_and_garbage_under_the_mask(dev):
    """counts = (unpadded positions, unpadded miss positions) per segment; code indices and segment ids under the mask are not read"""
    from medtok_amd import ops
    v, types, tokens, weights = table_case(64, 4, 5)
    m = make_module((v, types, tokens, weights), seed=2)
    seg = segment_patterns(5, seed=10)["shuffled"]
    length = seg.shape[1]
    mask = mask_patterns(B, length, seed=11)["scattered"]
    clean = index_patterns(B, length, seed=12)["mixed"]
    clean[mask] = 0
    clean_seg = seg.clone()
    clean_seg[mask] = 0
    what = v._normalised_codebook()[0]
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in types)]
    outs = []
    for index, ids in ((clean, clean_seg), (with_garbage(clean, mask), with_garbage(seg, mask))):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out, counts = ops.embed_pool_segments(index.to(dev), ids.to(dev), 5, tokens, weights, what, regions, miss=m.miss_emb.detach().reshape(-1),
                                              pad_mask=mask.to(dev), normalize=True, status=status)
        assert int(status.item()) == 0
        outs.append((out, counts))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    select = (seg.unsqueeze(-1) == torch.arange(5).view(1, 1, -1)) & ~mask.unsqueeze(-1)
    live = select.sum(1)
    missed = (select & (clean == NUM_CODES).unsqueeze(-1)).sum(1)
    assert torch.equal(outs[0][1].cpu(), torch.stack([live, missed], -1).int())
    # the same ids at unpadded positions are errors; under the mask they raise nothing and change nothing
    with torch.no_grad():
        got, empty = m.pooled_segments(with_garbage(clean, mask).to(dev), with_garbage(seg, mask).to(dev), 5, padding_mask=mask.to(dev), normalize=True)
    assert torch.equal(got, outs[0][0]) and torch.equal(empty, outs[0][1][..., 0] == 0)


# ------------------------------------------------------------------ 3. errors and bad ids
def test_bad_segment_ids(dev):
    from medtok_amd import ops
    v, types, tokens, weights = table_case(64, 4, 5)
    m = make_module((v, types, tokens, weights), seed=3)
    n_segments = 5
    seg = segment_patterns(n_segments, seed=1)["ascending"]
    length = seg.shape[1]
    index = index_patterns(B, length, seed=4)["mixed"].to(dev)
    mask = torch.zeros(B, length, dtype=torch.bool)
    mask[0, 3], mask[2, length - 1] = True, True
    with torch.no_grad():
        clean, clean_empty = m.pooled_segments(index, seg.to(dev), n_segments, padding_mask=mask.to(dev))
    for bad_id in (-1, n_segments):
        under = seg.clone()
        under[0, 3], under[2, length - 1] = bad_id, bad_id                     # under the mask: nothing is raised, nothing changes
        with torch.no_grad():
            got, empty = m.pooled_segments(index, under.to(dev), n_segments, padding_mask=mask.to(dev))
        assert torch.equal(got, clean) and torch.equal(empty, clean_empty)
        bad = seg.clone()
        bad[1, 5], bad[2, 0] = bad_id, bad_id                                  # at unpadded positions
        with pytest.raises(ValueError, match="segment id"):
            m.pooled_segments(index, bad.to(dev), n_segments, padding_mask=mask.to(dev))
        with pytest.raises(ValueError, match="segment id"):
            m.pooled_segments(index, bad.to(dev), n_segments)
        # validate=False: the position joins no segment -- the comparator's selector drops it
        for normalize in (True, False):
            want, count = want_from_forward(m, index, bad.to(dev), n_segments, mask.to(dev), normalize)
            with torch.no_grad():
                got, empty = m.pooled_segments(index, bad.to(dev), n_segments, padding_mask=mask.to(dev), normalize=normalize, validate=False)
            print(f"bad id {bad_id} normalize={normalize}: rel {rel(got, want):.3e}")
            assert rel(got, want) <= RTOL and torch.equal(empty, count == 0)
        what = v._normalised_codebook()[0]
        regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in types)]
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _, counts = ops.embed_pool_segments(index, bad.to(dev), n_segments, tokens, weights, what, regions, miss=m.miss_emb.detach().reshape(-1),
                                            status=status)
        assert int(status.item()) == 1 << ops.EMBED_BAD_SEGMENT_BIT
        assert int(counts[..., 0].sum()) == B * length - 2


def test_bad_index_and_bad_slot(dev):
    from medtok_amd import MedTokEmbedding, ops
    v, types, tokens, weights = table_case(64, 4, 5)
    m = make_module((v, types, tokens, weights), seed=3)
    n_segments = 5
    seg = segment_patterns(n_segments, seed=1)["shuffled"].to(dev)
    length = seg.shape[1]
    index = index_patterns(B, length, seed=4)["mixed"].to(dev)
    bad = index.clone()
    bad[0, 1], bad[2, length - 1] = NUM_CODES + 3, -1
    with pytest.raises(ValueError, match="code index"):
        m.pooled_segments(bad, seg, n_segments)
    bad_seg = seg.clone()
    bad_seg[1, 1] = n_segments
    with pytest.raises(ValueError, match="code index"):                        # forward's errors come before the segment id's
        m.pooled_segments(bad, bad_seg, n_segments)
    # validate=False: a row of zeros that counts in its segment -- what forward(validate=False) gives, so the comparator as it stands
    for normalize in (True, False):
        want, count = want_from_forward(m, bad, seg, n_segments, None, normalize)
        with torch.no_grad():
            got, empty = m.pooled_segments(bad, seg, n_segments, normalize=normalize, validate=False)
        assert rel(got, want) <= RTOL and torch.equal(empty, count == 0)
    what = v._normalised_codebook()[0]
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in types)]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _, counts = ops.embed_pool_segments(bad, seg, n_segments, tokens, weights, what, regions, miss=m.miss_emb.detach().reshape(-1), status=status)
    assert int(status.item()) == 1 << ops.EMBED_BAD_INDEX_BIT
    assert int(counts[..., 0].sum()) == B * length                             # the bad positions count
    # a token id outside its region in slot 2 of code 7: forward's error, before the segment id's
    broken = tokens.clone()
    broken[7, 2, 1] = N_E
    mb = MedTokEmbedding(v, broken, weights, types=types)
    mb.miss_emb = m.miss_emb
    hit = index.clone()
    hit[1, 0] = 7
    for ids in (seg, bad_seg):
        with pytest.raises(ValueError, match="slot 2"):
            mb.pooled_segments(hit, ids, n_segments)
    for normalize in (True, False):
        want, _ = want_from_forward(mb, hit, seg, n_segments, None, normalize)
        with torch.no_grad():
            got, _ = mb.pooled_segments(hit, seg, n_segments, normalize=normalize, validate=False)
        assert rel(got, want) <= RTOL


# ------------------------------------------------------------------ 4. gradients
def grad_inputs(dev, n_segments):
    """row 0 mixed with misses, row 1 without a miss, row 2 fully padded, row 3 all miss; shuffled segments, one of them empty"""
    length = 3 * chunk() + 5
    gen = torch.Generator(device="cpu").manual_seed(length)
    index = torch.randint(0, NUM_CODES, (4, length), generator=gen)
    index[0, torch.rand(length, generator=gen) < 0.3] = NUM_CODES
    index[0, 0] = NUM_CODES
    index[3] = NUM_CODES
    mask = torch.rand(4, length, generator=gen) < 0.3
    mask[0, 0] = False
    mask[2] = True
    seg = torch.randint(0, n_segments - 1, (4, length), generator=gen)         # the last segment stays empty
    seg[0, :chunk() + 3] = 0                                                    # a segment of several chunks
    return with_garbage(index, mask).to(dev), with_garbage(seg, mask).to(dev), mask.to(dev)


def composition64(t64, miss64, index, seg, n_segments, mask, normalize, w64=None, b64=None):
    safe = torch.where(mask, 0, index)
    rows = torch.cat([t64, miss64.reshape(1, -1)], 0)[safe]
    out, _ = segment_pool64(rows, seg, n_segments, mask, normalize)
    return out if w64 is None else F.linear(out, w64, b64)


@pytest.mark.parametrize("d,k,slots", [(64, 5, 4), (10, 5, 4), (768, 5, 1)])
def test_miss_row_and_projector_gradients(dev, d, k, slots):
    case = table_case(d, slots, k)
    t64 = table64(*case)
    n_segments = 4
    index, seg, mask = grad_inputs(dev, n_segments)
    for normalize in (True, False):
        for h in (None, 6):
            torch.manual_seed(h or 1)
            proj = None if h is None else nn.Linear(slots * d, h).to(dev)
            m = make_module(case, seed=7, projector=proj)
            up = torch.randn(4, n_segments, h or slots * d, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
            grads = []
            for _ in range(2):
                m.zero_grad(set_to_none=True)
                out, _ = m.pooled_segments(index, seg, n_segments, padding_mask=mask, normalize=normalize)
                (out * up).sum().backward()
                grads.append([p.grad.clone() for p in m.parameters()])
            for a, b in zip(*grads):
                assert torch.equal(a, b)                                             # two backward runs, the same bits
            miss64 = m.miss_emb.detach().double().requires_grad_()
            leaves = [miss64]
            w64 = b64 = None
            if proj is not None:
                w64, b64 = proj.weight.detach().double().requires_grad_(), proj.bias.detach().double().requires_grad_()
                leaves += [w64, b64]
            want = composition64(t64, miss64, index, seg, n_segments, mask, normalize, w64, b64)
            (want * up.double()).sum().backward()
            print(f"d={d} S={slots} normalize={normalize} H={h}: out rel {rel(out, want):.3e}")
            assert rel(out, want) <= RTOL
            got = {"miss_emb": m.miss_emb.grad}
            if proj is not None:
                got.update({"projector.weight": proj.weight.grad, "projector.bias": proj.bias.grad})
            for (name, g), leaf in zip(got.items(), leaves):
                err = rel(g.reshape(leaf.shape), leaf.grad)
                print(f"d={d} S={slots} normalize={normalize} H={h}: d {name} rel {err:.3e}")
                assert err <= RTOL, (name, err)


def test_codebook_gradient_through_the_composed_route(dev):
    from medtok_amd import MedTokEmbedding
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    _, types, tokens, weights = table_case(64, 4, 5)
    torch.manual_seed(21)
    v = VectorQuantizer(N_E, 64, 0.25, 0.0, True, True, [64, 64], num_head=4, k=5)
    with torch.no_grad():
        v.codebook.weight.normal_()
    v = v.to(dev)
    m = MedTokEmbedding(v, tokens, weights, types=types, freeze_codebook=False)
    n_segments = 4
    index, seg, mask = grad_inputs(dev, n_segments)
    up = torch.randn(4, n_segments, 256, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    for normalize in (True, False):
        m.zero_grad(set_to_none=True)
        v.zero_grad(set_to_none=True)
        out, empty = m.pooled_segments(index, seg, n_segments, padding_mask=mask, normalize=normalize)
        (out * up).sum().backward()
        cb64 = v.codebook.weight.detach().double().requires_grad_()
        miss64 = m.miss_emb.detach().double().requires_grad_()
        want = composition64(table64(v, types, tokens, weights, codebook=cb64), miss64, index, seg, n_segments, mask, normalize)
        (want * up.double()).sum().backward()
        errs = rel(out, want), rel(v.codebook.weight.grad, cb64.grad), rel(m.miss_emb.grad.reshape(-1), miss64.grad)
        print(f"composed route normalize={normalize}: rel out / d codebook / d miss {errs}")
        assert max(errs) <= RTOL
        with torch.no_grad():                                                    # and the kernels give the same function
            fused, fused_empty = m.pooled_segments(index, seg, n_segments, padding_mask=mask, normalize=normalize)
        assert rel(fused, want) <= RTOL and torch.equal(fused_empty, empty)
    bad = seg.clone()
    bad[0, 0] = n_segments
    with pytest.raises(ValueError, match="segment id"):
        m.pooled_segments(index, bad, n_segments, padding_mask=mask)


# ------------------------------------------------------------------ 5. graph
def test_step_replayed_from_a_hip_graph_is_bit_equal_to_eager(dev):
    """a validate=False call, forward and the miss row's backward: every step is a kernel launch and nothing is read back"""
    m = make_module(table_case(64, 4, 5), seed=9)
    n_segments = 5
    shape = (6, 3 * chunk() + 5)
    up = torch.randn(shape[0], n_segments, 256, device=dev, generator=torch.Generator(device=dev).manual_seed(2))

    def draw(seed):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        index = torch.randint(0, NUM_CODES + 1, shape, generator=gen)
        mask = torch.rand(shape, generator=gen) < 0.3
        seg = torch.randint(0, n_segments, shape, generator=gen)
        seg[0] = seed % n_segments                                             # a segment of several chunks
        return with_garbage(index, mask).to(dev), with_garbage(seg, mask).to(dev), mask.to(dev)
    index, seg, mask = draw(0)

    def step(index, seg, mask):
        out, empty = m.pooled_segments(index, seg, n_segments, padding_mask=mask, normalize=True, validate=False)
        return (out.detach(), empty) + torch.autograd.grad((out * up).sum(), [m.miss_emb])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up: the normalised codebook is cached, the library loaded
        step(index, seg, mask)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(index, seg, mask)
    for seed in (1, 2):
        fresh = draw(seed)
        for t, f in zip((index, seg, mask), fresh):
            t.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*fresh)
        assert len(eager) == len(captured) and all(torch.equal(a, b) for a, b in zip(captured, eager))
        assert float(eager[2].abs().max()) > 0


# ------------------------------------------------------------------ 6. many mostly-empty bags
def test_many_mostly_empty_bags(dev):
    """B = 64, V = 300, L = 20: 19,200 bags for 1,280 positions -- only short bags, finished by their own block without a partial row"""
    m = make_module(table_case(64, 4, 5), seed=4)
    batch, n_segments, length = 64, 300, 20
    gen = torch.Generator(device="cpu").manual_seed(6)
    index = torch.randint(0, NUM_CODES + 1, (batch, length), generator=gen)
    seg = torch.sort(torch.randint(0, n_segments, (batch, length), generator=gen), 1).values
    mask = torch.rand(batch, length, generator=gen) < 0.4
    index, seg, mask = with_garbage(index, mask).to(dev), with_garbage(seg, mask).to(dev), mask.to(dev)
    worst = check_values(m, index, seg, n_segments, mask, "many bags")
    with torch.no_grad():
        got, empty = m.pooled_segments(index, seg, n_segments, padding_mask=mask)
    assert got.shape == (batch, n_segments, 256) and int(empty.sum()) > batch * (n_segments - length)
    assert not bool(got[empty].any())                                          # every empty bag: zeros
    print(f"many bags: worst rel {worst:.3e}")
