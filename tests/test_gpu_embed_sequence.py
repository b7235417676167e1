"""GPU: MedTokEmbedding.sequence -- the consumer's input sequence (lookup + position rows + segment rows behind prefix rows) in the
lookup's launch (ops.embed_sequence, embed_folded_kernel) or, where the lookup does not run over folded tables, in one elementwise
launch over its fp32 rows (ops.embed_sequence_rows) -- and the gradients of the additive parts.

The comparator is the composition a user writes today, in torch on the module's own `forward`:

    r   = forward(index, mask, out_dtype=float32)
    x   = ((r + pe[:L]) + R0[b, g]) + R1[b, g]          g = segment_id[b, p]
    seq = cat([prefix, where(mask, r, x)], 1)

Values are compared bit for bit (fp32; 16-bit outputs against the fp32 result converted).  Gradients of the additive parts are compared
with the same composition in fp64 under autograd: exactly where the upstream gradient is integer-valued (every partial sum is then exact in
fp32 whatever the order), and otherwise per element within (m + 1) * 2^-24 * sum |g_i| over the element's m contributions -- the bound of
a recursive fp32 sum of m terms ((m - 1) roundings of at most 2^-24 of a partial sum that never exceeds sum |g_i|, first order), with two
roundings of slack; m and sum |g_i| are counted by running the comparator's backward on ones and on |g|."""
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
N_E = 96                                           # text [0, 32), graph [64, 96), shared [0, 96): regions of >= 16 codes (k = 16)
TYPES = {4: ("text", "graph", "shared", "shared"), 3: ("text", "graph", "shared"), 1: ("graph",)}
NUM_CODES = 50
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def table_case(e_dim, slots, k):
    """a VectorQuantizer(96, e_dim) with a random codebook and a random token table [NUM_CODES, slots, k]: made once per shape"""
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


def module(e_dim, slots, k, h=None, fold=None, seed=0, **kw):
    """a MedTokEmbedding over table_case(e_dim, slots, k); h: the projector's width (None: no projector)"""
    from medtok_amd import MedTokEmbedding
    v, types, tokens, weights = table_case(e_dim, slots, k)
    torch.manual_seed(seed)
    if h is not None:
        kw.update(projector=nn.Linear(slots * e_dim, h).to(tokens.device), fold=fold)
    return MedTokEmbedding(v, tokens, weights, types=types, **kw)


def draw(dev, batch, length, n_segments, n_prefix, width, seed, mask="scattered", miss=0.2, monotone=True):
    """-> dict(index, mask, seg, pe, r0, r1, prefix): about `miss` of the positions at the miss index; mask: None, "prefix" (each batch
    row keeps its first positions), "scattered", "row" (scattered, and batch row 1 fully padded); garbage below the mask; segment ids
    monotone along a row (visits in time order) or shuffled; pe holds two rows more than the positions"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    index = torch.randint(0, NUM_CODES, (batch, length), generator=gen)
    index[torch.rand(batch, length, generator=gen) < miss] = NUM_CODES
    seg = torch.randint(0, n_segments, (batch, length), generator=gen)
    seg = seg.sort(1).values if monotone else seg
    if mask is None:
        m = None
    else:
        if mask == "prefix":
            keep = torch.randint(0, length + 1, (batch, 1), generator=gen)
            m = torch.arange(length).view(1, -1) >= keep
        else:
            m = torch.rand(batch, length, generator=gen) < 0.3
            if mask == "row":
                m[1 % batch] = True
        n_bad = int(m.sum())
        index[m] = torch.tensor([-7, 2 ** 62, NUM_CODES + 3])[torch.arange(n_bad) % 3]
        seg[m] = torch.tensor([-7, 2 ** 40, n_segments])[torch.arange(n_bad) % 3]
    f = lambda *shape: torch.randn(*shape, generator=gen)
    out = dict(index=index, mask=m, seg=seg, pe=f(length + 2, width), r0=f(batch, n_segments, width), r1=f(batch, n_segments, width),
               prefix=f(batch, n_prefix, width))
    return {k: (None if t is None else t.to(dev)) for k, t in out.items()}


def compose(r, d, pe=True, r0=True, r1=True, prefix=True, drop_segments=None):
    """the composition on the lookup's rows r [B, L, W] (any float dtype: fp64 for the gradients' comparator); drop_segments: a bool
    [B, L] of positions that take no segment term (a bad id under validate=False)"""
    batch, length, _ = r.shape
    as_r = lambda t: t.to(r.dtype) if t.dtype != r.dtype else t
    x = r
    if pe and d["pe"] is not None:
        x = x + as_r(d["pe"])[:length]
    if r0 and d["seg"] is not None:
        n_segments = d["r0"].shape[1]
        ok = (d["seg"] >= 0) & (d["seg"] < n_segments)
        if drop_segments is not None:
            ok = ok & ~drop_segments
        g = torch.where(ok, d["seg"], 0)
        rows = torch.arange(batch, device=r.device).view(-1, 1)
        y = x + as_r(d["r0"])[rows, g]
        if r1:
            y = y + as_r(d["r1"])[rows, g]
        x = torch.where(ok.unsqueeze(-1), y, x)
    if d["mask"] is not None:
        x = torch.where(d["mask"].unsqueeze(-1), r, x)
    return torch.cat([as_r(d["prefix"]), x], 1) if prefix else x


def run(m, d, pe=True, r0=True, r1=True, prefix=True, **kw):
    terms = ([d["r0"]] if r0 else []) + ([d["r1"]] if r0 and r1 else [])
    return m.sequence(d["index"], d["mask"], position_rows=d["pe"] if pe else None, segment_id=d["seg"] if terms else None,
                      segment_rows=terms or None, prefix=d["prefix"] if prefix else None, **kw)


def check_values(m, d, **parts):
    """fp32 bit for bit against the composition, both 16-bit outputs against the fp32 result converted, the key mask"""
    with torch.no_grad():
        r = m(d["index"], d["mask"], out_dtype=torch.float32)
        want = compose(r, d, **parts)
        got, keys = run(m, d, **parts)
        assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got, want), f"max |diff| {float((got - want).abs().max())}"
        n_prefix = want.shape[1] - r.shape[1]
        assert keys.dtype == torch.bool and keys.shape == want.shape[:2] and not bool(keys[:, :n_prefix].any())
        assert torch.equal(keys[:, n_prefix:], d["mask"] if d["mask"] is not None else torch.zeros_like(keys[:, n_prefix:]))
        for dtype in (torch.float16, torch.bfloat16):
            half, _ = run(m, d, out_dtype=dtype, **parts)
            assert half.dtype == dtype and torch.equal(half, got.to(dtype))
    return got


# ------------------------------------------------------------------ 1. values over the folded tables
@pytest.mark.parametrize("n_prefix", [0, 3])
@pytest.mark.parametrize("slots,k,h", [(1, 5, 64), (4, 5, 64), (4, 16, 256), (4, 5, 300), (4, 5, 70)])
def test_folded_values(dev, slots, k, h, n_prefix):
    """16-lane groups, 32-lane groups, 64 entries per code, two column passes, a padded H; B * (P + L) = 3 * 37 (+ 9) rows are no
    multiple of the 4 / 8 / 16 rows a block holds; miss positions and a scattered mask with garbage below it"""
    m = module(64, slots, k, h, fold=True, seed=h)
    d = draw(dev, 3, 37, 5, n_prefix, h, seed=h + n_prefix)
    assert int((d["index"] == NUM_CODES).sum()) > 0 and bool(d["mask"].any())
    check_values(m, d)
    assert m.fold_builds == 1


# ------------------------------------------------------------------ 2. the rows form
@pytest.mark.parametrize("e_dim,slots,h,fold", [(64, 4, None, None), (10, 3, None, None), (64, 4, 256, False)])
def test_rows_form_values(dev, e_dim, slots, h, fold):
    """no projector (W = 256), no projector at e_dim = 10 with three slots (W = 30: no multiple of 4, and the codebook is padded to 12
    columns for the lookup), an unfolded projector"""
    m = module(e_dim, slots, 5, h, fold=fold, seed=3)
    width = h or slots * e_dim
    for n_prefix in (0, 3):
        check_values(m, draw(dev, 3, 37, 5, n_prefix, width, seed=e_dim + n_prefix))
    assert getattr(m, "fold_builds", 0) == 0


# ------------------------------------------------------------------ 3. optional parts, masks
@pytest.mark.parametrize("form", ["folded", "rows"])
def test_each_part_absent_and_every_mask(dev, form):
    m = module(64, 4, 5, 64, fold=True, seed=1) if form == "folded" else module(64, 4, 5)
    width = 64 if form == "folded" else 256
    for mask in (None, "prefix", "scattered", "row"):
        d = draw(dev, 3, 37, 5, 3, width, seed=11, mask=mask)
        check_values(m, d)
        if mask == "row":
            with torch.no_grad():                                  # a fully padded batch row: the lookup's rows, nothing added
                assert torch.equal(run(m, d)[0][1, 3:], m(d["index"], d["mask"])[1])
    d = draw(dev, 3, 37, 5, 3, width, seed=12)
    for absent in ("pe", "r0", "r1", "prefix"):
        check_values(m, d, **{absent: False})
    got = check_values(m, d, pe=False, r0=False, prefix=False)
    with torch.no_grad():
        assert torch.equal(got, m(d["index"], d["mask"]))            # with none of them: forward
        bare = draw(dev, 3, 37, 5, 0, width, seed=13, mask=None)
        seq, keys = m.sequence(bare["index"])
        assert torch.equal(seq, m(bare["index"])) and keys.shape == (3, 37) and not bool(keys.any())
    one, _ = m.sequence(d["index"], d["mask"], segment_id=d["seg"], segment_rows=d["r0"])       # one tensor in place of a sequence
    assert torch.equal(one.detach(), check_values(m, d, pe=False, r1=False, prefix=False))


# ------------------------------------------------------------------ 4. garbage under the mask, bad ids outside it
@pytest.mark.parametrize("form", ["folded", "rows"])
def test_garbage_under_the_mask_and_bad_ids(dev, form):
    from medtok_amd import ops
    m = module(64, 4, 5, 64, fold=True, seed=2) if form == "folded" else module(64, 4, 5)
    width = 64 if form == "folded" else 256
    d = draw(dev, 3, 37, 5, 3, width, seed=21)
    clean = dict(d)
    clean["index"] = torch.where(d["mask"], 0, d["index"])
    clean["seg"] = torch.where(d["mask"], 0, d["seg"])
    assert int((d["index"][d["mask"]] == 2 ** 62).sum()) > 0 and int((d["seg"][d["mask"]] == 2 ** 40).sum()) > 0
    with torch.no_grad():
        got = run(m, d, validate=True)[0]                            # does not raise
        assert torch.equal(got, run(m, clean)[0])
        # the status word of the launch itself: zero, as for clean inputs
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        parts = dict(pad_mask=d["mask"], position_rows=d["pe"], segment_id=d["seg"], segment_rows=[d["r0"], d["r1"]], prefix=d["prefix"], status=status)
        if form == "folded":
            p, q = m.projector, m.quantizer
            folded = ops.fold_projector(q._normalised_codebook()[0], m._regions(), p.weight.detach(), p.bias.detach(), m.miss_emb.detach().reshape(-1),
                                        e_dim=q.e_dim)
            low = ops.embed_sequence(d["index"], m.tokens, m.weights, *folded[:3], miss_row=folded[3], **parts)
        else:
            low = ops.embed_sequence_rows(m(d["index"], d["mask"]), **parts)
        assert torch.equal(low, got) and int(status.item()) == 0
        # bad segment ids at unpadded positions
        spots = (~d["mask"]).nonzero()[:2]
        for bad in (5, -1):
            broken = dict(d)
            broken["seg"] = d["seg"].clone()
            broken["seg"][spots[0, 0], spots[0, 1]] = bad
            with pytest.raises(ValueError, match="segment id"):
                run(m, broken)
            quiet = run(m, broken, validate=False)[0]
            drop = torch.zeros_like(d["mask"])
            drop[spots[0, 0], spots[0, 1]] = True
            assert torch.equal(quiet, compose(m(d["index"], d["mask"]), broken, drop_segments=drop))
            keep = ~drop
            assert torch.equal(quiet[:, 3:][keep], got[:, 3:][keep]) and not torch.equal(quiet[:, 3:][drop], got[:, 3:][drop])
        # a bad code index together with a bad segment id: the "code index" message wins
        broken["index"] = d["index"].clone()
        broken["index"][spots[1, 0], spots[1, 1]] = NUM_CODES + 1
        with pytest.raises(ValueError, match="code index"):
            run(m, broken)
        quiet = run(m, broken, validate=False)[0]                    # the bad index takes the adds like any unpadded position
        assert torch.equal(quiet, compose(m(broken["index"], d["mask"], validate=False), broken, drop_segments=drop))
        assert torch.equal(run(m, d)[0], got)


# ------------------------------------------------------------------ 5. gradients of the additive parts
def part_grads64(d, upstream, n_prefix):
    """d position_rows, d R0, d R1, d prefix of the composition in fp64 under autograd for the upstream gradient `upstream` (fp64).  The
    lookup's rows are constants of these gradients: zeros stand in."""
    leaves = {k: d[k].double().requires_grad_(True) for k in ("pe", "r0", "r1", "prefix")}
    dd = dict(d)
    dd.update(leaves)
    zeros = torch.zeros(d["index"].shape + (d["pe"].shape[1],), dtype=torch.float64, device=d["pe"].device)
    (compose(zeros, dd) * upstream).sum().backward()
    return [leaves[k].grad for k in ("pe", "r0", "r1", "prefix")]


def part_grads(m, d, upstream, out_dtype=None):
    leaves = [d[k].clone().requires_grad_(True) for k in ("pe", "r0", "r1", "prefix")]
    dd = dict(d)
    dd.update(zip(("pe", "r0", "r1", "prefix"), leaves))
    m.zero_grad()
    seq, _ = run(m, dd, out_dtype=out_dtype)
    seq.backward(upstream.to(seq.dtype))
    return [t.grad for t in leaves]


@pytest.mark.parametrize("form", ["folded", "rows"])
@pytest.mark.parametrize("batch,length,n_segments,h", [(2, 600, 7, 64), (5, 9, 3, 300)])
def test_part_gradients_exact(dev, form, batch, length, n_segments, h):
    """integer-valued upstream gradients in [-8, 8]: every sum is exact in fp32, so the fp64 composition's gradients are met exactly.
    L = 600: three chunks of 256 positions, the last partial"""
    m = module(64, 4, 5, h, fold=form == "folded", seed=4)
    for monotone in (True, False):
        d = draw(dev, batch, length, n_segments, 3, h, seed=length + monotone, mask="row", monotone=monotone)
        upstream = torch.randint(-8, 9, (batch, 3 + length, h), generator=torch.Generator(device="cpu").manual_seed(length)).to(dev)
        want = part_grads64(d, upstream.double(), 3)
        for out_dtype in (None, torch.bfloat16, torch.float16):         # a 16-bit upstream gradient holds these integers exactly
            got = part_grads(m, d, upstream, out_dtype)
            for name, a, b in zip(("position_rows", "segment_rows[0]", "segment_rows[1]", "prefix"), got, want):
                assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.double(), b), (name, monotone, out_dtype)
        assert float(want[1].abs().max()) > 0 and torch.equal(got[0][length:], torch.zeros_like(got[0][length:]))


@pytest.mark.parametrize("form", ["folded", "unfolded", "plain"])
def test_gradients_general_values(dev, form):
    """random upstream gradients: the additive parts within the bound of a recursive fp32 sum; the projector's weight and bias and
    miss_emb bit for bit what `forward`'s own autograd gives when fed g[:, P:]; two backward runs give the same bits"""
    h = None if form == "plain" else 64
    m = module(64, 4, 5, h, fold=None if h is None else form == "folded", seed=5)
    width = h or 256
    batch, length, n_segments, n_prefix = 2, 600, 7, 3
    d = draw(dev, batch, length, n_segments, n_prefix, width, seed=31, mask="scattered", monotone=False)
    upstream = torch.randn(batch, n_prefix + length, width, generator=torch.Generator(device="cpu").manual_seed(32)).to(dev)
    want = part_grads64(d, upstream.double(), n_prefix)
    sum_abs = part_grads64(d, upstream.double().abs(), n_prefix)
    count = part_grads64(d, torch.ones_like(upstream, dtype=torch.float64), n_prefix)
    got = part_grads(m, d, upstream)
    params = [t for t in ([m.projector.weight, m.projector.bias] if h else []) + [m.miss_emb]]
    own = [t.grad.clone() for t in params]
    for name, a, b, s, c in zip(("position_rows", "segment_rows[0]", "segment_rows[1]", "prefix"), got, want, sum_abs, count):
        err = (a.double() - b).abs()
        bound = (c + 1) * U * s
        print(f"{form} d {name}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, most contributions {int(c.max())}")
        assert bool((err <= bound).all()), name
    assert torch.equal(got[1], got[2])                                # both segment terms receive the same tensor
    again = part_grads(m, d, upstream)
    assert all(torch.equal(a, b) for a, b in zip(got, again)) and all(torch.equal(t.grad, o) for t, o in zip(params, own))
    m.zero_grad()
    m(d["index"], d["mask"]).backward(upstream[:, n_prefix:])
    for t, o in zip(params, own):
        assert float(o.abs().max()) > 0 and torch.equal(t.grad, o)


def test_codebook_gradient_through_the_rows_form(dev):
    """freeze_codebook=False: sequence reaches the codebook through the lookup's rows, bit-equal to `forward`'s route fed g[:, P:]"""
    from medtok_amd import MedTokEmbedding
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    _, types, tokens, weights = table_case(64, 4, 5)
    torch.manual_seed(6)
    v = VectorQuantizer(N_E, 64, 0.25, 0.0, True, True, [64, 64], num_head=4, k=5)      # its own quantiser: it collects a gradient
    with torch.no_grad():
        v.codebook.weight.normal_()
    v = v.to(dev).eval()
    for proj in (None, nn.Linear(256, 36).to(dev)):
        m = MedTokEmbedding(v, tokens, weights, types=types, freeze_codebook=False, projector=proj, fold=None if proj is None else True)
        width = 256 if proj is None else 36
        d = draw(dev, 3, 37, 5, 3, width, seed=41)
        upstream = torch.randn(3, 40, width, generator=torch.Generator(device="cpu").manual_seed(42)).to(dev)
        v.zero_grad(), m.zero_grad()
        seq, _ = run(m, d)
        assert torch.equal(seq.detach(), compose(m(d["index"], d["mask"]).detach(), d))     # (with grad on, as above: the same route)
        seq.backward(upstream)
        got = v.codebook.weight.grad.clone()
        v.zero_grad(), m.zero_grad()
        m(d["index"], d["mask"]).backward(upstream[:, 3:])
        assert float(got.abs().max()) > 0 and torch.equal(got, v.codebook.weight.grad)
        assert getattr(m, "fold_builds", 0) == 0


# ------------------------------------------------------------------ 6. no host read: a captured step replays on new contents
@pytest.mark.parametrize("form", ["folded", "rows"])
def test_step_captured_in_a_graph(dev, form):
    m = module(64, 4, 5, 64, fold=True, seed=7) if form == "folded" else module(64, 4, 5)
    width = 64 if form == "folded" else 256
    shape = dict(batch=4, length=300, n_segments=6, n_prefix=3, width=width)
    d = draw(dev, seed=0, **shape)
    leaves = [d[k].requires_grad_(True) for k in ("pe", "r0", "r1", "prefix")] + [p for p in m.parameters()]
    upstream = torch.randn(4, 303, width, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)

    def step():
        seq, keys = run(m, d, validate=False)
        return (seq.detach(), keys) + torch.autograd.grad((seq * upstream).sum(), leaves)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up: the tables are folded, the library loaded
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (1, 2):
        fresh = draw(dev, seed=seed, **shape)
        with torch.no_grad():
            for k in ("index", "mask", "seg", "pe", "r0", "r1", "prefix"):
                d[k].copy_(fresh[k])
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert len(eager) == len(captured) and all(torch.equal(a, b) for a, b in zip(captured, eager))
        assert all(float(t.abs().max()) > 0 for t in eager[2:])


# ------------------------------------------------------------------ 7. edges
def test_zero_positions_and_the_widest_segment_table(dev):
    from medtok_amd import _lib, ops
    for m, width in ((module(64, 4, 5, 64, fold=True, seed=8), 64), (module(64, 4, 5), 256)):
        prefix = torch.randn(2, 3, width, device=dev, requires_grad=True)
        seq, keys = m.sequence(torch.zeros(2, 0, dtype=torch.int64, device=dev), position_rows=torch.zeros(4, width, device=dev), prefix=prefix)
        assert torch.equal(seq, prefix) and keys.shape == (2, 3) and not bool(keys.any())
        seq.backward(torch.ones_like(seq))
        assert torch.equal(prefix.grad, torch.ones_like(prefix))
    assert _lib.load().medtok_embed_sequence_grad_workspace_bytes(2, 0, 5, 64) == 0
    g = torch.ones(2, 3, 64, device=dev)
    assert torch.equal(ops.embed_sequence_segment_grad(g, torch.zeros(2, 0, dtype=torch.int64, device=dev), 5, n_prefix=3), torch.zeros(2, 5, 64, device=dev))
    assert torch.equal(ops.embed_sequence_position_grad(g, 4, n_prefix=3), torch.zeros(4, 64, device=dev))
    # V = 4096 (the accumulators of a 4-column tile fill the 64 KiB of LDS), a width that needs two such tiles and is no multiple of 4
    gen = torch.Generator(device="cpu").manual_seed(9)
    seg = torch.randint(0, 4096, (1, 300), generator=gen).to(dev)
    g = torch.randint(-8, 9, (1, 300, 6), generator=gen).float().to(dev)
    want = torch.zeros(1, 4096, 6, device=dev).index_put_((torch.zeros_like(seg), seg), g, accumulate=True)
    assert torch.equal(ops.embed_sequence_segment_grad(g, seg, 4096), want)
