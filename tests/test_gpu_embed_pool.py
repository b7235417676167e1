"""GPU: MedTokEmbedding.pooled / ops.embed_pool -- the normalised mean of a bag of codes in one pass (embed_pool_*_kernel) -- and the
gradients behind it.

Comparator: torch fp64 on the GPU over the rows `module(index, mask, validate=False)` returns (the existing lookup, never the code
under test): normalise each row over its full width, masked sum, divide by the unmasked count, zeros for an empty bag.  Bar: rel() <=
1e-5 of the comparator's max magnitude (the RTOL and rel() of tests/test_gpu_embed.py).  An fp32 in-order pipeline over L <= 300 rows
of 8 .. 3072 floats stays under 1e-6 of it: per row ~2^-24 relative from the squared norm's sum, its root, the reciprocal and the
scaling, and the running sum of L unit rows adds at most L * 2^-24 of a sum that the mean divides by the same L; every figure is
printed before it is asserted.  The shapes of tests/test_gpu_embed.py: N_E = 96, regions text [0, 32), graph [64, 96), shared [0, 96)."""
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
BAGS = 3
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
    """(tests/test_gpu_embed_project.py::table_case) a VectorQuantizer(96, e_dim) with a random codebook and a random token table
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
    """(tests/test_gpu_embed_project.py::table64) the fp64 embedding table [num_codes, S * e_dim], differentiable in `codebook`"""
    cb = v.codebook.weight.detach().double() if codebook is None else codebook
    lo = torch.tensor([v._region(t)[0] for t in types], device=tokens.device).view(1, -1, 1)
    return (weights.double()[..., None] * F.normalize(cb, dim=-1)[tokens + lo]).sum(2).reshape(tokens.shape[0], -1)


def pool64(rows, mask, normalize):
    """the comparator's second half, fp64: rows [B, L, W] -> [B, W]"""
    rows = rows.double()
    if normalize:
        rows = rows / rows.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    keep = torch.ones(rows.shape[:2], dtype=torch.float64, device=rows.device) if mask is None else (~mask).double()
    live = keep.sum(1, keepdim=True)
    return torch.where(live > 0, (rows * keep.unsqueeze(-1)).sum(1) / live.clamp_min(1.0), torch.zeros_like(live))


def want_from_forward(module, index, mask, normalize):
    with torch.no_grad():
        return pool64(module(index, padding_mask=mask, validate=False), mask, normalize)


def mask_patterns(bags, length, seed):
    """name -> mask [bags, length] or None: none / a left-padded prefix per bag / scattered / one bag fully padded / one bag whose only
    unpadded position is its last"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    at = torch.arange(length).expand(bags, length)
    prefix = at < (torch.tensor([0.0, 0.4, 0.9])[torch.arange(bags) % 3] * length).floor().long().view(-1, 1)
    scattered = torch.rand(bags, length, generator=gen) < 0.5
    full = scattered.clone()
    full[1 % bags] = True
    last = torch.zeros(bags, length, dtype=torch.bool)
    last[bags - 1, :length - 1] = True
    return {"none": None, "prefix": prefix, "scattered": scattered, "one bag padded": full, "last only": last}


def index_patterns(bags, length, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    n = bags * length
    perm = torch.randperm(NUM_CODES, generator=gen).repeat(n // NUM_CODES + 1)[:n]
    mixed = torch.randint(0, NUM_CODES, (n,), generator=gen)
    mixed[torch.rand(n, generator=gen) < 0.2] = NUM_CODES
    return {"permutation": perm.view(bags, length), "one code": torch.full((bags, length), int(torch.randint(0, NUM_CODES, (1,), generator=gen))),
            "all miss": torch.full((bags, length), NUM_CODES), "mixed": mixed.view(bags, length)}


def with_garbage(index, mask):
    """garbage below the mask: those positions must not be read"""
    if mask is None:
        return index
    index = index.clone()
    index[mask] = torch.tensor(GARBAGE)[torch.arange(int(mask.sum())) % 2]
    return index


# ------------------------------------------------------------------ 1. values
LENGTHS = {"1": lambda c: 1, "C-1": lambda c: c - 1, "C": lambda c: c, "C+1": lambda c: c + 1, "3C+5": lambda c: 3 * c + 5}


@pytest.mark.parametrize("length_name", list(LENGTHS))
@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("d,k", [(8, 1), (40, 9), (64, 5), (64, 16), (768, 5)])
def test_values(dev, d, k, slots, length_name):
    case = table_case(d, slots, k)
    m = make_module(case, seed=d + k)
    worst = 0.0
    for length in (LENGTHS[length_name](chunk()),):
        for mname, mask in mask_patterns(BAGS, length, seed=length).items():
            for iname, index in index_patterns(BAGS, length, seed=length + 1).items():
                index = with_garbage(index, mask).to(dev)
                mk = None if mask is None else mask.to(dev)
                for normalize in (True, False):
                    want = want_from_forward(m, index, mk, normalize)
                    with torch.no_grad():
                        got = m.pooled(index, padding_mask=mk, normalize=normalize)
                        again = m.pooled(index, padding_mask=mk, normalize=normalize, validate=False)
                    err = rel(got, want)
                    worst = max(worst, err)
                    if err > RTOL / 10:
                        print(f"d={d} k={k} S={slots} L={length} mask={mname} index={iname} normalize={normalize}: rel {err:.3e}")
                    assert got.shape == (BAGS, slots * d) and got.dtype == torch.float32
                    assert torch.isfinite(got).all()
                    assert err <= RTOL, (length, mname, iname, normalize, err)
                    assert torch.equal(got, again)                                   # two calls, the same bits
                    if mask is not None:
                        empty = mk.all(1)
                        assert not bool(got[empty].any())                            # a bag without an unpadded position: zeros
    print(f"d={d} k={k} S={slots} L={length_name}: worst rel vs fp64 {worst:.3e}")


def test_many_bags_and_padded_e_dim(dev):
    """70 bags; e_dim = 10 (the codebook is padded to 12 columns for the kernels: the padding columns change no norm); rows of 3200
    floats (the widest instantiation, 16 float4 per lane, 12.5 of them in use; the 3072 of test_values takes the one of 12)"""
    c = chunk()
    for (d, k, slots), bags in (((64, 5, 4), 70), ((10, 5, 4), BAGS), ((800, 9, 4), BAGS)):
        m = make_module(table_case(d, slots, k), seed=5)
        length = c + 1
        mask = mask_patterns(bags, length, seed=3)["scattered"]
        gen = torch.Generator(device="cpu").manual_seed(bags)
        index = torch.randint(0, NUM_CODES + 1, (bags, length), generator=gen)
        index, mask = with_garbage(index, mask).to(dev), mask.to(dev)
        for normalize in (True, False):
            want = want_from_forward(m, index, mask, normalize)
            with torch.no_grad():
                got = m.pooled(index, padding_mask=mask, normalize=normalize)
            print(f"d={d} bags={bags} normalize={normalize}: rel {rel(got, want):.3e}")
            assert got.shape == (bags, slots * d) and rel(got, want) <= RTOL


# ------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("d,k,slots", [(8, 1, 1), (64, 5, 4), (768, 5, 4)])
def test_one_position_without_normalisation_is_the_forward_row(dev, d, k, slots):
    m = make_module(table_case(d, slots, k), seed=1)
    length = 2 * chunk() + 3
    where = [0, chunk() + 1, length - 1]                                    # the one unpadded position of each bag (bag 1: the miss row)
    index = torch.randint(0, NUM_CODES, (BAGS, length), generator=torch.Generator(device="cpu").manual_seed(d))
    index[1, where[1]] = NUM_CODES
    mask = torch.ones(BAGS, length, dtype=torch.bool)
    mask[torch.arange(BAGS), where] = False
    index, mask = with_garbage(index, mask).to(dev), mask.to(dev)
    with torch.no_grad():
        rows = m(index, padding_mask=mask)[torch.arange(BAGS), where]
        got = m.pooled(index, padding_mask=mask, normalize=False)
    assert torch.equal(got, rows)
    assert torch.equal(got[1], m.miss_emb.detach()[0])


def test_zero_weight_row_gives_finite_zeros(dev):
    from medtok_amd import MedTokEmbedding
    v, types, tokens, weights = table_case(64, 4, 5)
    weights = weights.clone()
    weights[3] = 0.0
    m = MedTokEmbedding(v, tokens, weights, types=types)
    index = torch.tensor([[3, 3, 3, 3], [3, 7, 3, 9], [1, 2, 3, 4]], device=dev)
    for normalize in (True, False):
        with torch.no_grad():
            got = m.pooled(index, normalize=normalize)
        assert torch.isfinite(got).all() and not bool(got[0].any())
        assert rel(got, want_from_forward(m, index, None, normalize)) <= RTOL


def test_garbage_under_the_mask_is_not_read(dev):
    from medtok_amd import ops
    v, types, tokens, weights = table_case(64, 4, 5)
    m = make_module((v, types, tokens, weights), seed=2)
    length = chunk() + 3
    mask = mask_patterns(BAGS, length, seed=11)["scattered"]
    clean = index_patterns(BAGS, length, seed=12)["mixed"]
    clean[mask] = 0
    dirty = with_garbage(clean, mask)
    assert not torch.equal(clean, dirty)
    what = v._normalised_codebook()[0]
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in types)]
    outs = []
    for index in (clean, dirty):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        pooled, counts = ops.embed_pool(index.to(dev), tokens, weights, what, regions, miss=m.miss_emb.detach().reshape(-1), pad_mask=mask.to(dev),
                                        status=status)
        assert int(status.item()) == 0
        outs.append((pooled, counts))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    live = (~mask).sum(1)
    missed = ((clean == NUM_CODES) & ~mask).sum(1)
    assert torch.equal(outs[0][1].cpu(), torch.stack([live, missed], 1).int())


# ------------------------------------------------------------------ 3. bad input
def test_bad_index_and_bad_slot(dev):
    from medtok_amd import MedTokEmbedding, ops
    v, types, tokens, weights = table_case(64, 4, 5)
    m = make_module((v, types, tokens, weights), seed=3)
    length = chunk() + 2
    index = index_patterns(BAGS, length, seed=4)["mixed"].to(dev)
    bad = index.clone()
    bad[0, 1], bad[2, length - 1] = NUM_CODES + 3, -1
    with pytest.raises(ValueError, match="code index"):
        m.pooled(bad)
    no_miss = make_module((v, types, tokens, weights), miss_row=False)
    with pytest.raises(ValueError, match="code index"):
        no_miss.pooled(torch.full((1, 3), NUM_CODES, device=dev))
    # validate=False: a row of zeros that counts in live_b -- what forward(validate=False) gives, so the comparator as it stands
    for normalize in (True, False):
        with torch.no_grad():
            got = m.pooled(bad, normalize=normalize, validate=False)
        assert rel(got, want_from_forward(m, bad, None, normalize)) <= RTOL
    what = v._normalised_codebook()[0]
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in types)]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _, counts = ops.embed_pool(bad, tokens, weights, what, regions, miss=m.miss_emb.detach().reshape(-1), status=status)
    assert int(status.item()) == 1 << ops.EMBED_BAD_INDEX_BIT
    assert counts[:, 0].tolist() == [length] * BAGS
    # a token id outside its region in slot 2 of code 7
    broken = tokens.clone()
    broken[7, 2, 1] = N_E
    mb = MedTokEmbedding(v, broken, weights, types=types)
    mb.miss_emb = m.miss_emb
    hit = index.clone()
    hit[1, 0] = 7
    with pytest.raises(ValueError, match="slot 2"):
        mb.pooled(hit)
    for normalize in (True, False):
        with torch.no_grad():
            got = mb.pooled(hit, normalize=normalize, validate=False)
        assert rel(got, want_from_forward(mb, hit, None, normalize)) <= RTOL
    status.zero_()
    ops.embed_pool(hit, broken, weights, what, regions, miss=m.miss_emb.detach().reshape(-1), status=status)
    assert int(status.item()) == 1 << 2


# ------------------------------------------------------------------ 4. gradients
def grad_inputs(dev, length):
    """bag 0 mixed with misses, bag 1 without a miss, bag 2 empty (fully padded), bag 3 all miss"""
    gen = torch.Generator(device="cpu").manual_seed(length)
    index = torch.randint(0, NUM_CODES, (4, length), generator=gen)
    index[0, torch.rand(length, generator=gen) < 0.3] = NUM_CODES
    index[0, 0] = NUM_CODES
    index[3] = NUM_CODES
    mask = torch.rand(4, length, generator=gen) < 0.3
    mask[0, 0] = False
    mask[2] = True
    return with_garbage(index, mask).to(dev), mask.to(dev)


def composition64(t64, miss64, index, mask, normalize, w64=None, b64=None):
    safe = torch.where(mask, 0, index)
    rows = torch.cat([t64, miss64.reshape(1, -1)], 0)[safe]
    out = pool64(rows, mask, normalize)
    return out if w64 is None else F.linear(out, w64, b64)


@pytest.mark.parametrize("d,k,slots", [(64, 5, 4), (10, 5, 4), (768, 5, 1)])
def test_miss_row_and_projector_gradients(dev, d, k, slots):
    case = table_case(d, slots, k)
    t64 = table64(*case)
    index, mask = grad_inputs(dev, chunk() + 5)
    for normalize in (True, False):
        for h in (None, 6):
            torch.manual_seed(h or 1)
            proj = None if h is None else nn.Linear(slots * d, h).to(dev)
            m = make_module(case, seed=7, projector=proj)
            up = torch.randn(4, h or slots * d, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
            grads = []
            for _ in range(2):
                m.zero_grad(set_to_none=True)
                out = m.pooled(index, padding_mask=mask, normalize=normalize)
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
            want = composition64(t64, miss64, index, mask, normalize, w64, b64)
            (want * up.double()).sum().backward()
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
    index, mask = grad_inputs(dev, chunk() + 5)
    up = torch.randn(4, 256, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    out = m.pooled(index, padding_mask=mask)
    (out * up).sum().backward()
    cb64 = v.codebook.weight.detach().double().requires_grad_()
    miss64 = m.miss_emb.detach().double().requires_grad_()
    want = composition64(table64(v, types, tokens, weights, codebook=cb64), miss64, index, mask, True)
    (want * up.double()).sum().backward()
    errs = rel(out, want), rel(v.codebook.weight.grad, cb64.grad), rel(m.miss_emb.grad.reshape(-1), miss64.grad)
    print(f"composed route: rel out / d codebook / d miss {errs}")
    assert max(errs) <= RTOL
    with torch.no_grad():                                                    # and the kernels give the same function
        assert rel(m.pooled(index, padding_mask=mask), want) <= RTOL


# ------------------------------------------------------------------ 5. graph
def test_pooled_replayed_from_a_hip_graph_is_bit_equal_to_eager(dev):
    m = make_module(table_case(64, 4, 5), seed=9)
    shape = (6, 3 * chunk() + 5)

    def draw(seed):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        index = torch.randint(0, NUM_CODES + 1, shape, generator=gen)
        mask = torch.rand(shape, generator=gen) < 0.3
        return with_garbage(index, mask).to(dev), mask.to(dev)
    index, mask = draw(0)
    with torch.no_grad():
        m.pooled(index, padding_mask=mask, validate=False)      # warm-up: the normalised codebook is cached, the library loaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m.pooled(index, padding_mask=mask, validate=False)
        for seed in (1, 2):
            i2, m2 = draw(seed)
            index.copy_(i2), mask.copy_(m2)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, m.pooled(i2, padding_mask=m2))


# ------------------------------------------------------------------ 6. bags without positions
def test_empty_bag_length_needs_no_workspace(dev):
    """bag_len == 0: the workspace query returns 0 and the C entry takes a NULL workspace; every bag is a row of zeros with counts (0, 0)"""
    import ctypes
    from medtok_amd import _lib, ops
    v, types, tokens, weights = table_case(64, 4, 5)
    m = make_module((v, types, tokens, weights), seed=1)
    with torch.no_grad():
        got = m.pooled(torch.zeros(5, 0, dtype=torch.int64, device=dev))
    assert got.shape == (5, 256) and not bool(got.any())
    lib = _lib.load()
    assert lib.medtok_embed_pool_workspace_bytes(5, 0, 256) == 0
    what = v._normalised_codebook()[0]
    regions = [v._region(t) for t in types]
    arr = ctypes.c_int64 * 4
    out = torch.full((5, 256), 3.0, device=dev)
    counts = torch.full((5, 2), 7, dtype=torch.int32, device=dev)
    rc = lib.medtok_embed_pool_f32(0, 0, 5, 0, tokens.data_ptr(), weights.data_ptr(), NUM_CODES, 4, 5, what.data_ptr(), N_E, 64,
                                   arr(*[lo for lo, _ in regions]), arr(*[hi - lo for lo, hi in regions]), 0, 1, out.data_ptr(), 0,
                                   counts.data_ptr(), 0, 0, 0, ops._stream(out))
    _lib.check(rc, "medtok_embed_pool_f32")
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(counts.any())
