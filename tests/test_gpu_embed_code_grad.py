"""GPU: the codebook's gradient through the embedding lookup -- ops.embed_codes_code_grad / medtok_embed_code_grad_f32 and
MedTokEmbedding(freeze_codebook=False) on top of it.

Bars: where every partial sum is exact in fp32 (integer upstream gradients, weights from {1, 0.5, 0.25}) the kernel must EQUAL an fp64
index_add_ restatement of the definition -- the order cannot matter there; with real-valued inputs 1e-5 of the result's scale against
fp64 (the RTOL and rel() of tests/test_gpu_embed.py), two calls the same bits, and a lone contribution w * g exactly."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
RTOL = 1e-5
TYPES = ("text", "graph", "shared", "shared")
N_E = 96                                           # three regions of >= 16 codes (k = 16): text [0, 32), graph [64, 96), shared [0, 96)
REGIONS4 = [(0, 32), (64, 32), (0, 96), (0, 96)]
REGIONS1 = [(64, 32)]                              # one slot: a region that does not start at 0
NUM_CODES = 50


def chunk():
    from medtok_amd import ops
    return ops.EMBED_CODE_GRAD_CHUNK


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def random_vq(dev, n_e, e_dim, k, seed=0):
    """(a copy of tests/test_gpu_embed.py::random_vq)"""
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(seed)
    v = VectorQuantizer(n_e, e_dim, 0.25, 0.0, True, True, [e_dim, e_dim], num_head=4 if e_dim % 4 == 0 else 2, k=k)
    with torch.no_grad():
        v.codebook.weight.normal_()
    return v.to(dev).eval()


def random_table(v, num_codes, k, seed, types=TYPES):
    """(a copy of tests/test_gpu_embed.py::random_table)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    dev = v.codebook.weight.device
    sizes = [hi - lo for lo, hi in (v._region(t) for t in types)]
    tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen) for s in sizes], 1).to(dev)
    weights = torch.softmax(torch.randn(num_codes, len(types), k, generator=gen), -1).to(dev)
    return tokens, weights


def mixed_index(n, num_codes, seed, miss=0.2, padded=0.15):
    """(a copy of tests/test_gpu_embed.py::mixed_index)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    index = torch.randint(0, num_codes, (n,), generator=gen)
    u = torch.rand(n, generator=gen)
    index[u < miss] = num_codes
    mask = u > 1.0 - padded
    index[mask] = torch.tensor([-7, 2 ** 40, num_codes + 3])[torch.arange(int(mask.sum())) % 3]
    return index, mask


def index_patterns(n, num_codes, rng):
    """(tests/test_gpu_embed.py::index_patterns) name -> (index [n], mask [n] or None)"""
    perm = np.resize(rng.permutation(num_codes), n).astype(np.int64)
    garbage = np.resize(np.array([-7, 2 ** 40], np.int64), n)
    mixed = rng.integers(0, num_codes, n)
    u = rng.random(n)
    mixed[u < 0.2] = num_codes
    mask = u > 0.7
    mixed[mask] = garbage[mask]
    return {"permutation": (perm, None), "one code": (np.full(n, int(rng.integers(0, num_codes)), np.int64), None),
            "all miss": (np.full(n, num_codes, np.int64), None), "all padded": (garbage, np.ones(n, bool)), "mixed": (mixed, mask)}


def restate(g, index, mask, tokens, weights, regions, n_codes):
    """the definition in fp64 with index_add_ -> (g_what [K, d], bins [K], slots_of_row [K, S] contribution counts per slot)"""
    num_codes, s, k = tokens.shape
    n = index.numel()
    d = g.shape[-1] // s
    dev = g.device
    padded = torch.zeros(n, dtype=torch.bool, device=dev) if mask is None else mask.reshape(-1) != 0
    index = index.reshape(-1)
    is_code = ~padded & (index >= 0) & (index < num_codes)
    safe = torch.where(is_code, index, 0)
    tok, w = tokens[safe], weights[safe]                                       # [n, S, k]
    lo = torch.tensor([r[0] for r in regions], device=dev).view(1, s, 1)
    size = torch.tensor([r[1] for r in regions], device=dev).view(1, s, 1)
    live = is_code.view(n, 1) & ((tok >= 0) & (tok < size)).all(-1)            # [n, S]: one bad id kills the slot
    rows = torch.where(live.unsqueeze(-1), tok + lo, 0).reshape(-1)
    live_c = live.unsqueeze(-1).expand(n, s, k).reshape(-1)
    contrib = (w.double().unsqueeze(-1) * g.double().reshape(n, s, 1, d)).reshape(-1, d) * live_c.unsqueeze(-1)
    g_what = torch.zeros(n_codes, d, dtype=torch.float64, device=dev).index_add_(0, rows, contrib)
    bins = torch.zeros(n_codes, dtype=torch.float64, device=dev).index_add_(0, rows, live_c.double())
    slot_of = torch.arange(s, device=dev).view(1, s, 1).expand(n, s, k).reshape(-1)
    per_slot = torch.zeros(n_codes * s, dtype=torch.float64, device=dev).index_add_(0, rows * s + slot_of, live_c.double()).view(n_codes, s)
    return g_what, bins, per_slot


def exact_table(s, k, seed, dev):
    """ids inside the regions and weights from {1, 0.5, 0.25}.  Four slots: code 0 meets row 3 from the text slot AND from a shared slot;
    the shared slots stay below row 90 and the graph slot below its id 26 (rows 64 .. 89), so rows 90 .. 95 never collect anything"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    regions = REGIONS4 if s == 4 else REGIONS1
    limits = [32, 26, 90, 90] if s == 4 else [32]
    tokens = torch.stack([torch.randint(0, lim, (NUM_CODES, k), generator=gen) for lim in limits], 1)
    if s == 4:
        tokens[0, 0, 0] = 3
        tokens[0, 2, 0] = 3
    weights = torch.tensor([1.0, 0.5, 0.25])[torch.randint(0, 3, (NUM_CODES, s, k), generator=gen)]
    return tokens.to(dev), weights.to(dev), regions


# ------------------------------------------------------------------ 1. exact indexing
@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("d", [64, 72, 768])
def test_exact_indexing_equals_the_restated_definition(dev, d, k, s):
    """integer upstream gradients in [-8, 8] and weights from {1, 0.5, 0.25}: every partial sum is a multiple of 0.25 below 2^24 / 4, exact
    in fp32 in ANY order, so the kernel must equal the fp64 restatement.  d = 64: the 16-lane form, 72: idle lanes, 768: three passes."""
    from medtok_amd import ops
    tokens, weights, regions = exact_table(s, k, seed=d + 17 * k + s, dev=dev)
    broken = tokens.clone()                                                    # one bad id in one slot of one used code
    bad_slot = s - 1
    broken[1, bad_slot, k - 1] = regions[bad_slot][1]                          # == size: one past the region
    rng = np.random.default_rng(d * 31 + k * 7 + s)
    seen_two_slots = seen_empty = False
    for n in (0, 1, 97, 3 * chunk() + 5):
        g = torch.from_numpy(rng.integers(-8, 9, (n, s * d)).astype(np.float32)).to(dev)
        for name, (index, mask) in index_patterns(n, NUM_CODES, rng).items():
            if name == "one code":
                index = np.zeros(n, np.int64) if n == 97 else np.full(n, 1, np.int64)    # (codes 0 and 1: the crafted rows)
            index = torch.from_numpy(index).to(dev)
            mask = None if mask is None else torch.from_numpy(mask).to(dev)
            for label, table in (("good", tokens), ("bad id", broken)):
                got_g, got_bins = ops.embed_codes_code_grad(g, index, table, weights, (N_E, d), regions, pad_mask=mask)
                want_g, want_bins, per_slot = restate(g, index, mask, table, weights, regions, N_E)
                assert got_g.shape == (N_E, d) and got_bins.shape == (N_E,) and got_g.dtype == got_bins.dtype == torch.float32
                assert torch.equal(got_bins.double(), want_bins), (n, name, label)
                assert torch.equal(got_g.double(), want_g), (n, name, label)
                assert float(got_g[want_bins == 0].abs().max() if bool((want_bins == 0).any()) else 0.0) == 0.0
                assert float(want_bins.sum()) <= n * s * k
                if name in ("all miss", "all padded"):
                    assert float(want_bins.sum()) == 0.0 and float(got_g.abs().max()) == 0.0
                if label == "good" and want_bins.sum() > 0:
                    seen_two_slots |= bool(((per_slot > 0).sum(1) >= 2).any())
                    seen_empty |= bool((want_bins == 0).any())
            # the bad id: slot bad_slot of code 1 loses all k contributions at every position on code 1, the other slots keep theirs
            on_code_1 = (index == 1) if mask is None else (index == 1) & ~mask
            good_bins = restate(g, index, mask, tokens, weights, regions, N_E)[1]
            assert float(good_bins.sum() - want_bins.sum()) == float(on_code_1.sum()) * k
    if s == 4:                                                                 # no hidden coverage gaps (the restatement alone)
        assert seen_two_slots and seen_empty


def test_a_strided_and_a_half_precision_upstream(dev):
    """g_out as a column block of a wider tensor (row stride, no copy needed) and in bf16 (converted to fp32 first)"""
    from medtok_amd import ops
    d, k, n = 72, 5, 97
    tokens, weights, regions = exact_table(4, k, seed=3, dev=dev)
    rng = np.random.default_rng(5)
    wide = torch.from_numpy(rng.integers(-8, 9, (n, 4 * d + 8)).astype(np.float32)).to(dev)
    index, mask = (torch.from_numpy(a).to(dev) for a in index_patterns(n, NUM_CODES, rng)["mixed"])
    want = ops.embed_codes_code_grad(wide[:, 4:4 + 4 * d].contiguous(), index, tokens, weights, (N_E, d), regions, pad_mask=mask)
    got = ops.embed_codes_code_grad(wide[:, 4:4 + 4 * d], index, tokens, weights, (N_E, d), regions, pad_mask=mask)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    half = ops.embed_codes_code_grad(wide[:, 4:4 + 4 * d].bfloat16().view(n, 1, 4 * d), index.view(n, 1), tokens, weights,
                                     torch.empty(N_E, d, device=dev), regions, pad_mask=mask.view(n, 1))
    assert torch.equal(half[0], want[0]) and torch.equal(half[1], want[1])     # (integers up to 8 are exact in bf16)


# ------------------------------------------------------------------ 2. chunk edges
def hot_table(dev, unit_weights=False):
    """code 7's twenty ids are twenty DIFFERENT codebook rows: each of them collects one contribution per position on code 7"""
    gen = torch.Generator(device="cpu").manual_seed(11)
    tokens = torch.stack([torch.randint(0, lim, (NUM_CODES, 5), generator=gen) for lim in (32, 32, 96, 96)], 1)
    tokens[7, 0] = torch.arange(0, 5)                                          # rows 0 .. 4
    tokens[7, 1] = torch.arange(0, 5)                                          # rows 64 .. 68
    tokens[7, 2] = torch.arange(10, 15)
    tokens[7, 3] = torch.arange(20, 25)
    weights = torch.softmax(torch.randn(NUM_CODES, 4, 5, generator=gen), -1)
    if unit_weights:
        weights = torch.ones_like(weights)
    return tokens.to(dev), weights.to(dev)


HOT_ROWS = {0: range(0, 5), 1: range(64, 69), 2: range(10, 15), 3: range(20, 25)}


@pytest.mark.parametrize("d", [64, 768])
def test_chunk_edges_with_one_hot_code(dev, d):
    from medtok_amd import ops
    c = chunk()
    tokens, weights = hot_table(dev)
    gen = torch.Generator(device="cpu").manual_seed(d)
    for n in (c - 1, c, c + 1, 2 * c, 2 * c + 1):
        g = torch.randn(n, 4 * d, generator=gen).to(dev)
        index = torch.full((n,), 7, dtype=torch.int64, device=dev)
        got_g, got_bins = ops.embed_codes_code_grad(g, index, tokens, weights, (N_E, d), REGIONS4)
        want_g, want_bins, _ = restate(g, index, None, tokens, weights, REGIONS4, N_E)
        err = rel(got_g, want_g)
        print(f"hot code d={d} n={n}: rel {err:.3e}")
        assert err <= RTOL and torch.equal(got_bins.double(), want_bins)
        assert all(float(got_bins[r]) == n for rows in HOT_ROWS.values() for r in rows) and float(got_bins.sum()) == 20 * n
        again = ops.embed_codes_code_grad(g, index, tokens, weights, (N_E, d), REGIONS4)
        assert torch.equal(again[0], got_g) and torch.equal(again[1], got_bins)     # two calls: the same bits
    # n <= CHUNK, all weights 1, a single unpadded position: the row IS that position's block of g_out, bit for bit
    tokens1, ones = hot_table(dev, unit_weights=True)
    for n in (1, c - 1, c):
        g = torch.randn(n, 4 * d, generator=gen).to(dev)
        index = torch.full((n,), 7, dtype=torch.int64, device=dev)
        mask = torch.ones(n, dtype=torch.bool, device=dev)
        p = n // 2
        mask[p] = False
        got_g, got_bins = ops.embed_codes_code_grad(g, index, tokens1, ones, (N_E, d), REGIONS4, pad_mask=mask)
        assert float(got_bins.sum()) == 20
        for slot, rows in HOT_ROWS.items():
            for r in rows:
                assert torch.equal(got_g[r], g[p, slot * d:(slot + 1) * d])
        # a lone contribution with weight w: w * g in fp32, exactly (fmaf(w, g, +0) rounds the product once)
        got_g, _ = ops.embed_codes_code_grad(g, index, tokens, weights, (N_E, d), REGIONS4, pad_mask=mask)
        for slot, rows in HOT_ROWS.items():
            for j, r in enumerate(rows):
                assert torch.equal(got_g[r], weights[7, slot, j] * g[p, slot * d:(slot + 1) * d])


# ------------------------------------------------------------------ 3. module gradients
def grad_case(dev, e_dim, seed, n=97, num_codes=300, k=5):
    """(tests/test_gpu_embed.py::grad_case) n = 97 positions, about 20 of them the miss index and 15 under the mask"""
    v = random_vq(dev, 600, e_dim, k, seed=seed)
    tokens, weights = random_table(v, num_codes, k, seed=seed + 1)
    index, mask = mixed_index(n, num_codes, seed=seed + 2)
    gen = torch.Generator(device="cpu").manual_seed(seed + 3)
    probe = torch.randn(n, 4 * e_dim, generator=gen)
    probe[mask] *= 1e6                                                      # gradient under the mask must be ignored
    return v, tokens, weights, index.to(dev), mask.to(dev), probe.to(dev)


def rows64(W64, tokens, weights, regions, index, mask, miss64):
    """tests/test_gpu_embed.py::embed_comparator's rows: the fp64 table lookup, differentiable in W64 and miss64"""
    lo = torch.tensor([r[0] for r in regions], device=W64.device).view(1, -1, 1)
    table = (weights.double()[..., None] * F.normalize(W64, dim=-1)[tokens + lo]).sum(2).reshape(tokens.shape[0], -1)
    return torch.cat([table, miss64], 0)[index] * (~mask).unsqueeze(-1)


def embed_comparator(W, tokens, weights, regions, index, mask, miss, probe, head=lambda rows: rows):
    """(tests/test_gpu_embed.py::embed_comparator, with an optional head behind the rows) -> (out, g_W, g_miss)"""
    W64 = W.detach().double().requires_grad_(True)
    miss64 = miss.detach().double().requires_grad_(True)
    out = head(rows64(W64, tokens, weights, regions, index, mask, miss64))
    (out * probe.double()).sum().backward()
    return out, W64.grad, miss64.grad


def batch_4x25(index, mask, probe, dev):
    """the 97 positions as a [4, 25] batch: three more under the mask"""
    return (torch.cat([index, index[:3]]).view(4, 25), torch.cat([mask, torch.ones(3, dtype=torch.bool, device=dev)]).view(4, 25),
            torch.cat([probe, probe[:3]]).view(4, 25, -1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("e_dim,case", [(64, "random"), (70, "random"), (768, "random"), (64, "hot"), (70, "hot"), (768, "hot")])
def test_module_gradients(dev, e_dim, case, dtype):
    from medtok_amd import MedTokEmbedding
    v, tokens, weights, index, mask, probe = grad_case(dev, e_dim, seed=e_dim + 23)
    num_codes = tokens.shape[0]
    if case == "hot":                                                       # one code at every position that is neither miss nor padded
        index = torch.where(index < num_codes, 7, index)
    index, mask, probe = batch_4x25(index, mask, probe, dev)
    m = MedTokEmbedding(v, tokens, weights, freeze_codebook=False)
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in TYPES)]
    safe = torch.where(mask, 0, index)
    upstream = probe.to(dtype).float()                                      # what reaches the rows: the probe rounded to out_dtype
    ref_out, ref_gW, ref_gm = embed_comparator(v.codebook.weight, tokens, weights, regions, safe, mask, m.miss_emb, upstream)

    def run():
        m.zero_grad(), v.zero_grad()
        out = m(index, padding_mask=mask, out_dtype=dtype)
        assert out.dtype == dtype and out.shape == (4, 25, 4 * e_dim)
        (out.float() * probe).sum().backward()
        return out.detach(), v.codebook.weight.grad.clone(), m.miss_emb.grad.clone()
    out, gW, gm = run()
    errs = rel(gW, ref_gW), rel(gm, ref_gm)
    print(f"module e_dim={e_dim} {case} {dtype}: rel d codebook / d miss {errs}")
    assert gW.shape == v.codebook.weight.shape and max(errs) <= RTOL
    if dtype == torch.float32:
        assert rel(out, ref_out) <= RTOL
    with torch.no_grad():
        assert torch.equal(out, m(index, padding_mask=mask, out_dtype=dtype))   # the rows of the no-grad forward, bit for bit
    out2, gW2, gm2 = run()
    assert torch.equal(out, out2) and torch.equal(gW, gW2) and torch.equal(gm, gm2)      # two runs: the same bits
    with pytest.raises(ValueError, match="code index"):                     # validate=True: the same errors from the one status word
        m(torch.where(mask, index, num_codes + 1))


def test_every_position_dead_gives_a_gradient_of_zeros(dev):
    from medtok_amd import MedTokEmbedding
    v, tokens, weights, index, mask, probe = grad_case(dev, 64, seed=5)
    m = MedTokEmbedding(v, tokens, weights, freeze_codebook=False)
    num_codes = tokens.shape[0]
    for idx, msk in ((torch.full_like(index, num_codes), None), (index, torch.ones_like(mask)), (index[:0], None)):
        m.zero_grad(), v.zero_grad()
        out = m(idx, padding_mask=msk)
        (out * probe[:idx.numel()]).sum().backward()
        grad = v.codebook.weight.grad
        assert grad is not None and grad.shape == v.codebook.weight.shape and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("e_dim", [64, 70, 768])
def test_module_gradients_through_pooled_and_projector(dev, e_dim):
    from medtok_amd import MedTokEmbedding
    v, tokens, weights, index, mask, _ = grad_case(dev, e_dim, seed=e_dim + 41)
    index, mask, _ = batch_4x25(index, mask, torch.zeros(97, 1, device=dev), dev)
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in TYPES)]
    safe = torch.where(mask, 0, index)
    gen = torch.Generator(device="cpu").manual_seed(e_dim)
    # pooled(normalize=True): the normalised rows' mean over each bag's unpadded positions
    m = MedTokEmbedding(v, tokens, weights, freeze_codebook=False)
    probe = torch.randn(4, 4 * e_dim, generator=gen).to(dev)
    keep = (~mask).double()

    def pool64(rows):
        return (F.normalize(rows, dim=-1) * keep.unsqueeze(-1)).sum(1) / keep.sum(1, keepdim=True)
    assert float(keep.sum(1).min()) > 0
    ref_out, ref_gW, ref_gm = embed_comparator(v.codebook.weight, tokens, weights, regions, safe, mask, m.miss_emb, probe, head=pool64)

    def run_pooled():
        m.zero_grad(), v.zero_grad()
        out = m.pooled(index, padding_mask=mask, normalize=True)
        (out * probe).sum().backward()
        return out.detach(), v.codebook.weight.grad.clone(), m.miss_emb.grad.clone()
    out, gW, gm = run_pooled()
    errs = rel(out, ref_out), rel(gW, ref_gW), rel(gm, ref_gm)
    print(f"pooled e_dim={e_dim}: rel out / d codebook / d miss {errs}")
    assert max(errs) <= RTOL
    again = run_pooled()
    assert all(torch.equal(a, b) for a, b in zip((out, gW, gm), again))
    # a projector behind the lookup: the tables stay unfolded while the codebook trains
    torch.manual_seed(e_dim)
    proj = nn.Linear(4 * e_dim, 36).to(dev)
    mp = MedTokEmbedding(v, tokens, weights, freeze_codebook=False, projector=proj)
    probe = torch.randn(4, 25, 36, generator=gen).to(dev)
    w64, b64 = proj.weight.detach().double(), proj.bias.detach().double()
    ref_out, ref_gW, ref_gm = embed_comparator(v.codebook.weight, tokens, weights, regions, safe, mask, mp.miss_emb, probe,
                                               head=lambda rows: rows @ w64.t() + b64)

    def run_projected():
        mp.zero_grad(), v.zero_grad()
        out = mp(index, padding_mask=mask)
        (out * probe).sum().backward()
        return out.detach(), v.codebook.weight.grad.clone(), mp.miss_emb.grad.clone()
    out, gW, gm = run_projected()
    errs = rel(out, ref_out), rel(gW, ref_gW), rel(gm, ref_gm)
    print(f"projector e_dim={e_dim}: rel out / d codebook / d miss {errs}")
    assert max(errs) <= RTOL and mp.fold_builds == 0
    again = run_projected()
    assert all(torch.equal(a, b) for a, b in zip((out, gW, gm), again)) and mp.fold_builds == 0
    v.zero_grad()


# ------------------------------------------------------------------ 4. no host read: a captured fine-tuning gradient replays on new contents
def test_codebook_gradient_captured_in_a_graph(dev):
    from medtok_amd import MedTokEmbedding
    e_dim, k, num_codes, shape = 64, 5, 500, (6, 50)
    v = random_vq(dev, 900, e_dim, k, seed=9)
    m = MedTokEmbedding(v, *random_table(v, num_codes, k, seed=10), freeze_codebook=False)
    probe = torch.randn(*shape, 4 * e_dim, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)

    def draw(seed):
        index, mask = mixed_index(shape[0] * shape[1], num_codes, seed=seed)
        return index.view(shape).to(dev), mask.view(shape).to(dev)

    def grad_of(idx, msk):
        return torch.autograd.grad((m(idx, msk, validate=False) * probe).sum(), v.codebook.weight)[0]
    index, mask = draw(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up: the normalised codebook is cached, the library loaded
        grad_of(index, mask)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = grad_of(index, mask)
    for seed in (1, 2):
        i2, m2 = draw(seed)
        index.copy_(i2), mask.copy_(m2)
        graph.replay()
        torch.cuda.synchronize()
        eager = grad_of(i2, m2)
        assert float(eager.abs().max()) > 0 and torch.equal(captured, eager)


# ------------------------------------------------------------------ 5. no row-per-contribution temporary
def test_backward_makes_no_row_per_contribution_buffer(dev):
    """n * S * k * d * 4 = 252 MB of contribution rows at this shape; the backward may hold the upstream gradient (50 MB), the sort
    (16 bytes per contribution) and the chunk sums (2 n S k / CHUNK rows): its rise of the peak stays below half of that"""
    from medtok_amd import MedTokEmbedding
    n, s, k, d = 4096, 4, 5, 768
    v = random_vq(dev, 600, d, k, seed=2)
    tokens, weights = random_table(v, 300, k, seed=3)
    m = MedTokEmbedding(v, tokens, weights, freeze_codebook=False)
    index = torch.randint(0, 300, (n,), generator=torch.Generator(device="cpu").manual_seed(4)).to(dev)
    probe = torch.randn(n, s * d, generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    loss = (m(index, validate=False) * probe).sum()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"backward peak rise {rise / 1e6:.1f} MB; contribution rows would be {n * s * k * d * 4 / 1e6:.1f} MB")
    assert float(v.codebook.weight.grad.abs().max()) > 0
    assert rise < n * s * k * d * 4 // 2


# ------------------------------------------------------------------ 6. the ABI directly
def test_abi_workspace_one_byte_short_is_an_error_and_launches_nothing(dev):
    from medtok_amd import _lib
    lib = _lib.load()
    n, s, k, d = 97, 4, 5, 64
    tokens, weights, regions = exact_table(s, k, seed=1, dev=dev)
    rng = np.random.default_rng(2)
    g = torch.from_numpy(rng.integers(-8, 9, (n, s * d)).astype(np.float32)).to(dev)
    index = torch.from_numpy(rng.integers(0, NUM_CODES, n)).to(dev)
    arr = ctypes.c_int64 * s
    los, sizes = arr(*[r[0] for r in regions]), arr(*[r[1] for r in regions])
    need = lib.medtok_embed_code_grad_workspace_bytes(n, s, k, N_E, d)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    g_what = torch.full((N_E, d), 7.0, device=dev)
    bins = torch.full((N_E,), 7.0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes):
        return lib.medtok_embed_code_grad_f32(g.data_ptr(), 0, index.data_ptr(), 0, n, tokens.data_ptr(), weights.data_ptr(), NUM_CODES, s, k, N_E, d,
                                              los, sizes, g_what.data_ptr(), bins.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    rc = call(need - 1)
    assert rc != 0
    with pytest.raises(_lib.MedTokLibraryError, match="workspace too small"):
        _lib.check(rc, "medtok_embed_code_grad_f32")
    torch.cuda.synchronize()
    assert float((g_what - 7.0).abs().max()) == 0.0 and float((bins - 7.0).abs().max()) == 0.0 and int(ws.max()) == 0     # nothing ran
    assert call(need) == 0
    torch.cuda.synchronize()
    want_g, want_bins, _ = restate(g, index, None, tokens, weights, regions, N_E)
    assert torch.equal(g_what.double(), want_g) and torch.equal(bins.double(), want_bins)
