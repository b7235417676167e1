"""GPU: the scatter form of the folded lookup's gradients -- ops.embed_project_table_grad (medtok_embed_table_grad,
embed_grad_chunk_kernel) and MedTokEmbedding(grad_form="scatter").

The kernel is compared bit for bit with ops.embed_codes_code_grad on the upstream gradient tiled once per slot (the same contribution
order and chunking; that function is pinned to its host restatement in tests/test_gpu_embed_code_grad.py).  Module gradients are
compared with torch autograd over the float64 composition (the materialised table from the normalised codebook, indexing, the linear,
the sequence's additive parts) and with the "dense" module at the bar of tests/test_gpu_embed_project.py: rel() <= 1e-5 of the result's
scale."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
RTOL = 1e-5
NUM_CODES = 50
ROW_REGIONS = {4: [(0, 600), (600, 600), (1200, 300), (1200, 300)],      # two slots over one region
               1: [(300, 600)]}                                           # one slot: a region that does not start at row 0
TYPES = ("text", "graph", "shared", "shared")
B, L = 3, 37


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def mixed_index(n, num_codes, seed, miss=0.2, padded=0.15):
    """(tests/test_gpu_embed.py::mixed_index) about `miss` of the positions at the miss index, `padded` of them under the mask with
    garbage below it -> (index, mask), CPU"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    index = torch.randint(0, num_codes, (n,), generator=gen)
    u = torch.rand(n, generator=gen)
    index[u < miss] = num_codes
    mask = u > 1.0 - padded
    index[mask] = torch.tensor([-7, 2 ** 40, num_codes + 3])[torch.arange(int(mask.sum())) % 3]
    return index, mask


# ------------------------------------------------------------------ 1. the kernel, bit for bit
def kernel_case(dev, s, k, seed, n=B * L):
    """a token table over ROW_REGIONS[s] with one bad id in one slot of code 3, and n positions: padded ones with garbage below the
    mask, miss positions, two unpadded indices outside the table, code 3 at an unpadded position"""
    regions = ROW_REGIONS[s]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    tokens = torch.stack([torch.randint(0, size, (NUM_CODES, k), generator=gen) for _, size in regions], 1)
    tokens[3, s - 1, k // 2] = regions[s - 1][1]                            # one past the slot's range: the slot of code 3 is dead
    weights = torch.softmax(torch.randn(NUM_CODES, s, k, generator=gen), -1)
    index, mask = mixed_index(n, NUM_CODES, seed + 1)
    free = (~mask).nonzero().reshape(-1)
    index[free[0]], index[free[1]], index[free[2]] = 3, NUM_CODES + 5, -3
    assert bool(mask.any()) and int((index[~mask] == NUM_CODES).sum()) > 0
    return tokens.to(dev), weights.to(dev), regions, index.to(dev), mask.to(dev)


def rows_of(regions):
    return max(lo + size for lo, size in regions)


@pytest.mark.parametrize("hp", [8, 64, 68, 100])
@pytest.mark.parametrize("k", [5, 9])
@pytest.mark.parametrize("s", [1, 4])
def test_kernel_equals_the_code_gradient_of_the_tiled_upstream(dev, s, k, hp):
    from medtok_amd import ops
    tokens, weights, regions, index, mask = kernel_case(dev, s, k, seed=100 * s + 10 * k + hp)
    n, rows = index.numel(), rows_of(regions)
    gen = torch.Generator(device="cpu").manual_seed(hp)
    g = torch.randn(n, hp, generator=gen).to(dev)
    want_G, want_bins = ops.embed_codes_code_grad(g.repeat(1, s), index, tokens, weights, (rows, hp), regions, pad_mask=mask)
    got_G, got_bins = ops.embed_project_table_grad(g, index, tokens, weights, regions, pad_mask=mask)
    assert got_G.shape == (rows, hp) and got_bins.shape == (rows,) and got_G.dtype == got_bins.dtype == torch.float32
    assert torch.equal(got_bins, want_bins) and torch.equal(got_G, want_G)
    assert float(got_bins.sum()) > 0 and float(got_G.abs().max()) > 0
    assert float(got_G[got_bins == 0].abs().max()) == 0.0                       # rows without a contribution: exactly zero
    # a [B, L] batch is the same call
    again = ops.embed_project_table_grad(g.view(B, L, hp), index.view(B, L), tokens, weights, regions, pad_mask=mask.view(B, L))
    assert torch.equal(again[0], got_G) and torch.equal(again[1], got_bins)     # two calls: the same bits
    # 16-bit upstream gradients are read as they are; widening is exact
    for dtype in (torch.float16, torch.bfloat16):
        g16 = g.to(dtype)
        want16 = ops.embed_project_table_grad(g16.float(), index, tokens, weights, regions, pad_mask=mask)
        got16 = ops.embed_project_table_grad(g16, index, tokens, weights, regions, pad_mask=mask)
        assert torch.equal(got16[0], want16[0]) and torch.equal(got16[1], want16[1])
        assert torch.equal(got16[1], got_bins)
    # a column block of a wider tensor
    for dtype, off in ((torch.float32, 4), (torch.bfloat16, 8), (torch.float16, 8)):
        wide = torch.randn(n, hp + 2 * off, generator=gen).to(dev).to(dtype)
        block = wide[:, off:off + hp]
        assert not block.is_contiguous()
        want_b = ops.embed_project_table_grad(block.contiguous(), index, tokens, weights, regions, pad_mask=mask)
        got_b = ops.embed_project_table_grad(block, index, tokens, weights, regions, pad_mask=mask)
        assert torch.equal(got_b[0], want_b[0]) and torch.equal(got_b[1], want_b[1])
    # without a mask the garbage indices are bad indices: still no contribution, still the same bits as the tiled form
    want_n = ops.embed_codes_code_grad(g.repeat(1, s), index, tokens, weights, (rows, hp), regions)
    got_n = ops.embed_project_table_grad(g, index, tokens, weights, regions)
    assert torch.equal(got_n[0], want_n[0]) and torch.equal(got_n[1], want_n[1])


# ------------------------------------------------------------------ 2. chunk edges
@pytest.mark.parametrize("hp", [64, 100])
@pytest.mark.parametrize("n", [255, 256, 257, 600])
def test_chunk_edges_with_every_position_on_one_code(dev, n, hp):
    """the rows of code 7 collect n contributions each: one chunk, exactly one full chunk, two chunks, three chunks with a combine"""
    from medtok_amd import ops
    assert ops.EMBED_CODE_GRAD_CHUNK == 256
    tokens, weights, regions, _, _ = kernel_case(dev, 4, 5, seed=11)
    tokens[7] = torch.arange(20, device=dev).view(4, 5) * 7                     # twenty different rows (slots 2 and 3 share a region)
    rows = rows_of(regions)
    g = torch.randn(n, hp, generator=torch.Generator(device="cpu").manual_seed(n + hp)).to(dev)
    index = torch.full((n,), 7, dtype=torch.int64, device=dev)
    want_G, want_bins = ops.embed_codes_code_grad(g.repeat(1, 4), index, tokens, weights, (rows, hp), regions)
    got_G, got_bins = ops.embed_project_table_grad(g, index, tokens, weights, regions)
    assert torch.equal(got_bins, want_bins) and torch.equal(got_G, want_G)
    assert float(got_bins.max()) == n and float(got_bins.sum()) == 20 * n and int((got_bins > 0).sum()) == 20
    # against the definition in fp64 as well: the sum over the positions times the weight
    r = int(regions[1][0] + tokens[7, 1, 2])
    assert rel(got_G[r], weights[7, 1, 2].double() * g.double().sum(0)) <= RTOL
    half = ops.embed_project_table_grad(g.bfloat16(), index, tokens, weights, regions)
    assert torch.equal(half[0], ops.embed_project_table_grad(g.bfloat16().float(), index, tokens, weights, regions)[0])
    again = ops.embed_project_table_grad(g, index, tokens, weights, regions)
    assert torch.equal(again[0], got_G) and torch.equal(again[1], got_bins)


# ------------------------------------------------------------------ 3 / 4. module gradients
def random_vq(dev, n_e, e_dim, k, seed):
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(seed)
    v = VectorQuantizer(n_e, e_dim, 0.25, 0.0, True, True, [e_dim, e_dim], num_head=4, k=k)
    with torch.no_grad():
        v.codebook.weight.normal_()
    return v.to(dev).eval()


def module_case(dev, e_dim, h, seed, n_e=600, k=5, batch=B, length=L, n_segments=5, n_prefix=2):
    """a fresh quantizer (a test may step its codebook), a token table, a [batch, length] index with miss and padded positions, the
    sequence's parts and a probe for both routes"""
    v = random_vq(dev, n_e, e_dim, k, seed)
    gen = torch.Generator(device="cpu").manual_seed(seed + 1)
    sizes = [hi - lo for lo, hi in (v._region(t) for t in TYPES)]
    tokens = torch.stack([torch.randint(0, size, (NUM_CODES, k), generator=gen) for size in sizes], 1).to(dev)
    weights = torch.softmax(torch.randn(NUM_CODES, 4, k, generator=gen), -1).to(dev)
    index, mask = mixed_index(batch * length, NUM_CODES, seed + 2)
    f = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    seg = torch.randint(0, n_segments, (batch, length), generator=gen).sort(1).values.to(dev)
    d = dict(index=index.view(batch, length).to(dev), mask=mask.view(batch, length).to(dev), seg=seg, pe=f(length + 2, h),
             r0=f(batch, n_segments, h), r1=f(batch, n_segments, h), prefix=f(batch, n_prefix, h), probe=f(batch, length, h),
             probe_seq=f(batch, n_prefix + length, h))
    d["probe"][d["mask"]] *= 1e3                                                # (padded positions: only the bias sees them)
    return v, tokens, weights, d


def modules(v, tokens, weights, h, seed, **forms):
    """name -> MedTokEmbedding over one projector and one miss row; forms: name -> constructor arguments"""
    from medtok_amd import MedTokEmbedding
    torch.manual_seed(seed)
    proj = nn.Linear(4 * v.e_dim, h).to(tokens.device)
    out = {}
    for name, kw in forms.items():
        out[name] = m = MedTokEmbedding(v, tokens, weights, types=TYPES, projector=proj, **kw)
        m.miss_emb = next(iter(out.values())).miss_emb
    return out


def reference(v, tokens, weights, d, proj, miss, route):
    """torch autograd over the float64 composition -> (out, dict of gradients)"""
    W64 = v.codebook.weight.detach().double().requires_grad_(True)
    w64, b64 = proj.weight.detach().double().requires_grad_(True), proj.bias.detach().double().requires_grad_(True)
    miss64 = miss.detach().double().requires_grad_(True)
    lo = torch.tensor([v._region(t)[0] for t in TYPES], device=tokens.device).view(1, -1, 1)
    table = (weights.double()[..., None] * F.normalize(W64, dim=-1)[tokens + lo]).sum(2).reshape(tokens.shape[0], -1)
    index, mask = d["index"], d["mask"]
    ok = ~mask & (index >= 0) & (index <= NUM_CODES)
    emb = torch.cat([table, miss64.reshape(1, -1)], 0)[torch.where(ok, index, 0)] * ok.unsqueeze(-1)
    r = F.linear(emb, w64, b64)
    if route == "forward":
        out, probe = r, d["probe"]
    else:
        rows = torch.arange(index.shape[0], device=index.device).view(-1, 1)
        x = ((r + d["pe"].double()[:index.shape[1]]) + d["r0"].double()[rows, d["seg"]]) + d["r1"].double()[rows, d["seg"]]
        out, probe = torch.cat([d["prefix"].double(), torch.where(mask.unsqueeze(-1), r, x)], 1), d["probe_seq"]
    (out * probe.double()).sum().backward()
    return out.detach(), dict(dW=w64.grad, db=b64.grad, dmiss=miss64.grad, dcode=W64.grad)


def step(m, v, d, route, parts_grad=False, **kw):
    """one forward + backward of module m -> (out, dict of gradients)"""
    m.zero_grad(), v.zero_grad()
    parts = {}
    if route == "forward":
        out = m(d["index"], padding_mask=d["mask"], **kw)
        probe = d["probe"]
    else:
        parts = {name: d[name].clone().requires_grad_(parts_grad) for name in ("pe", "r0", "r1", "prefix")}
        out, _ = m.sequence(d["index"], d["mask"], position_rows=parts["pe"], segment_id=d["seg"], segment_rows=(parts["r0"], parts["r1"]),
                            prefix=parts["prefix"], **kw)
        probe = d["probe_seq"]
    (out.float() * probe).sum().backward()
    grads = dict(dW=m.projector.weight.grad.clone(), db=m.projector.bias.grad.clone(), dmiss=m.miss_emb.grad.clone(),
                 dcode=None if v.codebook.weight.grad is None else v.codebook.weight.grad.clone())
    if parts_grad:
        grads.update({name: t.grad.clone() for name, t in parts.items()})
    return out.detach(), grads


@pytest.mark.parametrize("route", ["forward", "sequence"])
@pytest.mark.parametrize("h", [32, 66])
@pytest.mark.parametrize("e_dim", [64, 32])
def test_module_gradients_frozen_codebook(dev, e_dim, h, route):
    v, tokens, weights, d = module_case(dev, e_dim, h, seed=e_dim + h)
    ms = modules(v, tokens, weights, h, seed=h, scatter=dict(fold=True, grad_form="scatter"), dense=dict(fold=True, grad_form="dense"))
    ref_out, ref = reference(v, tokens, weights, d, ms["scatter"].projector, ms["scatter"].miss_emb, route)
    out_d, dense = step(ms["dense"], v, d, route, parts_grad=route == "sequence")
    out_s, got = step(ms["scatter"], v, d, route, parts_grad=route == "sequence")
    assert torch.equal(out_s, out_d) and rel(out_s, ref_out) <= RTOL            # the same kernel over the same tables
    assert got["dcode"] is None and dense["dcode"] is None
    for name in ("dW", "db", "dmiss"):
        errs = rel(got[name], ref[name]), rel(dense[name], ref[name]), rel(got[name], dense[name])
        print(f"frozen e_dim={e_dim} H={h} {route} {name}: rel scatter / dense vs fp64 {errs[:2]}, scatter vs dense {errs[2]}")
        assert got[name].shape == ref[name].shape and float(got[name].abs().max()) > 0
        assert max(errs) <= RTOL
    if route == "sequence":                                                     # the additive parts: the same arithmetic in both forms
        for name in ("pe", "r0", "r1", "prefix"):
            assert torch.equal(got[name], dense[name]) and float(got[name].abs().max()) > 0
    out2, again = step(ms["scatter"], v, d, route, parts_grad=route == "sequence")
    assert torch.equal(out2, out_s) and all(torch.equal(again[name], t) for name, t in got.items() if t is not None)     # two runs: the same bits
    # a 16-bit output sends a 16-bit gradient to the sums: the fp32 result on that gradient widened
    if route == "forward":
        m = ms["scatter"]
        out16, got16 = step(m, v, d, route, out_dtype=torch.bfloat16)
        assert out16.dtype == torch.bfloat16 and torch.equal(out16, out_s.to(torch.bfloat16))
        _, dense16 = step(ms["dense"], v, d, route, out_dtype=torch.bfloat16)
        for name in ("dW", "db", "dmiss"):
            assert rel(got16[name], dense16[name]) <= RTOL
    assert ms["scatter"].fold_builds == 1 and ms["dense"].fold_builds == 1


@pytest.mark.parametrize("route", ["forward", "sequence"])
@pytest.mark.parametrize("h", [32, 66])
@pytest.mark.parametrize("e_dim", [64, 32])
def test_module_gradients_training_codebook(dev, e_dim, h, route):
    v, tokens, weights, d = module_case(dev, e_dim, h, seed=e_dim + h + 7)
    ms = modules(v, tokens, weights, h, seed=h + 1, scatter=dict(fold=True, grad_form="scatter", freeze_codebook=False),
                 dense=dict(fold=True, grad_form="dense", freeze_codebook=False), frozen=dict(fold=True))
    m = ms["scatter"]
    ref_out, ref = reference(v, tokens, weights, d, m.projector, m.miss_emb, route)
    with torch.no_grad():
        frozen_out = (ms["frozen"](d["index"], padding_mask=d["mask"]) if route == "forward" else
                      ms["frozen"].sequence(d["index"], d["mask"], position_rows=d["pe"], segment_id=d["seg"], segment_rows=(d["r0"], d["r1"]),
                                            prefix=d["prefix"])[0])
    out_s, got = step(m, v, d, route)
    assert m.fold_builds == 1 and torch.equal(out_s, frozen_out) and rel(out_s, ref_out) <= RTOL
    out_d, dense = step(ms["dense"], v, d, route)
    assert ms["dense"].fold_builds == 0                                         # the dense form: a training codebook switches the fold off
    for name in ("dcode", "dW", "db", "dmiss"):
        errs = rel(got[name], ref[name]), rel(dense[name], ref[name]), rel(got[name], dense[name])
        print(f"training e_dim={e_dim} H={h} {route} {name}: rel scatter / dense vs fp64 {errs[:2]}, scatter vs dense {errs[2]}")
        assert got[name].shape == ref[name].shape and float(got[name].abs().max()) > 0
        assert max(errs) <= RTOL
    # codebook rows no live contribution reaches: exactly zero
    index, mask = d["index"].reshape(-1), d["mask"].reshape(-1)
    codes = index[~mask & (index >= 0) & (index < NUM_CODES)]
    lo = torch.tensor([v._region(t)[0] for t in TYPES], device=dev).view(1, -1, 1)
    reached = torch.zeros(v.codebook.weight.shape[0], dtype=torch.bool, device=dev)
    reached[(tokens[codes] + lo).reshape(-1)] = True
    assert bool(reached.any()) and bool((~reached).any())
    assert float(got["dcode"][~reached].abs().max()) == 0.0 and float(got["dcode"][reached].abs().max()) > 0
    out2, again = step(m, v, d, route)
    assert torch.equal(out2, out_s) and all(torch.equal(again[name], got[name]) for name in got)       # two runs: the same bits
    assert m.fold_builds == 1                                                   # no optimiser step: the tables were folded once
    # one fold per optimiser step and not otherwise
    opt = torch.optim.SGD([v.codebook.weight, *m.projector.parameters(), m.miss_emb], lr=1e-3)
    for builds in (2, 3):
        opt.step()
        out3, _ = step(m, v, d, route)
        assert m.fold_builds == builds and not torch.equal(out3, out_s)
        step(m, v, d, route)
        assert m.fold_builds == builds


def test_every_position_dead(dev):
    """all positions padded, all at a bad index (validate=False), none at all: the codebook, the projector's weight and the miss row get
    gradients of exactly zero (the bias does not: such positions are the bias row, and its gradient is the column sum of g as in the
    dense form); all positions at the miss index: the codebook's gradient is exactly zero"""
    h = 32
    v, tokens, weights, d = module_case(dev, 64, h, seed=3)
    m = modules(v, tokens, weights, h, seed=2, scatter=dict(fold=True, grad_form="scatter", freeze_codebook=False))["scatter"]
    index, mask, probe = d["index"], d["mask"], d["probe"]
    for idx, msk, all_zero in ((index, torch.ones_like(mask), True), (torch.full_like(index, NUM_CODES + 9), None, True),
                               (index[:0], None, True), (torch.full_like(index, NUM_CODES), None, False)):
        m.zero_grad(), v.zero_grad()
        out = m(idx, padding_mask=msk, validate=False)
        (out * probe[:idx.shape[0]]).sum().backward()
        grad = v.codebook.weight.grad
        assert grad is not None and grad.shape == v.codebook.weight.shape and float(grad.abs().max()) == 0.0
        if all_zero:
            assert float(m.projector.weight.grad.abs().max()) == 0.0 and float(m.miss_emb.grad.abs().max()) == 0.0
            assert rel(m.projector.bias.grad, probe[:idx.shape[0]].double().sum((0, 1))) <= RTOL
        else:
            assert float(m.projector.weight.grad.abs().max()) > 0 and float(m.miss_emb.grad.abs().max()) > 0


# ------------------------------------------------------------------ 5. no activation
def test_a_training_step_makes_no_activation(dev):
    """n = 16,384 positions, S = 4, e_dim = 64: the [n, S * e_dim] activation is 16.8 MB.  The rise of the peak over one forward +
    backward with a training codebook stays below that in the scatter form (its own buffers -- the sort, the chunk sums, the [n, H]
    rows and their gradient -- are about half of it) and exceeds it in the dense form, which unfolds"""
    n, s, e_dim, h = 16384, 4, 64, 32
    limit = n * s * e_dim * 4
    v, tokens, weights, _ = module_case(dev, e_dim, h, seed=21)
    ms = modules(v, tokens, weights, h, seed=5, scatter=dict(fold=True, grad_form="scatter", freeze_codebook=False),
                 dense=dict(fold=True, grad_form="dense", freeze_codebook=False))
    gen = torch.Generator(device="cpu").manual_seed(6)
    index = torch.randint(0, NUM_CODES + 1, (n,), generator=gen).to(dev)
    probe = torch.randn(n, h, generator=gen).to(dev)
    rises = {}
    for name in ("scatter", "dense"):
        m = ms[name]
        for timed in (False, True):                                             # the first step: library, caches, tables, the .grad tensors
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            m(index, validate=False).backward(probe)
            torch.cuda.synchronize()
            rises[name] = torch.cuda.max_memory_allocated() - before
        assert float(v.codebook.weight.grad.abs().max()) > 0 and float(m.projector.weight.grad.abs().max()) > 0
    print(f"peak rise of one step: scatter {rises['scatter'] / 1e6:.2f} MB, dense {rises['dense'] / 1e6:.2f} MB; [n, S * e_dim] is {limit / 1e6:.2f} MB")
    assert ms["scatter"].fold_builds == 1 and ms["dense"].fold_builds == 0
    assert rises["dense"] > limit                                               # the test can tell the two apart
    assert rises["scatter"] < limit


# ------------------------------------------------------------------ 6. graph capture
def test_a_fine_tuning_step_through_sequence_is_captured_in_a_graph(dev):
    h = 32
    v, tokens, weights, d = module_case(dev, 64, h, seed=31, batch=6, length=50)
    m = modules(v, tokens, weights, h, seed=4, scatter=dict(fold=True, grad_form="scatter", freeze_codebook=False))["scatter"]
    parts = [d[name].clone().requires_grad_(True) for name in ("pe", "r0", "r1", "prefix")]
    wrt = [m.projector.weight, m.projector.bias, m.miss_emb, v.codebook.weight] + parts
    index, mask, seg = d["index"].clone(), d["mask"].clone(), d["seg"].clone()

    def grads_of(idx, msk, sg):
        seq, _ = m.sequence(idx, msk, position_rows=parts[0], segment_id=sg, segment_rows=(parts[1], parts[2]), prefix=parts[3], validate=False)
        return torch.autograd.grad((seq * d["probe_seq"]).sum(), wrt)

    def draw(seed):
        i2, m2 = mixed_index(index.numel(), NUM_CODES, seed)
        s2 = torch.randint(0, 5, seg.shape, generator=torch.Generator(device="cpu").manual_seed(seed)).sort(1).values
        return i2.view(index.shape).to(dev), m2.view(mask.shape).to(dev), s2.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up: the normalised codebook and the tables are cached, the library loaded
        grads_of(index, mask, seg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    builds = m.fold_builds
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = grads_of(index, mask, seg)
    for seed in (1, 2):
        i2, m2, s2 = draw(seed)
        index.copy_(i2), mask.copy_(m2), seg.copy_(s2)
        graph.replay()
        torch.cuda.synchronize()
        eager = grads_of(i2, m2, s2)
        for got, want in zip(captured, eager):
            assert float(want.abs().max()) > 0 and torch.equal(got, want)
    assert m.fold_builds == builds == 1


# ------------------------------------------------------------------ 7. the ABI directly
def test_abi_workspace_one_byte_short_is_an_error_and_launches_nothing(dev):
    from medtok_amd import _lib, ops
    lib = _lib.load()
    s, k, hp = 4, 5, 64
    tokens, weights, regions, index, mask = kernel_case(dev, s, k, seed=1)
    n, rows = index.numel(), rows_of(regions)
    g = torch.randn(n, hp, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    arr = ctypes.c_int64 * s
    los, sizes = arr(*[r[0] for r in regions]), arr(*[r[1] for r in regions])
    need = lib.medtok_embed_table_grad_workspace_bytes(n, s, k, rows, hp)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    G = torch.full((rows, hp), 7.0, device=dev)
    bins = torch.full((rows,), 7.0, device=dev)
    pad = mask.view(torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes):
        return lib.medtok_embed_table_grad(g.data_ptr(), 0, 0, index.data_ptr(), pad.data_ptr(), n, tokens.data_ptr(), weights.data_ptr(), NUM_CODES,
                                           s, k, rows, hp, los, sizes, G.data_ptr(), bins.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    rc = call(need - 1)
    assert rc != 0
    with pytest.raises(_lib.MedTokLibraryError, match="workspace too small"):
        _lib.check(rc, "medtok_embed_table_grad")
    torch.cuda.synchronize()
    assert float((G - 7.0).abs().max()) == 0.0 and float((bins - 7.0).abs().max()) == 0.0 and int(ws.max()) == 0     # nothing ran
    assert call(need) == 0
    torch.cuda.synchronize()
    want_G, want_bins = ops.embed_project_table_grad(g, index, tokens, weights, regions, pad_mask=mask)
    assert torch.equal(G, want_G) and torch.equal(bins, want_bins)
