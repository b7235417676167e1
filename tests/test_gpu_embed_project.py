"""GPU: MedTokEmbedding with a projector -- the consumers' nn.Linear folded into the lookup (ops.fold_projector / ops.embed_project,
embed_folded_kernel) -- against torch fp64, against the unfolded path, and under autograd.

Bar: rel() <= 1e-5 of the output's scale, the RTOL and rel() of tests/test_gpu_embed.py and tests/test_gpu_decode.py; the existing
fp32 composition F.linear(module(index, mask), W, b) must meet it on the same inputs, so the inputs are known to be fair.  Half
outputs and repeated calls are compared bit for bit."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
RTOL = 1e-5
N_E = 96                                           # text [0, 32), graph [64, 96), shared [0, 96): regions of >= 16 codes (k = 16)
TYPES = {4: ("text", "graph", "shared", "shared"), 1: ("graph",)}        # one slot: a region that does not start at 0
NUM_CODES = 50
WIDTHS = (4, 6, 36, 260)                           # H: 6 is padded to 8; 260 is one float4 more than a 64-lane pass
POSITIONS = (1, 63, 257)


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


@functools.lru_cache(maxsize=None)
def table_case(e_dim, slots, k):
    """a VectorQuantizer(96, e_dim) with a random codebook, a random token table [NUM_CODES, slots, k] and the fp64 embedding table
    (miss row not included: it belongs to a module) -- made once per shape and left unchanged"""
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


def table64(v, types, tokens, weights, codebook=None):
    cb = v.codebook.weight.detach().double() if codebook is None else codebook
    lo = torch.tensor([v._region(t)[0] for t in types], device=tokens.device).view(1, -1, 1)
    return (weights.double()[..., None] * F.normalize(cb, dim=-1)[tokens + lo]).sum(2).reshape(tokens.shape[0], -1)


def comparator(table, miss64, index, mask, w64, b64):
    """F.linear(table64[index], W64, b64), the bias row at padded positions"""
    safe = torch.where(mask, 0, index)
    emb = torch.cat([table, miss64.reshape(1, -1)], 0)[safe] * (~mask).unsqueeze(-1)
    return F.linear(emb, w64, b64)


def make_modules(case, h, seed, **kw):
    """(folded, unfolded, plain) modules over one projector and one miss row"""
    from medtok_amd import MedTokEmbedding
    v, types, tokens, weights = case
    torch.manual_seed(seed)
    proj = nn.Linear(len(types) * v.e_dim, h).to(tokens.device)
    folded = MedTokEmbedding(v, tokens, weights, types=types, projector=proj, fold=True, **kw)
    unfolded = MedTokEmbedding(v, tokens, weights, types=types, projector=proj, fold=False, **kw)
    plain = MedTokEmbedding(v, tokens, weights, types=types, **kw)
    unfolded.miss_emb = folded.miss_emb
    plain.miss_emb = folded.miss_emb
    return folded, unfolded, plain


# ------------------------------------------------------------------ 1-4. output, path agreement, half outputs, repeatability
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("slots", [4, 1])
@pytest.mark.parametrize("e_dim", [64, 8])
def test_folded_output(dev, e_dim, slots, k):
    case = table_case(e_dim, slots, k)
    v, types, tokens, weights = case
    t64 = table64(*case)
    for h in WIDTHS:
        folded, unfolded, plain = make_modules(case, h, seed=h)
        w64, b64 = folded.projector.weight.detach().double(), folded.projector.bias.detach().double()
        miss64 = folded.miss_emb.detach().double()
        for n in POSITIONS:
            index, mask = mixed_index(n, NUM_CODES, seed=n + h)
            index, mask = index.to(dev), mask.to(dev)
            want = comparator(t64, miss64, index, mask, w64, b64)
            with torch.no_grad():
                got = folded(index, padding_mask=mask)
                comp = F.linear(plain(index, padding_mask=mask), folded.projector.weight, folded.projector.bias)
                other = unfolded(index, padding_mask=mask)
                errs = rel(got, want), rel(comp, want), rel(other, want), rel(got, other)
                print(f"e={e_dim} S={slots} k={k} H={h} n={n}: rel folded/composition/unfolded vs fp64 {errs[:3]}, folded vs unfolded {errs[3]}")
                assert got.shape == (n, h) and got.dtype == torch.float32 and other.shape == (n, h)
                assert errs[1] <= RTOL                                  # the inputs are fair: the existing fp32 composition meets the bar
                assert errs[0] <= RTOL and errs[2] <= RTOL and errs[3] <= RTOL
                if bool(mask.any()):
                    assert torch.equal(got[mask], folded.projector.bias.detach().expand(int(mask.sum()), -1))     # padded: the bias row
                assert torch.equal(folded(index, padding_mask=mask), got)                                          # two calls, the same bits
                for dtype in (torch.float16, torch.bfloat16):
                    half = folded(index, padding_mask=mask, out_dtype=dtype)
                    assert half.dtype == dtype and torch.equal(half, got.to(dtype))
        assert folded.fold_builds == 1 and unfolded.fold_builds == 0


def test_batch_shapes_out_autocast_and_padded_e_dim(dev):
    """a [B, L] index gives [B, L, H]; out= is filled (H = 6: through the padded width); autocast picks the dtype; e_dim = 70 (the
    codebook padded to 72 columns for the kernels) folds to the same function"""
    from medtok_amd.tokenizer import MedTokLookup
    case = table_case(70, 4, 5)
    t64 = table64(*case)
    for h in (6, 36):
        folded, unfolded, _ = make_modules(case, h, seed=3)
        index, mask = mixed_index(7 * 19, NUM_CODES, seed=5)
        index, mask = index.view(7, 19).to(dev), mask.view(7, 19).to(dev)
        want = comparator(t64, folded.miss_emb.detach().double(), index.reshape(-1), mask.reshape(-1),
                          folded.projector.weight.detach().double(), folded.projector.bias.detach().double())
        with torch.no_grad():
            got = folded(index, padding_mask=mask)
            assert got.shape == (7, 19, h) and rel(got.reshape(-1, h), want) <= RTOL and rel(unfolded(index, padding_mask=mask), got) <= RTOL
            for m in (folded, unfolded):
                out = torch.full((7 * 19, h), 3.0, device=dev)
                assert m(index, padding_mask=mask, out=out) is out and torch.equal(out, m(index, padding_mask=mask).reshape(-1, h))
            with torch.autocast("cuda", dtype=torch.bfloat16):
                assert torch.equal(folded(index, padding_mask=mask), got.to(torch.bfloat16))
                assert folded(index, padding_mask=mask, out_dtype=torch.float32).dtype == torch.float32
        for m in (folded, unfolded):                       # with grad enabled too, a call that fills `out` builds no graph
            filled = m(index, padding_mask=mask, out=torch.empty(7 * 19, h, device=dev))
            assert filled.grad_fn is None and not filled.requires_grad and torch.equal(filled, got.reshape(-1, h) if m is folded else
                                                                                        m(index, padding_mask=mask).detach().reshape(-1, h))
    v, types, tokens, weights = case
    layer = MedTokLookup([f"C{i}" for i in range(NUM_CODES)], None, tokens.cpu().numpy(), weights.cpu().numpy(), quantizer=v).embedding_layer(
        projector=nn.Linear(280, 6).to(dev), fold=True)
    assert layer.fold is True and layer(torch.arange(5, device=dev)).shape == (5, 6)


# ------------------------------------------------------------------ 5. the status word
def test_bad_indices_and_ids(dev):
    case = table_case(64, 4, 5)
    v, types, tokens, weights = case
    folded, unfolded, _ = make_modules(case, 36, seed=1)
    n = 50
    good, _ = mixed_index(n, NUM_CODES, seed=9, padded=0.0)
    good[11] = 5
    good = good.to(dev)
    with torch.no_grad():
        want = folded(good)
        for bad_index in (-1, NUM_CODES + 1, 2 ** 40):
            index = good.clone()
            index[11] = bad_index
            with pytest.raises(ValueError, match="code index"):
                folded(index)
            quiet = folded(index, validate=False)
            comp = unfolded(index, validate=False)
            assert rel(quiet, comp) <= RTOL and torch.equal(quiet[11], folded.projector.bias.detach())
            keep = torch.arange(n, device=dev) != 11
            assert torch.equal(quiet[keep], want[keep])
        from medtok_amd import MedTokEmbedding
        broken = MedTokEmbedding(v, tokens, weights, types=types, projector=folded.projector, fold=True)
        broken_unfolded = MedTokEmbedding(v, tokens, weights, types=types, projector=folded.projector, fold=False)
        broken.miss_emb = broken_unfolded.miss_emb = folded.miss_emb
        for m in (broken, broken_unfolded):
            m.tokens[5, 2, 2] = 300
            with pytest.raises(ValueError, match="slot 2 "):
                m(good)
        quiet, comp = broken(good, validate=False), broken_unfolded(good, validate=False)
        hit = good == 5
        assert int(hit.sum()) >= 1 and rel(quiet, comp) <= RTOL
        assert torch.equal(quiet[~hit], want[~hit]) and not torch.equal(quiet[hit], want[hit])
        assert torch.equal(folded(good), want)


# ------------------------------------------------------------------ 6. the cache of the folded tables
def test_folded_tables_follow_the_weights(dev):
    from medtok_amd import MedTokEmbedding
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    _, types, tokens, weights = table_case(64, 4, 5)
    torch.manual_seed(2)
    v = VectorQuantizer(N_E, 64, 0.25, 0.0, True, True, [64, 64], num_head=4, k=5)      # its own quantiser: the codebook is written below
    with torch.no_grad():
        v.codebook.weight.normal_()
    v = v.to(dev).eval()
    m = MedTokEmbedding(v, tokens, weights, types=types, projector=nn.Linear(256, 36).to(dev), fold=True)
    ref = MedTokEmbedding(v, tokens, weights, types=types, projector=m.projector, fold=False)
    ref.miss_emb = m.miss_emb
    index, mask = mixed_index(257, NUM_CODES, seed=4)
    index, mask = index.to(dev), mask.to(dev)
    with torch.no_grad():
        first = m(index, padding_mask=mask)
        assert m.fold_builds == 1
        assert torch.equal(m(index, padding_mask=mask), first) and m.fold_builds == 1          # an unchanged second call builds nothing
        last = first
        for step, change in enumerate((lambda: m.projector.weight.mul_(1.5), lambda: m.projector.bias.add_(1.0), lambda: m.miss_emb.mul_(-2.0),
                                       lambda: (v.codebook.weight.data.mul_(torch.linspace(0.5, 2.0, 64, device=dev)), v.invalidate_codebook_cache()))):
            change()
            got = m(index, padding_mask=mask)
            assert m.fold_builds == step + 2
            assert not torch.equal(got, last) and rel(got, ref(index, padding_mask=mask)) <= RTOL
            assert torch.equal(m(index, padding_mask=mask), got) and m.fold_builds == step + 2
            last = got
        # fold=None: 257 positions x 4 slots >= 3 x 256 table rows folds a cold cache; one position does not, until the cache is warm
        auto = MedTokEmbedding(v, tokens, weights, types=types, projector=m.projector)
        auto(index[:1], padding_mask=mask[:1])
        assert auto.fold_builds == 0
        auto(index, padding_mask=mask)
        auto(index[:1], padding_mask=mask[:1])
        assert auto.fold_builds == 1


# ------------------------------------------------------------------ 7. gradients
@pytest.mark.parametrize("e_dim,slots,k,h,n,chunk", [(64, 4, 5, 36, 257, 100), (8, 1, 16, 6, 63, 100), (70, 4, 5, 260, 257, 100), (8, 4, 1, 4, 1, 100),
                                                     (8, 4, 5, 6, 16384 + 37, None)])
def test_gradients(dev, monkeypatch, e_dim, slots, k, h, n, chunk):
    """chunk = 100: n = 257 is three blocks of positions.  chunk = None: the block length as shipped (16,384 positions: every entry of
    dW is one fp32 chain that long, then a second, short block is added.  With terms t of random sign the partial sums reach about
    sqrt(n) t, each of the n roundings is at most 2^-24 of one, and they add up like a random walk: about n * 2^-24 t = 1e-3 t against
    a scale of a few sqrt(n) t = 400 t, a few 1e-6: the bar of 1e-5 of the scale stands at this length too)"""
    from medtok_amd import autograd
    if chunk is not None:
        monkeypatch.setattr(autograd, "EMBED_PROJECT_GRAD_CHUNK", chunk)
    else:
        assert autograd.EMBED_PROJECT_GRAD_CHUNK < n < 2 * autograd.EMBED_PROJECT_GRAD_CHUNK
    case = table_case(e_dim, slots, k)
    v, types, tokens, weights = case
    folded, unfolded, _ = make_modules(case, h, seed=h + n)
    index, mask = mixed_index(n, NUM_CODES, seed=n + 1)
    if n == 1:
        index[0], mask[0] = NUM_CODES, False                                  # the one position: a miss
    probe = torch.randn(n, h, generator=torch.Generator(device="cpu").manual_seed(n)).to(dev)
    index, mask = index.to(dev), mask.to(dev)
    w64 = folded.projector.weight.detach().double().requires_grad_(True)
    b64 = folded.projector.bias.detach().double().requires_grad_(True)
    miss64 = folded.miss_emb.detach().double().requires_grad_(True)
    want = comparator(table64(*case), miss64, index, mask, w64, b64)
    (want * probe.double()).sum().backward()

    def run(m):
        m.zero_grad(), v.zero_grad()
        out = m(index, padding_mask=mask)
        (out * probe).sum().backward()
        return out.detach(), m.projector.weight.grad.clone(), m.projector.bias.grad.clone(), m.miss_emb.grad.clone()
    for name, m in (("folded", folded), ("unfolded", unfolded)):
        out, gw, gb, gm = run(m)
        errs = rel(out, want), rel(gw, w64.grad), rel(gb, b64.grad), rel(gm, miss64.grad)
        print(f"{name} e={e_dim} S={slots} k={k} H={h} n={n}: rel out/dW/db/dmiss {errs}")
        assert gw.shape == w64.shape and gb.shape == b64.shape and gm.shape == folded.miss_emb.shape
        assert max(errs) <= RTOL
        assert v.codebook.weight.grad is None                                  # freeze_codebook=True: the table is a constant
        again = run(m)
        assert all(torch.equal(a, b) for a, b in zip((out, gw, gb, gm), again))          # two runs: the same bits
    out = run(folded)[0]
    with torch.no_grad():
        assert torch.equal(out, folded(index, padding_mask=mask))              # the autograd path runs the same forward


def test_codebook_gradient_when_not_frozen(dev):
    case = table_case(64, 4, 5)
    v, types, tokens, weights = case
    m, _, _ = make_modules(case, 36, seed=8, freeze_codebook=False)
    n = 97
    index, mask = mixed_index(n, NUM_CODES, seed=12)
    index, mask = index.to(dev), mask.to(dev)
    probe = torch.randn(n, 36, generator=torch.Generator(device="cpu").manual_seed(13)).to(dev)
    cb64 = v.codebook.weight.detach().double().requires_grad_(True)
    w64 = m.projector.weight.detach().double().requires_grad_(True)
    b64 = m.projector.bias.detach().double().requires_grad_(True)
    miss64 = m.miss_emb.detach().double().requires_grad_(True)
    want = comparator(table64(*case, codebook=cb64), miss64, index, mask, w64, b64)
    (want * probe.double()).sum().backward()
    m.zero_grad(), v.zero_grad()
    out = m(index, padding_mask=mask)
    (out * probe).sum().backward()
    errs = (rel(out, want), rel(v.codebook.weight.grad, cb64.grad), rel(m.projector.weight.grad, w64.grad), rel(m.projector.bias.grad, b64.grad),
            rel(m.miss_emb.grad, miss64.grad))
    v.zero_grad()
    print("unfrozen: rel out/d codebook/dW/db/dmiss", errs)
    assert max(errs) <= RTOL and m.fold_builds == 0


# ------------------------------------------------------------------ 8. no host read: a captured forward replays on new contents
def test_forward_captured_in_a_graph(dev):
    case = table_case(64, 4, 5)
    m, _, _ = make_modules(case, 36, seed=6)
    shape = (6, 50)

    def draw(seed):
        index, mask = mixed_index(shape[0] * shape[1], NUM_CODES, seed=seed)
        return index.view(shape).to(dev), mask.view(shape).to(dev)
    index, mask = draw(0)
    with torch.no_grad():
        m(index, padding_mask=mask, validate=False)            # warm-up: the tables are folded, the library loaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m(index, padding_mask=mask, validate=False)
        assert m.fold_builds == 1
        for seed in (1, 2):
            i2, m2 = draw(seed)
            index.copy_(i2), mask.copy_(m2)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, m(i2, padding_mask=m2))
