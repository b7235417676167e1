"""GPU: MedTokEmbedding / ops.embed_codes -- code indices through the stored token table to embeddings -- and the miss row's gradient.

Bars: against the C oracle (its own search, soft_assign raw) the lookup kernel must agree BIT for bit, as must a half-precision output
with the converted fp32 output and the module with VectorQuantizer.decode on the gathered rows; against the reference's own numbers
(golden fixtures) and torch fp64 comparators, 1e-5 of the output's scale (the RTOL and rel() of tests/test_gpu_decode.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-5
TYPES = ("text", "graph", "shared", "shared")
N_E = 96                                           # three regions of >= 16 codes (k = 16): text [0, 32), graph [64, 96), shared [0, 96)
REGIONS4 = [(0, 32), (64, 32), (0, 96), (0, 96)]
REGIONS1 = [(64, 32)]                              # one slot: a region that does not start at 0


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def make_vq(name, g, dev):
    """(a copy of tests/test_gpu_decode.py::make_vq)"""
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    D, n_e = int(g["e_dim"]), int(g["n_e"])
    heads = int(g["num_head"]) if "num_head" in g else 4
    v = VectorQuantizer(n_e, D, float(g["beta"]), 0.0, True, True, [D, D], num_head=heads, k=int(g["k"]))
    v.load_state_dict(synth.det_state_dict(v, name, int(g["seed"])), strict=True)
    for layer in v.cross_attn.model:
        layer.multihead_attn.dropout = 0.0
        layer.dropout.p = 0.0
    return v.to(dev)


def random_vq(dev, n_e, e_dim, k, seed=0):
    """(a copy of tests/test_gpu_decode.py::random_vq)"""
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(seed)
    v = VectorQuantizer(n_e, e_dim, 0.25, 0.0, True, True, [e_dim, e_dim], num_head=4 if e_dim % 4 == 0 else 2, k=k)
    with torch.no_grad():
        v.codebook.weight.normal_()
    return v.to(dev).eval()


def random_table(v, num_codes, k, seed, types=TYPES):
    """random region-local ids and softmax weights [num_codes, S, k] on the quantiser's device"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    dev = v.codebook.weight.device
    sizes = [hi - lo for lo, hi in (v._region(t) for t in types)]
    tokens = torch.stack([torch.randint(0, s, (num_codes, k), generator=gen) for s in sizes], 1).to(dev)
    weights = torch.softmax(torch.randn(num_codes, len(types), k, generator=gen), -1).to(dev)
    return tokens, weights


def mixed_index(n, num_codes, seed, miss=0.2, padded=0.15):
    """about `miss` of the positions at the miss index, `padded` of them under the mask with garbage below it -> (index, mask), CPU"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    index = torch.randint(0, num_codes, (n,), generator=gen)
    u = torch.rand(n, generator=gen)
    index[u < miss] = num_codes
    mask = u > 1.0 - padded
    index[mask] = torch.tensor([-7, 2 ** 40, num_codes + 3])[torch.arange(int(mask.sum())) % 3]
    return index, mask


# ------------------------------------------------------------------ 1. bits against the C oracle
_ORACLE_TABLES = {}


def oracle_table(oracle, num_codes, d, k, slots):
    """a table of num_codes rows built by the oracle's own search over `slots` regions of one codebook, made once per shape and shared:
    (tokens [num_codes, S, k], weights, what [N_E, d], regions, zq [num_codes, S * d] = soft_assign(raw=True) per slot, miss [S * d])"""
    key = (num_codes, d, k, slots)
    if key not in _ORACLE_TABLES:
        rng = np.random.default_rng(num_codes * 1000003 + d * 101 + k * 7 + slots)
        regions = REGIONS4 if slots == 4 else REGIONS1
        what, wsq = oracle.rownorm(rng.standard_normal((N_E, d), dtype=np.float32))
        idxs, ws, zqs = [], [], []
        for lo, size in regions:
            xhat, xsq = oracle.rownorm(rng.standard_normal((num_codes, d), dtype=np.float32))
            idx, dist = oracle.topk_search(xhat, xsq, what[lo:lo + size], wsq[lo:lo + size], k)
            w, zq, _ = oracle.soft_assign(xhat, what[lo:lo + size], idx, dist, raw=True)
            idxs.append(idx.reshape(num_codes, k)), ws.append(w.reshape(num_codes, k)), zqs.append(zq)
        miss = rng.standard_normal(slots * d, dtype=np.float32)
        _ORACLE_TABLES[key] = (np.stack(idxs, 1), np.stack(ws, 1), what, regions, np.concatenate(zqs, 1), miss)
    return _ORACLE_TABLES[key]


def index_patterns(n, num_codes, rng):
    """name -> (index [n], mask [n] or None, expected status)"""
    perm = np.resize(rng.permutation(num_codes), n).astype(np.int64)
    garbage = np.resize(np.array([-7, 2 ** 40], np.int64), n)
    mixed = rng.integers(0, num_codes, n)
    u = rng.random(n)
    mixed[u < 0.2] = num_codes
    mask = u > 0.7
    mixed[mask] = garbage[mask]
    return {"permutation": (perm, None), "one code": (np.full(n, int(rng.integers(0, num_codes)), np.int64), None),
            "all miss": (np.full(n, num_codes, np.int64), None), "all padded": (garbage, np.ones(n, bool)), "mixed": (mixed, mask)}


def expected_rows(zq, miss, index, mask, num_codes):
    want = np.zeros((len(index), zq.shape[1]), np.float32)
    live = np.ones(len(index), bool) if mask is None else ~mask
    code = live & (index >= 0) & (index < num_codes)
    want[code] = zq[index[code]]
    want[live & (index == num_codes)] = miss
    return want


@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("num_codes", [1, 50, 3000])
@pytest.mark.parametrize("d,k", [(8, 1), (40, 9), (64, 5), (64, 16), (96, 16), (768, 5), (768, 16)])
def test_embed_bits_against_the_oracle(oracle, dev, d, k, num_codes, slots):
    """every n in {1, 33, 700} (none a multiple of the items per block) x every index pattern, at each table shape: d = 64 is the last
    width on the 16-lane form, d = 96 the first on the 64-lane form (idle lanes)"""
    from medtok_amd import ops
    tokens, weights, what, regions, zq, miss = oracle_table(oracle, num_codes, d, k, slots)
    T = lambda a: torch.from_numpy(a).to(dev)
    tokens, weights, what, miss_t = T(tokens), T(weights), T(what), T(miss)
    rng = np.random.default_rng(d * 31 + k + num_codes)
    for n in (1, 33, 700):
        for name, (index, mask) in index_patterns(n, num_codes, rng).items():
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            out = ops.embed_codes(T(index), tokens, weights, what, regions, miss=miss_t, pad_mask=None if mask is None else T(mask), status=status)
            assert out.shape == (n, slots * d) and out.dtype == torch.float32
            assert int(status.item()) == 0, (n, name)
            assert np.array_equal(out.cpu().numpy(), expected_rows(zq, miss, index, mask, num_codes)), (n, name)


def test_embed_into_a_column_block_and_batch_shapes(oracle, dev):
    """a [B, L] index gives [B, L, S * d]; an `out` that is a column block of a wider tensor leaves the neighbouring columns untouched;
    a uint8 mask is a bool mask"""
    from medtok_amd import ops
    num_codes, d, k = 50, 64, 5
    tokens, weights, what, regions, zq, miss = oracle_table(oracle, num_codes, d, k, 4)
    T = lambda a: torch.from_numpy(a).to(dev)
    index, mask = index_patterns(7 * 19, num_codes, np.random.default_rng(5))["mixed"]
    want = expected_rows(zq, miss, index, mask, num_codes)
    args = (T(tokens), T(weights), T(what), regions)
    out = ops.embed_codes(T(index).view(7, 19), *args, miss=T(miss).view(1, -1), pad_mask=T(mask).view(7, 19))
    assert out.shape == (7, 19, 4 * d) and np.array_equal(out.cpu().numpy().reshape(-1, 4 * d), want)
    wide = torch.full((7 * 19, 4 * d + 24), -7.0, device=dev)
    got = ops.embed_codes(T(index), *args, miss=T(miss), pad_mask=T(mask.astype(np.uint8)), out=wide[:, 8:8 + 4 * d])
    assert got.data_ptr() == wide[:, 8:].data_ptr()
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, 8:8 + 4 * d], want)
    assert (got[:, :8] == -7.0).all() and (got[:, 8 + 4 * d:] == -7.0).all()


# ------------------------------------------------------------------ 2. half-precision output: the fp32 result, rounded once
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d,k", [(64, 5), (768, 5), (64, 16)])
def test_half_output_is_the_converted_fp32_output(dev, d, k, dtype):
    from medtok_amd import ops
    v = random_vq(dev, 600, d, k, seed=d + k)
    num_codes, n = 300, 517
    tokens, weights = random_table(v, num_codes, k, seed=1)
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in TYPES)]
    what = v._normalised_codebook()[0]
    miss = torch.randn(4 * d, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    index, mask = mixed_index(n, num_codes, seed=3)
    index[mask] = 0                                            # (in-range indices under the mask here: status must stay 0)
    index, mask = index.to(dev), mask.to(dev)
    full = ops.embed_codes(index, tokens, weights, what, regions, miss=miss, pad_mask=mask)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    half = ops.embed_codes(index, tokens, weights, what, regions, miss=miss, pad_mask=mask, out_dtype=dtype, status=status)
    assert half.dtype == dtype and half.shape == full.shape and int(status.item()) == 0
    assert torch.equal(half, full.to(dtype))
    assert float(half[mask].float().abs().max()) == 0.0 and torch.equal(half[index == num_codes][0], miss.to(dtype))
    wide = torch.full((n, 4 * d + 8), 3.0, dtype=dtype, device=dev)
    ops.embed_codes(index, tokens, weights, what, regions, miss=miss, pad_mask=mask, out=wide[:, 4:4 + 4 * d], out_dtype=dtype)
    assert torch.equal(wide[:, 4:4 + 4 * d], half) and bool((wide[:, :4] == 3.0).all()) and bool((wide[:, 4 + 4 * d:] == 3.0).all())


def test_module_output_dtype_follows_autocast(dev):
    from medtok_amd import MedTokEmbedding
    v = random_vq(dev, 600, 64, 5, seed=4)
    m = MedTokEmbedding(v, *random_table(v, 100, 5, seed=5))
    index = torch.arange(101, device=dev)
    with torch.no_grad():
        full = m(index)
        assert full.dtype == torch.float32 and torch.equal(m(index, out_dtype=torch.bfloat16), full.to(torch.bfloat16))
        for dtype in (torch.float16, torch.bfloat16):
            with torch.autocast("cuda", dtype=dtype):
                assert torch.equal(m(index), full.to(dtype))
                assert m(index, out_dtype=torch.float32).dtype == torch.float32


# ------------------------------------------------------------------ 3. agreement with the existing decode
@pytest.mark.parametrize("e_dim", [64, 70, 768])
def test_module_equals_decode_on_the_gathered_rows(dev, e_dim):
    """(e_dim = 70: the codebook is padded to 72 columns for the kernels and the result cut back, as decode does)"""
    from medtok_amd import MedTokEmbedding
    k, num_codes = 5, 400
    v = random_vq(dev, 600, e_dim, k, seed=e_dim)
    tokens, weights = random_table(v, num_codes, k, seed=6)
    m = MedTokEmbedding(v, tokens, weights)
    assert (m.num_embeddings, m.embedding_dim, m.miss_index) == (num_codes + 1, 4 * e_dim, num_codes)
    index, _ = mixed_index(3 * 211, num_codes, seed=7, padded=0.0)
    index = index.view(3, 211).to(dev)
    with torch.no_grad():
        got = m(index)
        assert got.shape == (3, 211, 4 * e_dim)
        code = index < num_codes
        assert bool((~code).any()) and torch.equal(got[code], v.decode(tokens[index[code]], weights[index[code]]))
        assert torch.equal(got[~code], m.miss_emb.detach().expand(int((~code).sum()), -1))
        # what the reference's consumer computes: med_code_emb[index] over the decoded table with the miss row appended
        table = torch.cat([v.decode(tokens, weights), m.miss_emb.detach()], 0)
        assert torch.equal(got, table[index])
        # global ids at construction: the same module
        glob = torch.stack([v.global_token_ids(tokens[:, i], t) for i, t in enumerate(TYPES)], 1)
        assert torch.equal(MedTokEmbedding(v, glob, weights, global_ids=True, miss_row=False)(index[code]), got[code])


@pytest.mark.parametrize("name", ["f3_forward_d64", "f4_forward_d128", "f19_forward_b64", "f22_forward_d70", "f23_forward_k9", "f24_forward_b256_d64"])
def test_module_reference_tokens_all_slots(golden, dev, name):
    """the REFERENCE's ids and weights as the table: module(arange) against the fixture's eval embeddings (the fixtures, rel() and bar
    of tests/test_gpu_decode.py::test_decode_reference_tokens_all_slots)"""
    from medtok_amd import MedTokEmbedding
    g = golden(name)
    v = make_vq(name, g, dev).eval()
    slots = ("text", "graph", "shared_text", "shared_graph")
    tokens = np.stack([g[f"{s}.idx"] for s in slots], 1)
    weights = np.stack([g[f"{s}.w"] for s in slots], 1)
    want = np.concatenate([g["eval.specific_embedding_text"], g["eval.specific_embedding_graph"],
                           g["eval.shared_text_embedding"], g["eval.shared_graph_embedding"]], 1)
    m = MedTokEmbedding(v, tokens, weights)
    with torch.no_grad():
        emb = m(torch.arange(tokens.shape[0], device=dev))
    err = rel(emb, want)
    print(name, "rel", err)
    assert emb.shape == want.shape
    assert err <= RTOL


# ------------------------------------------------------------------ 4. bad indices and bad ids are an error, not a fault
def test_bad_indices_and_ids_raise_value_error(dev):
    from medtok_amd import MedTokEmbedding
    e_dim, k, num_codes, n = 64, 5, 200, 50
    v = random_vq(dev, 900, e_dim, k, seed=3)
    tokens, weights = random_table(v, num_codes, k, seed=8)
    m = MedTokEmbedding(v, tokens, weights)
    bare = MedTokEmbedding(v, tokens, weights, miss_row=False)
    good, _ = mixed_index(n, num_codes, seed=9, padded=0.0)
    good[11] = 5
    good = good.to(dev)
    with torch.no_grad():
        want = m(good)
        for module, bad_index in ((m, -1), (m, num_codes + 1), (m, 2 ** 40), (bare, num_codes)):
            index = good.clone()
            if module is bare:
                index[index == num_codes] = 0
            index[11] = bad_index
            ref = module(torch.where(index == bad_index, 5, index))
            out = torch.full_like(want, 3.0)
            with pytest.raises(ValueError, match="code index"):
                module(index, out=out)
            keep = torch.ones(n, dtype=torch.bool, device=dev)
            keep[11] = False
            assert torch.equal(out[keep], ref[keep])                        # every other row is still right
            assert float(out[11].abs().max()) == 0.0                        # the offending one: zeros
            quiet = module(index, validate=False)                           # nothing read back, nothing raised
            assert torch.equal(quiet, out)
            mask = torch.zeros(n, dtype=torch.bool, device=dev)
            mask[11] = True
            assert torch.equal(module(index, padding_mask=mask)[keep], ref[keep])      # under the mask it is no error
        # a bad token id planted in the table: the error names its slot
        for slot, bad_id in ((0, -1), (1, 300), (3, 2 ** 40)):
            broken = MedTokEmbedding(v, tokens, weights)
            broken.load_state_dict(m.state_dict())                          # (the same miss row)
            broken.tokens[5, slot, 2] = bad_id
            with pytest.raises(ValueError, match=f"slot {slot} "):
                broken(good)
            quiet = broken(good, validate=False).view(n, 4, e_dim)
            hit = torch.zeros(n, 4, dtype=torch.bool, device=dev)
            hit[good == 5, slot] = True
            assert int(hit.sum()) >= 1 and float(quiet[hit].abs().max()) == 0.0 and torch.equal(quiet[~hit], want.view(n, 4, e_dim)[~hit])
            assert torch.equal(broken(good[good != 5]), want[good != 5])    # rows that do not touch the bad id raise nothing
        assert torch.equal(m(good), want)                                   # the next call on the module works


# ------------------------------------------------------------------ 5. gradients
def grad_case(dev, e_dim, seed, n=97, num_codes=300, k=5):
    """n = 97 positions, about 20 of them the miss index and 15 under the mask"""
    v = random_vq(dev, 600, e_dim, k, seed=seed)
    tokens, weights = random_table(v, num_codes, k, seed=seed + 1)
    index, mask = mixed_index(n, num_codes, seed=seed + 2)
    gen = torch.Generator(device="cpu").manual_seed(seed + 3)
    probe = torch.randn(n, 4 * e_dim, generator=gen)
    probe[mask] *= 1e6                                                      # gradient under the mask must be ignored
    assert 10 <= int((index[~mask] == num_codes).sum()) <= 30 and 8 <= int(mask.sum()) <= 25
    return v, tokens, weights, index.to(dev), mask.to(dev), probe.to(dev)


@pytest.mark.parametrize("e_dim", [64, 70, 768])
def test_miss_row_gradient(dev, e_dim):
    from medtok_amd import MedTokEmbedding
    v, tokens, weights, index, mask, probe = grad_case(dev, e_dim, seed=e_dim)
    num_codes = tokens.shape[0]
    m = MedTokEmbedding(v, tokens, weights)
    assert m.freeze_codebook and v.codebook.weight.requires_grad

    def run(idx, msk, dtype=None, g=probe):
        m.zero_grad(), v.zero_grad()
        out = m(idx, padding_mask=msk, out_dtype=dtype)
        (out.float() * g).sum().backward()
        return out.detach(), m.miss_emb.grad.clone()
    out, grad = run(index, mask)
    sel = (index == num_codes) & ~mask
    want = probe.double()[sel].sum(0, keepdim=True)
    err = rel(grad, want)
    print("miss grad", e_dim, "rows", int(sel.sum()), "rel", err)
    assert grad.shape == m.miss_emb.shape == (1, 4 * e_dim) and err <= RTOL
    assert v.codebook.weight.grad is None                                   # freeze_codebook=True: the table is a constant
    with torch.no_grad():
        assert torch.equal(out, m(index, padding_mask=mask))                # the autograd path runs the same forward
    out2, grad2 = run(index, mask)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)              # two runs: the same bits
    # a [B, L] batch and a half-precision output / upstream gradient: the same sum, from fp32 copies of the rounded rows
    n = index.numel()
    pad_to = torch.cat([index, index[:3]]).view(4, 25), torch.cat([mask, torch.ones(3, dtype=torch.bool, device=dev)]).view(4, 25)
    _, grad_b = run(*pad_to, g=torch.cat([probe, probe[:3]]).view(4, 25, -1))
    assert n == 97 and torch.equal(grad_b, grad)
    # no position is a miss: exactly zero (also where the only miss indices are under the mask)
    _, none = run(torch.where(sel, 0, index), mask)
    assert float(none.abs().max()) == 0.0
    # no gradient wanted: plain forward
    m.miss_emb.requires_grad_(False)
    assert not m(index, padding_mask=mask).requires_grad


@pytest.mark.parametrize("n", [1, 255, 256, 257, 700])
def test_miss_grad_kernel_block_edges(dev, n):
    """ops.embed_codes_miss_grad around its 256-position blocks, against fp64, with every position a miss and with one"""
    from medtok_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(n)
    g = torch.randn(n, 260, generator=gen).to(dev)
    every = torch.full((n,), 9, dtype=torch.int64, device=dev)
    got = ops.embed_codes_miss_grad(g, every, 9)
    err = rel(got, g.double().sum(0))
    print("miss grad kernel", n, "rel", err)
    assert got.shape == (260,) and err <= RTOL
    last = torch.zeros(n, dtype=torch.int64, device=dev)
    last[n - 1] = 9
    assert torch.equal(ops.embed_codes_miss_grad(g, last, 9), g[n - 1])
    assert float(ops.embed_codes_miss_grad(g, last, 9, pad_mask=last == 9).abs().max()) == 0.0
    assert torch.equal(ops.embed_codes_miss_grad(g.half(), last, 9), g[n - 1].half().float())


def embed_comparator(W, tokens, weights, regions, index, mask, miss, probe):
    """tests/test_gpu_decode.py::comparator extended by the gather: fp64 autograd of the table lookup -> (out, g_W, g_miss)"""
    W64 = W.detach().double().requires_grad_(True)
    miss64 = miss.detach().double().requires_grad_(True)
    lo = torch.tensor([r[0] for r in regions], device=W.device).view(1, -1, 1)
    table = (weights.double()[..., None] * F.normalize(W64, dim=-1)[tokens + lo]).sum(2).reshape(tokens.shape[0], -1)
    out = torch.cat([table, miss64], 0)[index] * (~mask).unsqueeze(-1)
    (out * probe.double()).sum().backward()
    return out, W64.grad, miss64.grad


@pytest.mark.parametrize("e_dim,case", [(64, "random"), (768, "random"), (70, "random"), (64, "hot"), (768, "hot")])
def test_codebook_gradient_when_not_frozen(dev, e_dim, case):
    from medtok_amd import MedTokEmbedding
    v, tokens, weights, index, mask, probe = grad_case(dev, e_dim, seed=e_dim + 11)
    num_codes = tokens.shape[0]
    if case == "hot":                                                       # one code at every position that is neither miss nor padded
        index = torch.where(index < num_codes, 7, index)
    m = MedTokEmbedding(v, tokens, weights, freeze_codebook=False)
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in TYPES)]
    safe = torch.where(mask, 0, index)
    ref_out, ref_gW, ref_gm = embed_comparator(v.codebook.weight, tokens, weights, regions, safe, mask, m.miss_emb, probe)
    m.zero_grad(), v.zero_grad()
    out = m(index, padding_mask=mask)
    (out * probe).sum().backward()
    errs = rel(out, ref_out), rel(v.codebook.weight.grad, ref_gW), rel(m.miss_emb.grad, ref_gm)
    print("unfrozen", e_dim, case, "rel out/g_codebook/g_miss", errs)
    assert max(errs) <= RTOL
    with torch.no_grad():
        assert torch.equal(out, m(index, padding_mask=mask))                # the composed path gives the kernel's rows
    with pytest.raises(ValueError, match="code index"):
        m(torch.where(mask, index, num_codes + 1))


# ------------------------------------------------------------------ 6. no host read: a captured forward replays on new contents
def test_forward_captured_in_a_graph(dev):
    from medtok_amd import MedTokEmbedding
    e_dim, k, num_codes, shape = 64, 5, 500, (6, 50)
    v = random_vq(dev, 900, e_dim, k, seed=9)
    m = MedTokEmbedding(v, *random_table(v, num_codes, k, seed=10))

    def draw(seed):
        index, mask = mixed_index(shape[0] * shape[1], num_codes, seed=seed)
        return index.view(shape).to(dev), mask.view(shape).to(dev)
    index, mask = draw(0)
    with torch.no_grad():
        m(index, padding_mask=mask, validate=False)            # warm-up: the normalised codebook is cached, the library loaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m(index, padding_mask=mask, validate=False)
        for seed in (1, 2):
            i2, m2 = draw(seed)
            index.copy_(i2), mask.copy_(m2)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, m(i2, padding_mask=m2))


# ------------------------------------------------------------------ 7. from a lookup and from the two-file output of inference
def test_from_dir_and_lookup_embedding_layer(dev, tmp_path):
    from medtok_amd import MedTokEmbedding, inference
    from medtok_amd.tokenizer import MedTokLookup, MultimodalTokenizer, make_inputs
    torch.manual_seed(5)
    D, bsz = 64, 8
    model = MultimodalTokenizer(text_dim=D, graph_out_channels=D, codebook_size=3000, codebook_embed_dim=D, k=5).to(dev).eval()
    batches = []
    for i in range(3):
        text, mask, nodes, batch = synth.ragged_batch(f"embed.batch{i}", bsz, 12, 6, D, i)
        batches.append(make_inputs(text_features=text.to(dev), attention_mask=mask.to(dev), graph_node_features=nodes.to(dev),
                                   batch=batch.to(dev), code_indices=torch.arange(bsz * i, bsz * (i + 1))))
    emb, tok, wt = inference.run_inference(model, batches, out_dir=str(tmp_path / "two"), save_embeddings=False)
    assert sorted(p.name for p in (tmp_path / "two").iterdir()) == ["tokens_all.npy", "weights_all.npy"]
    codes = [f"C{i:03d}" for i in range(24)]
    lookup = MedTokLookup.from_dir(tmp_path / "two", codes, quantizer=model.quantize)
    order = [23, 0, 5, 5, 17]
    for layer in (MedTokEmbedding.from_dir(tmp_path / "two", model.quantize), lookup.embedding_layer()):
        assert layer.num_embeddings == 25 and layer.embedding_dim == 4 * D
        assert np.array_equal(layer.tokens.cpu().numpy(), tok) and np.array_equal(layer.weights.cpu().numpy(), wt)
        with torch.no_grad():
            rows = layer(torch.tensor(order, device=dev))
        # bit for bit: the same kernel arithmetic on the same table
        assert np.array_equal(rows.cpu().numpy(), lookup.embed([codes[i] for i in order]))
        assert rel(rows, emb[order]) <= RTOL
    moved = MedTokEmbedding.from_dir(tmp_path / "two", model.quantize, miss_row=False).cpu()
    assert not moved.tokens.is_cuda and moved.quantizer.codebook.weight.is_cuda           # buffers travel with .to(); the quantiser is only referenced
