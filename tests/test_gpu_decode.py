"""GPU: decode -- (token ids, weights) back to embeddings -- forward and backward.

Bars: against the C oracle (soft_assign, raw) the decode kernel must agree BIT for bit; against the reference's own numbers (golden
fixtures), against the forward that produced the tokens and against a torch fp64 comparator, 1e-5 of the output's scale
(BASELINE.json:north_star, the RTOL of tests/test_gpu_modules.py, with the same rel())."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def make_vq(name, g, dev, dropout_off=True):
    """(a copy of tests/test_gpu_modules.py::make_vq)"""
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    D, n_e = int(g["e_dim"]), int(g["n_e"])
    heads = int(g["num_head"]) if "num_head" in g else 4
    v = VectorQuantizer(n_e, D, float(g["beta"]), 0.0, True, True, [D, D], num_head=heads, k=int(g["k"]))
    v.load_state_dict(synth.det_state_dict(v, name, int(g["seed"])), strict=True)
    if dropout_off:
        for layer in v.cross_attn.model:
            layer.multihead_attn.dropout = 0.0
            layer.dropout.p = 0.0
    return v.to(dev)


def random_vq(dev, n_e, e_dim, k, seed=0):
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(seed)
    v = VectorQuantizer(n_e, e_dim, 0.25, 0.0, True, True, [e_dim, e_dim], num_head=4 if e_dim % 4 == 0 else 2, k=k)
    with torch.no_grad():
        v.codebook.weight.normal_()
    return v.to(dev).eval()


def oracle_case(oracle, rng, n, n_e, d, k):
    """random rows and codes -> (idx, w, what, zq): the oracle's own search, weights and raw code mix"""
    x = rng.standard_normal((n, d), dtype=np.float32)
    W = rng.standard_normal((n_e, d), dtype=np.float32)
    xhat, xsq = oracle.rownorm(x)
    what, wsq = oracle.rownorm(W)
    idx, dist = oracle.topk_search(xhat, xsq, what, wsq, k)
    w, zq, _ = oracle.soft_assign(xhat, what, idx, dist, raw=True)
    return idx, w, what, zq


# ------------------------------------------------------------------ 1. bits against the C oracle
@pytest.mark.parametrize("n,n_e,d,k", [
    (1, 17, 8, 1), (33, 17, 8, 5), (700, 300, 40, 8), (33, 1000, 64, 9), (700, 20000, 64, 5), (700, 2000, 64, 16),
    (33, 500, 96, 16), (1, 64, 768, 5), (700, 4096, 768, 5), (33, 300, 768, 9), (33, 300, 768, 16), (700, 100, 96, 1),
])
def test_decode_bits_against_the_oracle(oracle, dev, n, n_e, d, k):
    from medtok_amd import ops
    rng = np.random.default_rng(n * 1000003 + n_e * 101 + d * 7 + k)
    idx, w, what, zq = oracle_case(oracle, rng, n, n_e, d, k)
    T = lambda a: torch.from_numpy(a).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.decode_tokens(T(idx), T(w), T(what), status=status)
    assert out.shape == (n, d) and int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy(), zq)


@pytest.mark.parametrize("d,k", [(64, 5), (768, 5), (40, 9), (96, 16)])
def test_decode_four_slots_three_regions_one_call(oracle, dev, d, k):
    """S = 4 slots over three different regions of one table in ONE launch (region-local ids), and into a column block of a wider
    tensor whose other columns stay untouched."""
    from medtok_amd import ops
    rng = np.random.default_rng(d * 31 + k)
    n, n_e = 257, 900
    regions = [(0, 300), (600, 300), (0, 900), (0, 900)]            # text third, graph third, whole table twice
    W = rng.standard_normal((n_e, d), dtype=np.float32)
    what, wsq = oracle.rownorm(W)
    idxs, ws, zqs = [], [], []
    for lo, size in regions:
        x = rng.standard_normal((n, d), dtype=np.float32)
        xhat, xsq = oracle.rownorm(x)
        idx, dist = oracle.topk_search(xhat, xsq, what[lo:lo + size], wsq[lo:lo + size], k)
        w, zq, _ = oracle.soft_assign(xhat, what[lo:lo + size], idx, dist, raw=True)
        idxs.append(idx), ws.append(w), zqs.append(zq)
    tokens = torch.from_numpy(np.stack(idxs, 1)).to(dev)
    weights = torch.from_numpy(np.stack(ws, 1)).to(dev)
    want = np.concatenate(zqs, 1)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.decode_tokens(tokens, weights, torch.from_numpy(what).to(dev), regions, status=status)
    assert int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    wide = torch.full((n, 4 * d + 24), -7.0, device=dev)
    ops.decode_tokens(tokens, weights, torch.from_numpy(what).to(dev), regions, out=wide[:, 8:8 + 4 * d])
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, 8:8 + 4 * d], want)
    assert (got[:, :8] == -7.0).all() and (got[:, 8 + 4 * d:] == -7.0).all()


# ------------------------------------------------------------------ 2. against the reference's own numbers
@pytest.mark.parametrize("name", ["f1_specific_d64", "f2_specific_d768", "f20_specific_k12", "f21_specific_k16_d768"])
def test_decode_reference_tokens_specific(golden, dev, name):
    """The REFERENCE's ids and weights -> the reference's eval zq.  (Every fixture used here and below was checked on the CPU in fp64,
    normalize(W)[lo + idx] . w against the stored embedding: 4.5e-7 .. 5.8e-6, the largest at f21 -- all inside the bar; none dropped.)"""
    g = golden(name)
    v = make_vq(name, g, dev).eval()
    for t in ("text", "graph"):
        idx, w = torch.from_numpy(g[f"{t}.idx"]).to(dev), torch.from_numpy(g[f"{t}.w"]).to(dev)
        with torch.no_grad():
            zq = v.decode(idx, w, types=t)
        err = rel(zq, g[f"{t}.eval.zq"])
        print(name, t, "rel", err)
        assert zq.shape == g[f"{t}.eval.zq"].shape
        assert err <= RTOL


@pytest.mark.parametrize("name", ["f3_forward_d64", "f4_forward_d128", "f19_forward_b64", "f22_forward_d70", "f23_forward_k9", "f24_forward_b256_d64"])
def test_decode_reference_tokens_all_slots(golden, dev, name):
    """all four slots in ONE call against the fixture's eval embeddings in assemble() order (f22: e_dim = 70, the padded path)"""
    g = golden(name)
    v = make_vq(name, g, dev).eval()
    slots = ("text", "graph", "shared_text", "shared_graph")
    tokens = torch.from_numpy(np.stack([g[f"{s}.idx"] for s in slots], 1)).to(dev)
    weights = torch.from_numpy(np.stack([g[f"{s}.w"] for s in slots], 1)).to(dev)
    want = np.concatenate([g["eval.specific_embedding_text"], g["eval.specific_embedding_graph"],
                           g["eval.shared_text_embedding"], g["eval.shared_graph_embedding"]], 1)
    with torch.no_grad():
        emb = v.decode(tokens, weights)
    err = rel(emb, want)
    print(name, "rel", err)
    assert emb.shape == want.shape
    assert err <= RTOL


# ------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("n,e_dim,k", [(1, 64, 1), (33, 64, 5), (4097, 64, 16), (33, 768, 1), (4097, 768, 5), (1, 768, 16)])
def test_round_trip_quantize_pooled(dev, n, e_dim, k):
    from medtok_amd import inference
    v = random_vq(dev, 3000, e_dim, k, seed=n + e_dim + k)
    gen = torch.Generator(device="cpu").manual_seed(n * 7 + k)
    h = torch.randn(n, 2 * e_dim, generator=gen).to(dev)
    pt, pg = torch.randn(n, e_dim, generator=gen).to(dev), torch.randn(n, e_dim, generator=gen).to(dev)
    embedding, tokens, weights = inference.quantize_pooled(v, h, pt, pg)
    with torch.no_grad():
        dec = v.decode(tokens, weights)
        err = rel(dec, embedding)
        print("round trip", n, e_dim, k, "rel", err)
        assert dec.shape == embedding.shape and err <= RTOL
        glob = torch.stack([v.global_token_ids(tokens[:, i], t) for i, t in enumerate(("text", "graph", "shared", "shared"))], 1)
        assert torch.equal(v.decode(glob, weights, global_ids=True), dec)
        # one slot at a time, [N, k] with a single type string: the same bits as its block of the four-slot call
        one = v.decode(tokens[:, 1].contiguous(), weights[:, 1].contiguous(), types="graph")
        assert torch.equal(one, dec[:, e_dim:2 * e_dim])


def tokenizer_and_batches(dev, n_batches, bsz, D=64):
    """a MultimodalTokenizer without encoders (pre-computed features, as tests/test_gpu_modules.py drives it) and its input batches"""
    from medtok_amd.tokenizer import MultimodalTokenizer, make_inputs
    torch.manual_seed(5)
    m = MultimodalTokenizer(text_dim=D, graph_out_channels=D, codebook_size=3000, codebook_embed_dim=D, k=5).to(dev).eval()
    batches = []
    for i in range(n_batches):
        text, mask, nodes, batch = synth.ragged_batch(f"decode.batch{i}", bsz, 12, 6, D, i)
        batches.append(make_inputs(text_features=text.to(dev), attention_mask=mask.to(dev), graph_node_features=nodes.to(dev),
                                   batch=batch.to(dev), code_indices=torch.arange(bsz * i, bsz * (i + 1))))
    return m, batches


def test_round_trip_detokenize(dev):
    m, (batch,) = tokenizer_and_batches(dev, 1, 24)
    with torch.no_grad():
        embedding, tokens, weights = m(batch)
        dec = m.detokenize(tokens, weights)
    err = rel(dec, embedding)
    print("detokenize rel", err)
    assert dec.shape == embedding.shape == (24, 256) and err <= RTOL


# ------------------------------------------------------------------ 4. backward against a torch fp64 comparator
def comparator(W, tokens, weights, regions, probe):
    """(w[..., None] * F.normalize(W)[ids]).sum(2) under autograd in double, on the same device -> (out, g_weights, g_W)"""
    W64 = W.detach().double().requires_grad_(True)
    w64 = weights.detach().double().requires_grad_(True)
    lo = torch.tensor([r[0] for r in regions], device=W.device).view(1, -1, 1)
    out = (w64[..., None] * F.normalize(W64, dim=-1)[tokens + lo]).sum(2).reshape(tokens.shape[0], -1)
    (out * probe.double()).sum().backward()
    return out, w64.grad, W64.grad


@pytest.mark.parametrize("e_dim,k,case", [(64, 1, "random"), (64, 5, "random"), (64, 16, "random"), (768, 1, "random"), (768, 5, "random"),
                                          (768, 16, "random"), (64, 5, "hot"), (768, 5, "hot"), (64, 5, "twice"), (768, 16, "twice"), (70, 5, "random")])
def test_decode_backward_against_fp64(dev, e_dim, k, case):
    n_e, n = 600, 97
    v = random_vq(dev, n_e, e_dim, k, seed=e_dim + k)
    types = ("text", "graph", "shared", "shared")
    regions = [(lo, hi - lo) for lo, hi in (v._region(t) for t in types)]
    gen = torch.Generator(device="cpu").manual_seed(e_dim * 13 + k)
    if case == "hot":                     # every row of every slot picks code 0: one segment of N * S * k rows
        tokens = torch.zeros(n, 4, k, dtype=torch.int64)
    else:                                 # half of every region is never used: zero gradient rows
        tokens = torch.stack([torch.randint(0, size // 2, (n, k), generator=gen) for _, size in regions], 1)
    if case == "twice" and k > 1:         # a row that lists one code twice
        tokens[3, :, 1] = tokens[3, :, 0]
        tokens[40, 2, k - 1] = tokens[40, 2, 0]
    tokens = tokens.to(dev)
    weights = torch.softmax(torch.randn(n, 4, k, generator=gen), -1).to(dev)
    probe = torch.randn(n, 4 * e_dim, generator=gen).to(dev)
    ref_out, ref_gw, ref_gW = comparator(v.codebook.weight, tokens, weights, regions, probe)

    def run():
        v.zero_grad()
        w = weights.clone().requires_grad_(True)
        out = v.decode(tokens, w)
        (out * probe).sum().backward()
        return out.detach(), w.grad.clone(), v.codebook.weight.grad.clone()
    out, gw, gW = run()
    errs = rel(out, ref_out), rel(gw, ref_gw), rel(gW, ref_gW)
    print("backward", e_dim, k, case, "rel out/g_w/g_codebook", errs)
    assert max(errs) <= RTOL
    if case != "hot":
        lo_t, hi_t = v._region("text")
        unused = torch.ones(n_e, dtype=torch.bool, device=dev)
        for s, (lo, size) in enumerate(regions):
            unused[(tokens[:, s] + lo).reshape(-1)] = False
        assert bool(unused.any()) and float(gW[unused].abs().max()) == 0.0
    out2, gw2, gW2 = run()
    assert torch.equal(out, out2) and torch.equal(gw, gw2) and torch.equal(gW, gW2)
    # either gradient alone
    v.zero_grad()
    w = weights.clone().requires_grad_(True)
    v.codebook.weight.requires_grad_(False)
    try:
        (v.decode(tokens, w) * probe).sum().backward()
        assert torch.equal(w.grad, gw) and v.codebook.weight.grad is None
    finally:
        v.codebook.weight.requires_grad_(True)
    v.zero_grad()
    (v.decode(tokens, weights) * probe).sum().backward()
    assert torch.equal(v.codebook.weight.grad, gW)


# ------------------------------------------------------------------ 5. bad ids are an error, not a fault
def test_bad_ids_raise_value_error(dev):
    e_dim, k, n = 64, 5, 50
    v = random_vq(dev, 900, e_dim, k, seed=3)
    size = {"text": 300, "graph": 300, "shared": 900}
    types = ("text", "graph", "shared", "shared")
    gen = torch.Generator(device="cpu").manual_seed(1)
    good = torch.stack([torch.randint(0, size[t], (n, k), generator=gen) for t in types], 1).to(dev)
    weights = torch.softmax(torch.randn(n, 4, k, generator=gen), -1).to(dev)
    with torch.no_grad():
        want = v.decode(good, weights)
        for slot, (row, bad_id) in enumerate(((7, -1), (11, size["graph"]), (13, 2 ** 40))):
            tokens = good.clone()
            tokens[row, slot, 2] = bad_id
            out = torch.full_like(want, 3.0)
            with pytest.raises(ValueError, match=f"slot {slot} "):
                v.decode(tokens, weights, out=out)
            keep = torch.ones(n, 4, dtype=torch.bool, device=dev)
            keep[row, slot] = False
            assert torch.equal(out.view(n, 4, e_dim)[keep], want.view(n, 4, e_dim)[keep])      # every other block is still right
            assert float(out.view(n, 4, e_dim)[row, slot].abs().max()) == 0.0                    # the bad one: zeros
            quiet = v.decode(tokens, weights, validate=False)                                   # nothing read back, nothing raised
            assert torch.equal(quiet, out)
        assert torch.equal(v.decode(good, weights), want)                                       # the next call on the module works
    # under autograd the forward raises the same way, and a backward over a flagged row gives it no gradient
    tokens = good.clone()
    tokens[5, 1, 0] = 10 ** 9
    w = weights.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="slot 1 "):
        v.decode(tokens, w)
    v.zero_grad()
    out = v.decode(tokens, w, validate=False)
    out.sum().backward()
    assert float(w.grad[5, 1].abs().max()) == 0.0 and bool(torch.isfinite(v.codebook.weight.grad).all())
    assert float(w.grad[5, 0].abs().max()) > 0.0


# ------------------------------------------------------------------ 6. no host read: a captured decode replays on new contents
def test_decode_captured_in_a_graph(dev):
    e_dim, k, n = 64, 5, 300
    v = random_vq(dev, 900, e_dim, k, seed=9)
    gen = torch.Generator(device="cpu").manual_seed(2)
    sizes = (300, 300, 900, 900)

    def draw():
        t = torch.stack([torch.randint(0, s, (n, k), generator=gen) for s in sizes], 1).to(dev)
        return t, torch.softmax(torch.randn(n, 4, k, generator=gen), -1).to(dev)
    tokens, weights = draw()
    with torch.no_grad():
        v.decode(tokens, weights, validate=False)              # warm-up: the normalised codebook is cached, the library loaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = v.decode(tokens, weights, validate=False)
        for _ in range(2):
            t2, w2 = draw()
            tokens.copy_(t2), weights.copy_(w2)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, v.decode(t2, w2))


# ------------------------------------------------------------------ 7. lookup without the embedding table
def test_lookup_from_tokens_and_two_file_inference(dev, tmp_path):
    from medtok_amd import inference
    from medtok_amd.tokenizer import MedTokLookup
    m, batches = tokenizer_and_batches(dev, 3, 8)
    emb, tok, wt = inference.run_inference(m, batches, out_dir=str(tmp_path / "two"), save_embeddings=False)
    assert sorted(p.name for p in (tmp_path / "two").iterdir()) == ["tokens_all.npy", "weights_all.npy"]
    codes = [f"C{i:03d}" for i in range(24)]
    offs = (0, 2000, 0, 0)
    for lk in (MedTokLookup.from_tokens(codes, tok, wt, m.quantize, region_offsets=offs),
               MedTokLookup.from_dir(tmp_path / "two", codes, region_offsets=offs, quantizer=m.quantize)):
        one = lk.embed("C005")
        many = lk.embed(["C023", "C000", "C005"])
        assert one.shape == (256,) and many.shape == (3, 256) and one.dtype == np.float32
        assert rel(one, emb[5]) <= RTOL and rel(many, emb[[23, 0, 5]]) <= RTOL
        assert np.array_equal(lk.tokenize("C005"), tok[5] + np.array(offs).reshape(4, 1))
    with pytest.raises(FileNotFoundError):
        MedTokLookup.from_dir(tmp_path / "two", codes)
    # the default still writes the three files, and a lookup over them never needs a quantiser
    # (a second forward of the same batches is compared at the bar, not bit for bit: tokenizer.global_mean_pool sums node features with
    # torch's index_add_, float atomics whose order -- and so the last bit of the graph slot's input -- may change from call to call;
    # the lookup must serve exactly what THIS run wrote)
    emb3, tok3, _ = inference.run_inference(m, batches, out_dir=str(tmp_path / "three"))
    assert sorted(p.name for p in (tmp_path / "three").iterdir()) == ["embeddings_all.npy", "tokens_all.npy", "weights_all.npy"]
    assert np.array_equal(tok3, tok) and rel(emb3, emb) <= RTOL
    full = MedTokLookup.from_dir(tmp_path / "three", codes)
    assert full.quantizer is None and np.array_equal(full.embed("C005"), emb3[5])
    assert np.array_equal(full.embed(["C023", "C000"]), np.load(tmp_path / "three" / "embeddings_all.npy")[[23, 0]])
