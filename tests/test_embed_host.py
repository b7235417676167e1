"""CPU: the argument checks of the embedding lookup (ops.embed_codes, MedTokEmbedding) and of its C entry points; no GPU needed."""
import numpy as np
import pytest
import torch


def small_vq(e_dim=8, n_e=30, k=3):
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(0)
    return VectorQuantizer(n_e, e_dim, 0.25, 0.0, True, True, [e_dim, e_dim], k=k).eval()


def table(num_codes=6, s=2, k=3):
    return torch.zeros(num_codes, s, k, dtype=torch.int64), torch.ones(num_codes, s, k)


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from medtok_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    tok, w = table()
    what = torch.ones(10, 8)
    index = torch.zeros(4, 5, dtype=torch.int64)
    mask = torch.zeros(4, 5, dtype=torch.bool)
    for args, kw in (
            ((index.int(), tok, w, what), {}),                                              # index must be int64
            ((index.float(), tok, w, what), {}),
            ((index.numpy(), tok, w, what), {}),
            ((index, tok, w[:, :, :2], what), {}),                                          # tokens and weights disagree
            ((index, tok, w[:5], what), {}),
            ((index, tok.int(), w, what), {}),
            ((index, tok, w, what[:, :6]), {}),                                             # d % 4
            ((index, tok, w, what), {"pad_mask": mask[:, :4]}),                             # mask of another shape
            ((index, tok, w, what), {"pad_mask": mask.reshape(-1)}),
            ((index, tok, w, what), {"pad_mask": mask.float()}),                            # mask of another type
            ((index, tok, w, what), {"miss": torch.ones(15)}),                              # miss of the wrong width
            ((index, tok, w, what), {"miss": torch.ones(2, 8)}),
            ((index, tok, w, what), {"miss": torch.ones(16, dtype=torch.float64)}),
            ((index, torch.zeros(6, 2, 17, dtype=torch.int64), torch.ones(6, 2, 17), what), {}),        # k = 17
            ((index, torch.zeros(6, 5, 3, dtype=torch.int64), torch.ones(6, 5, 3), what), {}),          # five slots
            ((index, tok, w, what), {"out": torch.zeros(20, 17)}),                          # out of the wrong shape
            ((index, tok, w, what), {"out": torch.zeros(19, 16)}),
            ((index, tok, w, what), {"out": torch.zeros(20, 16, dtype=torch.float16)}),     # out of another type than out_dtype
            ((index, tok, w, what), {"out": torch.zeros(20, 16), "out_dtype": torch.bfloat16}),
            ((index, tok, w, what), {"out_dtype": torch.float64}),                          # unknown out_dtype
            ((index, tok, w, what), {"out_dtype": torch.int32}),
            ((index, tok, w, what), {"regions": [(0, 10)]}),                                # one region for two slots
            ((index, tok, w, what), {"regions": [(0, 10), (5, 6)]}),                        # region past the table
    ):
        with pytest.raises(ValueError):
            ops.embed_codes(*args, **kw)
    with pytest.raises(ValueError):
        ops.embed_codes_miss_grad(torch.ones(4, 5, 16), index.int(), 6)
    with pytest.raises(ValueError):
        ops.embed_codes_miss_grad(torch.ones(4, 4, 16), index, 6)                           # g_out of another leading shape
    with pytest.raises(ValueError):
        ops.embed_codes_miss_grad(torch.ones(4, 5, 16), index, 6, pad_mask=mask[:2])
    # the module: constructor and forward
    from medtok_amd import MedTokEmbedding
    v = small_vq()
    tok4, w4 = table(6, 4, 3)
    for bad_tokens, bad_weights, kw in (
            (tok4.int(), w4, {}),
            (tok4, w4[:, :, :2], {}),
            (tok4[:, :3], w4[:, :3], {}),                                                   # three slots for four types
            (tok4, w4, {"types": ("text", "graph", "shared", "image")}),
            (torch.zeros(6, 4, 17, dtype=torch.int64), torch.ones(6, 4, 17), {}),
            (torch.zeros(6, 5, 3, dtype=torch.int64), torch.ones(6, 5, 3), {"types": ("text",) * 5}),
    ):
        with pytest.raises(ValueError):
            MedTokEmbedding(v, bad_tokens, bad_weights, **kw)
    m = MedTokEmbedding(v, tok4, w4)
    for args, kw in (((index.int(),), {}), ((index,), {"padding_mask": mask[:, :4]}), ((index,), {"out_dtype": torch.float64}),
                     ((index,), {"out": torch.zeros(20, 31)})):
        with pytest.raises(ValueError):
            m(*args, **kw)


def test_cpu_tensors_raise_library_error():
    from medtok_amd import MedTokEmbedding, ops
    from medtok_amd._lib import MedTokLibraryError
    tok, w = table()
    what, index = torch.ones(10, 8), torch.zeros(4, 5, dtype=torch.int64)
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        ops.embed_codes(index, tok, w, what)
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        ops.embed_codes(index, tok, w, what, miss=torch.ones(16), pad_mask=index == 1, out_dtype=torch.bfloat16)
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        ops.embed_codes_miss_grad(torch.ones(4, 5, 16), index, 6)
    m = MedTokEmbedding(small_vq(), *table(6, 4, 3))
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        m(index)
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        m(index, padding_mask=index == 1, validate=False)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """argument errors come back through the return code and medtok_last_error() before anything is launched"""
    import ctypes as C
    from medtok_amd import _lib
    lib = _lib.load()
    assert lib.medtok_abi_version() == _lib.ABI_VERSION == 4            # (4: the timing probes' two entry points left the ABI)
    one = (C.c_int64 * 4)(0, 0, 0, 0), (C.c_int64 * 4)(10, 10, 10, 10)
    # (index, pad, n, tokens, weights, num_codes, slots, topk, what, n_codes, d, lo, size, miss, out, out_stride[, bf16], status, stream)
    for fn, tail in ((lib.medtok_embed_codes_f32, (0, None)), (lib.medtok_embed_codes_f16, (0, 0, None)), (lib.medtok_embed_codes_f16, (1, 0, None))):
        assert fn(0, 0, 0, 0, 0, 6, 4, 5, 0, 10, 8, *one, 0, 0, 0, *tail) == 0                  # n = 0: nothing to do
        for args in ((0, 0, 0, 0, 0, 6, 5, 5, 0, 10, 8, *one, 0, 0, 0),        # five slots
                     (0, 0, 0, 0, 0, 6, 4, 17, 0, 10, 8, *one, 0, 0, 0),       # topk
                     (0, 0, 0, 0, 0, 6, 4, 5, 0, 10, 6, *one, 0, 0, 0),        # d % 4
                     (0, 0, 0, 0, 0, 6, 4, 5, 0, 9, 8, *one, 0, 0, 0),         # regions past the table
                     (0, 0, 0, 0, 0, 6, 4, 5, 0, 10, 8, *one, 0, 0, 28),       # out_stride below slots * d
                     (0, 0, 0, 0, 0, 0, 4, 5, 0, 10, 8, *one, 0, 0, 0),        # an empty token table
                     (0, 0, 5, 0, 0, 6, 4, 5, 0, 10, 8, *one, 0, 0, 0)):       # n > 0 with NULL pointers
            assert fn(*args, *tail) != 0
            assert b"embed_codes" in lib.medtok_last_error()
    # (g_out, g_stride, index, pad, n, num_codes, width, g_miss, ws, ws_bytes, stream)
    assert lib.medtok_embed_codes_miss_grad_workspace_bytes(0, 256) == 0
    assert lib.medtok_embed_codes_miss_grad_workspace_bytes(257, 256) >= 2 * 256 * 4
    for args in ((0, 0, 0, 0, 5, 6, 256, 0, 0, 0, None),                       # no g_miss
                 (0, 0, 0, 0, 5, 6, 256, 16, 0, 0, None),                      # n > 0 with NULL pointers
                 (16, 0, 16, 0, 5, 6, 0, 16, 0, 0, None),                      # width
                 (16, 128, 16, 0, 5, 6, 256, 16, 0, 0, None),                  # g_stride below width
                 (16, 0, 16, 0, 5, 6, 256, 16, 0, 0, None)):                   # no workspace
        assert lib.medtok_embed_codes_miss_grad_f32(*args) != 0
        assert b"embed_codes_miss_grad" in lib.medtok_last_error()


def test_state_dict_holds_the_table_and_the_miss_row():
    from medtok_amd import MedTokEmbedding
    from medtok_amd.embedding import MedTokEmbedding as same
    assert MedTokEmbedding is same
    v = small_vq()
    rng = np.random.default_rng(0)
    tok = rng.integers(0, 10, (6, 4, 3))
    wt = rng.random((6, 4, 3)).astype(np.float32)
    m = MedTokEmbedding(v, tok, wt)
    assert (m.num_embeddings, m.embedding_dim, m.miss_index) == (7, 32, 6)
    assert m.quantizer is v and not any(p is v.codebook.weight for p in m.parameters())      # referenced, not a submodule
    sd = m.state_dict()
    assert sorted(sd) == ["miss_emb", "tokens", "weights"]
    assert sd["miss_emb"].shape == (1, 32) and isinstance(m.miss_emb, torch.nn.Parameter)
    assert np.array_equal(sd["tokens"].numpy(), tok) and np.array_equal(sd["weights"].numpy(), wt)
    tok[0, 0, 0] += 1                                                  # the buffers are the module's own
    assert int(m.tokens[0, 0, 0]) == tok[0, 0, 0] - 1
    other = MedTokEmbedding(v, np.zeros_like(tok), np.zeros_like(wt))
    assert not torch.equal(other.miss_emb, m.miss_emb)
    other.load_state_dict(sd, strict=True)
    assert torch.equal(other.tokens, m.tokens) and torch.equal(other.weights, m.weights) and torch.equal(other.miss_emb, m.miss_emb)
    # without a miss row there is no such key and no such index; global ids lose their region offsets once, at construction
    bare = MedTokEmbedding(v, tok, wt, miss_row=False)
    assert sorted(bare.state_dict()) == ["tokens", "weights"] and bare.miss_index is None and bare.num_embeddings == 6
    glob = np.stack([tok[:, i] + v._region(t)[0] for i, t in enumerate(("text", "graph", "shared", "shared"))], 1)
    assert v._region("graph")[0] > 0
    assert torch.equal(MedTokEmbedding(v, glob, wt, global_ids=True).tokens, torch.from_numpy(tok))


def test_lookup_embedding_layer_needs_a_quantiser():
    from medtok_amd.tokenizer import MedTokLookup
    rng = np.random.default_rng(1)
    emb, tok, wt = rng.standard_normal((3, 32)).astype(np.float32), rng.integers(0, 10, (3, 4, 3)), rng.random((3, 4, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="quantizer"):
        MedTokLookup(["A", "B", "C"], emb, tok, wt).embedding_layer()
    layer = MedTokLookup.from_tokens(["A", "B", "C"], tok, wt, small_vq()).embedding_layer(miss_row=False)
    assert layer.num_embeddings == 3 and np.array_equal(layer.tokens.numpy(), tok)
