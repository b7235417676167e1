"""CPU: the argument checks of decode (no GPU needed) and the unchanged behaviour of a MedTokLookup built the old way."""
import numpy as np
import pytest
import torch


def small_vq(e_dim=8, n_e=30, k=3):
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(0)
    return VectorQuantizer(n_e, e_dim, 0.25, 0.0, True, True, [e_dim, e_dim], k=k).eval()


def test_cpu_tensors_raise_library_error():
    from medtok_amd import ops
    from medtok_amd._lib import MedTokLibraryError
    tokens, weights, what = torch.zeros(4, 2, 3, dtype=torch.int64), torch.ones(4, 2, 3), torch.ones(10, 8)
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        ops.decode_tokens(tokens, weights, what)
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        ops.decode_tokens_backward(torch.ones(4, 16), tokens, weights, what)
    v = small_vq()
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        v.decode(torch.zeros(4, 4, 3, dtype=torch.int64), torch.ones(4, 4, 3))
    with pytest.raises(MedTokLibraryError, match="no CPU path"):
        v.decode(torch.zeros(4, 3, dtype=torch.int64), torch.ones(4, 3), types="graph")


def test_shape_dtype_and_type_errors_come_before_any_library_call(monkeypatch):
    from medtok_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    v = small_vq()
    tok, w = torch.zeros(4, 4, 3, dtype=torch.int64), torch.ones(4, 4, 3)
    for bad_tokens, bad_weights, kw in (
            (tok.int(), w, {}),                                         # ids must be int64
            (tok, w.double(), {}),                                      # weights must be fp32
            (tok, w[:, :, :2], {}),                                     # shapes disagree
            (tok[:, :3], w[:, :3], {}),                                 # three slots for four types
            (tok, w, {"types": ("text", "graph", "shared", "image")}),  # unknown region
            (tok, w, {"types": ()}),
            (tok[:, 0], w[:, 0], {}),                                   # [N, k] needs a single type string
            (tok, w, {"types": "text"}),
            (torch.zeros(4, 4, 17, dtype=torch.int64), torch.ones(4, 4, 17), {}),     # k above the kernels' list length
            (tok, w, {"out": torch.zeros(4, 4 * 8 + 1)}),               # out of the wrong shape
            (tok.numpy(), w, {}),
    ):
        with pytest.raises(ValueError):
            v.decode(bad_tokens, bad_weights, **kw)
    what = torch.ones(10, 8)
    t2, w2 = torch.zeros(4, 2, 3, dtype=torch.int64), torch.ones(4, 2, 3)
    for args, kw in (
            ((t2.int(), w2, what), {}),
            ((t2, w2, what[:, :6]), {}),                                # d % 4
            ((t2, w2, what), {"regions": [(0, 10)]}),                   # one region for two slots
            ((t2, w2, what), {"regions": [(0, 10), (5, 6)]}),           # region past the table
            ((t2, w2, what), {"regions": [(0, 0), (0, 10)]}),           # empty region
            ((torch.zeros(4, 5, 3, dtype=torch.int64), torch.ones(4, 5, 3), what), {}),      # five slots
            ((t2, w2[:, :1], what), {}),
    ):
        with pytest.raises(ValueError):
            ops.decode_tokens(*args, **kw)
    with pytest.raises(ValueError):
        ops.decode_tokens_backward(torch.ones(4, 15), t2, w2, what)     # g_out of the wrong width
    with pytest.raises(ValueError):
        ops.decode_tokens_backward(torch.ones(4, 16), t2, w2, what, want_g_w=False, want_g_code=False)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """argument errors come back through the return code and medtok_last_error() before anything is launched"""
    import ctypes as C
    from medtok_amd import _lib
    lib = _lib.load()
    assert lib.medtok_abi_version() == 4 == _lib.ABI_VERSION
    one = (C.c_int64 * 4)(0, 0, 0, 0), (C.c_int64 * 4)(10, 10, 10, 10)
    assert lib.medtok_decode_tokens_f32(0, 0, 0, 4, 5, 0, 10, 8, *one, 0, 0, 0, None) == 0                    # n = 0: nothing to do
    assert lib.medtok_decode_tokens_backward_f32(0, 0, 0, 0, 0, 4, 5, 0, 10, 8, *one, 16, 0, 0, 0, None) == 0
    for args in ((0, 0, 0, 5, 5, 0, 10, 8, *one, 0, 0, 0, None),        # five slots
                 (0, 0, 0, 4, 17, 0, 10, 8, *one, 0, 0, 0, None),       # topk
                 (0, 0, 0, 4, 5, 0, 10, 6, *one, 0, 0, 0, None),        # d % 4
                 (0, 0, 0, 4, 5, 0, 9, 8, *one, 0, 0, 0, None),         # regions past the table
                 (0, 0, 0, 4, 5, 0, 10, 8, *one, 0, 28, 0, None),       # out_stride below slots * d
                 (0, 0, 5, 4, 5, 0, 10, 8, *one, 0, 0, 0, None)):       # n > 0 with NULL pointers
        assert lib.medtok_decode_tokens_f32(*args) != 0
        assert b"decode_tokens" in lib.medtok_last_error()
    assert lib.medtok_decode_tokens_backward_f32(0, 0, 0, 0, 0, 4, 5, 0, 10, 8, *one, 0, 0, 0, 0, None) != 0   # nothing to compute
    assert lib.medtok_decode_tokens_backward_f32(0, 0, 0, 0, 0, 4, 5, 0, 10, 8, *one, 0, 16, 0, 0, None) != 0  # g_code without g_ids


def test_lookup_built_the_old_way_is_unchanged(tmp_path):
    from medtok_amd.inference import save_outputs
    from medtok_amd.tokenizer import MedTokLookup
    rng = np.random.default_rng(0)
    codes = ["A", "B", "C"]
    emb = rng.standard_normal((3, 32)).astype(np.float32)
    tok = rng.integers(0, 10, (3, 4, 5))
    wt = rng.random((3, 4, 5)).astype(np.float32)
    lk = MedTokLookup(codes, emb, tok, wt, (0, 20, 0, 0))
    assert lk.quantizer is None                       # with embeddings, embed never touches a quantiser
    assert np.array_equal(lk.embed("B"), emb[1]) and np.array_equal(lk.embed(["C", "A"]), emb[[2, 0]])
    assert np.array_equal(lk.tokenize("B"), tok[1] + np.array([0, 20, 0, 0]).reshape(4, 1))
    ids, w = lk.encode("C")
    assert ids.shape == (20,) and np.array_equal(w, wt[2].reshape(-1)) and len(lk) == 3

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the quantiser was used although embeddings were given")
    assert np.array_equal(MedTokLookup(codes, emb, tok, wt, quantizer=Untouchable()).embed("A"), emb[0])
    with pytest.raises(ValueError):
        MedTokLookup(codes, emb[:2], tok, wt)
    with pytest.raises(ValueError, match="quantizer"):
        MedTokLookup(codes, None, tok, wt)
    with pytest.raises(KeyError):
        lk.embed("Z")
    # the files: three by default, two with save_embeddings=False; from_dir without the table asks for a quantiser
    save_outputs(tmp_path / "three", emb, tok, wt)
    assert sorted(p.name for p in (tmp_path / "three").iterdir()) == ["embeddings_all.npy", "tokens_all.npy", "weights_all.npy"]
    assert np.array_equal(MedTokLookup.from_dir(tmp_path / "three", codes).embed("C"), emb[2])
    save_outputs(tmp_path / "two", None, tok, wt, save_embeddings=False)
    assert sorted(p.name for p in (tmp_path / "two").iterdir()) == ["tokens_all.npy", "weights_all.npy"]
    with pytest.raises(FileNotFoundError, match="quantizer"):
        MedTokLookup.from_dir(tmp_path / "two", codes)
