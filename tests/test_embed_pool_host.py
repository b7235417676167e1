"""CPU: bag pooling (ops.embed_pool / MedTokEmbedding.pooled) -- the argument checks, the workspace query as host arithmetic, the
exported symbols, and that nothing here has a CPU path."""
import ctypes

import pytest
import torch
import torch.nn as nn

N_E, E_DIM, K, NUM_CODES = 96, 8, 5, 10
REGIONS = [(0, 32), (64, 32), (0, 96), (0, 96)]


def make(**kw):
    from medtok_amd import MedTokEmbedding
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(0)
    v = VectorQuantizer(N_E, E_DIM, 0.25, 0.0, True, True, [E_DIM, E_DIM], num_head=4, k=K)
    tokens = torch.randint(0, 32, (NUM_CODES, 4, K))
    weights = torch.softmax(torch.randn(NUM_CODES, 4, K), -1)
    return MedTokEmbedding(v, tokens, weights, **kw)


def table():
    return torch.zeros(NUM_CODES, 4, K, dtype=torch.int64), torch.zeros(NUM_CODES, 4, K), torch.zeros(N_E, E_DIM)


def test_new_symbols_are_exported_and_bound():
    from medtok_amd import _lib
    lib = ctypes.CDLL(str(_lib.library_path()))
    for name in ("medtok_embed_pool_workspace_bytes", "medtok_embed_pool_f32", "medtok_embed_pool_miss_grad_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.load().medtok_abi_version() == _lib.ABI_VERSION == 4          # entries were added: the version stays


def test_workspace_query_is_host_arithmetic():
    from medtok_amd import _lib, ops
    ws = _lib.load().medtok_embed_pool_workspace_bytes
    c = ops.EMBED_POOL_CHUNK
    assert c == 16
    r256 = lambda b: (b + 255) // 256 * 256
    # partial sums [bags, chunks, width] fp32 + counts [bags, chunks, 2] int32, each rounded up to 256 bytes
    for bags, bag_len, width in ((1, 1, 4), (3, c, 256), (3, c + 1, 256), (16, 256, 3072), (4096, 64, 256), (70, 3 * c + 5, 40)):
        chunks = (bag_len + c - 1) // c
        assert ws(bags, bag_len, width) == r256(bags * chunks * width * 4) + r256(bags * chunks * 8), (bags, bag_len, width)
    assert ws(8, 64, 256) > ws(4, 64, 256)                                     # grows with the bags,
    assert ws(4, 64 + 1, 256) > ws(4, 64, 256) == ws(4, 64 - c + 1, 256)       # with the chunks per bag (not inside one chunk),
    assert ws(4, 64, 512) > ws(4, 64, 256)                                     # and with the width
    assert ws(0, 64, 256) == 0 and ws(4, 0, 256) == 0
    assert ws(-1, 64, 256) == 0 and ws(4, -1, 256) == 0 and ws(4, 64, 0) == 0  # bad shapes: 0, no trap
    assert ws(2 ** 20, 2 ** 12, 4096) == 2 ** 20 * 2 ** 8 * (4096 * 4 + 8)      # 64-bit: 4 TiB of partial sums are only counted


def test_embed_pool_argument_checks():
    from medtok_amd import ops
    tokens, weights, what = table()
    index = torch.zeros(3, 7, dtype=torch.int64)
    with pytest.raises(ValueError, match="int64"):
        ops.embed_pool(index.int(), tokens, weights, what, REGIONS)
    for bad in (torch.zeros(7, dtype=torch.int64), torch.zeros(3, 7, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[bags, bag_len\]"):
            ops.embed_pool(bad, tokens, weights, what, REGIONS)
    with pytest.raises(ValueError, match="pad_mask"):
        ops.embed_pool(index, tokens, weights, what, REGIONS, pad_mask=torch.zeros(3, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="pad_mask"):
        ops.embed_pool(index, tokens, weights, what, REGIONS, pad_mask=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="miss"):
        ops.embed_pool(index, tokens, weights, what, REGIONS, miss=torch.zeros(4 * E_DIM + 1))
    with pytest.raises(ValueError, match="expected int64 tokens"):
        ops.embed_pool(index, tokens.int(), weights, what, REGIONS)
    with pytest.raises(ValueError, match="regions"):
        ops.embed_pool(index, tokens, weights, what, REGIONS[:3])
    with pytest.raises(ValueError, match="unsupported"):                        # rows wider than the kernels hold
        ops.embed_pool(index, tokens, weights, torch.zeros(N_E, 1028), REGIONS)
    t17, w17 = torch.zeros(NUM_CODES, 4, 17, dtype=torch.int64), torch.zeros(NUM_CODES, 4, 17)
    with pytest.raises(ValueError, match="unsupported"):
        ops.embed_pool(index, t17, w17, what, REGIONS)
    with pytest.raises(ValueError, match="counts"):
        ops.embed_pool_miss_grad(torch.zeros(3, 32), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="g_out"):
        ops.embed_pool_miss_grad(torch.zeros(4, 32), torch.zeros(3, 2, dtype=torch.int32))


def test_cpu_tensors_raise_library_error():
    from medtok_amd import ops
    from medtok_amd._lib import MedTokLibraryError
    tokens, weights, what = table()
    index = torch.zeros(3, 7, dtype=torch.int64)
    with pytest.raises(MedTokLibraryError):
        ops.embed_pool(index, tokens, weights, what, REGIONS)
    with pytest.raises(MedTokLibraryError):
        ops.embed_pool_miss_grad(torch.zeros(3, 32), torch.zeros(3, 2, dtype=torch.int32))
    for kw in ({}, {"projector": nn.Linear(4 * E_DIM, 6)}, {"freeze_codebook": False}):
        with pytest.raises(MedTokLibraryError):
            make(**kw).pooled(index)


def test_pooled_argument_checks():
    m = make()
    with pytest.raises(ValueError, match="int64"):
        m.pooled(torch.zeros(3, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        m.pooled([[1, 2]])
    for bad in (torch.zeros(7, dtype=torch.int64), torch.zeros(3, 7, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[bags, bag_len\]"):
            m.pooled(bad)
    index = torch.zeros(3, 7, dtype=torch.int64)
    with pytest.raises(ValueError, match="pad_mask"):
        m.pooled(index, padding_mask=torch.zeros(7, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="pad_mask"):
        m.pooled(index, padding_mask=torch.zeros(3, 7, dtype=torch.int64))


def test_launch_limit_is_checked_on_the_host():
    """one launch holds 2^24 - 1 blocks of 256 threads: more chunks (or bags) than that is a named error before anything is launched or
    any pointer is looked at (every pointer here is NULL: a call that got past the limit would end at the NULL check)"""
    from medtok_amd import _lib
    lib = _lib.load()
    arr = ctypes.c_int64 * 4
    los, sizes = arr(0, 64, 0, 0), arr(32, 32, 96, 96)
    fake = 0

    def call(bags, bag_len):
        return lib.medtok_embed_pool_f32(fake, 0, bags, bag_len, fake, fake, NUM_CODES, 4, K, fake, N_E, E_DIM, los, sizes, 0, 1, fake, 0, 0, 0,
                                         fake, 1 << 62, 0)
    for bags, bag_len in ((1 << 24, 1), (1 << 20, 16 * 16 + 1), ((1 << 24) - 1, 17)):
        rc = call(bags, bag_len)
        assert rc != 0
        with pytest.raises(_lib.MedTokLibraryError, match="exceed one launch"):
            _lib.check(rc, "medtok_embed_pool_f32")
