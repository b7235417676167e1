"""CPU: segment pooling (ops.embed_pool_segments / MedTokEmbedding.pooled_segments) -- the argument checks, raised before the library is
touched, the workspace query as host arithmetic, the C entry's named limits, and the exported symbols."""
import ctypes

import pytest
import torch

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


@pytest.fixture
def no_library(monkeypatch):
    """the library must not be touched: loading it is an error for the length of the test"""
    from medtok_amd import _lib

    def refuse(*a, **kw):
        raise AssertionError("the library was loaded before the argument check")
    monkeypatch.setattr(_lib, "load", refuse)


def test_new_symbols_are_exported_and_bound():
    from medtok_amd import _lib
    lib = ctypes.CDLL(str(_lib.library_path()))
    for name in ("medtok_embed_pool_segments_workspace_bytes", "medtok_embed_pool_segments_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.load().medtok_abi_version() == _lib.ABI_VERSION == 4          # entries were added: the version stays


def test_header_documents_the_order_and_the_chunk():
    from pathlib import Path
    from medtok_amd import ops
    text = (Path(__file__).resolve().parents[1] / "include" / "medtok_vq.h").read_text()
    assert "#define MEDTOK_EMBED_POOL_CHUNK 16" in text and ops.EMBED_POOL_CHUNK == 16
    assert "#define MEDTOK_EMBED_POOL_MAX_WIDTH 4096" in text and ops.EMBED_POOL_MAX_WIDTH == 4096
    assert "((w0 + w1) + w2) + w3" in text and "medtok_embed_pool_segments_f32" in text


def expected_workspace(batch, length, n_segments, width):
    """12 bytes per bag, the sort's two digit tables, 16 bytes per position, ceil(2 B L / 16) partial rows of `width` floats and their
    (count, miss) pairs; every part rounded up to 256 bytes"""
    r256 = lambda b: (b + 255) // 256 * 256
    n, bags = batch * length, batch * n_segments
    q = (2 * n + 15) // 16
    return (r256(bags * 4) + 2 * r256((bags + 1) * 4) + r256(65536 * 4) + r256((65536 + 1) * 4) + 4 * r256(n * 4) + r256(q * width * 4)
            + r256(q * 8))


def test_workspace_query_is_host_arithmetic():
    from medtok_amd import _lib
    ws = _lib.load().medtok_embed_pool_segments_workspace_bytes
    for shape in ((1, 1, 1, 4), (3, 16, 5, 256), (3, 17, 5, 256), (3, 53, 1, 3072), (64, 20, 300, 256), (256, 2000, 100, 256), (7, 0, 3, 40),
                  (2 ** 10, 2 ** 20, 2 ** 10, 4096)):
        assert ws(*shape) == expected_workspace(*shape), shape
    assert ws(8, 64, 5, 256) > ws(4, 64, 5, 256) and ws(4, 65, 5, 256) > ws(4, 64, 5, 256)
    assert ws(4, 64, 500, 256) > ws(4, 64, 5, 256) and ws(4, 64, 5, 512) > ws(4, 64, 5, 256)
    assert ws(0, 64, 5, 256) == 0                                              # nothing to do
    for bad in ((-1, 64, 5, 256), (4, -1, 5, 256), (4, 64, 0, 256), (4, 64, -3, 256), (4, 64, 5, 0), (4, 64, 5, 4097),
                (2 ** 16, 2 ** 15, 5, 256), (2 ** 16, 8, 2 ** 15, 256), (1, 8, 2 ** 31 - 1, 256)):
        assert ws(*bad) == 0, bad                                              # unsupported shapes: 0, no trap
    assert ws(1, 8, 2 ** 31 - 2, 256) > 0 and ws(1, 2 ** 31 - 1, 1, 4) > 0     # the last supported ones are only counted


def test_embed_pool_segments_argument_checks(no_library):
    from medtok_amd import ops
    tokens, weights, what = table()
    index = torch.zeros(3, 7, dtype=torch.int64)
    seg = torch.zeros(3, 7, dtype=torch.int64)
    with pytest.raises(ValueError, match="int64"):
        ops.embed_pool_segments(index.int(), seg, 2, tokens, weights, what, REGIONS)
    for bad in (torch.zeros(7, dtype=torch.int64), torch.zeros(3, 7, 2, dtype=torch.int64)):          # index not 2-D
        with pytest.raises(ValueError, match=r"\[batch, length\]"):
            ops.embed_pool_segments(bad, seg, 2, tokens, weights, what, REGIONS)
    for bad in (seg.int(), seg[:, :6], seg.t(), seg.float(), None, [[0] * 7] * 3):                      # segment_id shape or dtype
        with pytest.raises(ValueError, match="segment_id"):
            ops.embed_pool_segments(index, bad, 2, tokens, weights, what, REGIONS)
    for v in (0, -1):
        with pytest.raises(ValueError, match="n_segments"):
            ops.embed_pool_segments(index, seg, v, tokens, weights, what, REGIONS)
    with pytest.raises(ValueError, match=r"2\^31"):                             # B * V + 1 >= 2^31
        ops.embed_pool_segments(index, seg, (2 ** 31 - 1 + 2) // 3, tokens, weights, what, REGIONS)
    with pytest.raises(ValueError, match="pad_mask"):
        ops.embed_pool_segments(index, seg, 2, tokens, weights, what, REGIONS, pad_mask=torch.zeros(3, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="miss"):
        ops.embed_pool_segments(index, seg, 2, tokens, weights, what, REGIONS, miss=torch.zeros(4 * E_DIM + 1))
    with pytest.raises(ValueError, match="unsupported"):                        # rows wider than EMBED_POOL_MAX_WIDTH
        ops.embed_pool_segments(index, seg, 2, tokens, weights, torch.zeros(N_E, ops.EMBED_POOL_MAX_WIDTH // 4 + 4), REGIONS)
    t17, w17 = torch.zeros(NUM_CODES, 4, 17, dtype=torch.int64), torch.zeros(NUM_CODES, 4, 17)
    with pytest.raises(ValueError, match="unsupported"):                        # slots * k > 64
        ops.embed_pool_segments(index, seg, 2, tokens=t17, weights=w17, what=what, regions=REGIONS)


def test_pooled_segments_argument_checks(no_library):
    m = make()
    index = torch.zeros(3, 7, dtype=torch.int64)
    seg = torch.zeros(3, 7, dtype=torch.int64)
    with pytest.raises(ValueError, match="int64"):
        m.pooled_segments(index.int(), seg, 2)
    for bad in (torch.zeros(7, dtype=torch.int64), torch.zeros(3, 7, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[B, L\]"):
            m.pooled_segments(bad, seg, 2)
    for bad in (seg.int(), seg[:2], None):
        with pytest.raises(ValueError, match="segment_id"):
            m.pooled_segments(index, bad, 2)
    with pytest.raises(ValueError, match="n_segments"):
        m.pooled_segments(index, seg, 0)
    with pytest.raises(ValueError, match="pad_mask"):
        m.pooled_segments(index, seg, 2, padding_mask=torch.zeros(7, 3, dtype=torch.bool))


def test_cpu_tensors_raise_library_error():
    from medtok_amd import ops
    from medtok_amd._lib import MedTokLibraryError
    tokens, weights, what = table()
    index = torch.zeros(3, 7, dtype=torch.int64)
    with pytest.raises(MedTokLibraryError):
        ops.embed_pool_segments(index, index, 2, tokens, weights, what, REGIONS)
    for kw in ({}, {"freeze_codebook": False}):
        with pytest.raises(MedTokLibraryError):
            make(**kw).pooled_segments(index, index, 2)


def test_limits_are_named_errors_before_any_pointer_is_looked_at():
    """every pointer here is NULL: a call that got past a limit would end at the NULL check instead"""
    from medtok_amd import _lib
    lib = _lib.load()
    arr = ctypes.c_int64 * 4
    los, sizes = arr(0, 64, 0, 0), arr(32, 32, 96, 96)

    def call(batch, length, v, slots=4, k=K, d=E_DIM, ws_bytes=1 << 62):
        rc = lib.medtok_embed_pool_segments_f32(0, 0, 0, batch, length, v, 0, 0, NUM_CODES, slots, k, 0, N_E, d, los, sizes, 0, 0, 0, 0, 0, 0, 0,
                                                ws_bytes, 0)
        assert rc != 0
        return rc
    for args, words in (((2 ** 16, 2 ** 15, 5), "positions reach 2\\^31"), ((2 ** 16, 8, 2 ** 15), "bags reach 2\\^31"),
                        ((1, 8, 2 ** 31 - 1), "bags reach 2\\^31"), ((3, 7, 0), "n_segments must be >= 1"), ((3, 7, -2), "n_segments must be >= 1"),
                        ((3, 7, 2, 4, 17), "exceed one wavefront"), ((3, 7, 2, 4, K, 1028), "MEDTOK_EMBED_POOL_MAX_WIDTH"),
                        ((2 ** 12, 2 ** 18, 4), "exceed one launch"), ((3, 7, 2, 4, K, E_DIM, 1024), "workspace too small")):
        with pytest.raises(_lib.MedTokLibraryError, match=words):
            _lib.check(call(*args), "medtok_embed_pool_segments_f32")
