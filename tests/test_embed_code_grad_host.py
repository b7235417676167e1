"""CPU: the codebook gradient of the embedding lookup (ops.embed_codes_code_grad / medtok_embed_code_grad_f32) -- the argument checks, the
workspace query as host arithmetic, the 2^31 limit, the exported chunk constant, and that nothing here has a CPU path."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
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
    return torch.zeros(NUM_CODES, 4, K, dtype=torch.int64), torch.zeros(NUM_CODES, 4, K)


def test_new_symbols_are_exported_and_bound():
    from medtok_amd import _lib
    lib = ctypes.CDLL(str(_lib.library_path()))
    for name in ("medtok_embed_code_grad_workspace_bytes", "medtok_embed_code_grad_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.load().medtok_abi_version() == _lib.ABI_VERSION == 4          # entries were added: the version stays


def test_chunk_constant_equals_the_headers_macro():
    from medtok_amd import ops
    text = (ROOT / "include" / "medtok_vq.h").read_text()
    assert int(re.search(r"#define\s+MEDTOK_EMBED_CODE_GRAD_CHUNK\s+(\d+)", text).group(1)) == ops.EMBED_CODE_GRAD_CHUNK
    # the kernels take it from that header: no second definition that could drift
    assert not re.search(r"#define\s+MEDTOK_EMBED_CODE_GRAD_CHUNK", (ROOT / "medtok_amd" / "csrc" / "embed_grad_kernels.h").read_text())


def test_argument_checks_raise_before_any_library_call():
    from medtok_amd import ops
    tokens, weights = table()
    index = torch.zeros(3, 7, dtype=torch.int64)
    g = torch.zeros(3, 7, 4 * E_DIM)
    shape = (N_E, E_DIM)
    f = ops.embed_codes_code_grad
    with pytest.raises(ValueError, match="int64"):
        f(g, index.int(), tokens, weights, shape, REGIONS)
    with pytest.raises(ValueError, match="expected int64 tokens"):
        f(g, index, tokens.int(), weights, shape, REGIONS)
    with pytest.raises(ValueError, match="expected int64 tokens"):
        f(g, index, tokens, weights.double(), shape, REGIONS)
    with pytest.raises(ValueError, match="g_out"):
        f(g.double(), index, tokens, weights, shape, REGIONS)
    with pytest.raises(ValueError, match="g_out"):
        f(torch.zeros(3, 7, 4 * E_DIM + 4), index, tokens, weights, shape, REGIONS)
    with pytest.raises(ValueError, match="g_out"):
        f(torch.zeros(3, 6, 4 * E_DIM), index, tokens, weights, shape, REGIONS)
    with pytest.raises(ValueError, match="not inside"):
        f(g, index, tokens, weights, shape, [(0, 32), (64, 33), (0, 96), (0, 96)])
    with pytest.raises(ValueError, match="regions"):
        f(g, index, tokens, weights, shape, REGIONS[:3])
    t17, w17 = torch.zeros(NUM_CODES, 4, 17, dtype=torch.int64), torch.zeros(NUM_CODES, 4, 17)
    with pytest.raises(ValueError, match="unsupported"):
        f(g, index, t17, w17, shape, REGIONS)
    with pytest.raises(ValueError, match="pad_mask"):
        f(g, index, tokens, weights, shape, REGIONS, pad_mask=torch.zeros(3, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="pad_mask"):
        f(g, index, tokens, weights, shape, REGIONS, pad_mask=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="d % 4"):
        f(torch.zeros(3, 7, 4 * 6), index, tokens, weights, (N_E, 6), REGIONS)
    with pytest.raises(ValueError, match="shape"):
        f(g, index, tokens, weights, (N_E,), REGIONS)
    # the codebook itself in place of its shape: the same checks
    with pytest.raises(ValueError, match="g_out"):
        f(torch.zeros(3, 7, 4 * E_DIM + 4), index, tokens, weights, torch.zeros(N_E, E_DIM), REGIONS)


def test_cpu_tensors_raise_library_error():
    from medtok_amd import ops
    from medtok_amd._lib import MedTokLibraryError
    tokens, weights = table()
    index = torch.zeros(3, 7, dtype=torch.int64)
    with pytest.raises(MedTokLibraryError):
        ops.embed_codes_code_grad(torch.zeros(3, 7, 4 * E_DIM), index, tokens, weights, (N_E, E_DIM), REGIONS)
    with pytest.raises(MedTokLibraryError):
        ops.embed_codes_code_grad(torch.zeros(3, 7, 4 * E_DIM), index, tokens, weights, torch.zeros(N_E, E_DIM), REGIONS)
    with pytest.raises(MedTokLibraryError):
        make(freeze_codebook=False)(index)


def test_workspace_query_is_host_arithmetic():
    from medtok_amd import _lib, ops
    ws = _lib.load().medtok_embed_code_grad_workspace_bytes
    c = ops.EMBED_CODE_GRAD_CHUNK
    r256 = lambda b: (b + 255) // 256 * 256
    sort_table = 256 * 256                                                       # the radix sort's (digit, wave) counts

    def want(n, s, k, n_codes, d):
        m = n * s * k
        # histogram / chunk counts, offsets, first chunks; the sort's count tables; two (key, payload) buffers; the chunk sums
        return (r256(n_codes * 4) + 2 * r256((n_codes + 1) * 4) + r256(sort_table * 4) + r256((sort_table + 1) * 4) + 4 * r256(m * 4)
                + r256((2 * m + c - 1) // c * d * 4))
    for shape in ((1, 1, 1, 1, 4), (97, 4, 5, 96, 64), (3 * c + 5, 4, 16, 96, 768), (4096, 4, 5, 49152, 768), (56770, 4, 5, 49152, 768)):
        assert ws(*shape) == want(*shape) > 0, shape
    assert ws(0, 4, 5, 96, 64) > 0                                               # positive (the per-row tables) without a position
    prev = 0
    for n in (0, 1, 2, 255, 256, 257, 4096, 100000):                             # non-decreasing in n ...
        cur = ws(n, 4, 5, 96, 768)
        assert cur >= prev
        prev = cur
    prev = 0
    for n_codes in (1, 2, 63, 64, 65, 96, 4096, 49152, 2 ** 31 - 1):             # ... and in K
        cur = ws(97, 4, 5, n_codes, 768)
        assert cur >= prev
        prev = cur
    # the row-per-contribution buffer of the composed route is not in it: 20 bytes per contribution + 8 d / CHUNK, not 4 d
    assert ws(4096, 4, 5, 96, 768) < 4096 * 4 * 5 * 768 * 4 // 20
    # n * S * k >= 2^31: 0; the largest n below it is only counted (64-bit)
    assert ws((2 ** 31 - 1) // 20 + 1, 4, 5, 96, 768) == 0 and ws(2 ** 31, 1, 1, 96, 768) == 0 and ws(2 ** 40, 4, 16, 96, 768) == 0
    assert ws((2 ** 31 - 1) // 20, 4, 5, 96, 768) == want((2 ** 31 - 1) // 20, 4, 5, 96, 768)
    assert ws(2 ** 31 - 1, 1, 1, 96, 4) > 0
    for bad in ((-1, 4, 5, 96, 768), (4, 0, 5, 96, 768), (4, 5, 5, 96, 768), (4, 4, 17, 96, 768), (4, 4, 5, 0, 768), (4, 4, 5, 2 ** 31, 768),
                (4, 4, 5, 96, 6), (4, 4, 5, 96, 0)):
        assert ws(*bad) == 0, bad                                                # bad shapes: 0, no trap


def test_two_to_the_31_contributions_is_a_named_error_before_any_pointer():
    """every pointer here is NULL: a call that got past the limit would end at the NULL check"""
    from medtok_amd import _lib, ops
    lib = _lib.load()
    arr = ctypes.c_int64 * 4
    los, sizes = arr(0, 64, 0, 0), arr(32, 32, 96, 96)

    def call(n, slots, k):
        return lib.medtok_embed_code_grad_f32(0, 0, 0, 0, n, 0, 0, NUM_CODES, slots, k, N_E, E_DIM, los, sizes, 0, 0, 0, 1 << 62, 0)
    for n, slots, k in (((2 ** 31 - 1) // 20 + 1, 4, 5), (2 ** 31, 1, 1), (2 ** 27, 1, 16), (2 ** 40, 4, 16)):
        rc = call(n, slots, k)
        assert rc != 0
        with pytest.raises(_lib.MedTokLibraryError, match=r"reach 2\^31"):
            _lib.check(rc, "medtok_embed_code_grad_f32")
    rc = call((2 ** 31 - 1) // 20, 4, 5)                                         # one below: past the limit, stopped at the NULL check
    assert rc != 0
    with pytest.raises(_lib.MedTokLibraryError, match="required"):
        _lib.check(rc, "medtok_embed_code_grad_f32")
    # the op raises its ValueError before it looks at a device (a meta index: no storage of 2^31 / 20 positions)
    tokens, weights = table()
    n = (2 ** 31 - 1) // 20 + 1
    with pytest.raises(ValueError, match=r"2\^31"):
        ops.embed_codes_code_grad(torch.empty(n, 4 * E_DIM, device="meta"), torch.empty(n, dtype=torch.int64, device="meta"), tokens, weights,
                                  (N_E, E_DIM), REGIONS)
