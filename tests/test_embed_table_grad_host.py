"""CPU: the per-table-row sums of the folded lookup's upstream gradient (ops.embed_project_table_grad / medtok_embed_table_grad) and
MedTokEmbedding(grad_form=...) -- the workspace query as host arithmetic, the limits as named errors before any pointer is looked at,
the op's argument checks before the library is asked for anything, and the switch's validation."""
import ctypes

import pytest
import torch
import torch.nn as nn

N_E, E_DIM, K, NUM_CODES, HP = 96, 8, 5, 10, 12
ROW_REGIONS = [(0, 32), (32, 32), (64, 32), (64, 32)]             # two slots over one region, as the default's two "shared" slots


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
    for name in ("medtok_embed_table_grad_workspace_bytes", "medtok_embed_table_grad"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.load().medtok_abi_version() == _lib.ABI_VERSION == 4          # entries were added: the version stays


def test_workspace_query_is_host_arithmetic():
    from medtok_amd import _lib, ops
    ws = _lib.load().medtok_embed_table_grad_workspace_bytes
    assert ws(111, 4, 5, 1800, 64) > 0
    # n * S * k >= 2^31 and hp % 4 != 0: 0, no trap
    assert ws((2 ** 31 - 1) // 20 + 1, 4, 5, 1800, 64) == 0 and ws(2 ** 31, 1, 1, 1800, 64) == 0 and ws(2 ** 40, 4, 16, 1800, 64) == 0
    assert ws((2 ** 31 - 1) // 20, 4, 5, 1800, 64) > 0
    for hp in (1, 2, 3, 62, 66):
        assert ws(111, 4, 5, 1800, hp) == 0, hp
    assert ws(111, 4, 5, 2 ** 31, 64) == 0 and ws(111, 4, 5, 2 ** 31 - 1, 64) > 0
    prev = 0
    for n in (0, 1, 2, 255, 256, 257, 4096, 16384, 100000):                      # monotone in n
        cur = ws(n, 4, 5, 1800, 64)
        assert cur >= prev
        prev = cur
    assert ws(100000, 4, 5, 1800, 64) > ws(4096, 4, 5, 1800, 64) > ws(0, 4, 5, 1800, 64)
    # strictly below the upstream gradient tiled per slot, the form it must not use: [n * S, hp] floats
    n, s, hp = 16384, 4, 32
    assert ws(n, s, 5, 2400, hp) < n * s * hp * 4
    # what it is: the sort (16 bytes per contribution), 12 bytes per table row, the sort's count tables, the chunk sums
    c = ops.EMBED_CODE_GRAD_CHUNK
    r256 = lambda b: (b + 255) // 256 * 256
    m, rows = n * s * 5, 2400
    assert ws(n, s, 5, rows, hp) == (r256(rows * 4) + 2 * r256((rows + 1) * 4) + r256(256 * 256 * 4) + r256((256 * 256 + 1) * 4) + 4 * r256(m * 4)
                                     + r256((2 * m + c - 1) // c * hp * 4))


def _call(lib, n, slots, k, rows, hp, ws_bytes=1 << 62, g_dtype=0):
    """every pointer NULL except the regions: a call that got past the limits ends at a NULL check"""
    arr = ctypes.c_int64 * 4
    los, sizes = arr(0, 32, 64, 64), arr(32, 32, 32, 32)
    return lib.medtok_embed_table_grad(0, g_dtype, 0, 0, 0, n, 0, 0, NUM_CODES, slots, k, rows, hp, los, sizes, 0, 0, 0, ws_bytes, 0)


def test_limits_are_named_errors_before_any_pointer():
    from medtok_amd import _lib
    lib = _lib.load()
    E = _lib.MedTokLibraryError
    for n, slots, k in (((2 ** 31 - 1) // 20 + 1, 4, 5), (2 ** 31, 1, 1), (2 ** 27, 1, 16), (2 ** 40, 4, 16)):
        rc = _call(lib, n, slots, k, 96, HP)
        assert rc != 0
        with pytest.raises(E, match=r"contributions reach 2\^31"):
            _lib.check(rc, "medtok_embed_table_grad")
    rc = _call(lib, 7, 4, 5, 2 ** 31, HP)
    assert rc != 0
    with pytest.raises(E, match=r"table_rows = 2147483648 reach 2\^31"):
        _lib.check(rc, "medtok_embed_table_grad")
    for hp in (6, 13, 66):
        rc = _call(lib, 7, 4, 5, 96, hp)
        assert rc != 0
        with pytest.raises(E, match="not a multiple of 4"):
            _lib.check(rc, "medtok_embed_table_grad")
    need = lib.medtok_embed_table_grad_workspace_bytes(7, 4, 5, 96, HP)
    rc = _call(lib, 7, 4, 5, 96, HP, ws_bytes=need - 1)
    assert rc != 0
    with pytest.raises(E, match="workspace too small"):
        _lib.check(rc, "medtok_embed_table_grad")
    rc = _call(lib, 7, 4, 5, 96, HP, g_dtype=3)
    assert rc != 0
    with pytest.raises(E, match="g_dtype"):
        _lib.check(rc, "medtok_embed_table_grad")
    rc = _call(lib, 7, 4, 5, 96, HP, ws_bytes=need)                              # past every limit: stopped at the NULL check
    assert rc != 0
    with pytest.raises(E, match="required"):
        _lib.check(rc, "medtok_embed_table_grad")


def test_argument_checks_raise_before_any_library_call():
    from medtok_amd import ops
    tokens, weights = table()
    index = torch.zeros(3, 7, dtype=torch.int64)
    g = torch.zeros(3, 7, HP)
    f = ops.embed_project_table_grad
    with pytest.raises(ValueError, match="int64"):
        f(g, index.int(), tokens, weights, ROW_REGIONS)
    with pytest.raises(ValueError, match="expected int64 tokens"):
        f(g, index, tokens.int(), weights, ROW_REGIONS)
    with pytest.raises(ValueError, match="expected int64 tokens"):
        f(g, index, tokens, weights.double(), ROW_REGIONS)
    with pytest.raises(ValueError, match="g must be"):
        f(g.double(), index, tokens, weights, ROW_REGIONS)
    with pytest.raises(ValueError, match="Hp % 4"):
        f(torch.zeros(3, 7, HP + 2), index, tokens, weights, ROW_REGIONS)
    with pytest.raises(ValueError, match="g must be"):
        f(torch.zeros(3, 6, HP), index, tokens, weights, ROW_REGIONS)
    with pytest.raises(ValueError, match="g must be"):
        f(None, index, tokens, weights, ROW_REGIONS)
    with pytest.raises(ValueError, match="regions"):
        f(g, index, tokens, weights, ROW_REGIONS[:3])
    with pytest.raises(ValueError, match="offset >= 0 and size >= 1"):
        f(g, index, tokens, weights, [(0, 32), (32, 0), (64, 32), (64, 32)])
    with pytest.raises(ValueError, match="offset >= 0 and size >= 1"):
        f(g, index, tokens, weights, [(-1, 32), (32, 32), (64, 32), (64, 32)])
    with pytest.raises(ValueError, match="row_regions"):
        f(g, index, tokens, weights, 5)
    with pytest.raises(ValueError, match=r"table rows reach 2\^31"):
        f(g, index, tokens, weights, [(0, 32), (32, 32), (64, 32), (2 ** 31 - 32, 32)])
    t17, w17 = torch.zeros(NUM_CODES, 4, 17, dtype=torch.int64), torch.zeros(NUM_CODES, 4, 17)
    with pytest.raises(ValueError, match="unsupported"):
        f(g, index, t17, w17, ROW_REGIONS)
    with pytest.raises(ValueError, match="pad_mask"):
        f(g, index, tokens, weights, ROW_REGIONS, pad_mask=torch.zeros(3, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="pad_mask"):
        f(g, index, tokens, weights, ROW_REGIONS, pad_mask=torch.zeros(3, 7))
    # 2^31 contributions: before a device is looked at (meta tensors: no storage of 2^31 / 20 positions)
    n = (2 ** 31 - 1) // 20 + 1
    with pytest.raises(ValueError, match=r"2\^31 contributions"):
        f(torch.empty(n, HP, device="meta"), torch.empty(n, dtype=torch.int64, device="meta"), tokens, weights, ROW_REGIONS)
    for dt in (torch.float16, torch.bfloat16):                                   # 16-bit g is taken as it is: past the checks, no CPU path
        from medtok_amd._lib import MedTokLibraryError
        with pytest.raises(MedTokLibraryError):
            f(g.to(dt), index, tokens, weights, ROW_REGIONS)


def test_grad_form_validation():
    proj = lambda: nn.Linear(4 * E_DIM, 6)
    assert make(projector=proj()).grad_form == "dense"                           # the default
    assert make(projector=proj(), grad_form="scatter").grad_form == "scatter"
    assert make(grad_form="dense").grad_form == "dense"
    for bad in ("Scatter", "sorted", None, True, 1):
        with pytest.raises(ValueError, match="grad_form"):
            make(projector=proj(), grad_form=bad)
    with pytest.raises(ValueError, match="without a projector"):
        make(grad_form="scatter")
    with pytest.raises(ValueError, match="without a projector"):
        make(grad_form="scatter", freeze_codebook=False)
