"""CPU: MedTokEmbedding.sequence and the ops behind it (ops.embed_sequence / _rows / _segment_grad / _position_grad) -- the exported
symbols, the constants against the header, the workspace query as host arithmetic, the limits named before any pointer is looked at, the
argument checks, and that nothing here has a CPU path."""
import ctypes
import re
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
N_E, E_DIM, K, NUM_CODES = 96, 8, 5, 10          # regions: text [0, 32), graph [64, 96), shared [0, 96) twice: 256 table rows
ROWS = [(0, 32), (32, 32), (64, 96), (160, 96)]
NEW = ("medtok_embed_sequence_f32", "medtok_embed_sequence_f16", "medtok_embed_sequence_rows_f32", "medtok_embed_sequence_rows_f16",
       "medtok_embed_sequence_grad_workspace_bytes", "medtok_embed_sequence_segment_grad_f32", "medtok_embed_sequence_position_grad_f32")


def make(projector=None, **kw):
    from medtok_amd import MedTokEmbedding
    from medtok_amd.vector_quantization_soft_one_new import VectorQuantizer
    torch.manual_seed(0)
    v = VectorQuantizer(N_E, E_DIM, 0.25, 0.0, True, True, [E_DIM, E_DIM], num_head=4, k=K)
    tokens = torch.randint(0, 32, (NUM_CODES, 4, K))
    weights = torch.softmax(torch.randn(NUM_CODES, 4, K), -1)
    if projector is not None:
        kw["projector"] = projector
    return MedTokEmbedding(v, tokens, weights, **kw)


def test_new_symbols_are_exported_and_bound():
    from medtok_amd import _lib
    lib = ctypes.CDLL(str(_lib.library_path()))
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.load().medtok_abi_version() == _lib.ABI_VERSION == 4          # entries were added: the version stays


def test_constants_equal_the_headers_macros():
    from medtok_amd import ops
    text = (ROOT / "include" / "medtok_vq.h").read_text()
    macro = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))
    assert macro("MEDTOK_EMBED_BAD_SEGMENT_BIT") == ops.EMBED_BAD_SEGMENT_BIT == 5
    assert macro("MEDTOK_EMBED_SEQ_MAX_TERMS") == ops.EMBED_SEQ_MAX_TERMS == 2
    assert macro("MEDTOK_EMBED_SEQ_GRAD_CHUNK") == ops.EMBED_SEQ_GRAD_CHUNK == 256
    assert macro("MEDTOK_EMBED_SEQ_MAX_SEGMENTS") == ops.EMBED_SEQ_MAX_SEGMENTS == 4096
    # the kernels take them from that header: no second definition that could drift
    assert not re.search(r"#define\s+MEDTOK_EMBED_", (ROOT / "medtok_amd" / "csrc" / "embed_sequence_kernels.h").read_text())


def test_workspace_query_is_host_arithmetic():
    from medtok_amd import _lib, ops
    ws = _lib.load().medtok_embed_sequence_grad_workspace_bytes
    c = ops.EMBED_SEQ_GRAD_CHUNK
    r256 = lambda b: (b + 255) // 256 * 256
    want = lambda b, l, v, w: r256(b * ((l + c - 1) // c) * v * w * 4)         # the chunk sums [B, chunks, V, W] fp32
    for shape in ((1, 1, 1, 1), (2, 600, 7, 64), (5, 9, 3, 300), (256, 2000, 100, 64), (3, 257, 4096, 30)):
        assert ws(*shape) == want(*shape) > 0, shape
    assert ws(2, 0, 7, 64) == 0 and ws(0, 600, 7, 64) == 0                     # no position, no batch row: nothing to keep
    base = (4, 1000, 50, 64)
    for axis in range(4):                                                       # it grows with B, L, V and W
        more = list(base)
        more[axis] *= 2
        assert ws(*more) > ws(*base), axis
    assert ws(2, c, 7, 64) < ws(2, c + 1, 7, 64) == ws(2, 2 * c, 7, 64)        # by whole chunks
    assert ws(2, 600, 4096, 64) > 0 and ws(2, 600, 4097, 64) == 0              # V beyond the LDS accumulators: 0
    for bad in ((-1, 600, 7, 64), (2, -1, 7, 64), (2, 600, 0, 64), (2, 600, 7, 0), (2 ** 31, 600, 7, 64), (2, 2 ** 31, 7, 64)):
        assert ws(*bad) == 0, bad                                               # bad shapes: 0, no trap


def test_limits_are_named_errors_before_any_pointer():
    """every pointer here is NULL: a call that got past the limit would end at the NULL check"""
    from medtok_amd import _lib
    lib = _lib.load()
    rc = lib.medtok_embed_sequence_segment_grad_f32(0, 0, 0, 2, 600, 3, 4097, 64, 0, 0, 0, 0)
    assert rc != 0
    with pytest.raises(_lib.MedTokLibraryError, match=r"n_segments=4097 unsupported \(1 \.\. 4096\)"):
        _lib.check(rc, "medtok_embed_sequence_segment_grad_f32")
    rc = lib.medtok_embed_sequence_segment_grad_f32(0, 0, 0, 2, 600, 3, 4096, 64, 0, 0, 0, 0)     # one below: stopped at the NULL check
    with pytest.raises(_lib.MedTokLibraryError, match="required"):
        _lib.check(rc, "medtok_embed_sequence_segment_grad_f32")
    arr = ctypes.c_int64 * 4
    los, sizes = arr(0, 32, 64, 160), arr(32, 32, 96, 96)

    def sequence(batch, length, n_prefix):
        return lib.medtok_embed_sequence_f32(0, 0, batch, length, 0, 0, NUM_CODES, 4, K, 0, 256, 8, los, sizes, 0, 0, 0, 0, 0, 0, 0, 0, 0, n_prefix,
                                             0, 0, 0, 0)

    def rows(batch, length, n_prefix):
        return lib.medtok_embed_sequence_rows_f32(0, 0, batch, length, 30, 0, 0, 0, 0, 0, 0, 0, n_prefix, 0, 0, 0)
    for call, entry in ((sequence, "medtok_embed_sequence_f32"), (rows, "medtok_embed_sequence_rows_f32")):
        for shape in ((2 ** 20, 2 ** 11, 0), (2 ** 20, 2 ** 11 - 3, 3), (2 ** 31, 1, 0), (1, 2 ** 31, 0)):
            rc = call(*shape)
            assert rc != 0
            with pytest.raises(_lib.MedTokLibraryError, match=r"reach 2\^31"):
                _lib.check(rc, entry)
        rc = call(2 ** 20, 2 ** 11 - 4, 3)                                      # 2^31 - 2^20 rows: past the limit, stopped at a NULL check
        assert rc != 0
        with pytest.raises(_lib.MedTokLibraryError, match="required"):
            _lib.check(rc, entry)
    # the ops raise a ValueError before they look at a device (meta tensors: no storage)
    from medtok_amd import ops
    with pytest.raises(ValueError, match=r"2\^31"):
        ops.embed_sequence_rows(torch.empty(2 ** 20, 2 ** 11, 4, device="meta"))
    with pytest.raises(ValueError, match=r"2\^31"):
        ops.embed_sequence_position_grad(torch.empty(2 ** 20, 2 ** 11, 4, device="meta"), 2 ** 11)


def test_argument_checks_of_the_ops():
    from medtok_amd import ops
    table, bias = torch.zeros(256, 8), torch.zeros(8)
    tokens, weights = torch.zeros(NUM_CODES, 4, K, dtype=torch.int64), torch.zeros(NUM_CODES, 4, K)
    index = torch.zeros(3, 7, dtype=torch.int64)
    seg = torch.zeros(3, 7, dtype=torch.int64)
    f = lambda **kw: ops.embed_sequence(index, tokens, weights, table, ROWS, bias, **kw)
    g = lambda **kw: ops.embed_sequence_rows(torch.zeros(3, 7, 30), **kw)
    with pytest.raises(ValueError, match="int64"):
        ops.embed_sequence(index.int(), tokens, weights, table, ROWS, bias)
    with pytest.raises(ValueError, match=r"\[batch, length\]"):
        ops.embed_sequence(index.reshape(-1), tokens, weights, table, ROWS, bias)
    with pytest.raises(ValueError, match="rows must be"):
        ops.embed_sequence_rows(torch.zeros(21, 30))
    with pytest.raises(ValueError, match="rows must be"):
        ops.embed_sequence_rows(torch.zeros(3, 7, 30).double())
    with pytest.raises(ValueError, match="width = 3"):
        f(width=3)
    for call, w in ((f, 8), (g, 30)):
        with pytest.raises(ValueError, match="segment_rows without segment_id"):
            call(segment_rows=torch.zeros(3, 5, w))
        with pytest.raises(ValueError, match="segment_id without segment_rows"):
            call(segment_id=seg)
        with pytest.raises(ValueError, match="3 terms"):
            call(segment_id=seg, segment_rows=[torch.zeros(3, 5, w)] * 3)
        with pytest.raises(ValueError, match="0 terms"):
            call(segment_id=seg, segment_rows=[])
        with pytest.raises(ValueError, match=r"segment_rows\[1\].*width"):
            call(segment_id=seg, segment_rows=[torch.zeros(3, 5, w), torch.zeros(3, 5, w + 4)])
        with pytest.raises(ValueError, match="one V"):
            call(segment_id=seg, segment_rows=[torch.zeros(3, 5, w), torch.zeros(3, 6, w)])
        with pytest.raises(ValueError, match="one V"):
            call(segment_id=seg, segment_rows=torch.zeros(2, 5, w))
        with pytest.raises(ValueError, match=r"segment_rows\[0\].*fp32"):
            call(segment_id=seg, segment_rows=torch.zeros(3, 5, w).half())
        with pytest.raises(ValueError, match="segment_id must be an int64"):
            call(segment_id=seg.int(), segment_rows=torch.zeros(3, 5, w))
        with pytest.raises(ValueError, match="segment_id must be an int64"):
            call(segment_id=seg[:, :6], segment_rows=torch.zeros(3, 5, w))
        with pytest.raises(ValueError, match="4097 segments"):
            call(segment_id=seg, segment_rows=torch.zeros(3, 4097, w))
        with pytest.raises(ValueError, match="position_rows.*width"):
            call(position_rows=torch.zeros(7, w + 1))
        with pytest.raises(ValueError, match="position_rows.*fp32"):
            call(position_rows=torch.zeros(7, w).double())
        with pytest.raises(ValueError, match="fewer than the 7 positions"):
            call(position_rows=torch.zeros(6, w))
        with pytest.raises(ValueError, match="prefix must be"):
            call(prefix=torch.zeros(2, 3, w))
        with pytest.raises(ValueError, match="prefix.*width"):
            call(prefix=torch.zeros(3, 3, w - 1))
        with pytest.raises(ValueError, match="prefix.*fp32"):
            call(prefix=torch.zeros(3, 3, w).bfloat16())
        with pytest.raises(ValueError, match="pad_mask"):
            call(pad_mask=torch.zeros(3, 6, dtype=torch.bool))
        with pytest.raises(ValueError, match="out_dtype"):
            call(out_dtype=torch.float64)
    gr = torch.zeros(3, 3 + 7, 30)
    with pytest.raises(ValueError, match="g must be"):
        ops.embed_sequence_segment_grad(gr.double(), seg, 5, n_prefix=3)
    with pytest.raises(ValueError, match="g must be"):
        ops.embed_sequence_segment_grad(gr, seg, 5, n_prefix=11)
    with pytest.raises(ValueError, match="segment_id must be"):
        ops.embed_sequence_segment_grad(gr, seg, 5, n_prefix=2)
    with pytest.raises(ValueError, match="4097 segments"):
        ops.embed_sequence_segment_grad(gr, seg, 4097, n_prefix=3)
    with pytest.raises(ValueError, match="pad_mask"):
        ops.embed_sequence_segment_grad(gr, seg, 5, pad_mask=torch.zeros(3, 8, dtype=torch.bool), n_prefix=3)
    with pytest.raises(ValueError, match="n_rows = 6"):
        ops.embed_sequence_position_grad(gr, 6, n_prefix=3)
    with pytest.raises(ValueError, match="pad_mask"):
        ops.embed_sequence_position_grad(gr, 7, pad_mask=torch.zeros(3, 7), n_prefix=3)


def test_argument_checks_of_sequence():
    index = torch.zeros(3, 7, dtype=torch.int64)
    seg = torch.zeros(3, 7, dtype=torch.int64)
    for m, w in ((make(), 4 * E_DIM), (make(nn.Linear(4 * E_DIM, 6), fold=True), 6), (make(nn.Linear(4 * E_DIM, 6), fold=False), 6)):
        with pytest.raises(ValueError, match="int64"):
            m.sequence(index.int())
        with pytest.raises(ValueError, match=r"index \[B, L\]"):
            m.sequence(index.reshape(-1))
        with pytest.raises(ValueError, match=r"index \[B, L\]"):
            m.sequence(index.reshape(3, 7, 1))
        with pytest.raises(ValueError, match="segment_rows without segment_id"):
            m.sequence(index, segment_rows=torch.zeros(3, 5, w))
        with pytest.raises(ValueError, match="3 terms"):
            m.sequence(index, segment_id=seg, segment_rows=[torch.zeros(3, 5, w)] * 3)
        with pytest.raises(ValueError, match="width"):
            m.sequence(index, segment_id=seg, segment_rows=torch.zeros(3, 5, w + 2))
        with pytest.raises(ValueError, match="width"):
            m.sequence(index, position_rows=torch.zeros(7, 8 if w == 6 else w + 4))     # (the padded width is not the public one)
        with pytest.raises(ValueError, match="fewer than"):
            m.sequence(index, position_rows=torch.zeros(6, w))
        with pytest.raises(ValueError, match="prefix must be"):
            m.sequence(index, prefix=torch.zeros(4, 3, w))
        with pytest.raises(ValueError, match="fp32"):
            m.sequence(index, prefix=torch.zeros(3, 3, w).half())
        with pytest.raises(ValueError, match="fp32"):
            m.sequence(index, position_rows=torch.zeros(7, w, dtype=torch.float64))
        with pytest.raises(ValueError, match="pad_mask"):
            m.sequence(index, torch.zeros(3, 6, dtype=torch.bool))
        with pytest.raises(ValueError, match="out_dtype"):
            m.sequence(index, out_dtype=torch.float64)


def test_cpu_tensors_raise_library_error():
    from medtok_amd import ops
    from medtok_amd._lib import MedTokLibraryError
    index = torch.zeros(3, 7, dtype=torch.int64)
    seg = torch.zeros(3, 7, dtype=torch.int64)
    for m, w in ((make(), 4 * E_DIM), (make(nn.Linear(4 * E_DIM, 6), fold=True), 6), (make(nn.Linear(4 * E_DIM, 6), fold=False), 6),
                 (make(nn.Linear(4 * E_DIM, 6)), 6)):
        with pytest.raises(MedTokLibraryError):
            m.sequence(index, position_rows=torch.zeros(7, w), segment_id=seg, segment_rows=torch.zeros(3, 5, w), prefix=torch.zeros(3, 3, w))
        with pytest.raises(MedTokLibraryError):
            m.sequence(index)
    table, bias = torch.zeros(256, 8), torch.zeros(8)
    tokens, weights = torch.zeros(NUM_CODES, 4, K, dtype=torch.int64), torch.zeros(NUM_CODES, 4, K)
    with pytest.raises(MedTokLibraryError):
        ops.embed_sequence(index, tokens, weights, table, ROWS, bias, position_rows=torch.zeros(7, 6), width=6)
    with pytest.raises(MedTokLibraryError):
        ops.embed_sequence_rows(torch.zeros(3, 7, 30), segment_id=seg, segment_rows=torch.zeros(3, 5, 30))
    with pytest.raises(MedTokLibraryError):
        ops.embed_sequence_segment_grad(torch.zeros(3, 10, 30), seg, 5, n_prefix=3)
    with pytest.raises(MedTokLibraryError):
        ops.embed_sequence_position_grad(torch.zeros(3, 10, 30).half(), 9, n_prefix=3)
