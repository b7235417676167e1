"""The rounded-operand reference of the half-precision attention backward (tests/attention_half_reference.py), pinned on the CPU:
with identity rounding it IS the oracle's backward (itself pinned to torch autograd, tests/test_oracle_golden.py), and the mask it
is handed is the mask the oracle's training forward applies."""
import numpy as np
import pytest

import attention_half_reference as R


def _ragged_case(d, p):
    """the ragged case of test_attention_train_forward_and_backward_match_oracle (tests/test_gpu_kernels.py)"""
    rng = np.random.default_rng(d + int(100 * p))
    q_len = np.array([40, 7, 0, 64, 33, 5], np.int64); kv_len = np.array([50, 33, 12, 100, 0, 1], np.int64)
    slot_kv = kv_len + np.array([0, 3, 0, 0, 4, 0])
    q_start, kv_start = np.cumsum(q_len) - q_len, np.cumsum(slot_kv) - slot_kv
    nq, nk = int(q_len.sum()) + 2, int(slot_kv.sum())
    q = (rng.standard_normal((nq, d)) * 0.3).astype(np.float32); kv = rng.standard_normal((nk, d)).astype(np.float32)
    d_out = rng.standard_normal((nq, d)).astype(np.float32)
    return q, q_start, q_len, kv, kv_start, kv_len, d_out


@pytest.mark.parametrize("d,p", [(64, 0.0), (64, 0.1), (128, 0.1)])
def test_identity_rounding_is_the_oracle_backward(oracle, d, p):
    """r = identity, acc = float64: dQ / dKV equal the oracle's within 2e-6 of each code's scale (the oracle stores fp32: 6e-8 of an
    entry's magnitude) -- the formulas, the orientation of the mask, keep_scale and the delta convention."""
    q, q_start, q_len, kv, kv_start, kv_len, d_out = _ragged_case(d, p)
    scale, seed = 0.2, 99
    out, lse, dq_o, dkv_o = oracle.shared_kv_attention_train(q, q_start, q_len, kv, kv_start, kv_len, scale, p, seed, d_out)
    masks = R.keep_masks(oracle, seed, q_start, q_len, kv_len, p)
    if p > 0:
        kept = sum(int(m.sum()) for m in masks) / float((q_len * kv_len).sum())
        assert 1 - p - 0.03 < kept < 1 - p + 0.03
    else:
        assert all(m.all() for m in masks)
    ref = R.backward(q, q_start, q_len, kv, kv_start, kv_len, d_out, out, lse, scale, masks, R.keep_scale_of(p), half=None, acc=np.float64)
    for b in range(len(q_len)):
        e_dq = R.code_error(dq_o, ref["dq"], ref["dq_scale"][b], int(q_start[b]), int(q_len[b]))
        e_dkv = R.code_error(dkv_o, ref["dkv"], ref["dkv_scale"][b], int(kv_start[b]), int(kv_len[b]))
        assert e_dq <= 2e-6 and e_dkv <= 2e-6, (b, e_dq, e_dkv)
    # the whole tensors too: rows of no code, slots past a code's keys and codes without a partner are zero in both
    assert np.abs(dq_o - ref["dq"]).max() <= 2e-6 * ref["dq_scale"].max() and np.abs(dkv_o - ref["dkv"]).max() <= 2e-6 * ref["dkv_scale"].max()
    own_q, own_k = np.zeros(len(q), bool), np.zeros(len(kv), bool)
    for b in range(len(q_len)):
        if kv_len[b] > 0:
            own_q[q_start[b]: q_start[b] + q_len[b]] = True
        if q_len[b] > 0:
            own_k[kv_start[b]: kv_start[b] + kv_len[b]] = True
    assert not ref["dq"][~own_q].any() and not ref["dkv"][~own_k].any()
    # the magnitude bounds the reference entry by entry, and a code's scale is positive where the code has queries and keys
    assert (np.abs(ref["dq"]) <= ref["dq_mag"] * (1 + 1e-12)).all() and (np.abs(ref["dkv"]) <= ref["dkv_mag"] * (1 + 1e-12)).all()
    both = (q_len > 0) & (kv_len > 0)
    assert (ref["dq_scale"][both] > 0).all() and (ref["dkv_scale"][both] > 0).all() and not ref["dq_scale"][~both].any()


def test_fp32_accumulation_and_rounding_move_the_reference_as_expected(oracle):
    """acc = float32 stays within 1e-4 of acc = float64 per code (fp32 products of a few hundred terms); rounding the operands to
    bf16 moves the result by far more than that -- the two switches do what they say."""
    import torch
    q, q_start, q_len, kv, kv_start, kv_len, d_out = _ragged_case(64, 0.1)
    out, lse = oracle.shared_kv_attention_train(q, q_start, q_len, kv, kv_start, kv_len, 0.2, 0.1, 99)
    masks = R.keep_masks(oracle, 99, q_start, q_len, kv_len, 0.1)
    args = (q, q_start, q_len, kv, kv_start, kv_len, d_out, out, lse, 0.2, masks, R.keep_scale_of(0.1))
    r64, r32 = R.backward(*args, half=None, acc=np.float64), R.backward(*args, half=None, acc=np.float32)
    h64 = R.backward(*args, half=torch.bfloat16, acc=np.float64)
    for b in range(len(q_len)):
        if q_len[b] == 0 or kv_len[b] == 0:
            continue
        e32 = R.code_error(r32["dq"], r64["dq"], r64["dq_scale"][b], int(q_start[b]), int(q_len[b]))
        eh = R.code_error(h64["dq"], r64["dq"], r64["dq_scale"][b], int(q_start[b]), int(q_len[b]))
        assert 0 < e32 <= 1e-4 < eh, (b, e32, eh)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_oracle_mask_is_the_mask_of_the_oracle_forward(oracle, p):
    """zero queries and one-hot keys: uniform probabilities, so out[r, j] = M[r, j] / (T (1 - p)) -- the mask the training forward
    applies, read off its output, equals oracle.att_keep_mask entry by entry (packed query row, key of the code)."""
    d, seed = 40, 1234
    q_len = np.array([5, 0, 7, 33], np.int64); kv_len = np.array([6, 3, 40, 1], np.int64)
    q_start, kv_start = np.cumsum(q_len) - q_len + 3, np.cumsum(kv_len) - kv_len       # (the first packed query row is not 0)
    nq, nk = int(q_len.sum()) + 3, int(kv_len.sum())
    kv_hot = np.zeros((nk, d), np.float32)
    for b in range(len(q_len)):
        for j in range(kv_len[b]):
            kv_hot[kv_start[b] + j, j] = 1.0
    out_hot, _ = oracle.shared_kv_attention_train(np.zeros((nq, d), np.float32), q_start, q_len, kv_hot, kv_start, kv_len, 0.4, p, seed)
    masks = R.keep_masks(oracle, seed, q_start, q_len, kv_len, p)
    ks = 1.0 / (1.0 - np.float32(p))
    for b in range(len(q_len)):
        got = out_hot[q_start[b]: q_start[b] + q_len[b], : kv_len[b]]
        assert masks[b].shape == got.shape
        assert np.array_equal(got > 0, masks[b])
        assert np.allclose(got, masks[b] * ks / max(int(kv_len[b]), 1), rtol=1e-6, atol=0)
    assert not np.array_equal(masks[2], R.keep_masks(oracle, seed + 1, q_start, q_len, kv_len, p)[2])
    assert oracle.att_keep_mask(seed, 0, 4, 9, 0.0).all()
