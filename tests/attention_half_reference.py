"""Rounded-operand reference of the half-precision attention backward (test code only: plain numpy / torch on the CPU).

Restates what shared_kv_attention_dq_kernel / shared_kv_attention_dkv_kernel (medtok_amd/csrc/attention_backward.h, HM = 1 / 2)
round and where, per code, with r(.) = round-to-nearest-even to the half type:

    Qr = r(q)   Kr = r(kv)   Gr = r(d_out)                    (att_load_rows_h / att_cvt16: once, on the way in)
    lse as given (fp32);  delta_r = <d_out_r, out_r> of the UNROUNDED fp32 rows (row_dot_kernel at the call site)
    S  = scale Qr Kr^T            P  = exp(S - lse)            PM = P o M keep_scale
    dP = (Gr Kr^T) o M keep_scale                              dS = P o (dP - delta) scale
    PM and dS pass through fp32 and then r(.)                  (att_pack8 rounds the fp32 LDS tiles)
    dQ = r(dS) Kr                 dKV = r(PM)^T Gr + r(dS)^T Qr

and a MAGNITUDE for every output entry -- the same sums with absolute values, (|P| (|dP| + |delta|) scale) |Kr| for dQ and
|PM|^T |Gr| + (|P| (|dP| + |delta|) scale)^T |Qr| for dKV: what an entry's rounding errors are relative to.  A code's SCALE is the
largest magnitude entry over its rows (a code with one key has dS = rounding noise and a reference of about 0: the largest
|reference| entry would not do).

acc = np.float64: everything in fp64.  acc = np.float32: the matrix products, exp and the elementwise chain in fp32 -- the kernel's
own precisions; the difference between the two is what fp32 accumulation may legitimately move.
The dropout mask comes in from outside (oracle.att_keep_mask): it is neither re-derived here nor recovered from the kernels.
"""
import numpy as np
import torch

HALF_ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def round_to(a, half):
    """r(.): a (float array) rounded to nearest even in `half` (None: identity), back as float64."""
    a = np.asarray(a)
    if half is None:
        return a.astype(np.float64)
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(half).to(torch.float64).numpy()


def keep_masks(oracle, seed, q_start, q_len, kv_len, dropout_p):
    """per code the [q_len, kv_len] keep mask of the oracle's stateless hash (packed query row, key of the code)"""
    return [oracle.att_keep_mask(seed, int(q_start[b]), int(q_len[b]), int(kv_len[b]), dropout_p) for b in range(len(q_len))]


def keep_scale_of(dropout_p):
    """1 / (1 - p) as the launch code takes it: in fp32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(dropout_p))) if dropout_p > 0 else 1.0


def backward(q, q_start, q_len, kv, kv_start, kv_len, d_out, out, lse, scale, masks, keep_scale, half=None, acc=np.float64):
    """dict: dq [nq, d], dkv [nk, d] (float64; rows of no code zero), dq_mag / dkv_mag (the magnitudes), delta / delta_mag [nq],
    and per code dq_scale, dkv_scale, ds_max, pm_max, q_max, kv_max, g_max (largest |r(dS)|, |r(PM)| and rounded-operand entries)."""
    q, kv, d_out, out = (np.asarray(a, np.float32) for a in (q, kv, d_out, out))
    lse = np.asarray(lse, np.float32)
    n = len(q_len)
    scale_a, ks_a = acc(np.float32(scale)), acc(np.float32(keep_scale))
    res = dict(dq=np.zeros(q.shape), dkv=np.zeros(kv.shape), dq_mag=np.zeros(q.shape), dkv_mag=np.zeros(kv.shape))
    if acc is np.float64:
        res["delta"] = (d_out.astype(np.float64) * out).sum(1)
    else:
        res["delta"] = (d_out * out).sum(1, dtype=np.float32).astype(np.float64)
    res["delta_mag"] = np.abs(d_out.astype(np.float64) * out).sum(1)
    for key in ("dq_scale", "dkv_scale", "ds_max", "pm_max", "q_max", "kv_max", "g_max"):
        res[key] = np.zeros(n)
    for b in range(n):
        qs, ql, ks, kl = int(q_start[b]), int(q_len[b]), int(kv_start[b]), int(kv_len[b])
        if ql == 0 or kl == 0:
            continue
        rows, keys = slice(qs, qs + ql), slice(ks, ks + kl)
        Qr, Kr, Gr = round_to(q[rows], half), round_to(kv[keys], half), round_to(d_out[rows], half)
        M = np.asarray(masks[b], bool)
        assert M.shape == (ql, kl)
        Qa, Ka, Ga = Qr.astype(acc), Kr.astype(acc), Gr.astype(acc)
        delta = res["delta"][rows].astype(acc)[:, None]
        S = (Qa @ Ka.T) * scale_a
        P = np.exp(S - lse[rows].astype(acc)[:, None])
        PM = np.where(M, P * ks_a, acc(0))
        dP = np.where(M, (Ga @ Ka.T) * ks_a, acc(0))
        dS = P * (dP - delta) * scale_a
        assert P.dtype == acc and dS.dtype == acc and PM.dtype == acc
        PMr, dSr = round_to(PM.astype(np.float32), half).astype(acc), round_to(dS.astype(np.float32), half).astype(acc)
        res["dq"][rows] = dSr @ Ka
        res["dkv"][keys] = PMr.T @ Ga + dSr.T @ Qa
        dS_mag = np.abs(P.astype(np.float64)) * (np.abs(dP.astype(np.float64)) + np.abs(delta.astype(np.float64))) * float(scale_a)
        res["dq_mag"][rows] = dS_mag @ np.abs(Kr)
        res["dkv_mag"][keys] = np.abs(PM.astype(np.float64)).T @ np.abs(Gr) + dS_mag.T @ np.abs(Qr)
        res["dq_scale"][b], res["dkv_scale"][b] = res["dq_mag"][rows].max(), res["dkv_mag"][keys].max()
        res["ds_max"][b], res["pm_max"][b] = np.abs(dSr).max(), np.abs(PMr).max()
        res["q_max"][b], res["kv_max"][b], res["g_max"][b] = np.abs(Qr).max(), np.abs(Kr).max(), np.abs(Gr).max()
    return res


def code_error(got, ref, scale, start, length):
    """largest |got - ref| over rows [start, start + length) divided by the code's scale (0 where nothing differs)"""
    if length == 0:
        return 0.0
    diff = float(np.abs(np.asarray(got, np.float64)[start: start + length] - ref[start: start + length]).max())
    if diff == 0.0:
        return 0.0
    return diff / scale if scale > 0 else float("inf")


def flips(ref, half):
    """(flip_dq, flip_dkv) per code: ONE half-precision ulp of the code's largest |dS| (|PM|) entry times its largest operand entry,
    over the code's scale -- a single PM / dS entry landing on the other side of a rounding boundary."""
    ulp = HALF_ULP[half]
    with np.errstate(divide="ignore", invalid="ignore"):
        f_dq = np.where(ref["dq_scale"] > 0, ulp * ref["ds_max"] * ref["kv_max"] / ref["dq_scale"], 0.0)
        f_dkv = np.where(ref["dkv_scale"] > 0,
                         ulp * np.maximum(ref["pm_max"] * ref["g_max"], ref["ds_max"] * ref["q_max"]) / ref["dkv_scale"], 0.0)
    return f_dq, f_dkv
