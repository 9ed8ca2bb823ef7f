"""Cases, references and the derived allowance of the row-sharded products (enlsip_gn_tsqr_products*): test infrastructure, CPU only.

References: J p, v = rx + J p, J' v and the three sums as correctly rounded sums of exact products (consumer_reference:
Dekker's two-product + math.fsum).

Allowance (derived, not measured).  u = 2^-53, gamma_k = k u / (1 - k u).  For ANY order of summation, with or without fused
multiply-adds, a sum of k products computed in FP64 differs from the exact one by at most gamma_k sum |a_i b_i|.
  * (J p)_r is a sum of n products: |Jp_c - Jp| <= gamma_n a, a = |J| |p|.  Adding rx: |v_c - v| <= gamma_{n+1} (|rx| + a).
  * (J' v_c)_j over the G shards is a sum of m products, then at most G + 2 further additions of partial sums that the chunked
    and ranked order makes explicit (the +0.0 starts, the rank additions): k = m + G + 2 bounds the depth whatever the chunking,
    so |g_c - J' v_c|_j <= gamma_k (|J|' |v_c|)_j, and |J' v_c - J' v|_j <= gamma_{n+1} (|J|' (|rx| + a))_j.
  * dot(rx,rx): gamma_k sum rx^2.  dot(Jp,Jp): gamma_k sum Jp_c^2 + sum (2 |Jp| e + e^2), e = gamma_n a, |Jp| <= a:
    (gamma_k + 3 gamma_{n+1}) sum a^2.  dot(Jp,rx): (gamma_k + 2 gamma_{n+1}) sum a |rx|.
The reference itself is rounded once (u |ref|) and, for J' v, formed from the rounded v (u |J|' |v|): 2 u of the magnitude is
added.  The bound is evaluated in FP64 from non-negative terms (relative error ~ m u) and multiplied by 1.001 to cover that.
"""
import math
import re
from pathlib import Path

import numpy as np

import consumer_reference as cr

ROOT = Path(__file__).resolve().parents[1]
HDR = ROOT / "enlsip.jl_amd" / "csrc" / "gn_kernels_tsqr_products.hpp"
U = cr.U


def _const(name):
    mt = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9]+)\s*;", HDR.read_text())
    assert mt, f"{name} not found in {HDR.name}"
    return int(mt.group(1))


def chunk_height():
    return _const("TP_CH")


def header_doubles():
    return _const("TP_HDR")


def msg_len(n):
    return (header_doubles() + n + 3 + 1) & ~1


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
NS = (1, 5, 64, 65)


def splits():
    """name -> shard heights.  Every height of {0, 1, 63, 64, 65, CH-1, CH, CH+1, 2CH+1} occurs, G in {1, 2, 3, 8}; a one-row shard,
    a zero-row shard (first, in the middle) and shards shorter than n = 64 / 65."""
    CH = chunk_height()
    return {
        "g1_2ch+1": (2 * CH + 1,),
        "g2_ch-1_1": (CH - 1, 1),
        "g3_65_0_ch": (65, 0, CH),
        "g8_all": (0, 1, 63, 64, 65, CH - 1, CH, CH + 1),
    }


def problem(seed, m, n, with_p=True):
    """Gaussian J (m x n), rx (m), p (n): no term of any sum is negligible"""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((m, n))
    rx = rng.standard_normal(m)
    p = rng.standard_normal(n) if with_p else None
    return J, rx, p


def case_seed(name, n, with_p):
    return 7100 + 97 * sorted(splits()).index(name) + 11 * n + (1 if with_p else 0)


# ---- references and bounds -------------------------------------------------------------------------------------------------------
class Reference:
    """grad = J' (rx + J p), Jp, sums = (dot(rx,rx), dot(Jp,Jp), dot(Jp,rx)) correctly rounded, and their allowances for G shards"""

    def __init__(self, J, rx, p, G):
        m, n = J.shape
        self.m, self.n, self.G = m, n, G
        a = np.abs(J) @ np.abs(p) if p is not None else np.zeros(m)
        self.Jp = cr.exact_matvec(J, p)[0] if (p is not None and m) else np.zeros(m)
        self.v = cr.exact_matvec(J, p, x0=rx)[0] if (p is not None and m) else rx.copy()
        self.grad = cr.exact_matvec(J.T, self.v)[0] if m else np.zeros(n)
        one = np.ones(1)
        dot = lambda x, y: cr.exact_matvec((x * 1.0)[None, :], y)[0][0] if m else 0.0
        self.sums = np.array([dot(rx, rx), dot(self.Jp, self.Jp), dot(self.Jp, rx)])
        k = m + G + 2
        gk, gn1 = gamma(k), gamma(n + 1)
        absJt = np.abs(J).T
        mag = absJt @ np.abs(self.v) if m else np.zeros(n)
        self.grad_bound = 1.001 * ((gk + 2 * U) * mag * (1.0 + gn1) + (gn1 * (absJt @ (np.abs(rx) + a)) if p is not None else 0.0))
        self.Jp_bound = 1.001 * (gamma(n) + U) * a
        srr, saa, sar = float(rx @ rx), float(a @ a), float(a @ np.abs(rx))
        self.sums_bound = 1.001 * np.array([(gk + 2 * U) * srr, (gk + 3 * gn1 + 2 * U) * saa, (gk + 2 * gn1 + 2 * U) * sar])

    def check(self, grad, sums, label, Jp=None):
        """None, or a description of the first entry outside its allowance"""
        eg = np.abs(np.asarray(grad) - self.grad)
        if not np.all(eg <= self.grad_bound):
            j = int(np.argmax(eg - self.grad_bound))
            return f"{label}: grad[{j}] off by {eg[j]:.3e}, allowance {self.grad_bound[j]:.3e}"
        es = np.abs(np.asarray(sums) - self.sums)
        if not np.all(es <= self.sums_bound):
            j = int(np.argmax(es - self.sums_bound))
            return f"{label}: sums[{j}] off by {es[j]:.3e}, allowance {self.sums_bound[j]:.3e}"
        if Jp is not None:
            ej = np.abs(np.asarray(Jp) - self.Jp)
            if not np.all(ej <= self.Jp_bound):
                j = int(np.argmax(ej - self.Jp_bound))
                return f"{label}: Jp[{j}] off by {ej[j]:.3e}, allowance {self.Jp_bound[j]:.3e}"
        return None


# ---- the chunked order, restated in NumPy ----------------------------------------------------------------------------------------
_BUTTERFLY = (1, 2, 7, 15, 16, 32)      # partner = lane ^ x at each level of wave_allsum (gn_device_utils.hpp)


def _wave_allsum(s):
    """s: (64, ...) lane partials -> the butterfly's value (identical in every lane; lane 0 taken)"""
    lanes = np.arange(64)
    for x in _BUTTERFLY:
        s = s + s[lanes ^ x]
    return s[0]


def _chunk_dot(A, v, CH):
    """A (rows x k), v (rows), rows <= CH: lane l adds rows l, l + 64, ... ascending from +0.0, then the butterfly"""
    rows, k = A.shape
    pad = (-rows) % 64
    Ap = np.concatenate([A * v[:, None], np.zeros((pad, k))]).reshape(-1, 64, k)
    s = np.zeros((64, k))
    for i in range(Ap.shape[0]):
        s = s + Ap[i]
    return _wave_allsum(s)


def shard_message(J, rx, p, CH, drop_last_row=False, skip_chunk=None):
    """body (n + 3) of one shard in the kernels' order (products rounded on their own: a restatement of the ORDER, not of the bits).
    Mutations: drop_last_row leaves the shard's last row out of every sum; skip_chunk leaves that chunk's partial out."""
    m, n = J.shape
    if p is not None:
        parts = []
        for w in range(4):
            s = np.zeros(m)
            for c in range(w, n, 4):
                s = s + J[:, c] * p[c]
            parts.append(s)
        Jp = (parts[0] + parts[1]) + (parts[2] + parts[3])
        v = rx + Jp
    else:
        Jp, v = np.zeros(m), rx
    rows = m - 1 if (drop_last_row and m > 0) else m
    body = np.zeros(n + 3)
    for ch, r0 in enumerate(range(0, rows, CH)):
        if skip_chunk is not None and ch == skip_chunk:
            continue
        sl = slice(r0, min(r0 + CH, rows))
        part = np.concatenate([_chunk_dot(J[sl], v[sl], CH),
                               _chunk_dot(np.stack([rx[sl], Jp[sl], Jp[sl]], axis=1) * np.stack([rx[sl], Jp[sl], rx[sl]], axis=1),
                                          np.ones(sl.stop - sl.start), CH)])
        body = body + part
    return body, Jp


def chunked_products(J, rx, p, heights, CH, drop_last_row_of=None, skip_chunk_of=None):
    """(grad, sums) over the shards in rank order, rank 0's value first"""
    n = J.shape[1]
    acc, lo = None, 0
    for g, h in enumerate(heights):
        body, _ = shard_message(J[lo:lo + h], rx[lo:lo + h], p, CH, drop_last_row=(g == drop_last_row_of),
                                skip_chunk=(0 if g == skip_chunk_of else None))
        acc = body if acc is None else acc + body
        lo += h
    return acc[:n], acc[n:]


def np_local_stage(J_loc, rx_loc, p, msg):
    """Stand-in for enlsip_gn_tsqr_products_local_dev in enlsip_gn.tsqr.tsqr_products (torch CPU tensors in, the message filled)"""
    import torch
    Jl = J_loc.numpy().T.copy()
    n = Jl.shape[1]
    body, Jp = shard_message(Jl, rx_loc.numpy(), None if p is None else np.asarray(p, dtype=np.float64), chunk_height())
    H = header_doubles()
    msg[2] = float(n)
    msg[H:H + n + 3] = torch.from_numpy(body)
    return torch.from_numpy(Jp) if p is not None else None


# ---- estimate cases of the GPU test: (name, n, t, kappa(A)) on one tall matrix ------------------------------------------------------
ESTIMATE_CASES = [
    ("n5_t0", 5, 0, 1.0),
    ("n5_t1", 5, 1, 1.0),
    ("n5_t5", 5, 5, 1e2),
    ("n64_t64", 64, 64, 1e2),
    ("n65_t1", 65, 1, 1.0),
    ("n12_t6_dup", 12, 6, "dup"),       # rank-deficient A: zero multipliers and grad_res with prankA < t
]
