"""Numpy model of the 2-term pairwise screen (csrc/assign.hip, "Two-term pairwise screen"), shared by
tests/test_pair_bound.py (CPU) and tests/test_gpu_pair_screen.py: the centre table and the pair table as
rqsid_prepare_centers / rqsid_pair_table build them, the row as the screen sees it (fp16 rounding with the
kernel's flush of subnormals), the two accumulators through tools/mfma_model.py's chain_dot, and the epilogue's
threshold.  fp32 steps of the kernel are taken in float64 and rounded once; the bound's own 1 + 1e-6 factors
cover that."""
import importlib.util
from pathlib import Path

import numpy as np

F32 = np.float32
_spec = importlib.util.spec_from_file_location("mfma_model", Path(__file__).resolve().parent.parent / "tools" / "mfma_model.py")
mfma_model = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfma_model)

KTRUNC = 16.0


def acc_rel(dim):
    return float(F32((KTRUNC + (dim // 16) / 2.0 + 1.0) * 2.0 ** -23 * 1.02))


def centre_f16(a):
    """to_f16 (assign_common.h): fp16 of a scaled centre element, 0 outside the normal range."""
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore"):
        h = a.astype(np.float16).astype(np.float64)
    return np.where((np.abs(a) >= 2.0 ** -14) & (np.abs(a) < 65504.0), h, 0.0)


def row_f16(v):
    """v_cvt_pk_f16_f32 with fp16 denormals flushed: round to nearest even, results below 2^-14 become 0."""
    with np.errstate(over="ignore"):
        h = np.asarray(v, F32).astype(np.float16).astype(np.float64)
    return np.where(np.abs(h) < 2.0 ** -14, 0.0, h)


def fp16_up(x):
    """The pair table's entry for a distance x (in table units): the least fp16 >= x, at least 2^-14 where
    x > 0, inf from 65504 on."""
    x = np.asarray(x, np.float64) * (1.0 + 1e-12)
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.minimum(x, 65504.0).astype(np.float16)
        low = h.astype(np.float64) < x
        h = np.where(low, np.nextafter(h, np.float16(np.inf)), h).astype(np.float64)
    h = np.where((x > 0) & (h < 2.0 ** -14), 2.0 ** -14, h)
    return np.where(x < 65504.0, h, np.inf)


class Table:
    """One candidate list's centres as the screen holds them."""

    def __init__(self, c, scale_from=None):
        c = np.asarray(c, F32)
        ref = c if scale_from is None else np.asarray(scale_from, F32)  # the scale is the whole table's
        m = float(np.abs(ref).max()) if ref.size else 0.0
        self.s = int(np.clip(14 - np.frexp(F32(m))[1], -100, 100)) if 0 < m <= 3.4e38 else 0
        cs = np.ldexp(c.astype(np.float64), self.s)
        self.ch = centre_f16(cs)
        self.cl = centre_f16((cs - self.ch) * 4096.0)
        cd = c.astype(np.float64)
        e1 = cd - np.ldexp(self.ch, -self.s)
        e2 = e1 - np.ldexp(self.cl, -self.s - 12)
        up = F32(1.0000002)
        self.csq = (cd * cd).sum(1).astype(F32)
        self.y = np.sqrt((cd * cd).sum(1)).astype(F32) * up
        self.z = np.sqrt((e2 * e2).sum(1)).astype(F32) * up
        self.w = np.sqrt((e1 * e1).sum(1)).astype(F32) * up
        self.c = cd
        dist = np.sqrt(((cd[:, None, :] - cd[None, :, :]) ** 2).sum(2))
        self.unit = 2.0 ** (7 - self.s)  # one table unit
        self.T = fp16_up(dist / self.unit)

    def ratios(self):
        def ratio_up(num, den):
            with np.errstate(divide="ignore", invalid="ignore"):
                r = num.astype(np.float64) / den * 1.000001
            return np.where(den > 0, r, np.where(num > 0, np.inf, 0.0))
        return float(ratio_up(self.z, self.y).max()), float(ratio_up(self.w, self.y).max()), float(self.y.max())


def screen(v, tab, norm=False, rl=1, dr=None):
    """The screen's view of rows v [n, d] (fp32: the residual chain's result before any normalisation) against
    the list tab: returns dict(P, thr_x, G, b, npass).  Candidate k of row i stays iff
    P[i, k] - P[i, b_i] <= thr_x[i] T[b_i, k] + G[i, k] + G[i, b_i] (G includes the 1e-30 of each side)."""
    v = np.asarray(v, F32)
    n, d = v.shape
    vd = v.astype(np.float64)
    vh = row_f16(v)
    with np.errstate(invalid="ignore", over="ignore"):
        en = float(1.001) * np.sqrt(((vd - vh) ** 2).sum(1)).astype(F32).astype(np.float64) + 1e-30
        nrm = np.sqrt((vd * vd).sum(1)).astype(F32).astype(np.float64)
    vn = nrm * 1.0001 + 1e-30
    if norm:
        inv_den = (1.0 / (nrm + 1e-8).astype(F32)).astype(F32).astype(np.float64)
    else:
        inv_den = np.ones(n)
    if dr is None:
        dr = 2.0 * 5.97e-8 if (norm and rl == 1) else 0.0
    dr = np.broadcast_to(np.asarray(dr, np.float64), (n,))
    ar = acc_rel(d)
    hn, vr, k2 = vn + en, vn * inv_den, 2.0 * inv_den * 1.000001
    gz, gw, gy = tab.ratios()
    Ag = k2 * (ar * hn) + 2.0 * dr + 7.2e-7 * vr
    Bg = k2 * hn * (1.0 + ar)
    Cg = k2 * hn * (2.0 * ar)
    A2 = (Ag + Bg * gz + Cg * gw + 2.39e-7 * gy) * 1.000001
    Ax = k2 * en * 1.000001 * tab.unit
    with np.errstate(invalid="ignore", over="ignore"):
        acc = mfma_model.chain_dot(vh, tab.ch).astype(np.float64)
        accl = mfma_model.chain_dot(vh, tab.cl).astype(np.float64)
        m2 = -2.0 * inv_den * 2.0 ** -tab.s
        dot = (accl * 2.0 ** -12 + acc).astype(F32).astype(np.float64)
        P = (m2[:, None] * dot + tab.csq[None, :]).astype(F32).astype(np.float64)
        b = np.argmin(np.where(np.isnan(P), np.inf, P), 1)
        G = A2[:, None] * tab.y[None, :].astype(np.float64) + 1e-30
        thr = Ax[:, None] * tab.T[b] + G + G[np.arange(n), b][:, None]
        margin = (P - P[np.arange(n), b][:, None]) - thr
        keep = ~(margin >= 0)
        finite = np.isfinite(A2 + Ax) & np.isfinite(P[np.arange(n), b])
        # The hardware's accumulators are not chain_dot's: each lies within the accumulation allowance of the exact
        # sums (acc: acc_rel |vh| |ch_k|, accl: acc_rel |vh| |cl_k 2^-12|, with |ch_k| <= |c_k| + |ec1_k| and
        # |cl_k 2^-12| <= |ec1_k| + |ec2_k|), so the two P_k differ by at most twice that, and a candidate whose
        # margin is inside it, for k and for b together, may fall either way on the device: keep_upper keeps it.
        # (Where the device picks another b', P_b' lies within that distance of P_b: b and b' both stay, here and
        # there, and the row is ambiguous either way.)
        sl = 2.0 * (k2 * ar * hn)[:, None] * (tab.y + 2.0 * tab.w + tab.z).astype(np.float64)[None, :]
        keep_upper = ~(margin - (sl + sl[np.arange(n), b][:, None]) >= 0)
    keep[~finite] = True
    keep_upper[~finite] = True
    return dict(P=P, Ax=Ax, A2=A2, G=G, b=b, npass=keep.sum(1), keep=keep, inv_den=inv_den, finite=finite,
                npass_upper=keep_upper.sum(1))


def true_scores(v, tab, norm):
    """S[i, k] = |c_k|^2 - 2 r_i . c_k in float64, r the reference's row: fl32(v / den) under normalisation."""
    v = np.asarray(v, F32)
    if norm:
        nrm = np.sqrt((v.astype(np.float64) ** 2).sum(1)).astype(F32)
        r = (v / (nrm + F32(1e-8))[:, None]).astype(F32).astype(np.float64)
    else:
        r = v.astype(np.float64)
    return (tab.c * tab.c).sum(1)[None, :] - 2.0 * r @ tab.c.T
