"""gatmh_hub_split_ref.py -- TEST INFRASTRUCTURE: the chunk-and-merge arithmetic of dory_gatmh_row_gather_hub_split (include/dorylus_hip.h;
csrc/gat_mh_rows.hip) restated in numpy, float32 throughout, for one layer on one partition without ghosts.

A row with more than `chunk` adjacency entries is cut into consecutive chunks of `chunk` entries, the last one shorter; the self edge is
the last entry of the id stream and goes with the last chunk.  Each chunk is walked on its own, the chunks of a row are folded IN CHUNK
ORDER, and the fold closes with the epilogue of the one-pass kernels:

  forward   chunk c:  m_c = max s,  den_c = sum exp(s - m_c),  den+_c (entries with el + er > 0),  acc_c = sum exp(s - m_c) z[src],  acc+_c
            merge:    M = max_c m_c,  f_c = exp(m_c - M),  den = sum_c f_c den_c  (likewise den+, acc, acc+)
            close:    o = acc / den,  op = acc+ / den,  m = M,  den,  dpos = den+ / den
  dst       chunk c:  alpha = exp(s - m) / den against the ROW's m / den;  t_c = sum alpha <do[v], z[src]>,  a1_c = sum alpha <.,.> l',
            a2_c = sum alpha l'   (l' = 1 where el + er > 0, else 0.2)
            merge:    plain sums;  close: t,  der = a1 - t a2
  src       chunk c (out-edges of u, entries = destinations v):  alpha = exp(lrelu(el[u] + er[v]) - m[v]) / den[v];
            S_c = sum alpha do[v],  S+_c (el + er > 0),  T_c = sum alpha t[v],  T+_c
            merge:    plain sums;  close: del = <z[u], 0.2 S + 0.8 S+> - (0.2 T + 0.8 T+),  dz = S + del a_l + der a_r

The kernels walk a chunk in batches of four entries with online rescaling; this file takes a chunk's maximum first -- the same value in exact
arithmetic, and what the merge formulas need is only that each chunk's state is (m_c, sums scaled by exp(-m_c))."""
import numpy as np

F = np.float32
SLOPE = F(0.2)


def row_chunks(ptr, v, chunk):
    """[(e0, e1, has_self)] of row v: one range for a row of at most `chunk` entries (chunk 0: never cut)"""
    b, e = int(ptr[v]), int(ptr[v + 1])
    if chunk == 0 or e - b <= chunk:
        return [(b, e, True)]
    out = []
    for c0 in range(b, e, chunk):
        c1 = min(c0 + chunk, e)
        out.append((c0, c1, c1 == e))
    return out


def _lrelu(x):
    return np.where(x > 0, x, SLOPE * x).astype(F)


def forward(colptr, rowidx, Z, el, er, K, chunk):
    N, KD = Z.shape
    D = KD // K
    Z3 = Z.astype(F).reshape(N, K, D)
    el, er = el.astype(F), er.astype(F)
    o, op = np.zeros((N, K, D), F), np.zeros((N, K, D), F)
    m, den, dpos = np.zeros((N, K), F), np.zeros((N, K), F), np.zeros((N, K), F)
    for v in range(N):
        states = []
        for e0, e1, has_self in row_chunks(colptr, v, chunk):
            src = np.concatenate([rowidx[e0:e1].astype(np.int64), [v] if has_self else []]).astype(np.int64)
            pre = (el[src] + er[v]).astype(F)                        # entries x K
            s = _lrelu(pre)
            mc = s.max(0)
            p = np.exp(s - mc, dtype=F)
            pp = np.where(pre > 0, p, F(0))
            states.append((mc, p.sum(0, dtype=F), pp.sum(0, dtype=F), np.einsum("ek,ekd->kd", p, Z3[src]).astype(F),
                           np.einsum("ek,ekd->kd", pp, Z3[src]).astype(F)))
        M = np.max([st[0] for st in states], axis=0)
        dn, dp, acc, accp = np.zeros(K, F), np.zeros(K, F), np.zeros((K, D), F), np.zeros((K, D), F)
        for mc, d_c, dp_c, a_c, ap_c in states:                      # in chunk order
            f = np.exp(mc - M, dtype=F)
            dn, dp = dn + f * d_c, dp + f * dp_c
            acc, accp = acc + f[:, None] * a_c, accp + f[:, None] * ap_c
        idn = F(1) / dn
        o[v], op[v], m[v], den[v], dpos[v] = acc * idn[:, None], accp * idn[:, None], M, dn, dp * idn
    return o.reshape(N, KD), op.reshape(N, KD), m, den, dpos


def dst_side(colptr, rowidx, Z, el, er, m, den, dO, K, chunk):
    N, KD = Z.shape
    D = KD // K
    Z3, dO3 = Z.astype(F).reshape(N, K, D), dO.astype(F).reshape(N, K, D)
    el, er, m, den = el.astype(F), er.astype(F), m.astype(F), den.astype(F)
    t, der = np.zeros((N, K), F), np.zeros((N, K), F)
    for v in range(N):
        tt, a1, a2 = np.zeros(K, F), np.zeros(K, F), np.zeros(K, F)
        idn = F(1) / den[v]
        for e0, e1, has_self in row_chunks(colptr, v, chunk):        # in chunk order
            src = np.concatenate([rowidx[e0:e1].astype(np.int64), [v] if has_self else []]).astype(np.int64)
            pre = (el[src] + er[v]).astype(F)
            al = np.exp(_lrelu(pre) - m[v], dtype=F) * idn
            lp = np.where(pre > 0, F(1), SLOPE)
            prod = np.einsum("kd,ekd->ek", dO3[v], Z3[src]).astype(F)
            tt, a1, a2 = tt + (al * prod).sum(0, dtype=F), a1 + (al * prod * lp).sum(0, dtype=F), a2 + (al * lp).sum(0, dtype=F)
        t[v], der[v] = tt, a1 - tt * a2
    return t, der


def src_side(rowptr, colidx, Z, el, er, m, den, t, der, dO, a_l, a_r, K, chunk):
    N, KD = Z.shape
    D = KD // K
    Z3, dO3 = Z.astype(F).reshape(N, K, D), dO.astype(F).reshape(N, K, D)
    el, er, m, den, t, der = (x.astype(F) for x in (el, er, m, den, t, der))
    al3, ar3 = a_l.astype(F).reshape(K, D), a_r.astype(F).reshape(K, D)
    lo, hi = SLOPE, F(1) - SLOPE
    dl, dz = np.zeros((N, K), F), np.zeros((N, K, D), F)
    for u in range(N):
        S, Sp, T, Tp = np.zeros((K, D), F), np.zeros((K, D), F), np.zeros(K, F), np.zeros(K, F)
        for e0, e1, has_self in row_chunks(rowptr, u, chunk):        # in chunk order
            dv = np.concatenate([colidx[e0:e1].astype(np.int64), [u] if has_self else []]).astype(np.int64)
            pre = (el[u] + er[dv]).astype(F)
            al = np.exp(_lrelu(pre) - m[dv], dtype=F) / den[dv]
            alp = np.where(pre > 0, al, F(0))
            S, Sp = S + np.einsum("ek,ekd->kd", al, dO3[dv]).astype(F), Sp + np.einsum("ek,ekd->kd", alp, dO3[dv]).astype(F)
            T, Tp = T + (al * t[dv]).sum(0, dtype=F), Tp + (alp * t[dv]).sum(0, dtype=F)
        dl[u] = (Z3[u] * (lo * S + hi * Sp)).sum(-1, dtype=F) - (lo * T + hi * Tp)
        dz[u] = S + dl[u][:, None] * al3 + der[u][:, None] * ar3
    return dl, dz.reshape(N, KD)
